"""Micro-probe of the fp32 1x1 GEMMs behind the encoders' depthwise stage and of the two descriptor heads: python tools/pw_s3_probe.py [reps] [batches]
Every layer of the table runs alone at B = 64, 8 and 1 (batches: comma list), through today's route (ops.conv_igemm: the one-pass
kernel the library picks, or the split-K pair with its second pass — both launches are inside the timed window) and through the
three-plane bf16 kernel (ops.pw_s3, whatever its size rule says).  Three passes of `reps` launches each after an untimed one,
alternating; s3/f32 = ratio of the medians, spread = the larger (max - min) / median of the two.  A layer wins where
s3/f32 < 1 - spread: the size rule in csrc/pw_s3.hip (pw3_measured_size) and the table of DESIGN section 4 come from this output.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccvpe_amd import models, ops       # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
batches = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [64, 8, 1]
GRD, SAT = {16: (20, 40), 32: (10, 20)}, {16: (32, 32), 32: (16, 16)}      # feature planes at 1/16 and 1/32 of 320 x 640 / 512 x 512
# (name, K, N, resolution, gate, residual, act, sides)
LAYERS = [("block 5 project", 240, 80, 16, True, False, ops.ACT_NONE, "ga"),
          ("blocks 6-7 project", 480, 80, 16, True, True, ops.ACT_NONE, "ga"),
          ("block 8 project", 480, 112, 16, True, False, ops.ACT_NONE, "ga"),
          ("blocks 9-10 project", 672, 112, 16, True, True, ops.ACT_NONE, "ga"),
          ("block 11 project", 672, 192, 32, True, False, ops.ACT_NONE, "ga"),
          ("blocks 12-14 project", 1152, 192, 32, True, True, ops.ACT_NONE, "ga"),
          ("block 15 project", 1152, 320, 32, True, False, ops.ACT_NONE, "ga"),
          ("_conv_head + swish", 320, 1280, 32, False, False, ops.ACT_SWISH, "ga"),
          ("ground descriptors", 1280, 126, 32, False, False, ops.ACT_NONE, "g"),
          ("aerial descriptor 2x2 s2", 1280, 1280, 32, False, False, ops.ACT_NONE, "A")]


def timed(fn):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


print("%-26s %-6s %3s %6s %5s %5s | %9s %5s | %9s %7s | %6s %6s %3s" % (
    "layer", "side", "B", "M", "K", "N", "f32 us", "split", "s3 us", "TF-eq", "s3/f32", "spread", "ok"), flush=True)
for b in batches:
    for name, k, n, res, gated, resid, act, sides in LAYERS:
        for side in sides:
            two = side == "A"
            h, w = (GRD if side == "g" else SAT)[res]
            ho, wo = (h // 2, w // 2) if two else (h, w)
            m, kk = b * ho * wo, (4 if two else 1) * k
            x = torch.randn((b, h, w, k), device="cuda")
            wt = torch.randn((n, kk), device="cuda") * kk ** -0.5
            wp = models._pad2(wt)
            w3 = models._pack_pw_s3(wp)
            gate = torch.rand((b, k), device="cuda") if gated else None
            r = torch.randn((b, ho, wo, n), device="cuda") if resid else None
            sc, sh = torch.rand((n,), device="cuda") + 0.5, torch.randn((n,), device="cuda")
            ldd = (n + 3) // 4 * 4
            kw = dict(batch=b, in_h=h, in_w=w, gate=gate, scale=sc, shift=sh, residual=r, act=act, ldd=ldd)
            cv = dict(kh=2, kw=2, stride=2) if two else {}
            before = ops.SPLIT_K_CALLS
            run_f = lambda: ops.conv_igemm(x, k, wp, n, **kw, **cv)
            run_f()
            split = ops.SPLIT_K_CALLS > before
            ok = ops.pw_s3_ok(x, k, w3, n, batch=b, in_h=h, in_w=w, two=two, gate=gate, residual=r, act=act, ldd=ldd)
            line = "%-26s %-6s %3d %6d %5d %5d" % (name, {"g": "ground", "a": "aerial", "A": "aerial"}[side], b, m, kk, n)
            if not ok:
                print(line + " | %9.1f %5s | not served" % (timed(run_f) * 1e3, "yes" if split else "no"), flush=True)
                continue
            run_s = lambda: ops.pw_s3(x, k, w3, n, two=two, **kw)
            timed(run_f), timed(run_s)                      # one untimed pass of each: clocks and caches settle
            tf, ts = [], []
            for _ in range(3):
                tf.append(timed(run_f))
                ts.append(timed(run_s))
            mf, ms = sorted(tf)[1], sorted(ts)[1]
            spread = max((max(t) - min(t)) / sorted(t)[1] for t in (tf, ts))
            print(line + " | %9.1f %5s | %9.1f %7.1f | %6.3f %6.3f %3d" % (
                mf * 1e3, "yes" if split else "no", ms * 1e3, 2.0 * m * n * kk / ms / 1e9, ms / mf, spread, ok), flush=True)
