"""Micro-probe of the fused MBConv front kernel of the fp32 early blocks (EfficientNet-B0 blocks 1-5, ground 160 x 320 and aerial
256 x 256 stem outputs): python tools/mbf_s3_probe.py [reps] [batches]
Every layer runs alone at B = 64, 8 and 1 (batches: comma list), through the fp32 kernel (ops.mbconv_front) and through the
three-plane bf16 form (ops.mbconv_front_s3, whatever its size rule says).  Three passes of `reps` launches each after an untimed
one, alternating; s3/f32 = ratio of the medians, spread = the larger (max - min) / median of the two.  A layer wins where
s3/f32 < 1 - spread: the size rule in csrc/mbconv_front.hip (mbf3_measured) and the table of DESIGN section 4 come from this output.
diff = max |y_s3 - y_f32| / max |y_f32| of the two outputs (fp32 rounding class; the tests compare both with fp64).
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccvpe_amd import models, ops       # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
batches = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [64, 8, 1]
# (block, k, s, cin, mid, ground plane, aerial plane)
BLOCKS = [(1, 3, 2, 16, 96, (160, 320), (256, 256)), (2, 3, 1, 24, 144, (80, 160), (128, 128)), (3, 5, 2, 24, 144, (80, 160), (128, 128)),
          (4, 5, 1, 40, 240, (40, 80), (64, 64)), (5, 3, 2, 40, 240, (40, 80), (64, 64))]


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


print("%-5s %-6s %3s %-7s %-9s | %9s | %9s | %6s %6s %3s | %8s" % (
    "block", "side", "B", "k s", "plane", "f32 us", "s3 us", "s3/f32", "spread", "ok", "diff"), flush=True)
for b in batches:
    for blk, k, s, cin, mid, grd, sat in BLOCKS:
        for side, (h, w) in (("ground", grd), ("aerial", sat)):
            circ = side == "ground"
            x = torch.randn((b, h, w, cin), device="cuda")
            we = models._pad2(torch.randn((mid, cin), device="cuda") * cin ** -0.5)
            w3 = models._pack_pw_s3(we)
            s0, s1 = (torch.rand((mid,), device="cuda") + 0.5 for _ in range(2))
            b0, b1 = (torch.randn((mid,), device="cuda") * 0.3 for _ in range(2))
            wd = torch.randn((k, k, mid), device="cuda") * 0.2
            run_f = lambda: ops.mbconv_front(x, we, s0, b0, wd, s1, b1, mid, k, s, circ)
            run_s = lambda: ops.mbconv_front_s3(x, w3, s0, b0, wd, s1, b1, mid, k, s, circ)
            ok = ops.mbconv_front_s3_ok(x, w3, mid, k, s)
            line = "%-5d %-6s %3d k%d s%d   %3dx%-5d" % (blk, side, b, k, s, h, w)
            if not ok:
                print(line + " | %9.1f | not served" % (timed(run_f) * 1e3), flush=True)
                continue
            yf, ys = run_f()[0], run_s()[0]
            diff = ((ys - yf).abs().max() / yf.abs().max()).item()
            del yf, ys
            timed(run_f), timed(run_s)                      # one untimed pass of each: clocks and caches settle
            tf, ts = [], []
            for _ in range(3):
                tf.append(timed(run_f))
                ts.append(timed(run_s))
            mf, ms = sorted(tf)[1], sorted(ts)[1]
            spread = max((max(t) - min(t)) / sorted(t)[1] for t in (tf, ts))
            print(line + " | %9.1f | %9.1f | %6.3f %6.3f %3d | %8.1e" % (mf * 1e3, ms * 1e3, ms / mf, spread, ok, diff), flush=True)
