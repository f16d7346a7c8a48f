"""Micro-probe of the fp32 Winograd conv.1 kernels on the narrow decoder levels: python tools/wino_probe.py [reps] [batches]
For each shape the current route (conv3x3_wino_kernel, on the localisation levels followed by the one-hypothesis match_level)
is timed against conv3x3_wino_n_kernel (on the localisation levels with the matching fused), three alternating passes of
`reps` launches each after an untimed one: n/w = ratio of the medians, spread = the larger (max - min) / median of the two.
A shape is routed (csrc/conv3x3_wino_n.hip WINO_N_MIN_PIXELS) only if n/w < 1 - spread.
First line: the premise check — conv3x3_wino_kernel at the loc 256 x 256 shape with N = 32 (one column tile) and N = 40 (two).
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccvpe_amd import models, ops       # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
batches = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [64, 8]
# (hw, c = n, L of the NEXT level or 0 = orientation branch: conv only, stride of the next level)
SHAPES = [(128, 80, 80, 1), (256, 40, 40, 1), (128, 64, 0, 1), (256, 32, 0, 1)]


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


def ab(fa, fb):
    ta, tb = [], []
    timed(fa), timed(fb)                # one untimed pass of each: clocks and caches settle
    for _ in range(3):
        ta.append(timed(fa))
        tb.append(timed(fb))
    ma, mb = sorted(ta)[1], sorted(tb)[1]
    return ma, mb, max((max(t) - min(t)) / sorted(t)[1] for t in (ta, tb))


def layer(b, hw, c, n):
    w = torch.randn((n, c, 3, 3), device="cuda") * (1.0 / (9 * c)) ** 0.5
    return torch.randn((b, hw, hw, c), device="cuda"), models._pack_wino(w), torch.randn((n,), device="cuda") * 0.1


# premise: what does the second column tile of N = 40 cost?
x, u40, b40 = layer(64, 256, 40, 40)
_, u32, b32 = layer(64, 256, 40, 32)
t32, t40, sp = ab(lambda: ops.conv3x3_wino(x, 40, u32, 32, batch=64, in_h=256, in_w=256, shift=b32),
                  lambda: ops.conv3x3_wino(x, 40, u40, 40, batch=64, in_h=256, in_w=256, shift=b40))
print("premise  conv3x3_wino 256x256 c0=40  N=32 %8.1f us  N=40 %8.1f us  second tile %.1f %% of N=40  spread %.3f"
      % (t32 * 1e3, t40 * 1e3, 100.0 * (t40 - t32) / t40, sp), flush=True)
del x

for b in batches:
    for hw, c, L, stride in SHAPES:
        x, u, bias = layer(b, hw, c, c)
        kw = dict(batch=b, in_h=hw, in_w=hw)
        if not ops.conv3x3_wino_n_ok(x, c, u, c, **kw):
            print("B=%-3d %dx%d N=%d: not served" % (b, hw, hw, c), flush=True)
            continue
        pairs = [("conv      ", lambda: ops.conv3x3_wino(x, c, u, c, shift=bias, **kw),
                  lambda: ops.conv3x3_wino_n(x, c, u, c, shift=bias, **kw), ops.conv3x3_wino_n_ok(x, c, u, c, **kw))]
        if L:
            ldo = (c + 1 + 7) // 8 * 8
            g = torch.randn((b, L), device="cuda")

            def cur():
                y = ops.conv3x3_wino(x, c, u, c, shift=bias, **kw)
                return ops.match_level(y, g, L, [0], 1, 0, stride, ldo, channels=c)
            pairs.append(("conv+match", cur, lambda: ops.conv3x3_match1(x, c, u, c, g, L, 0, stride, ldo, bias=bias, **kw),
                          ops.conv3x3_match1(x, c, u, c, None, L, 0, stride, ldo, bias=bias, query_only=True, **kw)))
        for what, cur, new, ok in pairs:
            tw, tn, sp = ab(cur, new)
            print("B=%-3d %dx%d N=%-3d %s  wino %8.1f us  wino_n %8.1f us  n/w %.3f  spread %.3f  %s  ok=%d"
                  % (b, hw, hw, c, what, tw * 1e3, tn * 1e3, tn / tw, sp, "WIN" if tn / tw < 1 - sp else "stay", ok), flush=True)
