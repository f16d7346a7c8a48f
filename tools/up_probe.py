"""Micro-probe of the folded deconv + 3x3 kernels on the decoder's shapes: python tools/up_probe.py [reps] [bf16]
In fp32 every shape with a skip is also timed through the three-plane bf16 kernel (ccvpe_upconv3x3_s3_f32, whatever its size
rule says): the per-level table of DESIGN section 4 and the rule in csrc/upconv_s3.hip come from this output.  Where the quad
form (csrc/upconv_s3q.hip) serves the shape, the per-parity form (s3) and the quad form (s3q) are timed side by side, three
passes of `reps` launches each after an untimed one, alternating: q/p = ratio of the medians, spread = the larger (max - min) / median of the two.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccvpe_amd import models, ops       # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
dt = torch.bfloat16 if len(sys.argv) > 2 and sys.argv[2] == "bf16" else torch.float32
# (batch, h1, c0, c1, n): loc levels 6..1, ori levels 6..2 (level 6: both decoders read the same 1304-channel buffer)
shapes = [(64, 8, 1304, 320, 640), (64, 16, 648, 112, 320), (64, 32, 328, 40, 160), (64, 64, 168, 24, 80), (64, 128, 88, 16, 40),
          (64, 256, 48, 0, 16),
          (64, 16, 640, 112, 256), (64, 32, 256, 40, 128), (64, 64, 128, 24, 64), (64, 128, 64, 16, 32)]
if os.environ.get("PROBE_SHAPE"):
    shapes = [tuple(int(v) for v in os.environ["PROBE_SHAPE"].split(","))]
kmult = 16 if dt == torch.float32 else 32


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


for (b, h1, c0, c1, n) in shapes:
    k = 4 * c0 + 9 * c1
    kp = (k + kmult - 1) // kmult * kmult
    x = torch.randn((b, h1, h1, c0), device="cuda").to(dt)
    sk = torch.randn((b, 2 * h1, 2 * h1, c1), device="cuda").to(dt) if c1 else None
    w = (torch.randn((4, (n + 15) // 16 * 16, kp), device="cuda") * 0.01).to(dt)
    sh = torch.zeros((9, n), device="cuda")
    ms = timed(lambda: ops.upconv3x3(x, c0, w, sh, n, batch=b, h1=h1, w1=h1, src1=sk, c1=c1, act=ops.ACT_RELU))
    m = 4 * b * h1 * h1
    line = "upconv h1=%-3d c0=%-4d c1=%-3d N=%-3d %9.1f us %7.1f TF" % (h1, c0, c1, n, ms * 1e3, 2.0 * m * n * k / ms / 1e9)
    w3 = models._pack_upconv_s3(w, c0, c1, dt)
    ok = ops.upconv3x3_s3_ok(x, c0, w3, n, batch=b, h1=h1, w1=h1, src1=sk, c1=c1)
    if ok:
        run3 = lambda form: ops.upconv3x3_s3(x, c0, w3, sh, n, batch=b, h1=h1, w1=h1, src1=sk, c1=c1, act=ops.ACT_RELU, form=form)
        quad = ops.upconv3x3_s3_form_ok(x, c0, w3, n, 2, batch=b, h1=h1, w1=h1, src1=sk, c1=c1) == 2
        tp, tq = [], []
        if quad:
            timed(lambda: run3(1)), timed(lambda: run3(2))          # one untimed pass of each: clocks and caches settle
        for _ in range(3 if quad else 1):
            tp.append(timed(lambda: run3(1)))
            if quad:
                tq.append(timed(lambda: run3(2)))
        ms3 = sorted(tp)[len(tp) // 2]
        line += "  | s3 %9.1f us %7.1f TF  x%.2f  ok=%d" % (ms3 * 1e3, 2.0 * m * n * k / ms3 / 1e9, ms / ms3, ok)
        if quad:
            msq = sorted(tq)[1]
            spread = max((max(t) - min(t)) / sorted(t)[1] for t in (tp, tq))
            auto = ops.upconv3x3_s3_form_ok(x, c0, w3, n, 0, batch=b, h1=h1, w1=h1, src1=sk, c1=c1)
            line += "  | s3q %9.1f us %7.1f TF  q/p %.3f  spread %.3f  auto=%d" % (msq * 1e3, 2.0 * m * n * k / msq / 1e9, msq / ms3, spread, auto)
    print(line, flush=True)
