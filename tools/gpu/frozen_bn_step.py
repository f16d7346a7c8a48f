"""B = 64 CVM_VIGOR training step, frozen BatchNorm (models.freeze_batchnorm) against batch statistics on the same box:
    python tools/gpu/frozen_bn_step.py [batch] [steps] [rounds]
The step is bench.py's training leg itself (bench.train_measure: device ground truth, train-mode forward, the losses, backward,
Adam), timed `rounds` times per mode in alternation on ONE model; the medians are what DESIGN section 5b quotes.  A forward
without autograd is timed per mode as well (the frozen forward drops the statistics pass of all 98 BatchNorms)."""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import bench                                                  # noqa: E402
from ccvpe_amd import models, synth                           # noqa: E402

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 64
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 8
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
dev = torch.device("cuda:0")
net = models.CVM_VIGOR("cuda", True)
net.load_state_dict(synth.synthetic_state_dict("vigor", 0), strict=True)
net = net.to(dev).train()
grd, sat = synth.synthetic_pair(batch, "vigor", 1234)
grd, sat = grd.to(dev), sat.to(dev)
torch.manual_seed(1234)


def forward_ms(n=5):
    with torch.no_grad():
        for _ in range(2):
            net(grd, sat)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            net(grd, sat)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


res = {"frozen": [], "batch": []}
fwd = {"frozen": [], "batch": []}
for r in range(rounds):
    for mode in ("batch", "frozen"):
        net.freeze_batchnorm(mode == "frozen")
        m = bench.train_measure(net, grd, sat, dev, batch, steps, 3, 0, 20)
        ms = m["elapsed"] / steps * 1e3
        res[mode].append(ms)
        fwd[mode].append(forward_ms())
        print("round %d %-6s step %.2f ms  no-grad forward %.2f ms  loss %.5g  peak %.1f GiB" % (
            r, mode, ms, fwd[mode][-1], m["loss"], m["peak_gib"]), flush=True)
mb, mf = statistics.median(res["batch"]), statistics.median(res["frozen"])
print("B = %d medians of %d alternating runs: batch-statistic step %.2f ms (%.0f pairs/s), frozen step %.2f ms (%.0f pairs/s), "
      "frozen / batch %.3f; no-grad forward %.2f -> %.2f ms" % (batch, rounds, mb, batch / mb * 1e3, mf, batch / mf * 1e3, mf / mb,
                                                             statistics.median(fwd["batch"]), statistics.median(fwd["frozen"])))
