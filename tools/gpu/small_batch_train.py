"""Small-batch training step, three ways: eager; GraphedTrainStep (forward + losses + backward in one hipGraph) followed by the
eager host-path Adam; GraphedTrainStep with the capturable device-side Adam inside (the whole iteration replayed):
    python tools/gpu/small_batch_train.py [batch ...]
CCVPE_SBT_OPT=1 additionally times the optimizer alone on the full parameter set: the one host-path launch against the
device path's two launches and its three with the global-norm pass."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from ccvpe_amd import graph, losses, models, optim, synth, targets      # noqa: E402


def build(batch):
    net = models.CVM_VIGOR("cuda", True)
    net.load_state_dict(synth.synthetic_state_dict("vigor", 0), strict=True)
    net = net.to("cuda:0").train()
    grd, sat = synth.synthetic_pair(batch, "vigor", 321)
    grd, sat = grd.cuda(), sat.cuda()
    u = synth.uniform((batch, 3), 17)
    center, angle = ((u[:, :2] - 0.5) * 300.0).cuda(), (u[:, 2] * 359.0).cuda()

    def loss_fn():
        gt, gt_flat, gt_ori, labels = targets.train_targets(center, angle, 20)
        out = net(grd, sat)
        nce = 0.0
        for lvl in range(6):
            nce = nce + losses.infoNCELoss(torch.flatten(out[3 + lvl], start_dim=1), torch.flatten(labels[lvl], start_dim=1))
        return losses.cross_entropy_loss(out[0], gt_flat) + 1e4 * nce / 6 + 1e1 * losses.orientation_loss(out[2], gt_ori, gt)
    return net, loss_fn


def timed(fn, steps=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


for batch in [int(a) for a in sys.argv[1:]] or [8]:
    net, loss_fn = build(batch)
    opt = optim.Adam(net.parameters(), lr=1e-4)

    def eager():
        opt.zero_grad(set_to_none=True)
        loss_fn().backward()
        opt.step()
    ms_e = timed(eager)
    del net, opt
    torch.cuda.empty_cache()
    net, loss_fn = build(batch)
    opt = optim.Adam(net.parameters(), lr=1e-4)
    step = graph.GraphedTrainStep(loss_fn, net)

    def graphed():
        step()
        opt.step()
    ms_g = timed(graphed)
    del net, opt, step
    torch.cuda.empty_cache()
    net, loss_fn = build(batch)
    opt = optim.Adam(net.parameters(), lr=1e-4, capturable=True)
    step = graph.GraphedTrainStep(loss_fn, net, optimizer=opt)
    ms_o = timed(step)
    print("B = %d: eager %.2f ms/step (%.0f pairs/s), graphed + host Adam %.2f ms/step (%.0f pairs/s), "
          "graphed with Adam inside %.2f ms/step (%.0f pairs/s), loss %.4g" %
          (batch, ms_e, batch / ms_e * 1e3, ms_g, batch / ms_g * 1e3, ms_o, batch / ms_o * 1e3, float(step.loss)))
    if os.environ.get("CCVPE_SBT_OPT") == "1":           # the optimizer alone, on the gradients the last replay left
        host = optim.Adam(net.parameters(), lr=1e-4)
        dev3 = optim.Adam(net.parameters(), lr=1e-4, max_grad_norm=1e30)
        print("    optimizer alone, %d tensors: host path (1 launch) %.3f ms, device path (2 launches) %.3f ms, "
              "with the norm pass (3 launches) %.3f ms" % (len(step.params), timed(host.step, 50), timed(opt.step, 50), timed(dev3.step, 50)))
        del host, dev3
    del net, opt, step
    torch.cuda.empty_cache()
