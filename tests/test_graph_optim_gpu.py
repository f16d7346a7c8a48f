"""GraphedTrainStep with the optimizer inside (ccvpe_amd/graph.py + the device path of ccvpe_amd/optim.py): three graphed
iterations - forward, losses, backward, gradient norm, clip, AdamW, all replayed - against three eager iterations of a twin
net (eager forward / backward, torch's clip_grad_norm_, the same device AdamW uncaptured).  The set-up is that of
test_graph_train_gpu.py: CVM_VIGOR, B = 2, and drop_connect_rate = 0 so that the random draws do not enter."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS, LR, WD = 3, 1e-4, 1e-2
# Worst relative loss difference, graphed vs eager, over the three steps of THIS comparison, measured on an MI355X: 0.0 - every
# loss, and every parameter after step 3, came out bit-identical (the graph replays the very kernels the eager step launches,
# all of them with a fixed summation order, and the device clip coefficient rounded as torch's clip_grad_norm_'s did).  The test
# holds the comparison to 4 x the measured value, never more than the 5e-3 test_train_trajectory_gpu.py allows: 4 x 0 = equality.
LOSS_REL_MEASURED = 0.0
LOSS_REL_BOUND = 4 * LOSS_REL_MEASURED
assert LOSS_REL_BOUND <= 5e-3


def _setup(synth_sd, batch):
    from ccvpe_amd import models, synth, targets
    net = models.CVM_VIGOR("cuda", True)
    net.load_state_dict(synth_sd("vigor", 0), strict=True)
    net = net.to("cuda:0").train()
    net.drop_connect_rate = 0.0
    grd, sat = synth.synthetic_pair(batch, "vigor", 321)
    grd, sat = grd.cuda(), sat.cuda()
    u = synth.uniform((batch, 3), 17)
    center = ((u[:, :2] - 0.5) * 300.0).cuda()
    angle = (u[:, 2] * 359.0).cuda()

    def loss_fn():
        from ccvpe_amd import losses
        gt, gt_flat, gt_ori, labels = targets.train_targets(center, angle, 20)
        out = net(grd, sat)
        nce = 0.0
        for lvl in range(6):
            nce = nce + losses.infoNCELoss(torch.flatten(out[3 + lvl], start_dim=1), torch.flatten(labels[lvl], start_dim=1))
        return losses.cross_entropy_loss(out[0], gt_flat) + 1e4 * nce / 6 + 1e1 * losses.orientation_loss(out[2], gt_ori, gt)
    return net, loss_fn, (grd, sat)


def _norm64(net):
    return math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in net.parameters() if p.grad is not None))


@pytest.fixture(scope="module")
def runs(synth_sd):
    """Both trajectories, run ONCE; the tests below only read what they left."""
    from ccvpe_amd import graph, optim
    r = dict(eager_loss=[], eager_norm=[], loss=[], norm=[], norm64=[])
    net_e, loss_e, _ = _setup(synth_sd, 2)
    opt_e = optim.AdamW(net_e.parameters(), lr=LR, weight_decay=WD, capturable=True)
    sch_e = torch.optim.lr_scheduler.StepLR(opt_e, step_size=1, gamma=0.5)
    max_norm = None
    for it in range(STEPS):
        opt_e.zero_grad(set_to_none=True)
        loss = loss_e()
        loss.backward()
        if max_norm is None:
            max_norm = _norm64(net_e) / 2                  # the first step's norm is twice the limit: the clip is active
        r["eager_norm"].append(float(torch.nn.utils.clip_grad_norm_(net_e.parameters(), max_norm)))
        opt_e.step()
        sch_e.step()
        r["eager_loss"].append(float(loss.detach()))
    net_g, loss_g, inputs = _setup(synth_sd, 2)
    opt_g = optim.AdamW(net_g.parameters(), lr=LR, weight_decay=WD, capturable=True, max_grad_norm=max_norm)
    sch_g = torch.optim.lr_scheduler.StepLR(opt_g, step_size=1, gamma=0.5)
    before = [p.detach().clone() for p in net_g.parameters()]
    step = graph.GraphedTrainStep(loss_g, net_g, optimizer=opt_g)
    torch.cuda.synchronize()
    r["built_params_same"] = all(torch.equal(a.view(torch.int32), p.detach().view(torch.int32)) for a, p in zip(before, net_g.parameters()))
    r["built_moments"] = max(max(float(st["exp_avg"].abs().max()), float(st["exp_avg_sq"].abs().max())) for st in opt_g.state.values())
    r["built_states"] = len(opt_g.state)
    r["built_steps"] = float(opt_g._steps.abs().max())
    for it in range(STEPS):
        loss = step()
        r["loss"].append(float(loss))
        r["norm"].append(float(opt_g.last_grad_norm))
        r["norm64"].append(_norm64(net_g))                 # the static gradients this replay wrote: what the norm pass read
        sch_g.step()
    torch.cuda.synchronize()
    r.update(net_e=net_e, net_g=net_g, opt_g=opt_g, max_norm=max_norm, inputs=inputs, loss_fn=loss_g, step=step,
             lr=(opt_e.param_groups[0]["lr"], opt_g.param_groups[0]["lr"]))
    return r


def test_graphed_iterations_match_eager(runs, synth_sd):
    init = synth_sd("vigor", 0)
    assert runs["lr"][0] == runs["lr"][1] == LR * 0.5 ** STEPS           # the scheduler drove both
    worst = 0.0
    for (name, a), b in zip(runs["net_e"].named_parameters(), runs["net_g"].parameters()):
        d = (a.detach() - b.detach()).abs().max().item()
        moved = (a.detach().cpu() - init[name]).abs().max().item()
        worst = max(worst, d / (2e-3 * moved + 1e-9))
        assert d <= 2e-3 * moved + 1e-9, (name, d, moved)
    for got, want in zip(runs["norm"], runs["norm64"]):
        assert abs(got - want) <= 1e-5 * want, (got, want)
    assert runs["norm64"][0] > 1.5 * runs["max_norm"]                    # clipped, as intended
    rel = max(abs(g - e) / abs(e) for g, e in zip(runs["loss"], runs["eager_loss"]))
    print("graphed vs eager: worst relative loss difference %.3g (bound %.3g), worst parameter d / bound %.3g, losses %s"
          % (rel, LOSS_REL_BOUND, worst, runs["loss"]))
    assert all(math.isfinite(x) for x in runs["loss"]) and len(set(runs["loss"])) == STEPS
    assert rel <= LOSS_REL_BOUND, (rel, runs["loss"], runs["eager_loss"])


def test_construction_changes_nothing_and_replays_count(runs):
    assert runs["built_params_same"]
    assert runs["built_states"] > 100 and runs["built_moments"] == 0.0 and runs["built_steps"] == 0.0
    opt = runs["opt_g"]
    counts = [float(st["step"]) for st in opt.state.values()]
    assert counts and all(c == float(STEPS) for c in counts)
    assert float(opt.skipped_steps) == 0.0


def test_packed_weights_follow_the_in_graph_update(runs, synth_sd):
    """eval() + forward after the graphed steps == a forward of a net freshly loaded from the same state_dict."""
    from ccvpe_amd import models
    net = runs["net_g"]
    grd, sat = runs["inputs"]
    net.eval()
    try:
        with torch.no_grad():
            got = [t.clone() for t in net(grd, sat)]
        fresh = models.CVM_VIGOR("cuda", True)
        fresh.load_state_dict(net.state_dict(), strict=True)
        fresh = fresh.to("cuda:0").eval()
        with torch.no_grad():
            want = fresh(grd, sat)
        torch.cuda.synchronize()
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    finally:
        net.train()


def test_host_path_optimizer_is_refused(runs):
    from ccvpe_amd import graph, optim
    with pytest.raises(ValueError, match="capturable=True"):
        graph.GraphedTrainStep(runs["loss_fn"], runs["net_g"], optimizer=optim.Adam(runs["net_g"].parameters(), lr=LR))
