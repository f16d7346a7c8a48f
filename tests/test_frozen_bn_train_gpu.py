"""Frozen-BatchNorm training mode on the MI355X: net.train() + net.freeze_batchnorm() against the REFERENCE in .train() with
every BatchNorm2d in .eval() (tests/golden/*_frozenbn*.npz, written by tools/make_golden_frozen.py): same synthetic weights,
same pair, same injected drop_connect draws, same deterministic loss (golden_util.train_loss).

Tolerances.  Forward: frozen BatchNorm is the eval arithmetic, so tests/test_forward_gpu.py's eval tolerances apply
(LOGIT_RTOL = 1e-5 of max |logit|, SCORE_ATOL = 2e-5), not the 1e-3 of the batch-statistic test.  Gradients:
golden_util.compare_grads at its default 3e-2 per tensor, and against the float64 gradients the form of
tests/test_train_backward_gpu.py::test_full_backward_vs_reference_autograd (the reference's own fp32 gradients sit a median
of 9.3e-4 and at most 1.43e-2 from the float64 ones, so the reference satisfies both)."""
import numpy as np
import pytest
import torch

import frozen_bn_util as FZ
import golden_util as G
from ccvpe_amd import synth

pytestmark = pytest.mark.gpu

LOGIT_RTOL = 1e-5          # tests/test_forward_gpu.py
SCORE_ATOL = 2e-5


def _net(synth_sd):
    from ccvpe_amd import models
    c = G.TRAIN_CASE
    net = models.CVM_VIGOR("cuda", c["circular"])
    net.load_state_dict(synth_sd(c["kind"], c["wseed"]), strict=True)
    return net.to("cuda:0").train()


def _step(net):
    c = G.TRAIN_CASE
    grd, sat = synth.synthetic_pair(c["batch"], c["grd"], c["pseed"])
    masks, _, _ = G.train_drop_masks(c["batch"])
    for p in net.parameters():
        p.grad = None
    out = net(grd.cuda(), sat.cuda(), drop_masks=masks)
    loss = G.train_loss(out)
    loss.backward()
    torch.cuda.synchronize()
    return out, loss


def _grads(net):
    return {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}


@pytest.fixture(scope="module")
def frozen_step(synth_sd):
    """ONE frozen B = 2 step, shared: (net, outputs, loss, gradients, buffers before the step)."""
    net = _net(synth_sd)
    assert net.bn_frozen is False
    assert net.freeze_batchnorm() is net and net.bn_frozen is True
    assert net.eval().bn_frozen is True and net.train().bn_frozen is True and net.training     # survives the toggles
    before = FZ.buffers_of(net.state_dict())
    out, loss = _step(net)
    return net, [t.detach() for t in out], loss.detach(), _grads(net), before


def test_frozen_forward_vs_reference_and_buffers_untouched(frozen_step):
    net, out, _, _, before = frozen_step
    want = G.load("fwd_vigor_frozenbn")
    got = G.summarize_forward([t.cpu() for t in out])
    scale = abs(want["logits_s4"]).max()
    print("logits max err %.3e of scale; score max err %.3e" % (
        abs(got["logits_s4"] - want["logits_s4"]).max() / scale,
        max(abs(got["score%d" % i] - want["score%d" % i]).max() for i in range(1, 7))))
    assert (got["top4_idx"][:, 0] == want["top4_idx"][:, 0]).all(), "arg-max pixel differs"
    G.assert_close(got["logits_s4"], want["logits_s4"], 0, LOGIT_RTOL * scale, "frozen logits")
    G.assert_close(got["top4_val"], want["top4_val"], 0, LOGIT_RTOL * scale, "frozen top4")
    for i in range(1, 7):
        assert got["score%d" % i].shape == want["score%d" % i].shape
        G.assert_close(got["score%d" % i], want["score%d" % i], 0, SCORE_ATOL, "frozen score%d" % i)
        G.assert_close(got["score%d_mean" % i], want["score%d_mean" % i], 0, SCORE_ATOL, "frozen score mean")
    after = net.state_dict()
    assert len(before) == 3 * 98
    for k, v in before.items():
        assert torch.equal(after[k], v), "%s changed in a frozen step" % k
    assert all(int(after[k]) == 0 for k in before if k.endswith("num_batches_tracked"))


def test_frozen_backward_vs_reference_autograd(frozen_step):
    net, _, _, grads, _ = frozen_step
    want = FZ.load_grads("grad_vigor_frozenbn")
    got = G.summarize_grads([(n, grads.get(n)) for n, _ in net.named_parameters()])
    assert len(got["names"]) == 520
    bad, med = G.compare_grads(got, want)
    assert not bad, "%d/%d parameter gradients off: %s" % (len(bad), len(want["names"]), bad[:12])
    truth = FZ.load_grads("grad_vigor_frozenbn_f64")
    e_ref, e_got = G.grad_rel_errors(want, truth), G.grad_rel_errors(got, truth)
    m_ref, m_got = float(np.median(list(e_ref.values()))), float(np.median(list(e_got.values())))
    worst = sorted(((e_got[n] / max(e_ref[n], 1e-3), n, e_got[n], e_ref[n]) for n in e_got), reverse=True)[:5]
    print("median rel err vs f64: reference %.3e, hip %.3e (max %.3e); vs reference %.3e; worst ratios %s" % (
        m_ref, m_got, max(e_got.values()), med, worst))
    assert m_got <= 3.0 * m_ref + 1e-3, (m_got, m_ref)
    assert all(e_got[n] <= max(3e-2, 4.0 * e_ref[n]) for n in e_got), worst
    # BatchNorm weight and bias still train
    assert float(grads["sat_efficientnet._blocks.5._bn1.weight"].abs().max()) > 0.0
    assert float(grads["grd_efficientnet._bn0.bias"].abs().max()) > 0.0


def test_two_frozen_steps_are_bit_identical(frozen_step, synth_sd):
    _, _, loss1, grads1, _ = frozen_step
    net2 = _net(synth_sd).freeze_batchnorm()
    _, loss2 = _step(net2)
    assert float(loss1) == float(loss2.detach())
    grads2 = _grads(net2)
    assert set(grads1) == set(grads2)
    for n in grads1:
        assert torch.equal(grads1[n], grads2[n]), n


def test_unfreezing_restores_the_batch_statistic_step(synth_sd):
    net = _net(synth_sd).freeze_batchnorm(True).freeze_batchnorm(False)
    assert net.bn_frozen is False
    before = FZ.buffers_of(net.state_dict())
    _step(net)
    after = net.state_dict()
    for k, v in before.items():
        if k.endswith("num_batches_tracked"):
            assert int(after[k]) == 1, k
        else:
            assert not torch.equal(after[k], v), "%s did not move in a batch-statistic step" % k
    got = G.summarize_grads([(n, p.grad) for n, p in net.named_parameters()])
    bad, _ = G.compare_grads(got, G.load("grad_vigor_trainmode"))
    assert not bad, "%d parameter gradients off: %s" % (len(bad), bad[:12])


def test_frozen_train_forward_equals_eval_forward_ori_prior(synth_sd):
    """train() + freeze_batchnorm() + drop_connect_rate = 0 is the eval arithmetic (what the reference's `model.eval()` +
    backward differentiates), through the unfused train-mode kernels: CVM_VIGOR_ori_prior(36), B = 1."""
    from ccvpe_amd import models
    net = models.CVM_VIGOR_ori_prior("cuda", 36, True)
    net.load_state_dict(synth_sd("vigor", 0), strict=True)
    net = net.to("cuda:0").train().freeze_batchnorm()
    net.drop_connect_rate = 0.0
    grd, sat = synth.synthetic_pair(1, "vigor", 4711)
    grd, sat = grd.cuda(), sat.cuda()
    out_t = net(grd, sat)
    assert out_t[0].requires_grad
    out_t = [t.detach() for t in out_t]
    out_e = net.eval()(grd, sat)
    torch.cuda.synchronize()
    assert len(out_t) == len(out_e) == 9
    assert [tuple(t.shape) for t in out_t] == [tuple(t.shape) for t in out_e]
    assert not out_e[0].requires_grad                       # eval() stays the graph-less inference path
    scale = float(out_e[0].abs().max())
    err = float((out_t[0] - out_e[0]).abs().max())
    print("logits: max err %.3e of scale" % (err / scale))
    assert err <= LOGIT_RTOL * scale, (err, scale)
    assert torch.equal(out_t[0].argmax(1), out_e[0].argmax(1))
    for a, b in zip(out_t[3:], out_e[3:]):
        assert float((a - b).abs().max()) <= SCORE_ATOL


def test_graphed_frozen_train_step_matches_eager(synth_sd):
    """GraphedTrainStep over a frozen B = 1 step: tests/test_graph_train_gpu.py's criterion (loss within 1e-5 relative, every
    gradient within 1e-4 of its scale, the same set of tensors), and no buffer moves in three replays."""
    from ccvpe_amd import graph, models, targets
    batch = 1
    net = models.CVM_VIGOR("cuda", True)
    net.load_state_dict(synth_sd("vigor", 0), strict=True)
    net = net.to("cuda:0").train().freeze_batchnorm()
    grd, sat = synth.synthetic_pair(batch, "vigor", 321)
    grd, sat = grd.cuda(), sat.cuda()
    u = synth.uniform((batch, 3), 17)
    center = ((u[:, :2] - 0.5) * 300.0).cuda()
    angle = (u[:, 2] * 359.0).cuda()
    before = FZ.buffers_of(net.state_dict())

    def loss_fn():                                    # the training scripts' loss, as in tests/test_graph_train_gpu.py
        from ccvpe_amd import losses
        gt, gt_flat, gt_ori, labels = targets.train_targets(center, angle, 20)
        out = net(grd, sat)
        nce = 0.0
        for lvl in range(6):
            nce = nce + losses.infoNCELoss(torch.flatten(out[3 + lvl], start_dim=1), torch.flatten(labels[lvl], start_dim=1))
        return losses.cross_entropy_loss(out[0], gt_flat) + 1e4 * nce / 6 + 1e1 * losses.orientation_loss(out[2], gt_ori, gt)
    torch.manual_seed(5)
    le = loss_fn()
    le.backward()
    le = le.detach()
    want = _grads(net)
    step = graph.GraphedTrainStep(loss_fn, net)
    step()
    step()
    torch.manual_seed(5)                              # the same drop_connect draws as the eager step
    lg = step()
    torch.cuda.synchronize()
    assert torch.isfinite(lg).all()
    assert abs(float(lg) - float(le)) <= 1e-5 * abs(float(le)), (float(lg), float(le))
    got = {n: p.grad for n, p in net.named_parameters() if p.grad is not None}
    assert set(got) == set(want)
    worst = 0.0
    for n in want:
        scale = float(want[n].abs().max()) + 1e-30
        worst = max(worst, float((got[n] - want[n]).abs().max()) / scale)
    assert worst <= 1e-4, worst
    after = net.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), "%s changed under the frozen graph" % k
