"""The loss kernels (csrc/heads.hip, csrc/heads_bwd.hip) through ccvpe_amd.losses and ccvpe_amd.ops against float64, every
gradient element and every per-row statistic under the error models of tests/loss_check.py, at the smallest shapes that reach
each reduction path (the `reaches` column of loss_check's case tables), and eval_postprocess at the edges of its arg-max scan.

Every case runs forward and backward twice and asserts bit-identical results.  One line per case with the measured
got / tolerance ratios and the float32 oracle's own ratio r32 is printed (kept in profiles/r13/loss_checks.txt).
"""
import os

import pytest
import torch
import torch.nn.functional as F

import loss_check as L
from ccvpe_amd import synth
from oracle import ccvpe_oracle as O

pytestmark = pytest.mark.gpu
TABLE = os.environ.get("CCVPE_LOSS_TABLE")   # optional: append the per-case lines to this file


def _report(ref, ratios):
    line = L.describe(ref, ratios) + "   [" + ref.case.reaches + "]"
    print(line)
    if TABLE:
        with open(TABLE, "a") as f:
            f.write(line + "\n")


def _same_bits(a, b):
    """bit-identical (torch.equal would call two NaNs different)"""
    return a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.int32), b.contiguous().reshape(-1).view(torch.int32))


def _twice(run):
    first, second = run(), run()
    for nm, a, b in zip(("loss", "grad", "rows"), first, second):
        if a is not None:
            assert _same_bits(a, b), "%s differs between two runs of the same inputs" % nm
    return first


def _infonce(s, lab, t, g):
    from ccvpe_amd import losses, ops
    b = s.shape[0]

    def run():
        sd, ld = s.cuda().requires_grad_(True), lab.cuda()
        lo = losses.infoNCELoss(sd, ld, t)
        (g * lo).backward()
        value, rows = ops.infonce_loss(sd.detach(), ld, t, want_rows=True)
        assert _same_bits(value, lo.detach()), "ops.infonce_loss and losses.infoNCELoss disagree"
        return lo.detach().cpu(), sd.grad.cpu(), rows[:4 * b + 1].cpu()
    return _twice(run)


@pytest.mark.parametrize("case", L.INFONCE_CASES, ids=[c.name for c in L.INFONCE_CASES])
def test_infonce_vs_float64(case):
    if case.real:
        from ccvpe_amd import targets
        labels = targets.train_targets(torch.tensor(L.REAL_CENTERS).cuda(), torch.tensor(L.REAL_ANGLES).cuda(), 20)[3][2]
        assert tuple(labels.shape) == (5, 20, 32, 32)
        ref = L.InfoNCERef(case, *L.infonce_inputs(case, labels=labels.cpu()))
        share = float((ref.lab > 1e-2).double().mean())
        assert 0 < share < 0.02, "level-3 labels are expected to be sparse (%.4f above 1e-2)" % share
    else:
        ref = L.cached_ref(case.name)
    assert ref.r32_grad <= L.R32_CAP and ref.r32_val <= L.R32_CAP
    for b in case.no_pos:
        assert float(ref.den[b]) == 0.0
    loss, grad, rows = _infonce(ref.s, ref.lab, case.t, case.g)
    pad = torch.zeros(4 * case.b + 4)
    pad[:4 * case.b + 1] = rows
    _report(ref, L.check(ref, loss=loss, grad=grad, rows=pad))
    for b in case.no_pos:                                  # den_b = 0: the row's gradient is exactly zero
        assert float(grad[b].abs().max()) == 0.0


def test_infonce_zero_upstream_gradient_gives_exact_zeros():
    ref = L.cached_ref("nce_b6_n16388")
    loss, grad, rows = _infonce(ref.s, ref.lab, ref.t, 0.0)
    assert float(grad.abs().max()) == 0.0 and bool(torch.isfinite(loss))


def test_infonce_without_any_positive_is_nonfinite_like_the_reference():
    """D = 0: the loss is -0 / 0 in the reference and in the kernel.  The gradient g / (D T) (den_b p_j - 0) is inf * 0 and the
    kernel writes NaN into every element, so a batch without positives cannot go unnoticed.  (Autograd through the oracle's
    torch.where, like the original's masked_select of nothing, hands back zeros beside its NaN loss: the selection's backward
    fills in 0 instead of multiplying by the infinite upstream factor.  Only the reference's value is therefore asserted.)"""
    ref = L.cached_ref("nce_b6_n16388")
    lab = ref.lab * 1e-3
    assert not bool((lab > 1e-2).any())
    assert not bool(torch.isfinite(O.infonce_loss(ref.s.double(), lab.double(), ref.t)))
    loss, grad, rows = _infonce(ref.s, lab, ref.t, ref.g)
    assert not bool(torch.isfinite(loss)) and not bool(torch.isfinite(grad).any())
    assert float(rows[4 * ref.case.b]) == 0.0


@pytest.mark.parametrize("case", L.CE_CASES, ids=[c.name for c in L.CE_CASES])
def test_cross_entropy_vs_float64(case):
    from ccvpe_amd import losses, ops
    ref = L.cached_ref(case.name)
    assert ref.r32_grad <= L.R32_CAP and ref.r32_val <= L.R32_CAP
    if case.peak_last:
        assert bool((ref.lg.argmax(1) == case.n - 1).all())
    if not case.normalised:
        assert float(ref.ls.min()) < 0.31 and float(ref.ls.max()) > 2.9

    def run():
        lgd, ld = ref.lg.cuda().requires_grad_(True), ref.lab.cuda()
        lo = losses.cross_entropy_loss(lgd, ld)
        lo.backward()
        assert torch.equal(ops.cross_entropy_loss(lgd.detach(), ld), lo.detach())
        return lo.detach().cpu(), lgd.grad.cpu(), None
    loss, grad, _ = _twice(run)
    _report(ref, L.check(ref, loss=loss, grad=grad))


@pytest.mark.parametrize("case", L.ORI_CASES, ids=[c.name for c in L.ORI_CASES])
def test_orientation_vs_float64(case):
    from ccvpe_amd import losses, ops
    ref = L.cached_ref(case.name)
    assert ref.r32_grad <= L.R32_CAP and ref.r32_val <= L.R32_CAP

    def run():
        od, gto, gt = ref.ori.cuda().requires_grad_(True), ref.gto.cuda(), ref.gt.cuda()
        lo = losses.orientation_loss(od, gto, gt)
        lo.backward()
        assert torch.equal(ops.orientation_loss(od.detach(), gto, gt), lo.detach())
        return lo.detach().cpu(), od.grad.cpu(), None
    loss, grad, _ = _twice(run)
    _report(ref, L.check(ref, loss=loss, grad=grad))


def test_eval_postprocess_scan_edges():
    """B = 5 on 512 x 512 maps: the maximum at index n - 1; at index 0; a tie between an element of thread 1023's (index 1023) and
    one of thread 0's in a later stride (index 2048); the same with thread 0's element first (3072 against 1023 + 5 * 1024); a tie of
    two elements of one thread (7 and 7 + 1024 * 200).  The smaller index wins, as numpy.argmax decides in O.eval_postprocess."""
    from ccvpe_amd import ops
    b, n = 5, 512 * 512
    heat = torch.softmax(synth.normal((b, n), 97, 3.0), dim=1)
    top = float(heat.max())
    first = [n - 1, 0, 1023, 3072, 7]
    for i, idx in enumerate([(n - 1,), (0,), (1023, 2048), (3072, 1023 + 5 * 1024), (7, 7 + 1024 * 200)]):
        heat[i, list(idx)] = top + 0.125
    heat = heat.reshape(b, 1, 512, 512)
    ori = F.normalize(synth.normal((b, 2, 512, 512), 98), dim=1)
    want = O.eval_postprocess(heat, ori)
    assert [int(y) * 512 + int(x) for y, x in want[:, :2]] == first
    got = ops.eval_postprocess(heat.cuda(), ori.cuda()).cpu()
    assert torch.equal(got, ops.eval_postprocess(heat.cuda(), ori.cuda()).cpu())
    assert torch.equal(got[:, :2], want[:, :2]), (got[:, :2], want[:, :2])
    assert torch.equal(got[:, 2:4], want[:, 2:4]) and torch.equal(got[:, 5], want[:, 5])        # values read, not computed
    assert float((got[:, 4] - want[:, 4]).abs().max()) < 1e-2                                   # degrees: acosf against float64 acos
