"""Frozen-BatchNorm backward (ccvpe_bn_act_bwd_frozen_f32 through backward.bn_act_bwd_frozen) against float64 torch autograd
on the CPU.  mean / var are CONSTANTS of the graph and deliberately not the batch statistics (offset mean, variance uniform
in 0.5 .. 1.5): the batch-statistic kernels, whose dx carries the statistics-correction terms, fail this comparison.
The loss is built as tests/test_backward_gpu.py::test_bn_act_bwd_vs_autograd builds it (gate, pooled-mean branch, dc_scale);
tolerance: that file's close() at 2e-4 of each output's scale.

Shapes [B, rows, C], the smallest that reach each branch of the row / channel tiling (256 threads = channel groups of 4 x
row lanes; 8 rows per workgroup at these sizes unless rows / 32 is larger):
  (2, 1, 16)     4 channel groups, 64 row lanes of which one has a row
  (2, 9, 144)    36 channel groups -> 7 row lanes and 4 idle threads; two workgroups per sample, the second with one row
  (3, 73, 1280)  320 channel groups -> two trips of the channel loop, the second partial; one row lane, so the two-row loop
                 and the odd tail both run; ragged last workgroup
  (2, 600, 24)   no activation + dc_scale with one entry exactly 0 (the _bn2 + drop_connect form); 34 workgroups per sample
  (2, 35, 16)    ReLU
"""
import pytest
import torch

from ccvpe_amd import synth

pytestmark = pytest.mark.gpu

ACT_NONE, ACT_RELU, ACT_SWISH = 0, 1, 2


@pytest.fixture(scope="module")
def bw():
    from ccvpe_amd import backward, _lib
    _lib.load()
    return backward


def close(got, want, tol, what):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = want.abs().max().item() + 1e-30
    err = (got - want).abs().max().item()
    print("%s: max err %.3e vs scale %.3e" % (what, err, scale))
    assert err <= tol * scale, "%s: max err %.3e vs scale %.3e" % (what, err, scale)


def _act(z, act):
    return z * torch.sigmoid(z) if act == ACT_SWISH else (torch.relu(z) if act == ACT_RELU else z)


def _case(b, rows, c, act, with_se, dcs_kind):
    """float64 autograd with constant statistics -> (device inputs, expected dx / dgamma / dbeta)."""
    eps = 1e-3
    x = (synth.normal((b, rows, c), 1900 + c) * 1.2 + 0.3).double().requires_grad_(True)
    gamma = (1.0 + 0.3 * synth.normal((c,), 1901)).double().requires_grad_(True)
    beta = (0.2 * synth.normal((c,), 1902)).double().requires_grad_(True)
    mean = (0.3 + 0.5 * synth.normal((c,), 1907)).double()               # NOT the batch mean
    var = synth.uniform((c,), 1908, 0.5, 1.5).double()                    # NOT the batch variance (that is ~1.44)
    gate = torch.sigmoid(synth.normal((b, c), 1903)).double() if with_se else None
    if dcs_kind == "zero":                                                # one sample dropped: scale exactly 0
        dcs = torch.tensor([0.0] + [1.0 / 0.7] * (b - 1), dtype=torch.float64)
    elif dcs_kind:
        dcs = (synth.uniform((b,), 1904) > 0.3).double() / 0.7
        dcs[-1] = 1.0 / 0.7
    else:
        dcs = None
    u = _act((x - mean) / torch.sqrt(var + eps) * gamma + beta, act)
    if dcs is not None:
        u = u * dcs.view(b, 1, 1)
    dv = synth.normal((b, rows, c), 1906).double()
    if with_se:
        pooled = u.mean(dim=1)                            # the squeeze branch: the loss also depends on the mean
        wm = synth.normal((b, c), 1905).double()
        loss = (u * gate.view(b, 1, c) * dv).sum() + (pooled * wm).sum()
    else:
        loss = (u * dv).sum()
    loss.backward()
    f = lambda t: None if t is None else t.detach().float().cuda().contiguous()      # noqa: E731
    args = dict(x=f(x), dv=f(dv), mean=f(mean), var=f(var), gamma=f(gamma), beta=f(beta), eps=eps, act=act,
                gate=f(gate), dmean=f(wm / rows) if with_se else None, dc_scale=f(dcs))
    return args, (x.grad, gamma.grad, beta.grad)


CASES = [(2, 1, 16, ACT_SWISH, False, None),
         (2, 9, 144, ACT_SWISH, True, None),
         (3, 73, 1280, ACT_SWISH, False, "random"),
         (2, 600, 24, ACT_NONE, False, "zero"),
         (2, 35, 16, ACT_RELU, False, None)]


@pytest.mark.parametrize("b,rows,c,act,with_se,dcs_kind", CASES)
def test_bn_act_bwd_frozen_vs_autograd(bw, b, rows, c, act, with_se, dcs_kind):
    a, (dx_w, dg_w, db_w) = _case(b, rows, c, act, with_se, dcs_kind)
    dx, dgamma, dbeta = bw.bn_act_bwd_frozen(a["x"], a["dv"], a["mean"], a["var"], a["gamma"], a["beta"], a["eps"], a["act"],
                                             gate=a["gate"], dmean=a["dmean"], dc_scale=a["dc_scale"])
    torch.cuda.synchronize()
    close(dx, dx_w, 2e-4, "frozen bn dx")
    close(dgamma, dg_w, 2e-4, "frozen dgamma")
    close(dbeta, db_w, 2e-4, "frozen dbeta")
    if dcs_kind == "zero":
        assert float(dx[0].abs().max()) == 0.0, "a dropped sample (dc_scale 0) must get an exactly zero gradient"
    # fixed-order merge, no atomics: a second call is bit-identical
    dx2, dgamma2, dbeta2 = bw.bn_act_bwd_frozen(a["x"], a["dv"], a["mean"], a["var"], a["gamma"], a["beta"], a["eps"], a["act"],
                                                gate=a["gate"], dmean=a["dmean"], dc_scale=a["dc_scale"])
    assert torch.equal(dx, dx2) and torch.equal(dgamma, dgamma2) and torch.equal(dbeta, dbeta2)


def test_frozen_entry_point_rejects_what_the_batch_statistic_one_rejects(bw):
    """channels % 4 and 16-byte alignment: CCVPE_EINVAL, nothing launched."""
    from ccvpe_amd import _lib
    x = torch.zeros((2, 8, 24), device="cuda")
    v = torch.ones((28,), device="cuda")
    with pytest.raises(_lib.CcvpeError):
        bw.bn_act_bwd_frozen(x[..., :6].contiguous(), x[..., :6].contiguous(), v[:6], v[:6], v[:6], v[:6], 1e-3, ACT_SWISH)
    with pytest.raises(_lib.CcvpeError):                                  # mean 4 bytes past a 16-byte boundary
        bw.bn_act_bwd_frozen(x, x, v[1:25], v[:24], v[:24], v[:24], 1e-3, ACT_SWISH)
