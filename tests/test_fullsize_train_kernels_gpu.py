"""The training step's size-dependent reduction kernels at B = 64 shapes, against float64 CPU references.

Every other value check of these kernels runs B <= 5 on planes of at most 40 x 48, where rows per workgroup, partial-row
counts, grid-stride trips and LDS budgets take other branches than the benchmarked step.  Each row of
tests/train_kernel_shapes.py asserts the branch it is there for (through the host geometry queries) before it compares values,
and every kernel runs twice and must give the same bits.

Inputs look like a trained network where the kernel's arithmetic depends on it: per-channel means up to 100 sigma, sigma spread
over 1e-3 ... 1e2, upstream gradients with a non-zero mean, heat maps with one dominant peak (h_max 0.5 ... 0.99).

Error model.  The reference is computed in float64 from the same fp32 inputs, so the difference is the kernel's own rounding.
A sum of terms t_i accumulated in fp32 along serial chains of at most L additions (per-thread rows, then the fixed-order lane
and partial-row merges) is off by at most L * eps * sum |t_i| (first order, eps = 2^-23); L is read from the kernel's geometry
(per row, next to each check), sum |t_i| is the same reduction over absolute values in float64.  Elementwise steps add a few eps of their
operands.  BatchNorm adds the conditioning: x - mean cancels |mean| / sigma digits, so the normalised value carries
eps * (|mean| + |x|) / sigma, and merging partial means (Chan's update) carries eps * |mean| / sigma relative to the variance.
Each check asserts max |got - want| / bound <= 1 and, where the small-shape tests use it, also max |got - want| <= 2e-4 of the
output's scale.  The printed `worst err / bound` is the margin; the faults these tests were checked against (a dropped
partial row, half of a workgroup's rows, every second grid-stride tile, half of a softmax row) move the affected outputs by
1e-4 ... 1 of their size, which is tens to thousands of bounds."""
import pytest
import torch
import torch.nn.functional as F

import train_kernel_shapes as S
from ccvpe_amd import synth

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
BN_EPS = 1e-3
SCALE_TOL = 2e-4


@pytest.fixture(scope="module")
def lib():
    from ccvpe_amd import _lib
    return _lib.load()


class Checks:
    """Collects every comparison of a row before asserting, so one run reports all margins."""

    def __init__(self, row):
        self.row, self.fails = row, []

    def __call__(self, what, got, want, bound, scale_tol=SCALE_TOL):
        got, want = got.detach().cpu().double(), want.detach().cpu().double()
        assert got.shape == want.shape, (self.row, what, got.shape, want.shape)
        err = (got - want).abs()
        scale = want.abs().max().item() + 1e-300
        rel = err.max().item() / scale
        worst = torch.where(err == 0, 0.0, err / bound).max().item()
        print("%s | %s: max err / scale %.2e, worst err / bound %.3f" % (self.row, what, rel, worst))
        if not worst <= 1.0:
            self.fails.append("%s: err / bound %.3g" % (what, worst))
        if scale_tol is not None and not rel <= scale_tol:
            self.fails.append("%s: err / scale %.3g > %g" % (what, rel, scale_tol))

    def same(self, what, a, b):
        if not torch.equal(a, b):
            self.fails.append("%s: two runs differ" % what)

    def done(self):
        assert not self.fails, "%s: %s" % (self.row, "; ".join(self.fails))


def trained_channels(c, seed):
    """Per-channel (mean, sigma) in float64: sigma log-spread over 1e-3 ... 1e2, |mean| up to 100 sigma (both extremes present)."""
    sd = 10.0 ** synth.uniform((c,), seed, -3.0, 2.0).double()
    r = synth.uniform((c,), seed + 1, -100.0, 100.0).double()
    sd[0], r[0] = 1e-3, 100.0
    sd[-1], r[-1] = 1e2, -100.0
    if c > 2:
        r[1] = 0.0
    return r * sd, sd


def trained_tensor(shape, seed):
    """[..., C] fp32 on the GPU with trained_channels statistics."""
    mu, sd = trained_channels(shape[-1], seed)
    z = synth.normal(shape, seed + 2, device="cuda")
    return (z * sd.float().cuda() + mu.float().cuda()).contiguous()


def grad_like(shape, seed, offset=0.3):
    """Upstream gradient: unit spread with a non-zero per-channel mean (fp32 on the GPU)."""
    off = synth.normal((shape[-1],), seed + 7, offset).cuda() + offset
    return (synth.normal(shape, seed, device="cuda") + off).contiguous()


def swish(z):
    return z * torch.sigmoid(z)


def dswish(z):
    s = torch.sigmoid(z)
    return s * (1.0 + z * (1.0 - s))


# ---- BatchNorm statistics + running update ------------------------------------------------------------------------

@pytest.mark.parametrize("row", S.BN_STATS, ids=[r[0] for r in S.BN_STATS])
def test_bn_stats_at_training_shapes(lib, row):
    from ccvpe_amd import ops
    name, rows, c, rpb, nblk = row
    assert lib.ccvpe_bn_stats_nblk(rows) == nblk, "%s: geometry changed" % name
    chk = Checks(name)
    x = trained_tensor((rows, c), 3000 + c)
    mu, sd = trained_channels(c, 3000 + c)
    rm0, rv0 = 0.9 * mu, 1.3 * sd * sd
    drm, drv = rm0.float().cuda(), rv0.float().cuda()
    mean, var = ops.bn_stats(x, drm, drv, 0.01)
    mean2, var2 = ops.bn_stats(x)
    chk.same("mean", mean, mean2)
    chk.same("var", var, var2)
    xr = x.cpu().double()
    del x
    m = xr.mean(0)
    dev = (xr - m).abs_().amax(0)                       # bounds |x - pivot| / 2 (the pivot is one of the values)
    v = xr.var(0, unbiased=False)
    del xr
    R = 256 // min(c // 4, 256)
    L = rpb // R + R + 2 * (4 + 16) + 8                 # rows per thread, row slices, two fold levels (4 rows + 16 lanes each)
    bm = EPS * (L * 2 * dev + 4 * m.abs())
    bv = EPS * (L * (v + 4 * dev * dev) + 16 * (m.abs() / v.sqrt()) * v)
    chk("mean", mean, m, bm)
    chk("biased var", var, v, bv)
    chk("running mean", drm, 0.99 * rm0 + 0.01 * m, 4 * EPS * (rm0.abs() + m.abs()) + 0.01 * bm)
    chk("running var", drv, 0.99 * rv0 + 0.01 * v * rows / (rows - 1), 4 * EPS * (rv0 + v) + 0.0101 * bv)
    chk.done()


# ---- BatchNorm apply (+ SE squeeze partials) and its backward --------------------------------------------------------

def _bn_inputs(b, rps, c, seed, with_extra):
    x = trained_tensor((b, rps, c), seed)
    xr = x.cpu().double()
    m64, v64 = xr.mean(dim=(0, 1)), xr.var(dim=(0, 1), unbiased=False)
    gamma = synth.uniform((c,), seed + 11, 0.5, 1.5) * torch.where(synth.uniform((c,), seed + 12) > 0.2, 1.0, -1.0)
    beta = synth.normal((c,), seed + 13, 0.5)
    dcs = res = None
    if with_extra:
        keep = synth.uniform((b,), seed + 14) > 0.25
        keep[0] = True                                  # at least one sample kept (drop_connect masks: 0 or 1 / keep_prob)
        dcs = keep.float() / 0.8
        res = synth.normal((b, rps, c), seed + 15, device="cuda")
    return x, xr, m64, v64, gamma, beta, dcs, res


@pytest.mark.parametrize("row", S.BN_ACT, ids=[r[0] for r in S.BN_ACT])
def test_bn_act_at_training_shapes(lib, row):
    from ccvpe_amd import ops
    name, b, rps, c, act, extra, nblk = row
    assert lib.ccvpe_bn_act_nblk(rps) == nblk, "%s: geometry changed" % name
    chk = Checks(name)
    x, xr, m64, v64, gamma, beta, dcs, res = _bn_inputs(b, rps, c, 3100 + c, extra)
    m32, v32 = m64.float(), v64.float()
    args = (x, m32.cuda(), v32.cuda(), gamma.cuda(), beta.cuda(), BN_EPS, act)
    kw = dict(residual=res, dc_scale=dcs.cuda() if extra else None, want_se=True)
    y, part = ops.bn_act(*args, **kw)
    y2, part2 = ops.bn_act(*args, **kw)
    chk.same("y", y, y2)
    chk.same("SE partials", part, part2)
    m, v, g, be = m32.double(), v32.double(), gamma.double(), beta.double()
    istd = 1.0 / torch.sqrt(v + BN_EPS)
    z = (xr - m) * istd * g + be
    want = swish(z) if act == 2 else z
    # z = x * sc + sh with sc = gamma / sqrt(var + eps), sh = beta - mean * sc: eps * (|x| + |mean|) * |sc| (the |mean| / sigma
    # cancellation), then the activation (|swish'| <= 1.1) and the output rounding
    dz = 8 * EPS * ((xr.abs() + m.abs()) * (g * istd).abs() + be.abs() + z.abs())
    bound = 1.1 * dz + 4 * EPS * want.abs()
    if extra:
        d = dcs.double().view(b, 1, 1)
        r = res.cpu().double()
        want = want * d + r
        bound = bound * d + 4 * EPS * want.abs() + 4 * EPS * r.abs()
    del z, dz
    chk("y", y, want, bound)
    rpb = max(rps // 32, 8)
    blk = torch.arange(rps) // rpb
    wpart = torch.zeros((b, nblk, c), dtype=torch.float64).index_add_(1, blk, want)
    apart = torch.zeros((b, nblk, c), dtype=torch.float64).index_add_(1, blk, want.abs())
    bpart = torch.zeros((b, nblk, c), dtype=torch.float64).index_add_(1, blk, bound)
    P = 256 // min(c // 4, 256)
    chk("SE partials", part, wpart, bpart + EPS * (rpb // P + P + 4) * apart)
    chk.done()


@pytest.mark.parametrize("row", S.BN_ACT, ids=[r[0] for r in S.BN_ACT])
def test_bn_act_bwd_at_training_shapes(lib, row):
    from ccvpe_amd import backward as bw
    name, b, rps, c, act, extra, nblk = row
    assert lib.ccvpe_bn_bwd_nblk(rps) == nblk, "%s: geometry changed" % name
    chk = Checks(name)
    x, xr, m64, v64, gamma, beta, dcs, _ = _bn_inputs(b, rps, c, 3200 + c, extra)
    dv = grad_like((b, rps, c), 3250 + c)
    m32, v32 = m64.float(), v64.float()
    args = (x, dv, m32.cuda(), v32.cuda(), gamma.cuda(), beta.cuda(), BN_EPS, act)
    kw = dict(dc_scale=dcs.cuda() if extra else None)
    dx, dgamma, dbeta = bw.bn_act_bwd(*args, **kw)
    dx2, dgamma2, dbeta2 = bw.bn_act_bwd(*args, **kw)
    chk.same("dx", dx, dx2)
    chk.same("dgamma", dgamma, dgamma2)
    chk.same("dbeta", dbeta, dbeta2)
    # float64 autograd through the batch statistics (train-mode BatchNorm), from the same fp32 values
    xa = xr.clone().requires_grad_(True)
    ga, ba = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    mean = xa.mean(dim=(0, 1))
    var = xa.var(dim=(0, 1), unbiased=False)
    z = (xa - mean) / torch.sqrt(var + BN_EPS) * ga + ba
    u = swish(z) if act == 2 else z
    if extra:
        u = u * dcs.double().view(b, 1, 1)
    dvr = dv.cpu().double()
    (u * dvr).sum().backward()
    del u, z, mean, var
    # error model, per element: z carries eps * (|x| + |mean|) / sigma (the cancellation), g = dv * dcs * act'(z) the act''
    # (<= 0.5 for swish) of it; dbeta / dgamma are chains of L adds; dx = gamma * istd * (g - dbeta / M - xhat * dgamma / M)
    m, v, g_, be = m32.double(), v32.double(), gamma.double(), beta.double()
    istd = 1.0 / torch.sqrt(v + BN_EPS)
    xh = (xr - m) * istd
    z = xh * g_ + be
    dxh = 8 * EPS * (xr.abs() + m.abs()) * istd
    dz = dxh * g_.abs() + 8 * EPS * (be.abs() + z.abs())
    du = dvr.abs() * (dcs.double().view(b, 1, 1) if extra else 1.0)
    ap = dswish(z) if act == 2 else torch.ones_like(z)
    gg = du * ap.abs()
    dg = du * (0.5 * dz if act == 2 else 0.0) + 4 * EPS * gg
    del z, ap
    P = 256 // min(c // 4, 256)
    L = (max(rps // 32, 8) + P - 1) // P + P + S.sum_parts_chain(nblk * b, 2 * c) + 8
    bb = dg.sum(dim=(0, 1)) + EPS * L * gg.sum(dim=(0, 1))
    bgm = (dg * xh.abs() + gg * dxh).sum(dim=(0, 1)) + EPS * L * (gg * xh.abs()).sum(dim=(0, 1))
    M = b * rps
    k = (g_ * istd).abs()
    bdx = k * (dg + 4 * EPS * gg + (bb + 4 * EPS * ba.grad.abs()) / M + dxh * ga.grad.abs() / M +
               xh.abs() * (bgm + 4 * EPS * ga.grad.abs()) / M) + 4 * EPS * xa.grad.abs()
    del gg, dg, dxh, xh
    chk("dbeta", dbeta, ba.grad, bb)
    chk("dgamma", dgamma, ga.grad, bgm)
    chk("dx", dx, xa.grad, bdx)
    chk.done()


@pytest.mark.parametrize("row", S.BN_SE, ids=[r[0] for r in S.BN_SE])
def test_bn_se_block_backward_at_training_shapes(lib, row):
    """An MBConv _bn1 + squeeze-excite, forward and backward as the training step chains them (train.py: bn_act(want_se) ->
    se_gate; se_bn_bwd_reduce -> se_bwd on the forward's own squeeze partials -> se_bn_bwd_apply), plus the three-pass
    se_dgate partials, against float64 autograd of the whole block.  Tolerance: 2e-4 of each output's scale, as the
    small-shape tests (per-(sample, channel) sums of <= 51 200 terms, eps * sqrt(L) * |mean| / sigma stays below 1e-4)."""
    from ccvpe_amd import backward as bw, ops
    name, b, h, w, c, cs, nblk = row
    hw = h * w
    assert lib.ccvpe_bn_act_nblk(hw) == nblk and lib.ccvpe_bn_bwd_nblk(hw) == nblk, "%s: geometry changed" % name
    chk = Checks(name)
    x, xr, m64, v64, gamma, beta, _, _ = _bn_inputs(b, hw, c, 3300 + c, False)
    dv = grad_like((b, hw, c), 3350 + c)
    w1 = synth.normal((cs, c), 3360 + c, c ** -0.5)
    b1 = synth.normal((cs,), 3361 + c, 0.1)
    w2 = synth.normal((c, cs), 3362 + c, cs ** -0.5)
    b2 = synth.normal((c,), 3363 + c, 0.1)
    m32, v32 = m64.float().cuda(), v64.float().cuda()
    gd, bd = gamma.cuda(), beta.cuda()
    w1d, b1d, w2t, b2d = w1.cuda(), b1.cuda(), w2.t().contiguous().cuda(), b2.cuda()

    def run():
        u, part = ops.bn_act(x, m32, v32, gd, bd, BN_EPS, ops.ACT_SWISH, want_se=True)
        gate = ops.se_gate(part, hw, w1d, b1d, w2t, b2d)
        sums = bw.se_bn_bwd_reduce(x, dv, m32, v32, gd, bd, BN_EPS, ops.ACT_SWISH)
        dmean, dw1, db1, dw2, db2 = bw.se_bwd(part, hw, sums[0].unsqueeze(1), w1d, b1d, w2t, b2d)
        dx, dgamma, dbeta = bw.se_bn_bwd_apply(x, dv, m32, v32, gd, bd, BN_EPS, ops.ACT_SWISH, gate, dmean, sums)
        dgp = bw.se_dgate_partials(x, dv, m32, v32, gd, bd, BN_EPS, ops.ACT_SWISH)
        return dict(u=u, gate=gate, dgate=sums[0], dgate3=dgp.sum(1), dw1=dw1, db1=db1, dw2=dw2, db2=db2, dx=dx,
                    dgamma=dgamma, dbeta=dbeta)

    got = run()
    again = run()
    for k in got:
        chk.same(k, got[k], again[k])
    xa = xr.clone().requires_grad_(True)
    ga, ba = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    w1a, b1a, w2a, b2a = (t.double().requires_grad_(True) for t in (w1, b1, w2, b2))
    mean, var = xa.mean(dim=(0, 1)), xa.var(dim=(0, 1), unbiased=False)
    u = swish((xa - mean) / torch.sqrt(var + BN_EPS) * ga + ba)
    z1 = u.mean(dim=1) @ w1a.t() + b1a
    gate = torch.sigmoid(swish(z1) @ w2a.t() + b2a)
    gate.retain_grad()
    (u * gate.unsqueeze(1) * dv.cpu().double()).sum().backward()
    chk("u (bn + swish)", got["u"], u.detach(), float("inf"))
    chk("gate", got["gate"], gate.detach(), float("inf"), 1e-5)
    chk("dgate (two-pass sums)", got["dgate"], gate.grad, float("inf"))
    chk("dgate (se_dgate partials)", got["dgate3"], gate.grad, float("inf"))
    for k, ref in (("dw1", w1a.grad), ("db1", b1a.grad), ("dw2", w2a.grad), ("db2", b2a.grad), ("dgamma", ga.grad),
                   ("dbeta", ba.grad), ("dx", xa.grad)):
        chk(k, got[k], ref, float("inf"))
    chk.done()


# ---- depthwise weight gradient, all-taps kernel ------------------------------------------------------------------

@pytest.mark.parametrize("row", S.DW_WGRAD, ids=[r[0] for r in S.DW_WGRAD])
def test_dwconv_wgrad_at_training_shapes(lib, row):
    from ccvpe_amd import backward as bw
    from oracle import ccvpe_oracle as orc
    name, b, h, w, c, k, s, circ, nblk = row
    assert lib.ccvpe_dwconv_wgrad_nblk(h, w, k, s) == nblk, "%s: geometry changed" % name
    chk = Checks(name)
    x = synth.normal((b, h, w, c), 3400 + c, device="cuda")
    pb, pa = orc.static_same_pad(224, k, s)
    ho = (h + pb + pa - k) // s + 1
    wo = (w + pb + pa - k) // s + 1
    dy = grad_like((b, ho, wo, c), 3401 + c)
    got = bw.dwconv_wgrad(x, dy, k, s, circ)
    chk.same("dw", got, bw.dwconv_wgrad(x, dy, k, s, circ))
    # float64: the padded input exactly as the oracle's same_conv pads it, then dW[ky,kx,c] = sum dy * xpad (shifted views)
    want = torch.zeros((k * k, c), dtype=torch.float64)
    absum = torch.zeros((k * k, c), dtype=torch.float64)
    for b0 in range(0, b, 4):
        xc = x[b0:b0 + 4].cpu().double().permute(0, 3, 1, 2)
        if circ:
            xc = F.pad(F.pad(xc, [pb, pa, 0, 0], mode="circular"), [0, 0, pb, pa])
        else:
            xc = F.pad(xc, [pb, pa, pb, pa])
        xc = xc.permute(0, 2, 3, 1)
        dc = dy[b0:b0 + 4].cpu().double()
        for ky in range(k):
            for kx in range(k):
                xs = xc[:, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (wo - 1) + 1:s, :]
                want[ky * k + kx] += (xs * dc).sum(dim=(0, 1, 2))
                absum[ky * k + kx] += (xs.abs() * dc.abs()).sum(dim=(0, 1, 2))
    rows = 1 if ho <= 64 else (2 if ho <= 128 else 4)
    P = 256 // min(c // 4, 64)
    strips = rows * ((wo + 3) // 4)                     # strips of 4 output columns, P row lanes, then the partial rows
    L = (strips + P - 1) // P * 4 + P + S.sum_parts_chain(nblk * b, k * k * c) + 8
    chk("dw", got, want, EPS * L * absum)
    chk.done()


# ---- head 3x3 conv backward ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", S.HEAD_BWD, ids=[r[0] for r in S.HEAD_BWD])
def test_head_conv_bwd_at_training_shapes(row):
    from ccvpe_amd import backward as bw
    name, b, h, w, cout, ntiles = row
    assert ((w + 63) // 64) * ((h + 3) // 4) * b == ntiles > S.HEAD_WGRAD_BLOCKS, "%s: not the grid-stride tile loop" % name
    chk = Checks(name)
    x = torch.relu(synth.normal((b, h, w, 16), 3500 + cout, device="cuda"))            # a ReLU output, as in the decoder
    wt = synth.normal((cout, 3, 3, 16), 3501, 0.1).cuda()
    dr = grad_like((b, cout, h, w), 3502, 0.2).contiguous()
    dx, dw, db = bw.head_conv3x3_bwd(x, wt, dr)
    dx2, dw2, db2 = bw.head_conv3x3_bwd(x, wt, dr)
    chk.same("dx", dx, dx2)
    chk.same("dw", dw, dw2)
    chk.same("dbias", db, db2)
    xn = x.cpu().double().permute(0, 3, 1, 2)
    drd = dr.cpu().double()
    wn = wt.cpu().double().permute(0, 3, 1, 2)
    want_dw = torch.nn.grad.conv2d_weight(xn, wn.shape, drd, padding=1)
    abs_dw = torch.nn.grad.conv2d_weight(xn.abs(), wn.shape, drd.abs(), padding=1)
    want_dx = torch.nn.grad.conv2d_input(xn.shape, wn, drd, padding=1)
    abs_dx = torch.nn.grad.conv2d_input(xn.shape, wn.abs(), drd.abs(), padding=1)
    trips = (ntiles + S.HEAD_WGRAD_BLOCKS - 1) // S.HEAD_WGRAD_BLOCKS
    L = trips * 256 + S.sum_parts_chain(S.HEAD_WGRAD_BLOCKS, cout * 145) + 8       # 256 pixels per tile, serial per thread
    chk("dw", dw, want_dw.permute(0, 2, 3, 1), EPS * L * abs_dw.permute(0, 2, 3, 1))
    chk("dbias", db, drd.sum(dim=(0, 2, 3)), EPS * L * drd.abs().sum(dim=(0, 2, 3)))
    chk("dx", dx, want_dx.permute(0, 2, 3, 1), EPS * (9 * cout + 4) * abs_dx.permute(0, 2, 3, 1))
    chk.done()


# ---- stem conv weight gradient -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", S.STEM_WGRAD, ids=[r[0] for r in S.STEM_WGRAD])
def test_stem_wgrad_at_training_shapes(lib, row):
    from ccvpe_amd import backward as bw
    from oracle import ccvpe_oracle as orc
    name, b, h, w, circ, nblk, partial = row
    assert lib.ccvpe_stem_wgrad_nblk(b, h, w) == nblk and ((w // 2) % 256 != 0) == partial, "%s: geometry changed" % name
    chk = Checks(name)
    img = synth.normal((b, 3, h, w), 3600 + w, device="cuda")
    dy = grad_like((b, h // 2, w // 2, 32), 3601 + w)
    got = bw.stem_conv_wgrad(img, dy, circ)
    chk.same("dw", got, bw.stem_conv_wgrad(img, dy, circ))
    pb, pa = orc.static_same_pad(224, 3, 2)
    want = torch.zeros((32, 3, 3, 3), dtype=torch.float64)
    absum = torch.zeros_like(want)
    for b0 in range(0, b, 4):
        xc = img[b0:b0 + 4].cpu().double()
        if circ:
            xc = F.pad(F.pad(xc, [pb, pa, 0, 0], mode="circular"), [0, 0, pb, pa])
        else:
            xc = F.pad(xc, [pb, pa, pb, pa])
        dc = dy[b0:b0 + 4].cpu().double().permute(0, 3, 1, 2)
        want += torch.nn.grad.conv2d_weight(xc, want.shape, dc, stride=2)
        absum += torch.nn.grad.conv2d_weight(xc.abs(), want.shape, dc.abs(), stride=2)
    L = 16 * 8 + 32 + S.sum_parts_chain(nblk, 27 * 32) + 8      # 16 rows x 8 pixels per lane, 32 lanes, the partial rows
    chk("dw", got, want.permute(2, 3, 1, 0), EPS * L * absum.permute(2, 3, 1, 0))
    chk.done()


# ---- matching backward -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", S.MATCH_BWD, ids=[r[0] for r in S.MATCH_BWD])
def test_match_level_bwd_at_training_shapes(lib, row):
    """Tolerance: 2e-4 of scale, as the small-shape test (dx sums <= 2 * 48 shift terms per element; dg sums hw * shifts
    terms per entry through <= 32 channel slices in fixed order: eps * L stays below 1e-4 for these sizes)."""
    from ccvpe_amd import backward as bw, ops
    from oracle import ccvpe_oracle as orc
    name, b, c, L, side, shifts, n_max, n_tail, stride, nblk, npad = row
    hw = side * side
    assert lib.ccvpe_match_bwd_nblk(hw, b, c) == nblk and S.npad_of(len(shifts)) == npad, "%s: geometry changed" % name
    chk = Checks(name)
    n = len(shifts)
    ldo = (c + 1 + n_tail + 7) // 8 * 8
    x = synth.normal((b, side, side, c), 3700 + c, device="cuda")
    g = synth.normal((b, L), 3701 + c, device="cuda")
    dsc = synth.normal((b, n, side, side), 3702 + c, device="cuda")
    ddst = synth.normal((b, side, side, ldo), 3703 + c, device="cuda")
    scores, _ = ops.match_level(x, g, L, shifts, n_max, n_tail, stride, ldo, channels=c)

    def run():
        dg = torch.zeros((b, L), device="cuda")
        return bw.match_level_bwd(x, g, L, shifts, n_max, n_tail, stride, scores, dsc, ddst, c, dg), dg

    dx, dg = run()
    dx2, dg2 = run()
    chk.same("dx", dx, dx2)
    chk.same("dg", dg, dg2)
    want_dx, want_dg = [], []
    for b0 in range(0, b, 8):                                   # samples are independent: bounded float64 graphs
        xa = x[b0:b0 + 8].cpu().double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        ga = g[b0:b0 + 8].cpu().double().requires_grad_(True)
        sc = orc.rotational_matching(xa, ga, shifts, stride)
        mx = sc[:, :n_max].max(dim=1, keepdim=True)[0]
        dst = torch.cat([F.normalize(xa, p=2, dim=1), mx] + ([sc[:, n - n_tail:]] if n_tail else []), dim=1)
        dd = ddst[b0:b0 + 8].cpu().double()
        ((sc * dsc[b0:b0 + 8].cpu().double()).sum() + (dst.permute(0, 2, 3, 1) * dd[..., :dst.shape[1]]).sum()).backward()
        want_dx.append(xa.grad.permute(0, 2, 3, 1))
        want_dg.append(ga.grad)
    chk("dx", dx, torch.cat(want_dx), float("inf"))
    chk("dg", dg, torch.cat(want_dg), float("inf"))
    chk.done()


# ---- softmax backward and the cross-entropy backward on peaked heat maps ------------------------------------------------

def _peaked_logits(rows, n, seed):
    """float64 logits with one dominant peak per row: h_max spread over 0.5 ... 0.99."""
    z = synth.normal((rows, n), seed, 2.0).double()
    hmax = torch.linspace(0.5, 0.99, rows, dtype=torch.float64)
    pos = (synth.uniform((rows,), seed + 1) * n).long().clamp_(max=n - 1)
    z[torch.arange(rows), pos] = -30.0
    rest = torch.logsumexp(z, dim=1)
    z[torch.arange(rows), pos] = rest + torch.log(hmax / (1.0 - hmax))
    return z


@pytest.mark.parametrize("row", S.SOFTMAX_BWD, ids=[r[0] for r in S.SOFTMAX_BWD])
def test_softmax_and_cross_entropy_bwd_on_peaked_heatmaps(row):
    from ccvpe_amd import backward as bw, losses
    name, rows, n = row
    chk = Checks(name)
    z = _peaked_logits(rows, n, 3800 + rows)
    h = torch.softmax(z, dim=1).float()
    assert 0.49 < h.max(dim=1)[0].min().item() and h.max().item() < 0.991
    dh = grad_like((rows, n), 3801, 0.5)
    dl = synth.normal((rows, n), 3802, 1e-3, device="cuda")
    hd = h.cuda()
    got = bw.softmax_bwd(hd, dh, dl)
    chk.same("softmax dlogits", got, bw.softmax_bwd(hd, dh, dl))
    hr, dhr, dlr = h.double(), dh.cpu().double(), dl.cpu().double()
    dot = (hr * dhr).sum(dim=1, keepdim=True)
    want = hr * (dhr - dot) + dlr
    L = n // 4096 + 4 + 6 + 16 + 8                    # per-thread chain of 4-wide rows, wave and workgroup sums
    bdot = EPS * L * (hr * dhr).abs().sum(dim=1, keepdim=True)
    chk("softmax dlogits", got, want, hr * (bdot + 4 * EPS * (dhr.abs() + dot.abs())) + 4 * EPS * (want.abs() + dlr.abs()))

    # cross-entropy: trained-like logits (the same peaks) against a peaked label map of unit mass
    lab = synth.uniform((rows, n), 3803).double() ** 40
    lab = (lab / lab.sum(dim=1, keepdim=True)).float()
    zf = z.float()
    lg = zf.cuda().requires_grad_(True)
    losses.cross_entropy_loss(lg, lab.cuda()).backward()
    lg2 = zf.cuda().requires_grad_(True)
    losses.cross_entropy_loss(lg2, lab.cuda()).backward()
    chk.same("cross-entropy dlogits", lg.grad, lg2.grad)
    zr, lr = zf.double(), lab.double()
    p = torch.softmax(zr, dim=1)
    ls = lr.sum(dim=1, keepdim=True)
    want = (p * ls - lr) / rows
    Lc = n // 1024 + 6 + 16 + 8
    span = zr.max(dim=1, keepdim=True)[0] - zr                 # exp(z - max): relative error eps * |z - max|
    bound = (p * ls * EPS * (2 * Lc + 4 * span + 8) + 4 * EPS * lr) / rows
    chk("cross-entropy dlogits", lg.grad, want, bound)
    chk.done()


# ---- bias-gradient column sums -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", S.COLSUM, ids=[r[0] for r in S.COLSUM])
def test_colsum_at_training_shapes(row):
    from ccvpe_amd import backward as bw
    name, rows, c, ld = row
    assert rows >= S.CS_ROWS * 256, "%s: not the many-rows branch" % name
    chk = Checks(name)
    dy = grad_like((rows, ld), 3900 + c, 0.5)
    got = bw.bias_grad(dy, c)
    chk.same("dbias", got, bw.bias_grad(dy, c))
    dr = dy.cpu().double()[:, :c]
    v = 4 if c % 4 == 0 and ld % 4 == 0 else 1
    R = 256 // min(c // v, 256)
    nblk = (rows + S.CS_ROWS - 1) // S.CS_ROWS
    L = S.CS_ROWS // R + R + S.sum_parts_chain(nblk, c) + 8
    chk("dbias", got, dr.sum(0), EPS * L * dr.abs().sum(0))
    chk.done()
