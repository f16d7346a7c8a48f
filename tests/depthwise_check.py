"""Float64 reference and elementwise error model for the depthwise conv kernels (dwconv_kernel, dwconv_plane_kernel, the
depthwise-only form of mbconv_plane_kernel, dw_dgrad_kernel), and the seeded inputs of tests/depthwise_kernel_shapes.py's rows.

Shared by tests/test_depthwise_forms_gpu.py (the kernels, on the MI355X) and tests/test_depthwise_check.py (CPU: torch's own float32
results must pass, results with one injected fault each must not).

THE REFERENCE.  k x k shifted multiply-adds in float64 on the padded tensor (no convolution backend), pads from
oracle.static_same_pad(224, k, stride): (1,1) / (2,2) at stride 1, (0,1) / (1,2) at stride 2; columns circular when asked, rows
always zero-padded.  S_i = the same sum over |x| |w|.  Input gradients are float64 autograd of that function, S'_j the same
transposed sum over |dy| |w|.

THE MODEL.  u = 2^-24, K = k^2.  None of the bounds is tuned to what a kernel gives.
  RAW output and input gradients:  |got_i - ref_i| <= K u S_i.  K products, each rounded once, and every term then passes through
    at most K - 1 additions: (1 + u)^K - 1 <= K u (1 + K u), any order, with or without FMA.  (Zero terms — padding, taps that meet
    no output at stride 2 — add nothing in any order, so an element with S_i = 0 must be exactly 0.)
  Fused output, z = sc conv + sh, ref = swish(z):
    tol_i = 1.1 (K + 2) u (|sc| S_i + |sh|) + (6 + 2 |z_i|) u |ref_i|.
    First term: the pre-activation (K + 2 roundings on the conv terms with the scale multiply and the shift add; the shift itself
    sees one) times swish's largest slope, 1.0998.  Second term: the activation's own relative error from common.h's sigmoidf,
    v * rcp(1 + exp2(-1.4427 v)): the constant and the product -1.4427 v are rounded (2 u relative = 2 |v| 1.4427 u absolute in the
    exponent, x ln 2 = 2 |v| u relative in 2^t), v_exp_f32 1 ulp = 2 u, the add u, v_rcp_f32 1 ulp = 2 u, the final multiply u: 6 + 2 |v|.
    The 1 ulp figures are the ones common.h's comment states; no other accuracy figure for the two transcendentals is documented
    for this target, so those stand.
  bf16 storage: x is rounded to bf16 before the reference is computed (weights, scale and shift are fp32 in both entry points);
    + 2^-8 |ref_i| for the one output rounding.
  Squeeze sums, per (sample, channel): float64 sum over the partial rows against the float64 sum of the reference,
    tol = sum_i tol_i (without the bf16 term: the partials are fp32 sums of unrounded outputs) + d u sum_i |ref_i|,
    d = the longest chain of fp32 additions a term passes through (depthwise_kernel_shapes.strip_chain / plane_chain / band_chain).
  The suite's older bars stay as a second condition: max error <= 1e-4 (fp32) / 1e-2 (bf16) of the tensor's maximum.
Every element is compared: no masks, no sampling.
"""
import functools

import torch
import torch.nn.functional as F

from ccvpe_amd import synth
from oracle import ccvpe_oracle as O

import depthwise_kernel_shapes as S

U = 2.0 ** -24
BF = torch.bfloat16


def rbf(t):
    """round to nearest bf16 and back: the values a bf16-storage kernel sees"""
    return t.to(BF).float()


def dw_inputs(row, bf16):
    """x [B,C,H,W] (bf16-rounded if asked), w [C,k,k], BN scale and shift [C] — float32, seeded per row"""
    seed = 7000 + 13 * row.c + 3 * row.h + row.w + 101 * row.k + 17 * row.s
    x = synth.normal((row.b, row.c, row.h, row.w), seed)
    wt = synth.normal((row.c, row.k, row.k), seed + 1, 1.0 / row.k)
    sc, sh = synth.uniform((row.c,), seed + 2, 0.5, 1.5), synth.normal((row.c,), seed + 3, 0.2)
    return (rbf(x) if bf16 else x), wt, sc, sh


def grad_input(row):
    """the upstream gradient of the row's input-gradient launch [B,C,*,*]: stride 1 takes the row's own shape as the gradient (the
    forward entry with reversed taps), stride 2 the output's"""
    shape = (row.b, row.c, row.h, row.w) if row.s == 1 else (row.b, row.c, row.geo.ho, row.geo.wo)
    return synth.normal(shape, 7900 + row.c + row.h + 7 * row.k)


def pad_same(x, k, stride, circular):
    """the 224-schedule SAME padding: columns wrapped or zero, rows zero"""
    pb, pa = O.static_same_pad(224, k, stride)
    w = x.shape[-1]
    if circular:
        x = x[..., torch.arange(-pb, w + pa) % w]
    else:
        x = F.pad(x, [pb, pa, 0, 0])
    return F.pad(x, [0, 0, pb, pa])


def dw_conv(x, wt, k, stride, circular, dtype, pad_fault=None, tap_fault=None):
    """depthwise conv of x [B,C,H,W] with wt [C,k,k] as k x k shifted multiply-adds in `dtype`.  pad_fault(xp) may alter the padded
    tensor and tap_fault(ky, kx, w_tap) one tap's weights (fault injection, tests/test_depthwise_check.py)."""
    xp = pad_same(x.to(dtype), k, stride, circular)
    if pad_fault is not None:
        xp = pad_fault(xp)
    ho, wo = S.out_dims(x.shape[2], x.shape[3], k, stride)
    wd = wt.to(dtype)
    acc = torch.zeros((x.shape[0], x.shape[1], ho, wo), dtype=dtype)
    for ky in range(k):
        for kx in range(k):
            tap = wd[:, ky, kx]
            if tap_fault is not None:
                tap = tap_fault(ky, kx, tap)
            acc = acc + xp[:, :, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride] * tap.view(1, -1, 1, 1)
    return acc


def bn_swish(conv, sc, sh):
    z = conv * sc.to(conv.dtype).view(1, -1, 1, 1) + sh.to(conv.dtype).view(1, -1, 1, 1)
    return z * torch.sigmoid(z)


def f32_chain(x, wt, sc, sh, k, stride, circular, **faults):
    """the fused operation in float32 from the written-out conv (accepts dw_conv's faults)"""
    return bn_swish(dw_conv(x, wt, k, stride, circular, torch.float32, **faults), sc, sh)


class DwRef:
    """float64 reference of one row: conv (RAW), S, z, ref = swish(z), the tolerances, and torch's own float32 CPU results"""

    def __init__(self, row, bf16):
        self.row, self.bf16 = row, bf16
        self.inputs = x, wt, sc, sh = dw_inputs(row, bf16)
        k, s, circ = row.k, row.s, row.circ
        kk = k * k
        self.conv = dw_conv(x, wt, k, s, circ, torch.float64)
        self.s_abs = dw_conv(x.abs(), wt.abs(), k, s, circ, torch.float64)
        sc64, sh64 = sc.double().view(1, -1, 1, 1), sh.double().view(1, -1, 1, 1)
        self.z = self.conv * sc64 + sh64
        self.ref = self.z * torch.sigmoid(self.z)
        self.tol_raw = kk * U * self.s_abs
        self.tol_fused = 1.1 * (kk + 2) * U * (sc64.abs() * self.s_abs + sh64.abs()) + (6 + 2 * self.z.abs()) * U * self.ref.abs()
        self.tol_bf16 = self.tol_fused + 2.0 ** -8 * self.ref.abs()
        self.f32_conv = O.same_conv(x, wt.view(row.c, 1, k, k), k, s, 224, circ, groups=row.c)
        self.f32_fused = O.swish(self.f32_conv * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))

    def grad(self, dy):
        """(float64 input gradient for the upstream gradient dy [B,C,Ho,Wo], its bound K u S')"""
        x, wt = self.inputs[0], self.inputs[1]
        row = self.row
        out = []
        for g, w_ in ((dy.double(), wt.double()), (dy.double().abs(), wt.double().abs())):
            x0 = torch.zeros(x.shape, dtype=torch.float64, requires_grad=True)
            y = dw_conv(x0, w_, row.k, row.s, row.circ, torch.float64)
            out.append(torch.autograd.grad(y, x0, g)[0])
        return out[0], row.k * row.k * U * out[1]


@functools.lru_cache(maxsize=4)
def cached_ref(row, bf16):
    return DwRef(row, bf16)


def old_rule_passes(got, ref, tol_of_scale):
    """the rule the operator tests use: max error relative to the tensor's maximum"""
    got, ref = got.detach().double(), ref.detach().double()
    return (got - ref).abs().max().item() <= tol_of_scale * (ref.abs().max().item() + 1e-30)


def _where(ratio):
    i = ratio.flatten().argmax().item()
    return tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))


def dw_check(got_nchw, ref, tol, bar, what):
    """|got_i - ref_i| <= tol_i for every element, and max error <= bar x the tensor's maximum.  Returns (max_i err_i / tol_i,
    max error relative to scale); prints them."""
    got = got_nchw.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: non-finite output" % what
    err = (got - ref).abs()
    ratio = err / tol.clamp_min(1e-300)                      # tol_i = 0 (S_i = 0): the element must be exact
    worst = ratio.max().item()
    scale = ref.abs().max().item() + 1e-30
    rel = err.max().item() / scale
    print("%s: max err/tol %.3f, max err %.3e = %.2e of scale" % (what, worst, err.max().item(), rel))
    if worst > 1.0:
        idx = _where(ratio)
        strips_per_row = (ref.shape[3] + S.DW_TW - 1) // S.DW_TW
        raise AssertionError("%s: %d elements outside the elementwise tolerance; worst at (b, channel, y, x) = %s (4-channel group %d, "
                             "strip %d): got %.9g want %.9g, err %.3e = %.2f x tol"
                             % (what, int((ratio > 1.0).sum()), idx, idx[1] // 4, idx[2] * strips_per_row + idx[3] // S.DW_TW,
                                got[idx].item(), ref[idx].item(), err[idx].item(), worst))
    assert rel <= bar, "%s: max err %.3e above %.0e of scale %.3e" % (what, err.max().item(), bar, scale)
    return worst, rel


def sum_check(part, dr, chain, bar, what):
    """squeeze partial rows [B,nblk,C] (fp32) against the float64 sums of the reference, per (sample, channel)"""
    got = part.detach().cpu().double().sum(1)
    want = dr.ref.sum(dim=(2, 3))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), "%s: non-finite squeeze partial" % what
    tol = dr.tol_fused.sum(dim=(2, 3)) + chain * U * dr.ref.abs().sum(dim=(2, 3))
    err = (got - want).abs()
    ratio = err / tol
    worst = ratio.max().item()
    scale = want.abs().max().item() + 1e-30
    rel = err.max().item() / scale
    print("%s: max err/tol %.3f (d = %d), max err %.3e = %.2e of scale" % (what, worst, chain, err.max().item(), rel))
    if worst > 1.0:
        idx = _where(ratio)
        raise AssertionError("%s: %d squeeze sums outside the elementwise tolerance; worst at (b, channel) = %s (4-channel group %d): "
                             "got %.9g want %.9g, err %.3e = %.2f x tol"
                             % (what, int((ratio > 1.0).sum()), idx, idx[1] // 4, got[idx].item(), want[idx].item(), err[idx].item(), worst))
    assert rel <= bar, "%s: max err %.3e above %.0e of scale %.3e" % (what, err.max().item(), bar, scale)
    return worst, rel
