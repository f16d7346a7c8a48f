"""Elementwise error model for the forward conv3x3 / MBConv band kernel checks, and the seeded cases it is applied to.

Shared by tests/test_forward_variants_gpu.py (the kernels, on the MI355X) and tests/test_forward_variant_check.py (CPU: the same
comparison applied to results with one injected fault each — the checker must be sharp enough to see them).

THE MODEL (3x3 rows).  u = 2^-24.  For output element i, S_i = sum_k |a_k w_k| + |bias| in float64 (one extra float64 conv of
absolute values).  Any fp32 evaluation of the sum, in any order, is within K u S_i of the exact value (K = 9 (c0 + c1) + 1 terms):
the rigorous ceiling.  Real summations sit far below it, so the tolerance is c u S_i with
    c = 4 x max_i err_i / (u S_i) of torch's own float32 CPU conv of the same row against float64,
computed per row in the test (on the table's rows the ratio is 1.6 - 3.1 with fp32 operands, so c = 6.5 - 12.6, and 0.7 - 1.3 with
bf16-rounded operands, whose products are exact in fp32, so c = 2.8 - 5.3); the factor 4 covers another summation order on the
matrix cores, and c <= K is asserted, so the tolerance never exceeds the rigorous ceiling.
    fp32, and bf16 storage writing fp32 (out_f32):   |got_i - ref_i| <= c u S_i
    bf16 storage:                                    |got_i - ref_i| <= 2^-8 |ref_i| + c u S_i
(2^-8 |ref_i|: ONE round-to-nearest of the exact value to 8 significand bits; the operands are rounded to bf16 before the
reference is computed, so products are exact in fp32 and only the accumulation and the output rounding remain.)  ReLU is
1-Lipschitz, so the same bounds hold after it with ref_i = relu(exact).  The suite's older bars stay as a second condition:
max error <= 1e-4 (fp32) / 1e-2 (bf16) of the tensor's maximum.  Every element is compared: no masks, no sampling.

THE MODEL (band rows).  S_i does not propagate through two swishes, so the accumulation term is measured instead:
A = 4 x max_i |float32 CPU chain_i - float64 chain_i| (on bf16-rounded operands), and |y_i - ref_i| <= 2^-8 |ref_i| + A.
Two kernels that both satisfy this hold fp32 values within 2A of each other before the output rounding and each rounding moves a
value by at most half a bf16 ulp, so band vs slice kernel: |a_i - b_i| <= ulp_bf16(max(|a_i|, |b_i|)) + 2A — "one bf16 ulp", with
the fp32 term that matters only where swish crosses zero (|y| < 1e-3) and an ulp of the result is smaller than fp32 round-off of
the pre-activation.  Squeeze partials: 2e-3 of scale, as in tests/test_bf16_gpu.py.
"""
import functools

import torch
import torch.nn.functional as F

from ccvpe_amd import synth
from oracle import ccvpe_oracle as O

U = 2.0 ** -24
BF = torch.bfloat16


def rbf(t):
    """round to nearest bf16 and back: the values a bf16-storage kernel sees"""
    return t.to(BF).float()


# ------------------------------------------------------------------------------------------------------------------------------
# 3x3 rows
# ------------------------------------------------------------------------------------------------------------------------------
def conv_inputs(row, bf16, batch=None):
    """(a [B,ld0,H,W], s [B,c1,H,W], wt [N,c0+c1,3,3], bias [N]) float32 for a forward_kernel_shapes.CONV3X3 row.  Channels
    row.real0 .. ld0 of `a` are zero (padding channels of a concat buffer; the kernel reads c0 of them and their weights are NOT
    zero, so a kernel that picked up a neighbour's data instead would show).  The batch is the leading axis of a hash stream
    indexed linearly, so a smaller `batch` is exactly the prefix of the larger case."""
    b = batch or row.b
    rnd = rbf if bf16 else (lambda t: t)
    seed = 9000 + 7 * row.n + row.h
    a = rnd(synth.normal((b, row.ld0, row.h, row.w), seed))
    if row.real0 < row.ld0:
        a[:, row.real0:] = 0
    s = rnd(synth.normal((b, row.c1, row.h, row.w), seed + 1))
    wt = rnd(synth.normal((row.n, row.c0 + row.c1, 3, 3), seed + 2, (1.0 / (9 * (row.c0 + row.c1))) ** 0.5))
    bias = synth.normal((row.n,), seed + 3, 0.1)
    return a, s, wt, bias


class ConvRef:
    """float64 reference of one row (pre-activation), S_i, torch's float32 result and the factor c derived from it"""

    def __init__(self, a, s, wt, bias, c0):
        x = torch.cat([a[:, :c0], s], 1)
        self.k_terms = 9 * x.shape[1] + 1
        self.ref = F.conv2d(x.double(), wt.double(), bias.double(), padding=1)
        self.s_abs = F.conv2d(x.double().abs(), wt.double().abs(), bias.double().abs(), padding=1)
        self.f32 = F.conv2d(x, wt, bias, padding=1)
        self.f32_ratio = (((self.f32.double() - self.ref).abs()) / (U * self.s_abs + 1e-300)).max().item()
        self.c = 4.0 * self.f32_ratio
        assert self.c <= self.k_terms, "c = %.1f above the rigorous ceiling K = %d" % (self.c, self.k_terms)

    def prefix(self, b):
        """the same reference for the first b images (a threshold pair shares one reference)"""
        r = object.__new__(ConvRef)
        r.k_terms, r.f32_ratio, r.c = self.k_terms, self.f32_ratio, self.c
        r.ref, r.s_abs, r.f32 = self.ref[:b], self.s_abs[:b], self.f32[:b]
        return r


def conv_check(got_nchw, cr, relu, bf16_storage, bf16_operands, what):
    """Assert the model above for every element; returns max_i err_i / tol_i (recorded in profiles/r09/variant_checks.txt)."""
    got = got_nchw.detach().cpu().double()
    ref = F.relu(cr.ref) if relu else cr.ref
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), "%s: non-finite output" % what
    err = (got - ref).abs()
    tol = cr.c * U * cr.s_abs
    if bf16_storage:
        tol = tol + 2.0 ** -8 * ref.abs()
    ratio = err / tol
    worst = ratio.max().item()
    scale = ref.abs().max().item() + 1e-30
    bar = 1e-2 if bf16_operands else 1e-4
    print("%s: max err/tol %.3f (c = %.1f), max err %.3e = %.2e of scale" % (what, worst, cr.c, err.max().item(), err.max().item() / scale))
    if worst > 1.0:
        i = ratio.flatten().argmax().item()
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
        bad = int((ratio > 1.0).sum())
        raise AssertionError("%s: %d elements outside the elementwise tolerance; worst at (b, n, y, x) = %s: got %.9g want %.9g, "
                             "err %.3e = %.2f x tol" % (what, bad, idx, got[idx].item(), ref[idx].item(), err[idx].item(), worst))
    assert err.max().item() <= bar * scale, "%s: max err %.3e above %.0e of scale %.3e" % (what, err.max().item(), bar, scale)
    return worst


def old_rule_passes(got, ref, tol_of_scale):
    """the rule the operator tests used before: max error relative to the tensor's maximum"""
    got, ref = got.detach().double(), ref.detach().double()
    return (got - ref).abs().max().item() <= tol_of_scale * (ref.abs().max().item() + 1e-30)


# ------------------------------------------------------------------------------------------------------------------------------
# band rows: expand 1x1 + BN + swish -> depthwise k x k + BN + swish (+ squeeze sums)
# ------------------------------------------------------------------------------------------------------------------------------
def band_inputs(row, batch=None, device=None):
    """x [B,cin,h,w] (bf16-rounded), w_exp [mid,cin] (bf16-rounded), s0, b0, w_dw [mid,k,k], s1, b1 — float32"""
    b, cin, mid, k = batch or row.b, row.cin, 6 * row.cin, row.k
    seed = 9500 + row.cin + row.h
    x = rbf(synth.normal((b, cin, row.h, row.w), seed, device=device))
    w_exp = rbf(synth.normal((mid, cin), seed + 1, (2.0 / cin) ** 0.5, device=device))
    s0, b0 = synth.uniform((mid,), seed + 2, 0.5, 1.5, device=device), synth.normal((mid,), seed + 3, 0.2, device=device)
    w_dw = synth.normal((mid, k, k), seed + 4, 1.0 / k, device=device)
    s1, b1 = synth.uniform((mid,), seed + 5, 0.5, 1.5, device=device), synth.normal((mid,), seed + 6, 0.2, device=device)
    return x, w_exp, s0, b0, w_dw, s1, b1


def band_chain(x, w_exp, s0, b0, w_dw, s1, b1, k, stride, circular, dtype, bn_shift_fault=None):
    """The fused front written out with plain tensor operations in `dtype` on x's device (a matrix product for the 1x1 conv,
    k x k shifted multiply-adds for the depthwise conv — no convolution backend involved, so float64 runs anywhere):
    swish(BN1(dw(swish(BN0(expand(x)))))), padding from the 224 schedule (oracle.same_conv), circular along W if asked.
    bn_shift_fault = (sample, slice): that 16-channel slice of that sample gets the PREVIOUS slice's BN0 shift (fault injection)."""
    c = lambda t: t.to(dtype)
    b, cin, h, w = x.shape
    mid = w_exp.shape[0]
    t = torch.matmul(c(w_exp), c(x).reshape(b, cin, h * w)).reshape(b, mid, h, w)
    shift0 = c(b0).view(1, mid, 1, 1).expand(b, mid, 1, 1)
    if bn_shift_fault is not None:
        smp, sl = bn_shift_fault
        shift0 = shift0.clone()
        shift0[smp, 16 * sl:16 * sl + 16] = c(b0)[16 * sl - 16:16 * sl].view(16, 1, 1)
    t = t * c(s0).view(1, mid, 1, 1) + shift0
    t = t * torch.sigmoid(t)
    pb, pa = O.static_same_pad(224, k, stride)
    if circular:
        t = F.pad(F.pad(t, [pb, pa, 0, 0], mode="circular"), [0, 0, pb, pa])
    else:
        t = F.pad(t, [pb, pa, pb, pa])
    ho, wo = (h + pb + pa - k) // stride + 1, (w + pb + pa - k) // stride + 1
    acc = torch.zeros((b, mid, ho, wo), dtype=dtype, device=x.device)
    wd = c(w_dw)
    for ky in range(k):
        for kx in range(k):
            acc += t[:, :, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride] * wd[:, ky, kx].view(1, mid, 1, 1)
    y = acc * c(s1).view(1, mid, 1, 1) + c(b1).view(1, mid, 1, 1)
    return y * torch.sigmoid(y)


def band_f32_cpu_chain(x, w_exp, s0, b0, w_dw, s1, b1, k, stride, circular):
    """torch's own float32 CPU convolutions of the same chain (the oracle's operators): its error against float64 sets A"""
    mid = w_exp.shape[0]
    t = O.swish(F.conv2d(x, w_exp.view(mid, -1, 1, 1)) * s0.view(1, -1, 1, 1) + b0.view(1, -1, 1, 1))
    return O.swish(O.same_conv(t, w_dw.view(mid, 1, k, k), k, stride, 224, circular, groups=mid) * s1.view(1, -1, 1, 1) + b1.view(1, -1, 1, 1))


def band_accum_term(inputs, k, stride, circular, samples=2):
    """A = 4 x max |float32 CPU chain - float64 chain| on the first `samples` images (a maximum over fewer elements is never
    larger, so using a part of a large batch only tightens the tolerance).  Returns (A, that error relative to the maximum,
    the float64 CPU chain of those images)."""
    cpu = [t.cpu() for t in inputs]
    cpu[0] = cpu[0][:samples]
    f32 = band_f32_cpu_chain(*cpu, k, stride, circular)
    f64 = band_chain(*cpu, k, stride, circular, torch.float64)
    err = (f32.double() - f64).abs().max().item()
    return 4.0 * err, err / (f64.abs().max().item() + 1e-30), f64


def bf16_ulp(t):
    """spacing of bf16 at the magnitude of t (8 significand bits; subnormals never occur at these magnitudes)"""
    m = t.abs().double().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(m)) - 7)


def band_check(got_nchw, ref64, accum, what):
    """|y_i - ref_i| <= 2^-8 |ref_i| + A for every element, and the 1e-2-of-scale bar; returns max err / tol.  `got` and `ref64`
    may live on the GPU (large rows)."""
    got, ref = got_nchw.detach().double(), ref64
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: non-finite output" % what
    err = (got - ref).abs()
    ratio = err / (2.0 ** -8 * ref.abs() + accum)
    worst = ratio.max().item()
    scale = ref.abs().max().item() + 1e-30
    print("%s: max err/tol %.3f (A = %.2e), max err %.3e = %.2e of scale" % (what, worst, accum, err.max().item(), err.max().item() / scale))
    if worst > 1.0:
        i = ratio.flatten().argmax().item()
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
        raise AssertionError("%s: %d elements outside the elementwise tolerance; worst at (b, channel, y, x) = %s (16-channel slice %d): "
                             "got %.9g want %.9g = %.2f x tol" % (what, int((ratio > 1.0).sum()), idx, idx[1] // 16, got[idx].item(),
                                                                  ref[idx].item(), worst))
    assert err.max().item() <= 1e-2 * scale, "%s: max err %.3e above 1e-2 of scale" % (what, err.max().item())
    return worst


def band_pair_check(a, b, accum, what):
    """band kernel vs slice-per-workgroup kernel: one bf16 ulp (+ 2A, see the module docstring), every element"""
    a, b = a.detach().double(), b.detach().double()
    tol = bf16_ulp(torch.maximum(a.abs(), b.abs())) + 2.0 * accum
    ratio = (a - b).abs() / tol
    worst = ratio.max().item()
    print("%s: max diff/tol %.3f, %d of %d elements differ" % (what, worst, int((a != b).sum()), a.numel()))
    assert worst <= 1.0, "%s: %d elements differ by more than one bf16 ulp (worst %.2f x)" % (what, int((ratio > 1.0).sum()), worst)
    return worst


@functools.lru_cache(maxsize=None)
def cached_conv_ref(row, bf16):
    a, s, wt, bias = conv_inputs(row, bf16)
    return ConvRef(a, s, wt, bias, row.c0)
