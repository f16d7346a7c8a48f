"""Float64 reference and elementwise error model for conv_wgrad_kernel (csrc/conv_wgrad.hip) and its merge
(sum_parts_lanes_kernel, csrc/common.h), the seeded inputs of tests/wgrad_kernel_shapes.py's rows, and a float32 emulation of the
kernel's split schedule that takes one injected fault at a time.

Shared by tests/test_wgrad_forms_gpu.py (the kernels, on the MI355X) and tests/test_wgrad_check.py (CPU: torch's own float32 result
and the emulated schedule must pass, results with one injected fault each must not).

THE REFERENCE.  Float64, per tap, no convolution backend: on the zero-padded input, X_tap[m, c] is the strided window of tap
(ky, kx) flattened over the output pixels m = (b, oy, ox), and
    dW[n, tap, c] = sum_m dY[m, n] X_tap[m, c]      (one matrix product per tap)
    A[n, tap, c]  = sum_m |dY[m, n]| |X_tap[m, c]|
    dbias[n] = sum_m dY[m, n],  Ab[n] = sum_m |dY[m, n]|.
Gated rows: X = u * gate[b, c] formed in float64 from the fp32 operands.

THE INPUTS.  Seeded per row with ccvpe_amd.synth.  Every float the kernel must not use is NaN: channels c0 .. ld0 of a wider source
row and columns N .. ldy of dY.  The kernel's masks are bitwise ANDs and output rows >= N are never stored (a matrix instruction's
output row depends on its own operand row only), so a correct kernel returns finite values; no poisoned value enters an
instruction whose result is stored.  Input channel 1 and dY column 2 are zero: those elements have A_i = 0 and must come out as
exactly 0.

THE MODEL, elementwise.  u = 2^-24, d = pps + S:
    |got_i - ref_i| <= d u A_i,    and A_i = 0 -> got_i = 0 exactly.
A term passes through at most pps accumulations inside its split (a matrix instruction's k products counted as k sequential fused
multiply-adds, one rounding each) and at most S additions in the merge; the gate product of the gated form is one more rounding,
covered because the first accumulation of a split and the first addition of the merge add to zero and are exact.  The bias gradient
passes through pps / 32 additions in a staging thread, 32 in the workgroup's fixed-order sum and the merge: the same d bounds it
for pps >= 64.  d <= M + S is asserted.  Nothing here is tuned to what the kernel gives.
The suite's older bar stays as a second condition: max error <= 2e-4 of the tensor's maximum.  Every element is compared.
"""
import functools

import torch

from ccvpe_amd import synth

import wgrad_kernel_shapes as S

U = 2.0 ** -24
OLD_BAR = 2e-4
SENTINEL = -768.0          # what dW / dbias hold before a launch: finite, so that an unwritten element fails the value check


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
def inputs(row, device=None):
    """(x0 [B,H,W,ld0], x1 [B,H,W,c1] or None, dy [B,Ho,Wo,ldy], gate [B,c0] or None) float32 on `device` (the same bits as on the
    CPU: synth's hash is integer arithmetic), with the unused floats poisoned"""
    ho, wo, _, _, _, _ = S.dims(row)
    seed = 9000 + 37 * row.num
    x0 = synth.normal((row.b, row.h, row.w, row.ld0), seed, device=device)
    x0[..., 1] = 0.0
    x0[..., row.c0:] = float("nan")
    x1 = synth.normal((row.b, row.h, row.w, row.c1), seed + 1, device=device) if row.c1 else None
    dy = synth.normal((row.b, ho, wo, row.ldy), seed + 2, device=device)
    dy[..., 2] = 0.0
    dy[..., row.n:] = float("nan")
    gate = synth.uniform((row.b, row.c0), seed + 3, 0.05, 1.0, device=device) if row.kind == "gated" else None
    return x0, x1, dy, gate


def used(row, x0, x1, dy, gate, dtype):
    """(X [B,H,W,ctot], dY [M,N]) in `dtype`: the floats the kernel may use, sources concatenated, the gate applied"""
    x = x0[..., :row.c0].to(dtype)
    if gate is not None:
        x = x * gate.to(dtype).view(row.b, 1, 1, row.c0)
    if x1 is not None:
        x = torch.cat([x, x1.to(dtype)], dim=-1)
    return x, dy[..., :row.n].to(dtype).reshape(-1, row.n)


def tap_columns(row, x, clamp_tap=None):
    """X_tap [M, ctot] for every tap in turn, from x [B,H,W,ctot] on the zero-padded plane.  clamp_tap = (ky, kx): that tap reads
    the nearest valid pixel where it should read padding (fault injection: a clamped address without its mask)."""
    ho, wo, m, ctot, taps, _ = S.dims(row)
    p, st = row.pad, row.stride
    xp = torch.nn.functional.pad(x, [0, 0, p, p, p, p])
    xc = torch.nn.functional.pad(x.permute(0, 3, 1, 2), [p, p, p, p], mode="replicate").permute(0, 2, 3, 1) if p else x
    for ky in range(row.k):
        for kx in range(row.k):
            src = xc if clamp_tap == (ky, kx) else xp
            yield src[:, ky:ky + (ho - 1) * st + 1:st, kx:kx + (wo - 1) * st + 1:st, :].reshape(m, ctot)


class WgRef:
    """float64 reference of one row: dW [N, taps, ctot] and A, dbias [N] and Ab, d, and the CPU copies of the inputs"""

    def __init__(self, row, device=None):
        self.row = row
        self.inputs = tuple(None if t is None else t.cpu() for t in inputs(row, device))
        _, _, m, _, _, _ = S.dims(row)
        x, dy = used(row, *self.inputs, torch.float64)
        dyt, dyt_abs = dy.t().contiguous(), dy.abs().t().contiguous()
        taps = [(dyt @ xt, dyt_abs @ xt.abs()) for xt in tap_columns(row, x)]          # one matrix product per tap
        self.dw = torch.stack([t[0] for t in taps], dim=1)
        self.a_dw = torch.stack([t[1] for t in taps], dim=1)
        self.db, self.a_db = dy.sum(0), dy.abs().sum(0)
        pl = S.plan(row)
        self.d = pl.pps + pl.s
        assert self.d <= m + pl.s, (row.name, self.d, m, pl.s)


@functools.lru_cache(maxsize=4)
def cached_ref(row, device=None):
    return WgRef(row, device)


# ------------------------------------------------------------------------------------------------------------------------------
# the comparison
# ------------------------------------------------------------------------------------------------------------------------------
def old_rule_passes(got, ref):
    """the rule the operator tests use: max error relative to the tensor's maximum"""
    got, ref = got.detach().cpu().double(), ref.double()
    return (got - ref).abs().max().item() <= OLD_BAR * (ref.abs().max().item() + 1e-30)


def wg_check(got, ref, a, d, what):
    """|got_i - ref_i| <= d u A_i for every element (A_i = 0: exact), and max error <= 2e-4 of the tensor's maximum.  Returns
    (max_i err_i / tol_i, max error relative to scale); prints them."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: %d non-finite elements" % (what, int((~torch.isfinite(got)).sum()))
    err = (got - ref).abs()
    tol = d * U * a
    ratio = err / tol.clamp_min(1e-300)
    worst = ratio.max().item()
    scale = ref.abs().max().item() + 1e-30
    rel = err.max().item() / scale
    print("%s: max err/tol %.3g (d = %d), max err %.3e = %.2e of scale" % (what, worst, d, err.max().item(), rel))
    if worst > 1.0:
        i = ratio.flatten().argmax().item()
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
        raise AssertionError("%s: %d elements outside the elementwise tolerance; worst at (n, tap, c) = %s: got %.9g want %.9g, "
                             "err %.3e = %.3g x tol" % (what, int((ratio > 1.0).sum()), idx, got[idx].item(), ref[idx].item(),
                                                        err[idx].item(), worst))
    assert rel <= OLD_BAR, "%s: max err %.3e above %.0e of scale %.3e" % (what, err.max().item(), OLD_BAR, scale)
    return worst, rel


# ------------------------------------------------------------------------------------------------------------------------------
# float32 results on the CPU: torch's own, and the kernel's schedule emulated
# ------------------------------------------------------------------------------------------------------------------------------
def torch_f32(row, x0, x1, dy, gate):
    """(dW [N, taps, ctot], dbias [N]) from torch's float32 convolution backward"""
    x, dy2 = used(row, x0, x1, dy, gate, torch.float32)
    ho, wo, _, ctot, taps, _ = S.dims(row)
    g = dy2.reshape(row.b, ho, wo, row.n).permute(0, 3, 1, 2)
    dw = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2), (row.n, ctot, row.k, row.k), g, stride=row.stride, padding=row.pad)
    return dw.permute(0, 2, 3, 1).reshape(row.n, taps, ctot), dy2.sum(0)


def _fma(acc, a, b):
    """fp32 fused multiply-add: the product of two fp32 numbers is exact in float64"""
    return (acc.double() + a.double() * b.double()).float()


def merge_f32(part, ln):
    """sum_parts_lanes_kernel<LN> on part [S, ...]: lane q adds partials q, q + 2 LN, .. into a0 and q + LN, q + 3 LN, .. into a1,
    then a0 + a1, then the LN lane sums in order"""
    nparts = part.shape[0]
    lanes = []
    for q in range(ln):
        a0, a1 = torch.zeros_like(part[0]), torch.zeros_like(part[0])
        k = q
        while k + ln < nparts:
            a0 = a0 + part[k]
            a1 = a1 + part[k + ln]
            k += 2 * ln
        if k < nparts:
            a0 = a0 + part[k]
        lanes.append(a0 + a1)
    out = lanes[0]
    for q in range(1, ln):
        out = out + lanes[q]
    return out


def schedule_f32(dy, xcols, s, pps, drop_last_pixel=False, recount_last_pixel=False):
    """the kernel's partials in float32: dy [M, N], xcols [M, ncols] -> (part [S, N, ncols], bias_part [S, N]).  Split k owns pixels
    k pps .. min((k + 1) pps, M) and adds them in pixel order, one fused multiply-add per (pixel, element); empty splits give
    zeros.  The bias partial is what the first column tile computes: staging row r adds pixels r, r + 32, .. of the split, then the
    32 rows are added in order.
    Faults: drop_last_pixel — pixel M - 1 is left out; recount_last_pixel — the rows behind pixel M - 1 in the last stage are
    not zeroed: one of them (reading the clamped address) adds pixel M - 1 again."""
    m, n = dy.shape
    ncols = xcols.shape[1]
    pad = s * pps + S.WG_BP - m
    keep = torch.ones(m, dtype=torch.bool)
    if drop_last_pixel:
        keep[m - 1] = False
    dyp = torch.cat([dy * keep.view(-1, 1), torch.zeros(pad, n)])
    xp = torch.cat([xcols, torch.zeros(pad, ncols)])
    if recount_last_pixel:
        dyp[m], xp[m] = dy[m - 1], xcols[m - 1]
    dys, xs = dyp[:s * pps].view(s, pps, n), xp[:s * pps].view(s, pps, ncols)
    part = torch.zeros(s, n, ncols)
    for j in range(pps):
        part = _fma(part, dys[:, j, :, None], xs[:, j, None, :])
    rows_ = torch.zeros(s, S.WG_BP, n)
    for st in range(pps // S.WG_BP):
        rows_ = rows_ + dys[:, st * S.WG_BP:(st + 1) * S.WG_BP]
    bias_part = torch.zeros(s, n)
    for r in range(S.WG_BP):
        bias_part = bias_part + rows_[:, r]
    return part, bias_part


def emulate_f32(row, x0, x1, dy, gate, s=None, pps=None, xcols_fault=None, part_fault=None, **faults):
    """(dW [N, taps, ctot], dbias [N]) by the kernel's schedule in float32 (s, pps: another split geometry than the row's own).
    xcols_fault(xcols [M, taps, ctot]) and part_fault(part, bias_part) may alter the staged columns and the partials."""
    pl = S.plan(row)
    s, pps = s or pl.s, pps or pl.pps
    _, _, m, ctot, taps, ncols = S.dims(row)
    x, dy2 = used(row, x0, x1, dy, gate, torch.float32)
    xcols = torch.stack(list(tap_columns(row, x, faults.pop("clamp_tap", None))), dim=1)            # [M, taps, ctot]
    if xcols_fault is not None:
        xcols = xcols_fault(xcols)
    part, bias_part = schedule_f32(dy2, xcols.reshape(m, ncols), s, pps, **faults)
    if part_fault is not None:
        part, bias_part = part_fault(part, bias_part)
    dw = merge_f32(part, S.merge_lanes(part.shape[0], row.n * ncols))
    return dw.view(row.n, taps, ctot), merge_f32(bias_part, S.merge_lanes(bias_part.shape[0], row.n))
