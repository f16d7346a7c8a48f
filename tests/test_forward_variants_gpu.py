"""Every conv3x3_kernel form and every mbconv_band_kernel instantiation of the B = 64 steps, ALONE, against float64, on the MI355X.

The rows are tests/forward_kernel_shapes.py: the smallest shape that still selects each form.  Before every launch the route
(ccvpe_conv_igemm_route / ccvpe_mbconv_front_route) and the form (ccvpe_conv3x3_variant / ccvpe_mbconv_band_plan: the
launchers' own decisions) are asserted, so a row cannot drift onto an easier kernel.

The comparison is ELEMENTWISE, not relative to the tensor's maximum (tests/forward_variant_check.py states the model in full and
tests/test_forward_variant_check.py shows on the CPU that it catches single faults the old rule lets through).  u = 2^-24,
S_i = float64 sum of |a_k w_k| + |bias| of element i, c = 4 x the largest err_i / (u S_i) of torch's own float32 CPU conv of the
same row (computed per row; c <= K, the rigorous any-order ceiling, is asserted):
    fp32, and bf16 storage with out_f32:   |got_i - ref_i| <= c u S_i
    bf16 storage:                          |got_i - ref_i| <= 2^-8 |ref_i| + c u S_i
and the suite's older bars (1e-4 / 1e-2 of the maximum) as a second condition.  Band rows: |y_i - ref_i| <= 2^-8 |ref_i| + A with
A = 4 x the largest error of the float32 CPU chain against float64; band vs slice kernel within one bf16 ulp (+ 2A); squeeze
partials within 2e-3 of scale.  Every element is compared.  The measured ratios are printed (profiles/r09/variant_checks.txt).
"""
import pytest
import torch

import forward_kernel_shapes as S
import forward_variant_check as V

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F32 = torch.float32


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from ccvpe_amd import ops as _ops, _lib
    _lib.load()
    return _ops


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2)


def _run_conv(ops, row, bf16, cr, batch=None):
    """one ConvRow in one type: route and form asserted, then no-activation and ReLU (and, for bf16, ReLU writing fp32), each twice
    (bit-identical), each against the float64 reference `cr`.  Returns the ReLU storage-type result for pair comparisons."""
    from ccvpe_amd.models import _pack_conv
    dt = BF if bf16 else F32
    want = row.bf16 if bf16 else row.f32
    b = batch or row.b
    a, s, wt, bias = V.conv_inputs(row, bf16, b)
    ad, sd = nhwc(a).to(dt).cuda(), nhwc(s).to(dt).cuda()
    wd, bd = _pack_conv(wt, dt).cuda(), bias.cuda()
    kw = dict(batch=b, in_h=row.h, in_w=row.w, kh=3, kw=3, pad=1, src1=sd, c1=row.c1, shift=bd, ld0=row.ld0)
    tag = "%s %s" % ("bf16" if bf16 else "fp32", row.name)
    keep = None
    for act, out_f32 in ((ops.ACT_NONE, False), (ops.ACT_RELU, False)) + (((ops.ACT_RELU, True),) if bf16 else ()):
        k = dict(kw, act=act, out_f32=out_f32)
        assert ops.conv_igemm(ad, row.c0, wd, row.n, route_only=True, **k) == ("conv3x3",) + row.tile, tag
        assert ops.conv_igemm(ad, row.c0, wd, row.n, variant_only=True, **k) == want, tag
        calls = ops.SPLIT_K_CALLS
        got = ops.conv_igemm(ad, row.c0, wd, row.n, **k)
        again = ops.conv_igemm(ad, row.c0, wd, row.n, **k)
        torch.cuda.synchronize()
        assert ops.SPLIT_K_CALLS == calls, tag + ": took the split-K path (generic kernel)"
        assert got.dtype == (F32 if out_f32 or not bf16 else BF)
        assert torch.equal(got, again), tag + ": two runs differ"
        relu = act == ops.ACT_RELU
        V.conv_check(nchw(got.float()), cr, relu, bf16 and not out_f32, bf16,
                     "%s%s%s" % (tag, " relu" if relu else "", " out_f32" if out_f32 else ""))
        if relu and not out_f32:
            keep = got
    return keep


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("row", S.CONV3X3, ids=lambda r: r.name)
def test_conv3x3_form_alone_vs_float64(ops, row, bf16):
    _run_conv(ops, row, bf16, V.cached_conv_ref(row, bf16))


@pytest.mark.parametrize("pair", S.CONV3X3_NW8_PAIRS, ids=lambda p: p[0].name)
def test_conv3x3_eight_wave_threshold_pair_vs_float64(ops, pair):
    """The 8-wave form (twice the pixel tile; fp32: one tap per stage under a 128-VGPR cap, bf16: a row of taps) and the 4-wave form
    of the SAME layer one image below the threshold: both against one float64 reference, and image by image against each other on
    the shared batch prefix (same K order per output element -> the same bits are expected, a bf16 ulp / c u S_i is allowed)."""
    hi, lo = pair
    bf16 = hi.f32 is None
    cr = V.cached_conv_ref(hi, bf16)
    got_hi = _run_conv(ops, hi, bf16, cr)
    got_lo = _run_conv(ops, lo, bf16, cr.prefix(lo.b))
    tol = cr.c * V.U * nhwc(cr.s_abs[:lo.b])
    a, b = got_hi[:lo.b].float().cpu().double(), got_lo.float().cpu().double()
    if bf16:
        tol = tol + V.bf16_ulp(torch.maximum(a.abs(), b.abs()))
    for i in range(lo.b):
        d = (a[i] - b[i]).abs()
        assert bool((d <= tol[i]).all()), "%s: image %d differs between the 8- and 4-wave forms (max %.3e)" % (hi.name, i, d.max().item())
    print("%s: 8-wave vs 4-wave, %d of %d elements differ" % (hi.name, int((a != b).sum()), a.numel()))
    V.cached_conv_ref.cache_clear()                         # the pair references are the large ones: not kept for the session


def _band_launch(ops, row, inp):
    from ccvpe_amd.models import _pack_conv
    x, w_exp, s0, b0, w_dw, s1, b1 = inp
    mid = 6 * row.cin
    xd = nhwc(x).to(BF)
    wp = _pack_conv(w_exp.cpu().view(mid, row.cin, 1, 1), BF).cuda()
    wd = w_dw.permute(1, 2, 0).contiguous()
    y, part = ops.mbconv_front(xd, wp, s0, b0, wd, s1, b1, mid, row.k, row.s, row.circ)
    torch.cuda.synchronize()
    return y, part


@pytest.mark.parametrize("row", S.BAND, ids=lambda r: r.name)
def test_mbconv_band_instantiation_alone_vs_float64(ops, row):
    """The fused bf16 front of the late blocks on the band-owner kernel, with the instantiation (and, on the rows marked deep, at
    least three slices per workgroup: the steady state of the producer / consumer pipeline, most with a short last group) asserted
    from the launcher's own plan.  Inputs are generated on the device (bit-identical to the CPU hash), the float64 chain runs as
    plain tensor operations on the device for the whole batch and on the CPU for the first two samples, where it must agree."""
    from ccvpe_amd import _lib
    lib = _lib.load()
    mid = 6 * row.cin
    assert lib.ccvpe_mbconv_front_route(row.h, row.w, row.cin, mid, row.k, row.s, 1, row.b) == 3, row.name
    plan = ops.mbconv_band_plan(row.h, row.w, row.cin, mid, row.k, row.s, row.b)
    assert plan is not None and (row.k, row.s, plan["nkk"], plan["tpw"], plan["ry"]) == row.inst, (row.name, plan)
    if row.deep:
        assert plan["cpg"] >= 3, (row.name, plan)
    inp = V.band_inputs(row, device="cuda")
    accum, f32_rel, ref_cpu = V.band_accum_term(inp, row.k, row.s, row.circ)
    ref = V.band_chain(*inp, row.k, row.s, row.circ, torch.float64)
    n = ref_cpu.shape[0]
    assert (ref[:n].cpu() - ref_cpu).abs().max().item() <= 1e-12 * ref_cpu.abs().max().item(), "float64 chain: device and CPU disagree"
    y, part = _band_launch(ops, row, inp)
    y2, part2 = _band_launch(ops, row, inp)
    assert y.dtype == BF and torch.equal(y, y2) and torch.equal(part, part2), row.name + ": two runs differ"
    r_band = V.band_check(nchw(y.float()), ref, accum, "band %s (float32 CPU chain: %.2e of scale)" % (row.name, f32_rel))
    sums = ref.sum(dim=(2, 3))
    scale = sums.abs().max().item()
    perr = (part.double().sum(1) - sums).abs().max().item()
    assert perr <= 2e-3 * scale, "%s: squeeze partials off by %.3e of scale" % (row.name, perr / scale)
    prev = lib.ccvpe_set_mbconv_plane_kernels(3)
    try:
        assert lib.ccvpe_mbconv_front_route(row.h, row.w, row.cin, mid, row.k, row.s, 1, row.b) == 2
        assert ops.mbconv_band_plan(row.h, row.w, row.cin, mid, row.k, row.s, row.b) is None
        y1, part1 = _band_launch(ops, row, inp)
    finally:
        lib.ccvpe_set_mbconv_plane_kernels(prev)
    r_slice = V.band_check(nchw(y1.float()), ref, accum, "slice kernel %s" % row.name)
    V.band_pair_check(y.float(), y1.float(), accum, "band vs slice kernel %s" % row.name)
    perr1 = (part1.double() - part.double()).abs().max().item()
    assert perr1 <= 1e-4 * part.abs().max().item(), "%s: squeeze partials, slice vs band kernel" % row.name
    print("%s: plan %s, partials %.2e of scale, band %.3f slice %.3f of tolerance" % (row.name, plan, perr / scale, r_band, r_slice))


def test_band_kernel_refused_for_lds_runs_the_slice_kernel(ops):
    """tests/forward_kernel_shapes.py BAND_LDS_REFUSED: the band kernel's shape test passes, its LDS need does not fit; the route says
    plane kernel and the fused call (which used to be recorded as the band kernel) computes the right values on it."""
    from ccvpe_amd import _lib
    h, w, cin, k, s = S.BAND_LDS_REFUSED
    row = S.BandRow("LDS-refused %d x %d x %d" % (h, w, cin), 3, h, w, cin, k, s, False, None, 0, 0, 0, False)
    assert _lib.load().ccvpe_mbconv_front_route(h, w, cin, 6 * cin, k, s, 1, row.b) == 2
    inp = V.band_inputs(row, device="cuda")
    accum, _, _ = V.band_accum_term(inp, k, s, False)
    y, part = _band_launch(ops, row, inp)
    V.band_check(nchw(y.float()), V.band_chain(*inp, k, s, False, torch.float64), accum, row.name)
