"""Every launched form of the depthwise kernels ALONE against float64, elementwise, on the MI355X.

The rows are tests/depthwise_kernel_shapes.py: the strip kernel (dwconv_kernel) at every geometry edge of its launcher, the plane
kernels (dwconv_plane_kernel, and mbconv_plane_kernel's depthwise-only form where the fused entry points prefer it) at the model's
late-block shapes and at the shapes the band geometry refuses.  Per row:
  * RAW fp32 (ccvpe_dwconv_raw_f32: what the training step launches), fused fp32 and bf16 (ccvpe_dwconv_f32 / _bf16: BN + swish +
    squeeze partials); plane rows with ccvpe_set_mbconv_plane_kernels at its default and at 0 (dwconv_plane_kernel);
  * the C ABI is called directly with y and se_partial carved out of larger allocations (offsets that are multiples of 16 bytes),
    pre-filled with NaN between canary values: every output element and partial row must have been written and be finite, no
    canary may change, two launches must give the same bits (fixed summation orders);
  * values and squeeze sums by the model of tests/depthwise_check.py (u = 2^-24, K = k^2): RAW |err_i| <= K u S_i; fused
    1.1 (K + 2) u (|sc| S_i + |sh|) + (6 + 2 |z_i|) u |ref_i|, + 2^-8 |ref_i| in bf16 storage; sums: the summed tolerances
    + d u sum |ref_i| with d the kernel's longest addition chain; and the older 1e-4 / 1e-2 of scale bars;
  * the input gradient bw.dwconv_dgrad: stride 1 with the row's shape as the gradient (the forward entry with reversed taps),
    stride 2 dw_dgrad_kernel, against float64 autograd of the reference within K u S'_j.
One line per check is printed (profiles/r15/depthwise_checks.txt).
"""
import ctypes

import pytest
import torch

import depthwise_check as C
import depthwise_kernel_shapes as S

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F32 = torch.float32
CANARY = -768.0            # exact in bf16
GUARD = 1024               # elements on each side: 4 KB / 2 KB, a multiple of 16 bytes


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from ccvpe_amd import _lib, backward, ops
    return _lib.load(), ops, backward


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _carve(n, dtype):
    """(the whole allocation, its n-element window): canaries around, NaN inside"""
    big = torch.full((n + 2 * GUARD,), CANARY, dtype=dtype, device="cuda")
    win = big[GUARD:GUARD + n]
    win.fill_(float("nan"))
    assert win.data_ptr() % 16 == 0
    return big, win


def _written(big, n, what):
    assert bool((big[:GUARD] == CANARY).all()) and bool((big[GUARD + n:] == CANARY).all()), what + ": wrote outside its buffer"
    assert bool(torch.isfinite(big[GUARD:GUARD + n].float()).all()), what + ": elements left unwritten or non-finite"


def _launch(env, row, form, xd, wp, sc, sh, nblk):
    """one launch through the C ABI; form: "raw" | "f32" | "bf16".  Returns (y [B,Ho,Wo,C], partial rows [B,nblk,C] or None)."""
    lib, ops, _ = env
    from ccvpe_amd._lib import check
    g = row.geo
    ny = row.b * g.ho * g.wo * row.c
    ybig, y = _carve(ny, BF if form == "bf16" else F32)
    tail = (row.b, row.h, row.w, row.c, row.k, row.s, int(row.circ), ops._stream())
    what = "%s %s" % (form, row.name)
    if form == "raw":
        check(lib.ccvpe_dwconv_raw_f32(_ptr(xd), _ptr(wp), _ptr(y), *tail), what)
        torch.cuda.synchronize()
        _written(ybig, ny, what)
        return y.view(row.b, g.ho, g.wo, row.c), None
    npart = row.b * nblk * row.c
    pbig, part = _carve(npart, F32)
    fn = lib.ccvpe_dwconv_bf16 if form == "bf16" else lib.ccvpe_dwconv_f32
    check(fn(_ptr(xd), _ptr(wp), _ptr(sc), _ptr(sh), _ptr(y), _ptr(part), *tail), what)
    torch.cuda.synchronize()
    _written(ybig, ny, what)
    _written(pbig, npart, what + " squeeze partials")
    return y.view(row.b, g.ho, g.wo, row.c), part.view(row.b, nblk, row.c)


def _twice(env, row, form, *args):
    y, part = _launch(env, row, form, *args)
    y2, part2 = _launch(env, row, form, *args)
    assert torch.equal(y, y2), "%s %s: two runs differ" % (form, row.name)
    assert part is None or torch.equal(part, part2), "%s %s: squeeze partials of two runs differ" % (form, row.name)
    return y, part


def _record(row, form, kernel, ratios):
    g = S.geometry(row.h, row.w, row.c, row.k, row.s)
    geo = ("ychunks %d cgx %d P %d strips %d groups %d RB %d nblk %d" % g[2:]) if row.family == "strip" else "plane"
    print("DWCHECK | %s | B %d | %s | %s | %s | Ho %d Wo %d %s"
          % (row.name, row.b, form, kernel, ", ".join("%s err/tol %.3f err/scale %.2e" % (n, r[0], r[1]) for n, r in ratios), g.ho, g.wo, geo))


def _fused(env, row, mode_name, kernel, nblk, chain, keep):
    """both storage types of the fused form at the current switch position"""
    for bf16 in (False, True):
        dr = C.cached_ref(row, bf16)
        x, wt, sc, sh = dr.inputs
        dt = BF if bf16 else F32
        form = "bf16" if bf16 else "f32"
        xd = nhwc(x).to(dt).cuda()
        wp = wt.permute(1, 2, 0).reshape(row.k * row.k, row.c).contiguous().cuda()
        y, part = _twice(env, row, form, xd, wp, sc.cuda(), sh.cuda(), nblk)
        assert part.shape[1] == nblk
        what = "fused %s %s%s" % (form, row.name, mode_name)
        d = chain(bf16)
        rv = C.dw_check(nchw(y.float()), dr.ref, dr.tol_bf16 if bf16 else dr.tol_fused, 1e-2 if bf16 else 1e-4, what)
        rs = C.sum_check(part, dr, d, 1e-2 if bf16 else 1e-4, what + " squeeze sums")
        _record(row, "fused %s%s" % (form, mode_name), kernel + " d=%d" % d, (("y", rv), ("sums", rs)))
        keep[form] = (y, part)


@pytest.mark.parametrize("row", S.rows(), ids=lambda r: r.name)
def test_depthwise_forms_alone_vs_float64(env, row):
    lib, ops, bw = env
    geo = S.geometry(row.h, row.w, row.c, row.k, row.s)
    assert geo == row.geo, (row.name, geo)
    strip = row.family == "strip"
    fwd = "dwconv_kernel" if strip else "dwconv_plane_kernel"
    tag = "<%d,%d>" % (row.k, row.s)
    dr = C.cached_ref(row, False)
    x, wt, sc, sh = dr.inputs
    xd = nhwc(x).cuda()
    wp = wt.permute(1, 2, 0).reshape(row.k * row.k, row.c).contiguous().cuda()

    # ---- RAW fp32: the training step's launch -----------------------------------------------------------------------------
    y, _ = _twice(env, row, "raw", xd, wp, None, None, 0)
    rv = C.dw_check(nchw(y), dr.conv, dr.tol_raw, 1e-4, "raw " + row.name)
    _record(row, "raw f32", fwd + tag + " RAW", (("y", rv),))

    # ---- fused fp32 / bf16 -------------------------------------------------------------------------------------------------
    if strip:
        nblk = lib.ccvpe_dwconv_nblk(row.h, row.w, row.c, row.s)
        assert nblk == row.geo.nblk, row.name
        _fused(env, row, "", fwd + tag, nblk, lambda bf16: S.strip_chain(geo), {})
    else:
        refused = row.name in S.PLANE_REFUSED
        kept = {}
        for mode in (7, 0):                                   # 7: the default (test_launch_state_gpu.py); 0: dwconv_plane_kernel
            prev = lib.ccvpe_set_mbconv_plane_kernels(mode)
            try:
                assert prev == 7, "another test left the MBConv plane kernel switch changed"
                nblk = lib.ccvpe_dwconv_nblk(row.h, row.w, row.c, row.s)
                assert nblk == (row.bands if mode else 1), (row.name, mode, nblk)
                band_form = mode == 7 and not refused
                kernel = ("mbconv_plane_kernel" if band_form else "dwconv_plane_kernel") + tag
                chain = ((lambda bf16: S.band_chain(row.h, row.w, row.c, geo.ho, geo.wo, row.s, row.bands)) if band_form
                         else (lambda bf16: S.plane_chain(geo.ho, geo.wo, bf16)))
                kept[mode] = {}
                _fused(env, row, " switch %d" % mode, kernel, nblk, chain, kept[mode])
            finally:
                lib.ccvpe_set_mbconv_plane_kernels(prev)
        if refused:                                           # the same kernel at both switch positions
            for form in ("f32", "bf16"):
                assert torch.equal(kept[7][form][0], kept[0][form][0]) and torch.equal(kept[7][form][1], kept[0][form][1]), \
                    "%s %s: the switch changed the result of a shape the band geometry refuses" % (form, row.name)

    # ---- input gradient ----------------------------------------------------------------------------------------------------
    dy = C.grad_input(row)
    want, tol = dr.grad(dy)
    dyd = nhwc(dy).cuda()
    got = bw.dwconv_dgrad(dyd, wp, row.h, row.w, row.k, row.s, row.circ)
    again = bw.dwconv_dgrad(dyd, wp, row.h, row.w, row.k, row.s, row.circ)
    torch.cuda.synchronize()
    assert torch.equal(got, again), row.name + ": two input-gradient runs differ"
    rg = C.dw_check(nchw(got), want, tol, 1e-4, "input gradient " + row.name)
    _record(row, "input gradient", ("dw_dgrad_kernel" + tag) if row.s == 2 else (fwd + "<%d,1> RAW, reversed taps" % row.k), (("dx", rg),))
