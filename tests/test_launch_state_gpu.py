"""Launch state that the driver keeps per device (csrc/common.h: ensure_dyn_lds over csrc/dev_cache.h) and the band kernel's
fallback without a sentinel value (csrc/mbconv_plane.hip: mbband_launch's `taken`), on the MI355X.  A wrong "already covered"
answer of the cache shows as a launch error (CCVPE_ELAUNCH raised as CcvpeError), never as a fault."""
import pytest
import torch
import torch.nn.functional as F

import forward_kernel_shapes as S
import forward_variant_check as V
from ccvpe_amd import synth
from oracle import ccvpe_oracle as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def dev(t):
    return t.cuda().contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def close(got, want, tol, what):
    """the rule of tests/test_ops_gpu.py: largest error relative to the reference's largest magnitude"""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = want.abs().max().item() + 1e-30
    err = (got - want).abs().max().item()
    assert err <= tol * scale, "%s: max err %.3e vs scale %.3e (rel %.3e)" % (what, err, scale, err / scale)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from ccvpe_amd import ops as _ops, _lib
    _lib.load()
    return _ops


def _match_lds_bytes(C, n_shifts):
    """dynamic LDS of match_kernel<float, NPAD, full window, VEC, vector-ALU form> (csrc/matching.hip: launch_match)"""
    lpp = 1
    while lpp < 32 and C > 24 * lpp:
        lpp *= 2
    assert lpp >= 16                      # any pitch works: S = C + 4
    tp = 256 // lpp
    return 4 * (2 * C + tp * (C + 4) + n_shifts * tp + 2 * tp + 4)


def test_dynamic_lds_grows_to_the_largest_request_on_one_device(ops):
    """One instantiation of launch_match (fp32, one hypothesis, 16-byte reads) asked for 26 KB, then 82 KB, then 26 KB again: the
    opt-in is raised for the second call and still covers the third.  Batch 2, one pixel; every result against float64 at the
    tolerances of tests/test_ops_gpu.py::test_match_level."""
    small, large = 640, 2048
    assert _match_lds_bytes(small, 1) < 48 * 1024 and _match_lds_bytes(large, 1) > 64 * 1024
    ref = {}
    for C in (small, large, small):
        stride = C // 16
        x = synth.normal((2, C, 1, 1), 70 + C)
        g = synth.normal((2, C + 5), 71 + C)          # wider row: exercises ldg
        ldo = (C + 1 + 7) // 8 * 8
        sc, cat = ops.match_level(dev(nhwc(x)), dev(g)[:, :C], C, [0], 1, 0, stride, ldo)
        torch.cuda.synchronize()
        if C not in ref:
            ref[C] = (O.rotational_matching(x.double(), g[:, :C].double(), [0], stride), F.normalize(x.double(), p=2, dim=1))
        want, xn = ref[C]
        close(sc, want, 2e-5, "scores C = %d" % C)
        catc = nchw(cat).cpu()
        close(catc[:, :C], xn, 1e-5, "normalised features C = %d" % C)
        close(catc[:, C], want[:, :1].max(dim=1)[0], 2e-5, "max over rotations C = %d" % C)
        assert (catc[:, C + 1:] == 0).all()


def _front(ops, row, inp):
    from ccvpe_amd.models import _pack_conv
    x, w_exp, s0, b0, w_dw, s1, b1 = inp
    mid = 6 * row.cin
    wp = _pack_conv(w_exp.cpu().view(mid, row.cin, 1, 1), BF).cuda()
    y, part = ops.mbconv_front(nhwc(x).to(BF), wp, s0, b0, w_dw.permute(1, 2, 0).contiguous(), s1, b1, mid, row.k, row.s, row.circ)
    torch.cuda.synchronize()
    return y, part


def _band_off(ops, lib, row, inp):
    prev = lib.ccvpe_set_mbconv_plane_kernels(3)
    try:
        assert lib.ccvpe_mbconv_front_route(row.h, row.w, row.cin, 6 * row.cin, row.k, row.s, 1, row.b) == 2
        return _front(ops, row, inp)
    finally:
        lib.ccvpe_set_mbconv_plane_kernels(prev)


def test_band_kernel_fallback_and_band_kernel_still_taken(ops):
    """bf16 storage, band kernel switched on (mode bit 4).  17 x 17 x 80, k = 3, stride 2 is inside the plane geometry but
    refused by mbband_plan outright: the route says plane kernel, the call returns CCVPE_OK (ops raises otherwise) and its output
    is bit-identical to the same call with the band kernel switched off.  The smallest band row at B = 1 still reaches the band
    kernel, and both are checked against the float64 chain (tests/forward_variant_check.py: band_check)."""
    from ccvpe_amd import _lib
    lib = _lib.load()
    assert lib.ccvpe_set_mbconv_plane_kernels(7) == 7, "another test left the band kernel switched off"
    fb = S.BandRow("17 x 17 x 80 k3 stride 2: refused by the band plan", 1, 17, 17, 80, 3, 2, False, None, 0, 0, 0, False)
    mid = 6 * fb.cin
    assert lib.ccvpe_mbconv_front_nblk(fb.h, fb.w, fb.cin, mid, fb.k, fb.s) > 0
    assert lib.ccvpe_mbconv_front_route(fb.h, fb.w, fb.cin, mid, fb.k, fb.s, 1, fb.b) == 2, "not band"
    assert ops.mbconv_band_plan(fb.h, fb.w, fb.cin, mid, fb.k, fb.s, fb.b) is None
    inp = V.band_inputs(fb, device="cuda")
    y, part = _front(ops, fb, inp)
    y_off, part_off = _band_off(ops, lib, fb, inp)
    assert torch.equal(y, y_off) and torch.equal(part, part_off), "the fallback differs from the plane kernel called directly"
    accum, _, _ = V.band_accum_term(inp, fb.k, fb.s, fb.circ, samples=1)
    V.band_check(nchw(y.float()), V.band_chain(*inp, fb.k, fb.s, fb.circ, torch.float64), accum, fb.name)

    row = min(S.BAND, key=lambda r: r.h * r.w * r.cin)._replace(b=1)
    mid = 6 * row.cin
    assert lib.ccvpe_mbconv_front_route(row.h, row.w, row.cin, mid, row.k, row.s, 1, 1) == 3, row.name
    plan = ops.mbconv_band_plan(row.h, row.w, row.cin, mid, row.k, row.s, 1)
    assert plan is not None and (row.k, row.s, plan["nkk"], plan["tpw"], plan["ry"]) == row.inst, (row.name, plan)
    inp = V.band_inputs(row, device="cuda")
    y, part = _front(ops, row, inp)
    accum, _, _ = V.band_accum_term(inp, row.k, row.s, row.circ, samples=1)
    V.band_check(nchw(y.float()), V.band_chain(*inp, row.k, row.s, row.circ, torch.float64), accum, "band, B = 1: " + row.name)
    y_off, _ = _band_off(ops, lib, row, inp)
    V.band_pair_check(y.float(), y_off.float(), accum, "band vs slice kernel, B = 1: " + row.name)


def test_dynamic_lds_opt_in_on_a_second_device(ops):
    """stem_dw_kernel always needs the opt-in.  Device 0 first, then device 1, each on its own current stream, at the smallest
    image the entry point accepts: a process-wide "already set" flag skips the driver call on device 1 and the launch fails
    there with CCVPE_ELAUNCH.  Same inputs, so the two outputs must agree bit for bit."""
    if torch.cuda.device_count() < 2:
        pytest.skip("one visible device: the per-device property rests on tests/test_dev_cache.py")
    assert ops.stem_dw_supported(3, 3, False) > 0
    x = synth.normal((1, 3, 3, 3), 4400)
    wt = synth.normal((32, 3, 3, 3), 4401, (1.0 / 27) ** 0.5).permute(2, 3, 1, 0).contiguous()
    s0, b0 = synth.uniform((32,), 4402, 0.5, 1.5), synth.normal((32,), 4403, 0.1)
    wd = synth.normal((32, 1, 3, 3), 4404, 1.0 / 3).reshape(32, 3, 3).permute(1, 2, 0).contiguous()
    s1, b1 = synth.uniform((32,), 4405, 0.5, 1.5), synth.normal((32,), 4406, 0.1)
    outs = []
    for d in (0, 1):
        with torch.cuda.device(d):
            args = [t.to("cuda:%d" % d) for t in (x, wt, s0, b0, wd, s1, b1)]
            y, part = ops.stem_dw(*args, False)
            torch.cuda.synchronize()
            outs.append((y.cpu(), part.cpu()))
    assert torch.isfinite(outs[0][0]).all() and outs[0][0].abs().max() > 0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "device 0 and device 1 differ"
