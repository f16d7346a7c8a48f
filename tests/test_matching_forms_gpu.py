"""Every launched form of the rotational matching ALONE against float64, elementwise, on the MI355X.

The rows are tests/matching_kernel_shapes.py: the vector-ALU form of match_kernel at default routing, its tiled matrix-core form
(each row again with ccvpe_set_match_mfma at 0: the vector-ALU NPAD 16 / 24 forms against the same reference), and all 32
instantiations of match_stream_kernel at the three geometries of its gate's floor.  Per row and switch position:
  * ccvpe_match_route must answer exactly what the row claims BEFORE anything is launched;
  * the C ABI is called directly, x with NaN in the columns past C when ldx > C and g in wider NaN-padded rows, scores and dstx
    carved out of larger allocations (offsets that are multiples of 16 bytes), pre-filled with NaN between canary values: every
    element must have been written and be finite, no canary may change, the padding columns must be exactly zero, and two
    launches must give the same bits (fixed summation orders);
  * values by the model of tests/matching_check.py with the addition chains of the form that ran (u = 2^-24):
    scores (d + 1) u S_i + ((d_w + 1)/2 + (d_g + 1)/2 + 4) u |ref_i|, normalised copy ((d_t + 1)/2 + 3) u |ref|, max and tail columns
    their scores' tolerances, + 2^-8 |ref| on bf16 output columns; and the older 2e-5 / 1e-5 / 1e-2 of scale bars.
One line per check is printed (profiles/r18/matching_checks.txt).
"""
import ctypes

import pytest
import torch

import matching_check as C
import matching_kernel_shapes as S

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F32 = torch.float32
CANARY = -768.0            # exact in bf16
GUARD = 1024               # elements on each side: 4 KB / 2 KB, a multiple of 16 bytes


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from ccvpe_amd import _lib, ops
    return _lib.load(), ops, torch.cuda.get_device_properties(0).multi_processor_count


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


def _device_inputs(row, ref):
    """x [B,HW,ldx] in the row's storage type (NaN past column C) and g [B,L+3] (NaN past column L) on the device"""
    hw = row.h * row.w
    xd = torch.full((row.b, hw, row.ldx), float("nan"), dtype=F32)
    xd[:, :, :row.c] = ref.x.permute(0, 2, 3, 1).reshape(row.b, hw, row.c)
    gd = torch.full((row.b, row.l + 3), float("nan"), dtype=F32)
    gd[:, :row.l] = ref.g
    return xd.to(BF if row.bf16 else F32).cuda(), gd.cuda()


def _launch(env, row, xd, gd, what):
    lib, ops, _ = env
    from ccvpe_amd._lib import check
    n, hw = len(row.shifts), row.h * row.w
    ns, nd = row.b * n * hw, row.b * hw * row.ldo
    sbig, sc = _carve(ns, F32)
    dbig, dx = _carve(nd, BF if row.bf16 else F32)
    sh = (ctypes.c_int * n)(*row.shifts)
    fn = lib.ccvpe_match_level_bf16 if row.bf16 else lib.ccvpe_match_level_f32
    check(fn(_ptr(xd), row.ldx, _ptr(gd), gd.stride(0), row.l, sh, n, row.n_max, row.n_tail, row.stride, row.woff, _ptr(sc), _ptr(dx),
             row.ldo, row.b, hw, row.c, ops._stream()), what)
    torch.cuda.synchronize()
    _written(sbig, ns, what + " scores")
    _written(dbig, nd, what + " concat rows")
    return sc.view(row.b, n, hw), dx.view(row.b, hw, row.ldo)


@pytest.mark.parametrize("row", S.rows(), ids=lambda r: r.name)
def test_matching_forms_alone_vs_float64(env, row):
    lib, ops, cus = env
    ref = C.cached_ref(row)
    xd, gd = _device_inputs(row, ref)
    for pos in row.switches:
        claim = row.claims[pos]
        what = "%s switch %d" % (row.name, pos)
        prev = lib.ccvpe_set_match_mfma(pos)
        try:
            assert prev == 2, "another test left the matching switch changed"
            S.assert_route(lib, row, claim, " at switch %d" % pos)
            sc, dx = _launch(env, row, xd, gd, what)
            sc2, dx2 = _launch(env, row, xd, gd, what + ", second launch")
        finally:
            lib.ccvpe_set_match_mfma(prev)
        assert torch.equal(sc, sc2) and torch.equal(dx, dx2), what + ": two launches differ"
        geo = ""
        if claim.form == S.STREAM:                            # at 256 CUs tests/test_matching_route.py holds the rows' run claims
            g = S.stream_geometry(row.b, row.h * row.w, cus)
            geo = " | %d CUs: %d tiles, %d per wave, runs of %d, %d workgroups, last holds %d, boundaries inside runs %s" % ((cus,) + tuple(g))
        res = C.match_check(ref, row, claim, sc, dx.float(), what, cus)
        print("MATCHCHECK | %s | switch %d | %s | d %s | %s%s"
              % (row.name, pos, S.instantiation(row, claim), tuple(S.match_chain(row, claim)),
                 ", ".join("%s err/tol %.3f err/scale %.2e" % t for t in res), geo))
