"""Every launched form of conv_wgrad_kernel ALONE against float64, elementwise, on the MI355X.

The rows are tests/wgrad_kernel_shapes.py: the six plain tiles and the five gated ones of the traced training step, at pixel splits
that end mid-stage, empty trailing splits, column tiles that span taps and sources, ragged row tiles, strided taps, the deconv's
swapped roles, grids that are no multiple of 8 and every lane count of the merge kernel.  Per row:
  * before the launch the tile (ccvpe_conv_wgrad_tile) and the split count (ccvpe_conv_wgrad_scratch_floats) are asserted;
  * the C ABI is called directly — the plain and the bias-fused entry (rows 1-13, 20-23) or the gated one (rows 14-19) — with the
    scratch buffer pre-filled with NaN and dW / dbias with a sentinel, each carved out of a larger allocation between canary
    values: every partial must have been written and be finite, the partials of empty splits must be zero, the bias partials must
    be untouched where no bias was asked for, no canary may change, and two launches must give the same bits;
  * every element of dW and dbias against float64 by the model of tests/wgrad_check.py: |err_i| <= (pps + S) u A_i, u = 2^-24,
    exactly 0 where A_i = 0, and the older 2e-4 of scale bar;
  * the public wrappers (backward.conv_wgrad with and without the bias, deconv_wgrad, conv1x1_wgrad_gated) give the same bits.
Inputs are generated on the device (the same bits as on the CPU) and the float64 reference is computed on the CPU.
One line per row is printed (profiles/r30/wgrad_checks.txt).
"""
import ctypes

import pytest
import torch

import wgrad_check as C
import wgrad_kernel_shapes as S

pytestmark = pytest.mark.gpu
CANARY = 1234.5
GUARD = 1024               # floats on each side: 4 KB, a multiple of 16 bytes


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from ccvpe_amd import _lib, backward, ops
    return _lib.load(), ops, backward


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _carve(n, fill):
    """(the whole allocation, its n-float window): canaries around, `fill` inside"""
    big = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.float32, device="cuda")
    win = big[GUARD:GUARD + n]
    win.fill_(fill)
    assert win.data_ptr() % 16 == 0
    return big, win


def _intact(big, n, what):
    assert bool((big[:GUARD] == CANARY).all()) and bool((big[GUARD + n:] == CANARY).all()), what + ": wrote outside its buffer"


def _launch(env, row, dev, entry):
    """one launch through the C ABI; entry: "plain" | "bias" | "gated".  Returns (dW [N, taps, ctot], dbias [N] or None)."""
    lib, ops, _ = env
    from ccvpe_amd._lib import check
    x0, x1, dy, gate = dev
    _, _, _, ctot, taps, ncols = S.dims(row)
    pl = row.plan
    n_dw = row.n * ncols
    what = "%s %s" % (entry, row.name)
    sbig, scratch = _carve(pl.s * (n_dw + row.n), float("nan"))
    wbig, dw = _carve(n_dw, C.SENTINEL)
    bbig, db = _carve(row.n, C.SENTINEL)
    geo = (row.b, row.h, row.w, row.k, row.k, row.stride, row.pad, row.n, ops._stream())
    if entry == "gated":
        check(lib.ccvpe_conv_wgrad_gated_f32(_ptr(x0), row.c0, row.ld0, _ptr(gate), _ptr(dy), row.ldy, _ptr(dw), _ptr(scratch),
                                             row.b, row.h, row.w, row.n, ops._stream()), what)
    elif entry == "bias":
        check(lib.ccvpe_conv_wgrad_bias_f32(_ptr(x0), row.c0, row.ld0, _ptr(x1), row.c1, row.c1, _ptr(dy), row.ldy, _ptr(dw), _ptr(db),
                                            _ptr(scratch), *geo), what)
    else:
        check(lib.ccvpe_conv_wgrad_f32(_ptr(x0), row.c0, row.ld0, _ptr(x1), row.c1, row.c1, _ptr(dy), row.ldy, _ptr(dw),
                                       _ptr(scratch), *geo), what)
    torch.cuda.synchronize()
    for big, n in ((sbig, scratch.numel()), (wbig, n_dw), (bbig, row.n)):
        _intact(big, n, what)
    part = scratch[:pl.s * n_dw].view(pl.s, n_dw)
    bias_part = scratch[pl.s * n_dw:].view(pl.s, row.n)
    assert bool(torch.isfinite(part).all()), what + ": partials left unwritten or non-finite"
    if pl.empty:
        assert bool((part[pl.s - pl.empty:] == 0).all()), what + ": an empty split's partial is not zero"
    if entry == "bias":
        assert bool(torch.isfinite(bias_part).all()), what + ": bias partials left unwritten or non-finite"
        assert not pl.empty or bool((bias_part[pl.s - pl.empty:] == 0).all()), what + ": an empty split's bias partial is not zero"
    else:
        assert bool(torch.isnan(bias_part).all()), what + ": wrote bias partials nobody asked for"
        assert bool((db == C.SENTINEL).all()), what + ": wrote a bias gradient nobody asked for"
    return dw.view(row.n, taps, ctot).clone(), (db.clone() if entry == "bias" else None)


def _twice(env, row, dev, entry):
    dw, db = _launch(env, row, dev, entry)
    dw2, db2 = _launch(env, row, dev, entry)
    assert torch.equal(dw, dw2), "%s %s: two runs differ" % (entry, row.name)
    assert db is None or torch.equal(db, db2), "%s %s: bias gradients of two runs differ" % (entry, row.name)
    return dw, db


def _flat(g, row):
    """a wrapper's OIHW view back to [N, taps, ctot]"""
    _, _, _, ctot, taps, _ = S.dims(row)
    return g.permute(0, 2, 3, 1).reshape(row.n, taps, ctot)


@pytest.mark.parametrize("row", S.rows(), ids=lambda r: r.name)
def test_wgrad_forms_alone_vs_float64(env, row):
    lib, ops, bw = env
    _, _, m, ctot, taps, ncols = S.dims(row)
    pl = S.plan(row)
    assert pl == row.plan, (row.name, pl)
    tile = lib.ccvpe_conv_wgrad_tile(row.n, ncols)
    assert (tile >> 16, tile & 0xffff) == (pl.tile, S.tile_cols(pl.tile)), (row.name, tile >> 16, tile & 0xffff)
    floats = lib.ccvpe_conv_wgrad_scratch_floats(row.b, row.h, row.w, row.k, row.k, row.stride, row.pad, ctot, row.n)
    assert floats // (row.n * ncols + row.n) == pl.s and floats % (row.n * ncols + row.n) == 0, (row.name, floats)

    ref = C.cached_ref(row, "cuda")
    dev = tuple(None if t is None else t.cuda() for t in ref.inputs)
    x0, x1, dy, gate = dev
    gated = row.kind == "gated"
    ratios = []
    if gated:
        dw, _ = _twice(env, row, dev, "gated")
        ratios.append(("dW", C.wg_check(dw, ref.dw, ref.a_dw, ref.d, "gated dW " + row.name)))
        got = bw.conv1x1_wgrad_gated(x0, gate, dy, row.n)
        assert torch.equal(_flat(got, row), dw), row.name + ": backward.conv1x1_wgrad_gated differs from the direct call"
    else:
        dw, _ = _twice(env, row, dev, "plain")
        dwb, db = _twice(env, row, dev, "bias")
        assert torch.equal(dw, dwb), row.name + ": the bias-fused launch changed dW"
        ratios.append(("dW", C.wg_check(dw, ref.dw, ref.a_dw, ref.d, "dW " + row.name)))
        ratios.append(("dbias", C.wg_check(db, ref.db, ref.a_db, ref.d, "dbias " + row.name)))
        if row.kind == "deconv":
            got = bw.deconv_wgrad(dy, x0)
            assert torch.equal(_flat(got, row), dw), row.name + ": backward.deconv_wgrad differs from the direct call"
        else:
            c0 = row.c0 if row.ld0 != row.c0 else None
            got = bw.conv_wgrad(x0, dy, row.n, row.k, row.k, row.stride, row.pad, x1, c0=c0)
            assert torch.equal(_flat(got, row), dw), row.name + ": backward.conv_wgrad differs from the direct call"
            got, gb = bw.conv_wgrad(x0, dy, row.n, row.k, row.k, row.stride, row.pad, x1, c0=c0, want_bias=True)
            assert torch.equal(_flat(got, row), dw) and torch.equal(gb, db), row.name + ": backward.conv_wgrad(want_bias) differs"
    # the zero input channel and the zero dY column: A_i = 0, exactly zero
    assert bool((dw[:, :, 1] == 0).all()) and bool((dw[2] == 0).all()), row.name
    print("WGCHECK | %s | conv_wgrad_kernel<%d,%d%s> | M %d tiles %d x %d S %d pps %d last %d px empty %d grid %% 8 = %d merge LN %d / %d | d = %d | %s"
          % (row.name, pl.tile, S.tile_cols(pl.tile), ",true" if gated else "", m, pl.tiles_n, pl.tiles_c, pl.s, pl.pps, pl.last_px,
             pl.empty, pl.grid_mod8, pl.ln_dw, pl.ln_bias, ref.d,
             ", ".join("%s err/tol %.3f err/scale %.2e" % (nm, r[0], r[1]) for nm, r in ratios)))
