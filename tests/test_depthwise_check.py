"""The depthwise table and its checker, without a GPU.

* every row's restated geometry (tests/depthwise_kernel_shapes.py) equals its expected columns and the launcher's own host-only
  query ccvpe_dwconv_nblk, and the rows' forms cover what the traced training step launches: a routing or geometry change shows up
  here as a stale row;
* torch's own float32 CPU results pass the elementwise comparison of tests/depthwise_check.py on every row (bf16-rounded for the
  bf16 cases): the reference is inside its own bounds;
* with ONE injected fault of the kind a strip / plane kernel makes, the comparison fails — each test prints whether the rule the
  operator tests use (maximum error relative to the tensor's maximum, 1e-4) would have let the fault through.
"""
import pytest
import torch

import depthwise_check as C
import depthwise_kernel_shapes as S

ROWS = S.rows()


def _row(text):
    return next(r for r in ROWS if text in r.name)


def _caught(fn, *args):
    with pytest.raises(AssertionError, match="outside the elementwise tolerance"):
        fn(*args)


def _old(name, got, ref):
    passes = C.old_rule_passes(got, ref, 1e-4)
    print("%s: old rule (1e-4 of scale) %s this fault" % (name, "PASSES" if passes else "fails"))
    return passes


def test_geometry_rows_are_current_and_cover_the_traced_forms():
    from ccvpe_amd import _lib
    lib = _lib.load()
    assert len({r.name for r in ROWS}) == len(ROWS)
    for r in ROWS:
        assert S.use_plane(r.h, r.w, r.c) == (r.family == "plane"), r.name
        assert S.geometry(r.h, r.w, r.c, r.k, r.s) == r.geo, (r.name, S.geometry(r.h, r.w, r.c, r.k, r.s))
        assert lib.ccvpe_dwconv_nblk(r.h, r.w, r.c, r.s) == (r.geo.nblk if r.family == "strip" else r.bands), r.name
        assert r.b in (2, 3) and 4 * r.b * r.c * r.h * r.w < 10e6, r.name
        if r.name in S.PLANE_REFUSED:
            assert r.bands == 1, r.name
    prev = lib.ccvpe_set_mbconv_plane_kernels(0)               # the round-5 chain: every plane row is one dwconv_plane_kernel row
    try:
        for r in S.PLANE:
            assert lib.ccvpe_dwconv_nblk(r.h, r.w, r.c, r.s) == 1, r.name
    finally:
        lib.ccvpe_set_mbconv_plane_kernels(prev)
    launched = {f for r in ROWS for f in S.forms(r)}
    assert set(S.TRACED) <= launched, sorted(set(S.TRACED) - launched)
    # the geometry properties the table is there for
    geos = [r.geo for r in S.STRIP]
    assert {g.p for g in geos} >= {32, 10, 7, 4, 1} and any(g.ychunks > 1 for g in geos) and {g.rb for g in geos} >= {1, 2, 8}
    assert any(g.strips % g.p for g in geos) and any(g.p * g.cgx < 256 for g in geos)
    totals = [r.b * r.geo.nblk * r.geo.ychunks for r in S.STRIP]
    assert any(t < 8 for t in totals) and any(t > 8 and t % 8 for t in totals)
    assert any(r.circ and r.w == r.k // 2 + 1 for r in S.STRIP)
    for ks in ((3, 1), (3, 2), (5, 1), (5, 2)):               # both paddings for every strip form, every plane form present
        assert {r.circ for r in S.STRIP if (r.k, r.s) == ks} == {False, True}, ks
        assert any((r.k, r.s) == ks for r in S.PLANE), ks


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.name)
def test_float32_cpu_results_are_inside_the_bounds(row):
    dr = C.cached_ref(row, False)
    C.dw_check(dr.f32_conv, dr.conv, dr.tol_raw, 1e-4, "fp32 CPU raw " + row.name)
    C.dw_check(dr.f32_fused, dr.ref, dr.tol_fused, 1e-4, "fp32 CPU fused " + row.name)
    # the written-out chain is the same function as torch's convolution
    C.dw_check(C.f32_chain(*dr.inputs, row.k, row.s, row.circ), dr.ref, dr.tol_fused, 1e-4, "fp32 written-out chain " + row.name)
    part = dr.f32_fused.sum(dim=(2, 3)).unsqueeze(1)            # one partial row, summed by torch in float32
    C.sum_check(part, dr, dr.f32_fused.shape[2] * dr.f32_fused.shape[3] - 1, 1e-4, "fp32 CPU squeeze sums " + row.name)
    dy = C.grad_input(row)
    want, tol = dr.grad(dy)
    x32 = dr.inputs[0].clone().requires_grad_(True)
    got = torch.autograd.grad(C.dw_conv(x32, dr.inputs[1], row.k, row.s, row.circ, torch.float32), x32, dy)[0]
    C.dw_check(got, want, tol, 1e-4, "fp32 CPU input gradient " + row.name)
    db = C.cached_ref(row, True)
    C.dw_check(C.rbf(db.f32_fused), db.ref, db.tol_bf16, 1e-2, "bf16 storage fused " + row.name)


def _raw32(dr):
    return C.dw_conv(*dr.inputs[:2], dr.row.k, dr.row.s, dr.row.circ, torch.float32)


def _fault_wrapped_column_read_as_zero_at_the_right_edge():
    row = _row("odd W, wrap meets")
    dr = C.cached_ref(row, False)
    pb, _ = C.O.static_same_pad(224, row.k, row.s)

    def fault(xp):
        xp = xp.clone()
        xp[..., pb + row.w:] = 0                                # the pad-after columns: zero instead of columns 0, 1
        return xp
    bad = C.f32_chain(*dr.inputs, row.k, row.s, row.circ, pad_fault=fault)
    assert torch.equal(bad[..., :-1], C.f32_chain(*dr.inputs, row.k, row.s, row.circ)[..., :-1]), "only the last output column"
    _old("wrapped column as zero", bad, dr.ref)
    _caught(C.dw_check, bad, dr.ref, dr.tol_fused, 1e-4, "wrapped column as zero")
    raw = C.dw_conv(*dr.inputs[:2], row.k, row.s, row.circ, torch.float32, pad_fault=fault)
    _caught(C.dw_check, raw, dr.conv, dr.tol_raw, 1e-4, "wrapped column as zero, raw")


def _fault_bottom_pad_row_read_from_the_last_row():
    row = _row("k5 s2 C144 36x41 zero")
    dr = C.cached_ref(row, False)
    pb, _ = C.O.static_same_pad(224, row.k, row.s)

    def fault(xp):
        xp = xp.clone()
        xp[:, :, pb + row.h:] = xp[:, :, pb + row.h - 1:pb + row.h]   # a clamped row address without its mask
        return xp
    bad = C.dw_conv(*dr.inputs[:2], row.k, row.s, row.circ, torch.float32, pad_fault=fault)
    assert torch.equal(bad[:, :, :-1], _raw32(dr)[:, :, :-1]), "only the last output row"
    _old("bottom pad row from row H - 1", bad, dr.conv)
    _caught(C.dw_check, bad, dr.conv, dr.tol_raw, 1e-4, "bottom pad row from row H - 1")


def _fault_one_tap_from_the_next_channel_group():
    row = _row("P = 7")
    dr = C.cached_ref(row, False)

    def fault(ky, kx, tap):
        if (ky, kx) != (2, 0):
            return tap
        tap = tap.clone()
        tap[40:44] = tap[44:48]
        return tap
    bad = C.dw_conv(*dr.inputs[:2], row.k, row.s, row.circ, torch.float32, tap_fault=fault)
    _old("tap (2, 0) of channels 40 .. 43 from the next group", bad, dr.conv)
    _caught(C.dw_check, bad, dr.conv, dr.tol_raw, 1e-4, "tap from the next channel group")
    # a thousandth of that difference on ONE channel: far below the old bar, still outside K u S
    def slight(ky, kx, tap):
        if (ky, kx) != (2, 0):
            return tap
        tap = tap.clone()
        tap[40] += (tap[44] - tap[40]) * 2.0 ** -10
        return tap
    bad = C.dw_conv(*dr.inputs[:2], row.k, row.s, row.circ, torch.float32, tap_fault=slight)
    assert _old("tap (2, 0) of channel 40 off by 2^-10 of the difference", bad, dr.conv), "the old rule lets this through"
    _caught(C.dw_check, bad, dr.conv, dr.tol_raw, 1e-4, "tap slightly off")


def _fault_last_partly_filled_strip_group_missing_from_the_squeeze_sum():
    row = _row("last group of 7")
    dr = C.cached_ref(row, False)
    g = row.geo
    good = dr.f32_fused
    strips = good.reshape(row.b, row.c, g.ho, -1)               # Wo = 33: 9 strips per row, the last one column wide
    sxn = (g.wo + S.DW_TW - 1) // S.DW_TW
    keep = torch.ones(g.ho * sxn, dtype=torch.bool)
    keep[(g.groups - 1) * g.p:] = False                         # the 7 strips of the last group
    assert int((~keep).sum()) == 7
    mask = keep.view(g.ho, sxn).repeat_interleave(S.DW_TW, dim=1)[:, :g.wo]
    part_good = good.sum(dim=(2, 3)).unsqueeze(1)
    part_bad = (strips * mask).sum(dim=(2, 3)).unsqueeze(1)
    C.sum_check(part_good, dr, g.ho * g.wo - 1, 1e-4, "unfaulted sums")
    _old("last strip group missing from the squeeze sum", part_bad.squeeze(1), dr.ref.sum(dim=(2, 3)))
    _caught(C.sum_check, part_bad, dr, S.strip_chain(g), 1e-4, "last strip group missing")


def _fault_bn_shift_from_the_previous_channel_group():
    row = _row("P = 4, RB = 8")
    dr = C.cached_ref(row, False)
    x, wt, sc, sh = dr.inputs
    sh2 = sh.clone()
    sh2[100:104] = sh[96:100]
    bad = C.bn_swish(dr.f32_conv, sc, sh2)
    _old("BN shift of channels 100 .. 103 from the previous group", bad, dr.ref)
    _caught(C.dw_check, bad, dr.ref, dr.tol_fused, 1e-4, "stale BN shift")
    db = C.cached_ref(row, True)
    badb = C.rbf(C.bn_swish(db.f32_conv, sc, sh2))
    print("bf16: old rule (1e-2 of scale) %s this fault" % ("PASSES" if C.old_rule_passes(badb, db.ref, 1e-2) else "fails"))
    _caught(C.dw_check, badb, db.ref, db.tol_bf16, 1e-2, "stale BN shift, bf16")


def _fault_second_strip_group_written_over_the_first():
    row = _row("RB = 2, Wo % 4 = 2")
    dr = C.cached_ref(row, False)
    g = row.geo
    sxn = (g.wo + S.DW_TW - 1) // S.DW_TW
    bad = dr.f32_conv.clone()
    bx, smp = 3, 1                                              # one workgroup of one sample
    for pl in range(g.p):
        src, dst = (bx * g.rb + 1) * g.p + pl, (bx * g.rb) * g.p + pl
        sy, sx, dy, dx = src // sxn, src % sxn * 4, dst // sxn, dst % sxn * 4
        n = min(4, g.wo - sx, g.wo - dx)
        bad[smp, :, dy, dx:dx + n] = dr.f32_conv[smp, :, sy, sx:sx + n]
    assert int((bad != dr.f32_conv).sum()) > 0 and torch.equal(bad[0], dr.f32_conv[0])
    _old("strips of rb = 1 written over those of rb = 0", bad, dr.conv)
    _caught(C.dw_check, bad, dr.conv, dr.tol_raw, 1e-4, "rb = 1 over rb = 0")


FAULTS = [_fault_wrapped_column_read_as_zero_at_the_right_edge, _fault_bottom_pad_row_read_from_the_last_row, _fault_one_tap_from_the_next_channel_group, _fault_last_partly_filled_strip_group_missing_from_the_squeeze_sum, _fault_bn_shift_from_the_previous_channel_group, _fault_second_strip_group_written_over_the_first]


@pytest.mark.parametrize("fault", FAULTS, ids=lambda f: f.__name__[7:])
def test_injected_fault_is_rejected(fault):
    fault()
