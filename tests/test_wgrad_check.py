"""The weight-gradient checker of tests/wgrad_check.py, without a GPU.

* torch's own float32 convolution backward and a float32 emulation of the kernel's split schedule (per-split sums in pixel order,
  then the merge by sum_parts_lanes_kernel's order) pass the elementwise comparison: the reference is inside its own bounds;
* with ONE injected fault of the kind conv_wgrad_kernel or its launcher can make, the comparison fails — each test prints whether
  the rule the operator tests use (maximum error relative to the tensor's maximum, 2e-4) would have let the fault through.
(The table's planner columns against the library are checked in tests/test_abi.py.)
"""
import pytest
import torch

import wgrad_check as C
import wgrad_kernel_shapes as S

ROWS = {r.num: r for r in S.rows()}
PASS_ROWS = [1, 2, 3, 4, 6, 11, 12, 14, 21]


def _caught(fn, *args):
    with pytest.raises(AssertionError, match="outside the elementwise tolerance"):
        fn(*args)


def _old(name, got, ref):
    passes = C.old_rule_passes(got, ref)
    print("%s: old rule (2e-4 of scale) %s this fault" % (name, "PASSES" if passes else "fails"))
    return passes


@pytest.mark.parametrize("num", PASS_ROWS, ids=lambda n: ROWS[n].name)
def test_float32_cpu_results_are_inside_the_bounds(num):
    row = ROWS[num]
    ref = C.cached_ref(row)
    for name, (dw, db) in (("torch float32", C.torch_f32(row, *ref.inputs)), ("emulated schedule", C.emulate_f32(row, *ref.inputs))):
        C.wg_check(dw, ref.dw, ref.a_dw, ref.d, "%s dW %s" % (name, row.name))
        C.wg_check(db, ref.db, ref.a_db, ref.d, "%s dbias %s" % (name, row.name))
        assert bool((dw[:, :, 1] == 0).all()) and bool((dw[2] == 0).all()) and db[2].item() == 0, "the zero channel and column"


def _dw_fault(name, row, **kw):
    """the emulated schedule with the fault must fail on dW; returns the faulted (dW, dbias)"""
    ref = C.cached_ref(row)
    good = C.emulate_f32(row, *ref.inputs, s=kw.get("s"), pps=kw.get("pps"))
    C.wg_check(good[0], ref.dw, ref.a_dw, ref.d, "unfaulted " + name)
    bad = C.emulate_f32(row, *ref.inputs, **kw)
    assert not torch.equal(bad[0], good[0])
    _old(name, bad[0], ref.dw)
    _caught(C.wg_check, bad[0], ref.dw, ref.a_dw, ref.d, name)
    return bad, good


def _fault_last_pixel_of_the_last_split_dropped():
    row = ROWS[1]
    ref = C.cached_ref(row)
    bad, _ = _dw_fault("last pixel dropped", row, drop_last_pixel=True)
    _old("last pixel dropped, dbias", bad[1], ref.db)
    _caught(C.wg_check, bad[1], ref.db, ref.a_db, ref.d, "last pixel dropped, dbias")


def _fault_invalid_rows_of_the_partial_last_stage_not_zeroed():
    row = ROWS[6]
    ref = C.cached_ref(row)
    bad, _ = _dw_fault("pixel M - 1 counted again", row, recount_last_pixel=True)
    _old("pixel M - 1 counted again, dbias", bad[1], ref.db)
    _caught(C.wg_check, bad[1], ref.db, ref.a_db, ref.d, "pixel M - 1 counted again, dbias")


def _fault_one_split_left_out_of_the_merge():
    def fault(part, bias_part):
        return torch.cat([part[:3], part[4:]]), bias_part
    _dw_fault("split 3 of 6 left out", ROWS[2], part_fault=fault)


def _fault_stale_value_in_an_empty_split():
    # row 22's geometry (trailing splits that own no pixel) at plane A's M: 8 splits of 192 px cover 1311 px with 7
    row = ROWS[1]
    s, pps = 8, 192
    assert (s - 1) * pps >= S.dims(row)[2] > (s - 2) * pps

    def fault(part, bias_part):
        assert bool((part[s - 1] == 0).all()) and bool((bias_part[s - 1] == 0).all()), "an empty split's partial is zero"
        part = part.clone()
        part[s - 1, 5, 7] = part[0, 5, 7] * 2.0 ** -6                # what an earlier, smaller launch left there
        return part, bias_part
    _dw_fault("stale value in the empty split", row, s=s, pps=pps, part_fault=fault)

    # a sixteenth of that: below the old bar, still outside d u A
    def slight(part, bias_part):
        part = part.clone()
        part[s - 1, 5, 7] = part[0, 5, 7] * 2.0 ** -10
        return part, bias_part
    ref = C.cached_ref(row)
    bad, _ = C.emulate_f32(row, *ref.inputs, s=s, pps=pps, part_fault=slight)
    assert _old("slighter stale value in the empty split", bad, ref.dw), "the old rule lets this through"
    _caught(C.wg_check, bad, ref.dw, ref.a_dw, ref.d, "slighter stale value in the empty split")


def _fault_border_tap_reads_a_clamped_pixel():
    _dw_fault("tap (0, 2) reads the nearest pixel for padding", ROWS[5], clamp_tap=(0, 2))


def _fault_column_to_source_map_off_by_one_piece_at_the_seam():
    row = ROWS[2]                                                     # c0 24 + c1 8

    def fault(xcols):
        xcols = xcols.clone()
        xcols[:, 4, row.c0:row.c0 + 4] = xcols[:, 4, row.c0 + 4:row.c0 + 8]   # tap 4: the first piece of source 1 reads its second
        return xcols
    _dw_fault("first piece of source 1 reads the next piece", row, xcols_fault=fault)


def _fault_row_n_minus_1_not_written():
    row = ROWS[4]                                                     # N 126: the last stored row is inside a 16-byte piece
    ref = C.cached_ref(row)
    dw, db = C.emulate_f32(row, *ref.inputs)
    dw, db = dw.clone(), db.clone()
    dw[row.n - 1], db[row.n - 1] = C.SENTINEL, C.SENTINEL
    _old("row N - 1 not written", dw, ref.dw)
    _caught(C.wg_check, dw, ref.dw, ref.a_dw, ref.d, "row N - 1 not written")
    _caught(C.wg_check, db, ref.db, ref.a_db, ref.d, "dbias row N - 1 not written")


def _fault_gate_of_the_neighbouring_sample_in_a_straddling_stage():
    row = ROWS[14]
    ref = C.cached_ref(row)
    x0, _, _, gate = ref.inputs
    ho, wo, m, _, _, _ = S.dims(row)
    hw, pps = ho * wo, row.plan.pps
    stage0 = hw // pps * pps + (hw % pps) // S.WG_BP * S.WG_BP         # the stage that holds the first pixel of sample 1
    assert stage0 < hw < stage0 + S.WG_BP

    def fault(xcols):
        xcols = xcols.clone()
        u = x0[..., :row.c0].reshape(m, row.c0)
        xcols[hw:stage0 + S.WG_BP, 0] = u[hw:stage0 + S.WG_BP] * gate[0]     # the gate of the stage's first row
        return xcols
    _dw_fault("straddling stage takes one sample's gate", row, xcols_fault=fault)


def _fault_dy_padding_column_added_into_the_last_bias_row():
    row = ROWS[4]                                                     # N 126 of ldy 128
    ref = C.cached_ref(row)
    _, db = C.emulate_f32(row, *ref.inputs)
    # the padding columns are NaN in the test inputs (a kernel that used one would fail the finite check); a finite stand-in
    # shows that the value check alone rejects the fault too
    pad_col = C.synth.normal((S.dims(row)[2],), 4242)
    bad = db.clone()
    bad[row.n - 1] += pad_col.sum()
    _old("padding column added into dbias[N - 1]", bad, ref.db)
    _caught(C.wg_check, bad, ref.db, ref.a_db, ref.d, "padding column added into dbias[N - 1]")
    nan = db.clone()
    nan[row.n - 1] += ref.inputs[2][..., row.n].sum()
    with pytest.raises(AssertionError, match="non-finite"):
        C.wg_check(nan, ref.db, ref.a_db, ref.d, "poisoned padding column added into dbias[N - 1]")


FAULTS = [_fault_last_pixel_of_the_last_split_dropped, _fault_invalid_rows_of_the_partial_last_stage_not_zeroed,
          _fault_one_split_left_out_of_the_merge, _fault_stale_value_in_an_empty_split, _fault_border_tap_reads_a_clamped_pixel,
          _fault_column_to_source_map_off_by_one_piece_at_the_seam, _fault_row_n_minus_1_not_written,
          _fault_gate_of_the_neighbouring_sample_in_a_straddling_stage, _fault_dy_padding_column_added_into_the_last_bias_row]


@pytest.mark.parametrize("fault", FAULTS, ids=lambda f: f.__name__[7:])
def test_injected_fault_is_rejected(fault):
    fault()
