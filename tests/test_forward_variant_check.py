"""The elementwise comparison of tests/forward_variant_check.py is sharp: applied to torch's own float32 / bf16 CPU results it
passes on the table rows, and with ONE injected fault of the kind a tiled kernel makes it fails — including faults that the rule
the operator tests used before (maximum error relative to the tensor's maximum: 1e-4 fp32, 1e-2 bf16) lets through.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from ccvpe_amd import synth

import forward_kernel_shapes as S
import forward_variant_check as V

SMALL = [r for r in S.CONV3X3 if 2 * r.b * r.h * r.w * r.n * 9 * (r.c0 + r.c1) < 1e9]      # a float64 conv well under a second


def _f32_conv(a, s, wt, bias, c0):
    return F.conv2d(torch.cat([a[:, :c0], s], 1), wt, bias, padding=1)


def _caught(fn, *args):
    with pytest.raises(AssertionError, match="outside the elementwise tolerance"):
        fn(*args)


@pytest.mark.parametrize("row", SMALL, ids=lambda r: r.name)
def test_unfaulted_cpu_results_pass(row):
    assert len(SMALL) == len(S.CONV3X3)
    cr = V.cached_conv_ref(row, False)
    assert 1.0 <= cr.f32_ratio <= 8.0 and cr.c <= cr.k_terms, "float32 CPU conv at %.2f u S: the model's premise" % cr.f32_ratio
    assert V.conv_check(cr.f32, cr, False, False, False, "fp32 CPU " + row.name) == pytest.approx(0.25)
    V.conv_check(F.relu(cr.f32), cr, True, False, False, "fp32 CPU relu " + row.name)
    cb = V.cached_conv_ref(row, True)
    V.conv_check(cb.f32, cb, False, False, True, "bf16 operands, fp32 out " + row.name)
    assert V.conv_check(V.rbf(F.relu(cb.f32)), cb, True, True, True, "bf16 storage relu " + row.name) <= 1.0


def _deep_case():
    """the widest decoder layer: K = 9 x 1344, N = 640, on 4 x 4 images as tests/test_bf16_gpu.py::test_conv3x3_bf16_two_sources.
    The last real channel of the decoder's concat buffers is the matching score, a cosine: here uniform in [-0.1, 0.1] against
    unit-variance features, which is what makes losing it a SMALL fault (about 2e-3 of the output's scale)."""
    row = S.ConvRow("K = 9 x 1344, N = 640", 1, 4, 4, 1024, 320, 640, 1024, 1024, (4, 5, 2), None, None)
    a, s, wt, bias = V.conv_inputs(row, True)
    s[:, -1] = V.rbf(synth.uniform((row.b, row.h, row.w), 77, -0.1, 0.1))
    return row, (a, s, wt, bias)


def test_dropped_last_input_channel_is_caught_where_the_old_rule_passes():
    row, (a, s, wt, bias) = _deep_case()
    cr = V.ConvRef(a, s, wt, bias, row.c0)
    V.conv_check(V.rbf(cr.f32), cr, False, True, True, "unfaulted")
    s2 = s.clone()
    s2[:, -1] = 0                                                        # the kernel stops one channel short of c0 + c1
    bad = V.rbf(_f32_conv(a, s2, wt, bias, row.c0))
    assert V.old_rule_passes(bad, cr.ref, 1e-2), "old rule (1e-2 of scale): PASSES this fault"
    _caught(V.conv_check, bad, cr, False, True, True, "last channel dropped")
    bad32 = _f32_conv(a, s2, wt, bias, row.c0)                            # the same fault with an fp32 result (out_f32)
    assert V.old_rule_passes(bad32, cr.ref, 2e-3), "old rule (2e-3 of scale, the fp32-out bar of test_igemm_bf16_1x1): PASSES this fault"
    _caught(V.conv_check, bad32, cr, False, False, True, "last channel dropped, fp32 out")


def test_truncation_instead_of_rounding_is_caught_where_the_old_rule_passes():
    row = S.CONV3X3[0]
    cr = V.cached_conv_ref(row, True)
    trunc = (cr.f32.view(torch.int32) & -65536).view(torch.float32)      # drop the low 16 bits: round toward zero
    assert V.old_rule_passes(trunc, cr.ref, 1e-2), "old rule (1e-2 of scale): PASSES this fault"
    _caught(V.conv_check, trunc, cr, False, True, True, "bf16 truncation")


def test_one_tap_of_one_chunk_dropped_in_one_column_tile_is_caught():
    row = S.CONV3X3[0]
    a, s, wt, bias = V.conv_inputs(row, False)
    cr = V.cached_conv_ref(row, False)
    w2 = wt.clone()
    w2[16:32, 8:16, 1, 2] = 0                                            # output columns 16 .. 31 miss tap (1, 2) of channels 8 .. 15
    bad = _f32_conv(a, s, w2, bias, row.c0)
    assert not V.old_rule_passes(bad, cr.ref, 1e-4), "old rule (1e-4 of scale): fails this fault too"
    _caught(V.conv_check, bad, cr, False, False, False, "tap dropped")
    ab, sb, wb, bb = V.conv_inputs(row, True)                            # bf16: the old 1e-2 is the question
    w2 = wb.clone()
    w2[16:32, 8:16, 1, 2] = 0
    crb = V.cached_conv_ref(row, True)
    badb = V.rbf(_f32_conv(ab, sb, w2, bb, row.c0))
    assert not V.old_rule_passes(badb, crb.ref, 1e-2), "old rule (1e-2 of scale): fails this fault too"
    _caught(V.conv_check, badb, crb, False, True, True, "tap dropped, bf16")


def test_missing_bias_on_the_ragged_columns_is_caught():
    row = next(r for r in S.CONV3X3 if r.n == 40)
    cr = V.cached_conv_ref(row, False)
    a, s, wt, bias = V.conv_inputs(row, False)
    bad = cr.f32.clone()
    bad[:, 32:] -= bias[32:].view(1, -1, 1, 1)                          # columns 32 .. 39: the partial 16-column group
    assert not V.old_rule_passes(bad, cr.ref, 1e-4), "old rule (1e-4 of scale): fails this fault too"
    _caught(V.conv_check, bad, cr, False, False, False, "bias missing on ragged N")
    one = cr.f32.clone()
    one[:, 39] -= bias[39] * 2.0 ** -10                                   # a thousandth of ONE column's bias
    assert V.old_rule_passes(one, cr.ref, 1e-4), "old rule: PASSES a 1e-3 error of one column's bias"
    _caught(V.conv_check, one, cr, False, False, False, "bias slightly off on one column")


def test_second_column_tile_reading_its_first_column_as_padding_is_caught():
    row = S.CONV3X3[0]                                                   # W = 20: the second column tile starts at x = 16
    a, s, wt, bias = V.conv_inputs(row, False)
    cr = V.cached_conv_ref(row, False)
    a2, s2 = a.clone(), s.clone()
    a2[..., 16], s2[..., 16] = 0, 0
    bad = cr.f32.clone()
    bad[..., 16:] = _f32_conv(a2, s2, wt, bias, row.c0)[..., 16:]        # only the second tile's outputs see the zeroed column
    assert not V.old_rule_passes(bad, cr.ref, 1e-4), "old rule (1e-4 of scale): fails this fault too"
    _caught(V.conv_check, bad, cr, False, False, False, "halo column as padding")


def test_band_chain_stale_bn_shift_on_one_slice_is_caught():
    row = S.BAND[0]._replace(b=2)
    inp = V.band_inputs(row)
    accum, f32_rel, _ = V.band_accum_term(inp, row.k, row.s, row.circ)
    assert f32_rel < 1e-5
    ref = V.band_chain(*inp, row.k, row.s, row.circ, torch.float64)
    good = V.rbf(V.band_chain(*inp, row.k, row.s, row.circ, torch.float32))
    assert V.band_check(good, ref, accum, "unfaulted band chain") <= 1.0
    # the written-out chain and torch's convolutions are the same function
    assert (V.band_f32_cpu_chain(*inp, row.k, row.s, row.circ).double() - ref).abs().max().item() <= accum / 4 * 1.0000001
    bad = V.rbf(V.band_chain(*inp, row.k, row.s, row.circ, torch.float32, bn_shift_fault=(1, 5)))
    assert not V.old_rule_passes(bad, ref, 1e-2), "old rule (1e-2 of scale): fails this fault too"
    _caught(V.band_check, bad, ref, accum, "slice 5 of sample 1 with slice 4's BN shift")
    assert torch.equal(bad[0], good[0]) and torch.equal(bad[1, :80], good[1, :80]) and torch.equal(bad[1, 96:], good[1, 96:])
    # one bf16 ulp between two results that round the same fp32 values differently is inside the pair tolerance; two are not
    up = (good.view(torch.int32) + 65536).view(torch.float32)
    V.band_pair_check(good, up, 0.0, "one ulp apart")
    with pytest.raises(AssertionError, match="more than one bf16 ulp"):
        V.band_pair_check(good, (good.view(torch.int32) + 2 * 65536).view(torch.float32), 0.0, "two ulps apart")


@pytest.mark.parametrize("row", [S.BAND[1], S.BAND[7], S.BAND[12]], ids=lambda r: r.name)
def test_unfaulted_band_chain_passes(row):
    """circular padding, stride 2 and the 16 x 16 plane: the float32 chain rounded to bf16 passes, on two samples of the row"""
    row = row._replace(b=2)
    inp = V.band_inputs(row)
    accum, _, _ = V.band_accum_term(inp, row.k, row.s, row.circ)
    ref = V.band_chain(*inp, row.k, row.s, row.circ, torch.float64)
    assert V.band_check(V.rbf(V.band_f32_cpu_chain(*inp, row.k, row.s, row.circ)), ref, accum, row.name) <= 1.0
