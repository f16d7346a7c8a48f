"""The matching checker, without a GPU.

* for every distinct (C, L, shifts, stride, window_offset) of tests/matching_kernel_shapes.py's rows, at a small pixel count, the
  float32 oracle's results pass the elementwise model of tests/matching_check.py with the TIGHTEST addition chains of the forms the
  row launches (and, rounded to bf16, the bf16 model): the reference is inside its own bounds, S_i > 0 everywhere;
* with ONE injected fault of the kind a matching kernel makes, the comparison fails — each prints whether the rule the operator
  tests use (maximum error relative to the tensor's maximum) would have let the fault through.
"""
import pytest
import torch

import matching_check as C
import matching_kernel_shapes as S

ROWS = S.rows()
SMALL = dict(b=2, h=4, w=5)            # 20 pixels: more than one 16-pixel tile


def _configs():
    seen, out = set(), []
    for r in ROWS:
        key = (r.c, r.l, r.shifts, r.stride, r.woff, r.bf16)
        if key in seen:
            continue
        seen.add(key)
        out.append(r._replace(ldx=r.c, **SMALL))
    return out


def _tightest(row):
    chains = [S.match_chain(row, row.claims[p]) for p in row.switches]
    return S.Chain(*(min(ch[i] for ch in chains) for i in range(4)))


def _check(row, chain, scores, dstx, what):
    """C.match_check with explicit chains: the row's first launched claim names the owner in a failure message"""
    return C.match_check(C.cached_ref(row), row, row.claims[row.switches[0]], scores, dstx, what, chain=chain)


def _good(row):
    ref = C.cached_ref(row)
    sc = C.oracle_scores(row, ref.x, ref.g)
    return ref, sc, C.assemble(row, ref.x, sc)


@pytest.mark.parametrize("row", _configs(), ids=lambda r: r.name)
def test_float32_oracle_is_inside_the_bounds(row):
    ref, sc, dstx = _good(row)
    assert bool((ref.s_abs > 0).all()) and bool(torch.isfinite(ref.s_abs).all()), "S_i > 0 everywhere"
    assert bool((ref.s_abs >= ref.scores.abs() * (1 - 1e-12)).all())
    res = _check(row, _tightest(row), sc, dstx, "fp32 oracle " + row.name)
    assert max(r[1] for r in res) <= 1.0


def _row(text, bf16=False):
    r = next(r for r in ROWS if text in r.name and r.bf16 == bf16)
    return r._replace(ldx=r.c, **SMALL)


def _caught(row, sc, dstx, what, part="scores"):
    with pytest.raises(AssertionError, match="%s: .*outside the elementwise tolerance" % part):
        _check(row, S.match_chain(row, row.claims[row.switches[0]]), sc, dstx, what)


def _old(name, got, ref, bar=2e-5):
    passes = C.old_rule_passes(got, ref, bar)
    print("%s: old rule (%.0e of scale) %s this fault" % (name, bar, "PASSES" if passes else "fails"))
    return passes


def _fault_one_shift_offset_off_by_one_channel():
    row = _row("tiled C160 npad32 20 shifts")
    ref, sc, dstx = _good(row)
    k = 13
    bad = sc.clone()
    bad[:, k] = C.O.rotational_matching(ref.x, ref.g, [row.shifts[k]], row.stride, row.woff + 1).reshape(row.b, -1)
    assert int((bad != sc).any(dim=2).any(dim=0).sum()) == 1
    _old("offset of shift 13 off by one channel", bad, ref.scores)
    _caught(row, bad, dstx, "offset off by one")


def _fault_total_norm_used_for_a_partial_window():
    row = _row("valu npad8 vec4 partial C80 L40")
    ref, sc, dstx = _good(row)
    gn = ref.g.norm(dim=1).view(row.b, 1, 1)
    wn = torch.stack([ref.x.index_select(1, C.window_index(row, i)).norm(dim=1) for i in row.shifts], dim=1).reshape(sc.shape)
    bad = sc * wn / ref.x.norm(dim=1).reshape(row.b, 1, -1)
    assert gn.shape[0] == row.b
    _old("total norm for a partial window", bad, ref.scores)
    _caught(row, bad, C.assemble(row, ref.x, bad), "total norm for a partial window")


def _fault_max_over_all_shifts_instead_of_n_max():
    row = _row("ori_prior(54)")
    ref, sc, dstx = _good(row)
    assert row.n_max == 7 < len(row.shifts)
    bad = C.assemble(row, ref.x, sc, n_max=len(row.shifts))
    assert bool((bad[:, :, row.c] != dstx[:, :, row.c]).any())
    _old("max over all 27 hypotheses", bad[:, :, row.c], ref.scores[:, :7].max(dim=1)[0])
    _caught(row, sc, bad, "max over all hypotheses", part="max column")


def _fault_tail_columns_start_one_shift_early():
    row = _row("tiled C320 npad32 partial 21 shifts, 9 tail")
    ref, sc, dstx = _good(row)
    bad = C.assemble(row, ref.x, sc, tail0=len(row.shifts) - row.n_tail - 1)
    _caught(row, sc, bad, "tail one shift early", part="tail columns")


def _fault_previous_samples_descriptor_for_the_first_16_pixels():
    row = _row("stream MTL2 NB5 C80 5x16x821")
    ref, sc, dstx = _good(row)
    bad = sc.clone()
    stale = C.O.rotational_matching(ref.x[1:2], ref.g[0:1], list(row.shifts), row.stride, row.woff).reshape(len(row.shifts), -1)
    bad[1, :, :16] = stale[:, :16]
    assert torch.equal(bad[0], sc[0]) and torch.equal(bad[1, :, 16:], sc[1, :, 16:])
    _old("sample 0's descriptor for the first tile of sample 1", bad, ref.scores)
    _caught(row, bad, C.assemble(row, ref.x, bad), "stale descriptor")


def _fault_non_zero_value_left_in_a_pad_channel():
    row = _row("tiled C104 npad32 20 shifts")
    assert row.c % 16 == 8
    ref, sc, dstx = _good(row)
    # channel C of one tile row holds v instead of 0: hypothesis i picks up v * gg[C + off_i] = v * g[off_i]
    v, b, p = 0.25, 1, 7
    offs = S.offsets(row.shifts, row.stride, row.woff, row.c)
    x64 = ref.x.double().reshape(row.b, row.c, -1)[b, :, p]
    g64 = ref.g.double()[b]
    bad = sc.clone()
    for k, i in enumerate(row.shifts):
        win = x64[C.window_index(row, i)]
        num = (win * g64).sum() + v * (g64[offs[k]] if offs[k] < row.l else 0.0)
        bad[b, k, p] = (num / (win.norm() * g64.norm())).float()
    assert int((bad != sc).sum()) > 0
    _old("0.25 left in pad channel C of one pixel", bad, ref.scores)
    _caught(row, bad, dstx, "pad channel not zero")


def _fault_one_k_slice_dropped():
    row = _row("tiled C200 npad32 vec2 20 shifts")
    ref, sc, dstx = _good(row)
    kb0, kb1 = row.claims[2].slices[3]
    x2 = ref.x.clone()
    x2[:, 16 * kb0:16 * kb1] = 0                                  # slice 3 (blocks 9..12) never added
    bad = C.oracle_scores(row, x2, ref.g)
    _old("K slice 3 of 4 dropped", bad, ref.scores)
    _caught(row, bad, dstx, "K slice dropped")


def _fault_x_rounded_to_bf16_in_an_fp32_row():
    for text in ("valu npad8 vec4 C80 7 shifts", "tiled C1280 npad32 20 shifts", "stream MTL1 NB2 C24"):
        row = _row(text)
        ref, sc, dstx = _good(row)
        xb = C.rbf(ref.x)
        bad = C.oracle_scores(row, xb, ref.g)
        assert _old("x rounded to bf16 (%s)" % text, bad, ref.scores, 1e-2), "a hundredth of scale lets this through"
        _caught(row, bad, dstx, "x rounded to bf16")
        with pytest.raises(AssertionError, match="normalised copy: .*outside the elementwise tolerance"):
            _check(row, S.match_chain(row, row.claims[row.switches[0]]), sc, C.assemble(row, xb, sc), "x rounded to bf16")


FAULTS = [_fault_one_shift_offset_off_by_one_channel, _fault_total_norm_used_for_a_partial_window, _fault_max_over_all_shifts_instead_of_n_max,
          _fault_tail_columns_start_one_shift_early, _fault_previous_samples_descriptor_for_the_first_16_pixels,
          _fault_non_zero_value_left_in_a_pad_channel, _fault_one_k_slice_dropped, _fault_x_rounded_to_bf16_in_an_fp32_row]


@pytest.mark.parametrize("fault", FAULTS, ids=lambda f: f.__name__[7:])
def test_injected_fault_is_rejected(fault):
    fault()


def test_padding_columns_must_be_exactly_zero():
    row = _row("valu npad8 vec2 C40 8 shifts")._replace(ldo=48)
    ref, sc, dstx = _good(row)
    dstx[1, 3, row.c + 5] = 1e-30
    with pytest.raises(AssertionError, match="padding columns are not exactly zero"):
        _check(row, _tightest(row), sc, dstx, "dirty padding")
