"""CPU checks of tests/stage_check.py, the harness behind tests/test_train_stages_gpu.py:
  * self-consistency: every stage kind at small sizes, the reference's own fp32 run passes `compare` against its fp64 run;
  * mutation checks: six subtly wrong steps, applied to the fp32 record, each BOTH fail `compare` AND move the tensor by
    less than 3 % relative L2 (the bar of golden_util.compare_grads), so the whole-model test could not have seen them there;
  * hook names: every call the Recorder wraps still exists with the parameter names it reads.
"""
import importlib
import inspect

import pytest
import torch
import torch.nn.functional as F

import stage_check as S
from ccvpe_amd import synth
from oracle import ccvpe_oracle as O

WHOLE_MODEL_BAR = 3e-2          # golden_util.compare_grads


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def both(fn, *args):
    return fn(*args, dtype=torch.float64), fn(*args, dtype=torch.float32)


def caught(stage, got, r64, r32):
    """compare() must refuse `got`; returns the failing rows' text."""
    with pytest.raises(AssertionError) as e:
        S.compare(stage, got, r64, r32)
    return str(e.value)


def block_params(sd, prefix, i):
    bp = "%s._blocks.%d" % (prefix, i)
    return bp, {k: v for k, v in sd.items() if k.startswith(bp + ".") and "running_" not in k and "num_batches" not in k}


def decoder_params(names, k_ref, cout, c_skip, c_mid, c_out, seed):
    """Reference-layout parameters of one decoder level at small widths."""
    deconv, conv = names
    shapes = {deconv + ".weight": (k_ref, cout, 2, 2), deconv + ".bias": (cout,),
              conv + ".0.weight": (c_mid, cout + c_skip, 3, 3), conv + ".0.bias": (c_mid,),
              conv + ".2.weight": (c_out, c_mid, 3, 3), conv + ".2.bias": (c_out,)}
    out = {}
    for j, (n, sh) in enumerate(sorted(shapes.items())):
        fan = sh[1] * 9 if len(sh) == 4 else 1
        out[n] = synth.normal(sh, seed + j, std=(2.0 / fan) ** 0.5 if len(sh) == 4 else 0.1)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# self-consistency
# ----------------------------------------------------------------------------------------------------------------------
def test_stem_self_consistent(synth_sd):
    sd = synth_sd("vigor", 0)
    for prefix, circular in (("grd_efficientnet", True), ("sat_efficientnet", False)):
        params = {n: sd[n] for n in (prefix + "._conv_stem.weight", prefix + "._bn0.weight", prefix + "._bn0.bias")}
        r64, r32 = both(S.ref_stem, synth.normal((3, 3, 16, 24), 11), params, prefix, circular, synth.normal((3, 32, 8, 12), 12))
        rows = S.compare("stem:" + prefix, r32, r64, r32)
        assert len(rows) == 2 * 4 and set(k for k in r64 if k.startswith("dp:")) == set("dp:" + n for n in params)


@pytest.mark.parametrize("i", [0, 1, 2, 3, 4, 10, 15])
@pytest.mark.parametrize("circular", [True, False])
def test_mbconv_self_consistent(synth_sd, i, circular):
    """Block 0 (no expand), 1 (stride 2), 2 (skip + drop), 3 (5x5 stride 2), 4 / 10 (5x5 skip), 15 (3x3, 192 -> 320)."""
    k, s, e, cin, cout, sched = S.block_schedule()[i]
    bp, params = block_params(synth_sd("vigor", 0), "grd_efficientnet", i)
    x = synth.normal((3, cin, 6, 10), 20 + i)
    drop = torch.tensor([1.0, 0.0, 1.0]) / (1 - 0.2 * i / 16) if S.skip_block(i) else None
    g = synth.normal((3, cout, 6 // s, 10 // s), 40 + i)
    r64, r32 = both(S.ref_mbconv, x, params, bp, i, circular, drop, g)
    assert tuple(r64["out:x"].shape) == tuple(g.shape) and r64["out:x"].dtype == torch.float64
    assert len(params) == (13 if e != 1 else 10)
    S.compare("block:%d" % i, r32, r64, r32)


def test_head_descriptors_self_consistent(synth_sd):
    sd = synth_sd("vigor", 0)
    p = "sat_efficientnet"
    params = {n: sd[n] for n in (p + "._conv_head.weight", p + "._bn1.weight", p + "._bn1.bias")}
    S.compare("head", *(lambda r: (r[1], r[0], r[1]))(both(S.ref_head, synth.normal((2, 320, 4, 5), 1), params, p,
                                                           synth.normal((2, 1280, 4, 5), 2))))
    params = {k: v for k, v in sd.items() if k.startswith("grd_feature_to_descriptor")}
    total = 6 * sum(synth.MODEL_SPECS["vigor"]["cd"])
    r64, r32 = both(S.ref_ground_descriptors, synth.normal((2, 1280, 10, 6), 3), params, synth.normal((2, total), 4))
    assert tuple(r64["out:gdesc"].shape) == (2, total) and len(params) == 24
    S.compare("gdesc", r32, r64, r32)
    params = {k: v for k, v in sd.items() if k.startswith("sat_feature_to_descriptors.1.")}
    r64, r32 = both(S.ref_aerial_descriptor, synth.normal((2, 1280, 4, 4), 5), params, synth.normal((2, 1280, 2, 2), 6))
    S.compare("sdesc", r32, r64, r32)


@pytest.mark.parametrize("c,L,shifts,n_max,n_tail,stride,woff", [
    (64, 64, list(range(8)), 8, 8, 8, 0),                    # level 1: the tail is the same eight scores
    (64, 64, [-2, -1, 0, 1, 2] + list(range(8)), 5, 8, 8, 0),   # ori_prior level 1: 5 localisation shifts + the 8-shift tail
    (64, 32, list(range(8)), 8, 0, 4, 0),                    # partial window L < C
    (64, 32, list(range(8)), 8, 0, 4, 16),                   # ... with a window offset
])
def test_match_level_self_consistent(c, L, shifts, n_max, n_tail, stride, woff):
    x, g = synth.normal((2, c, 4, 4), 1), synth.normal((2, L), 2)
    n = len(shifts)
    r64, r32 = both(S.ref_match_level, x, g, shifts, n_max, n_tail, stride, woff, synth.normal((2, n, 4, 4), 3),
                    synth.normal((2, c + 1, 4, 4), 4), synth.normal((2, n_tail, 4, 4), 5) if n_tail else None)
    assert tuple(r64["out:cat"].shape) == (2, c + 1, 4, 4) and ("out:tail" in r64) == bool(n_tail)
    S.compare("match", r32, r64, r32)


@pytest.mark.parametrize("last_cout", [0, 1, 2])
def test_decoder_level_self_consistent(last_cout):
    names = ("deconv2", "conv2") if not last_cout else ("deconv1_ori", "conv1_ori")
    c_skip = 0 if last_cout else 6
    params = decoder_params(names, 9, 8, c_skip, 8, last_cout or 8, 100)
    skip = synth.normal((2, c_skip, 12, 12), 7) if c_skip else None
    r64, r32 = both(S.ref_decoder_level, synth.normal((2, 9, 6, 6), 8), skip, params, names,
                    synth.normal((2, last_cout or 8, 12, 12), 9))
    assert ("din:skip" in r64) == bool(c_skip) and len([k for k in r64 if k.startswith("dp:")]) == 6
    S.compare("dec", r32, r64, r32)


def test_output_heads_self_consistent():
    logits = synth.normal((2, 256), 1, std=3.0)
    r64, r32 = both(S.ref_softmax_head, logits, synth.normal((2, 256), 2), synth.normal((2, 256), 3))
    S.compare("head_softmax", r32, r64, r32)
    only_logits = S.ref_softmax_head(logits, synth.normal((2, 256), 2), None)
    assert torch.equal(only_logits["din:logits"], synth.normal((2, 256), 2).double())
    r64, r32 = both(S.ref_normalize_head, synth.normal((2, 2, 8, 8), 4), synth.normal((2, 2, 8, 8), 5))
    S.compare("head_normalize", r32, r64, r32)
    raw = synth.normal((4, 8, 6, 5), 6)
    st64, st32 = S.ref_bn_stats(raw), S.ref_bn_stats(raw, torch.float32)
    S.compare("stats", st32, st64, st32)


def loss_link_case(b=3, n_rot=4):
    """Nine outputs and the targets of a step at small sizes (map 16 x 16, score levels 2 x 2 .. 7 x 7)."""
    hw = 16
    outs = [synth.normal((b, hw * hw), 1, std=3.0), None, F.normalize(synth.normal((b, 2, hw, hw), 2), dim=1)]
    outs[1] = torch.softmax(outs[0], dim=1).reshape(b, 1, hw, hw)
    labels = []
    for j in range(6):
        side = 2 + j
        outs.append(synth.uniform((b, n_rot, side, side), 10 + j, -1.0, 1.0))
        labels.append(synth.uniform((b, n_rot, side, side), 20 + j) ** 3)
    labels[2][0] *= 0.03                       # level 3: one sample with little label mass
    gt = synth.uniform((b, 1, hw, hw), 30) ** 8
    gt_flat = gt.flatten(1) / gt.flatten(1).sum(1, keepdim=True)
    gt_ori = F.normalize(synth.normal((b, 2, hw, hw), 31), dim=1)
    return outs, (gt, gt_flat, gt_ori, labels)


class _Rec(object):
    tape = None


def test_loss_link_self_consistent_and_mutations():
    """The loss link on a recorded step made of the float32 reference itself: it passes; a heat-map gradient is refused; one
    score level's gradient scaled as if the batch's label mass D had lost one row of three, and the value of the mix with
    infoNCE summed over five levels, are each caught by name."""
    outs, targets = loss_link_case()
    r64, r32 = S.ref_loss_mix(outs, targets), S.ref_loss_mix(outs, targets, dtype=torch.float32)
    assert set(r64) == {"out:loss"} | set("din:" + n for n in S.LOSS_OUTPUTS.values()) and r64["out:loss"].dtype == torch.float64
    want = (O.cross_entropy_loss(outs[0].double(), targets[1].double()) + 1e1 * O.orientation_loss(outs[2].double(), targets[2].double(), targets[0].double())
            + 1e4 * sum(O.infonce_loss(outs[3 + j].double().flatten(1), targets[3][j].double().flatten(1)) for j in range(6)) / 6)
    assert abs(float(r64["out:loss"] - want)) <= 1e-12 * abs(float(want))
    rec = _Rec()
    rec.outs = outs
    rec.gout = [r32["din:logits"], None, r32["din:ori"]] + [r32["din:scores%d" % (j + 1)] for j in range(6)]

    def link(gout, loss, want_key=None):
        rec.gout = gout
        chk = S.StepChecker(rec, {}, {}, want_key)
        chk.loss_link(targets, loss)
        return chk
    good = list(rec.gout)
    chk = link(good, float(r32["out:loss"]))
    chk.report.assert_ok()
    assert chk.stages == ["loss"] and chk.report.tensors() == 9 and not chk.loss_left_out and not chk.loss_crosschecks
    chk = link(good[:1] + [torch.zeros_like(outs[1])] + good[2:], float(r32["out:loss"]))
    chk.report.assert_ok()
    with pytest.raises(AssertionError, match="heat-map"):
        link(good[:1] + [1e-9 * torch.ones_like(outs[1])] + good[2:], float(r32["out:loss"]))
    with pytest.raises(AssertionError, match="received no gradient"):
        link(good[:5] + [None] + good[6:], float(r32["out:loss"]))
    # an output left out of the gradient comparison still enters the value
    chk = link(good, float(r32["out:loss"]), lambda key: key != ("loss", 8))
    chk.report.assert_ok()
    assert chk.loss_left_out == ["scores6"] and chk.report.tensors() == 8
    assert link(good, float(r32["out:loss"]), lambda key: key[0] != "loss").stages == []
    # mutations
    lab = targets[3][2]
    den = torch.where(lab > 1e-2, lab, torch.zeros_like(lab)).flatten(1).sum(1).double()
    light = int(den.argmin())
    scale = float(den.sum() / (den.sum() - den[light]))
    bad = list(good)
    bad[5] = good[5] * scale
    print("loss link: a row's label mass missing from D scales the level's gradient by %.5f" % scale)
    assert light == 0 and 1e-3 < scale - 1 < WHOLE_MODEL_BAR
    chk = link(bad, float(r32["out:loss"]))
    failed = [r[1] for r in chk.report.failures()]
    assert failed and all(name.startswith("din:scores3") for name in failed), failed
    nce5 = sum(O.infonce_loss(outs[3 + j].flatten(1), targets[3][j].flatten(1)) for j in range(5))
    five = float(r32["out:loss"]) - 1e4 * float(O.infonce_loss(outs[8].flatten(1), targets[3][5].flatten(1))) / 6
    assert abs(five - float(O.cross_entropy_loss(outs[0], targets[1]) + 1e4 * nce5 / 6 + 1e1 * O.orientation_loss(outs[2], targets[2], targets[0]))) < 1e-2
    failed = [r[1] for r in link(good, five).report.failures()]
    assert failed and all(name.startswith("out:loss") for name in failed), failed


def test_adapters_round_trip():
    t = synth.normal((2, 3, 4, 16), 1)                       # [x (9), max, tail (4), pad (2)]
    t[..., 14:] = 0
    cat, tail = S.match_cat_to_ref(t, 9, 4)
    assert torch.equal(cat[:, 0], t[..., 9]) and torch.equal(cat[:, 1:], t[..., :9].permute(0, 3, 1, 2))
    assert torch.equal(tail, t[..., 10:14].permute(0, 3, 1, 2))
    ori = S.cat_to_ref(t, [(0, 4, 9), (10, 0, 4)], 14)       # the orientation decoder's view: [tail, x]; the max column is unread
    assert torch.equal(ori[:, :4], tail) and torch.equal(ori[:, 4:], cat[:, 1:])
    with pytest.raises(AssertionError):
        S.cat_to_ref(t, [(0, 4, 9), (10, 0, 4)], 14, must_be_zero="unmapped")     # a gradient there would be lost
    t[..., 15] = 1.0
    with pytest.raises(AssertionError):
        S.match_cat_to_ref(t, 9, 4)
    assert torch.equal(S.to_nhwc(S.to_nchw(t)), t)


def test_noise_level_rule_and_report():
    """A parameter gradient below 1e-6 of the step's largest (by the fp64 reference alone) only has to stay at noise level."""
    big, tiny = torch.ones(4, dtype=torch.float64), torch.full((4,), 1e-9, dtype=torch.float64)
    r64 = {"dp:a": big, "dp:b": tiny}
    rep = S.Report().compare("s", {"dp:a": big.float(), "dp:b": torch.full((4,), 3e-5)}, r64, {"dp:a": big.float(), "dp:b": tiny.float()})
    assert not rep.failures() and rep.noise == [("s", "dp:b")]
    rep = S.Report().compare("s", {"dp:a": big.float(), "dp:b": torch.full((4,), 3e-4)}, r64, {"dp:a": big.float(), "dp:b": tiny.float()})
    assert [r[1] for r in rep.failures()] == ["dp:b [noise]"]
    rep = S.Report().compare("s", {"dp:b": tiny.float()}, {"dp:b": tiny}, {"dp:b": tiny.float()})
    rep.finish()
    assert rep.noise == []                     # alone it is the largest: compared as a value
    # floors by tensor kind; the bar follows the reference's own error with the factor 4
    e = torch.tensor([1.0, 1.0 + 1.5e-4], dtype=torch.float64)
    one = torch.ones(2, dtype=torch.float64)
    assert caught("s", {"out:x": e}, {"out:x": one}, {"out:x": one})
    S.compare("s", {"din:x": e}, {"din:x": one}, {"din:x": one})
    S.compare("s", {"out:x": e}, {"out:x": one}, {"out:x": torch.tensor([1.0, 1.0 + 5e-5], dtype=torch.float64)})


def test_relu_decision_at_the_discontinuity():
    """Only a disagreement at an element whose fp64 pre-activation is within 4 x the reference's own fp32 error of zero takes the
    taped decision; the references then differentiate the same function, and a disagreement anywhere else still fails."""
    names = ("deconv2", "conv2")
    params = decoder_params(names, 9, 8, 6, 8, 8, 100)
    args = (synth.normal((2, 9, 6, 6), 8), synth.normal((2, 6, 12, 12), 7), params, names, synth.normal((2, 8, 12, 12), 9))
    s64, s32 = {}, {}
    r64 = S.ref_decoder_level(*args, seen=s64)
    r32 = S.ref_decoder_level(*args, dtype=torch.float32, seen=s32)
    pre64, pre32, y = s64["pre"].clone(), s32["pre"].clone(), s32["pre"].clamp(min=0)
    assert S.relu_mask_at_discontinuity(pre64, pre32, y)[0] is None
    pre64[0, 0, 0, 0], pre32[0, 0, 0, 0], y[0, 0, 0, 0] = 1e-9, -2e-8, 0.0       # undetermined sign in fp32: the tape decides
    big = tuple(pre64.abs().argmax().item() // s % n for s, n in zip((8 * 144, 144, 12, 1), pre64.shape))
    y[big] = 0.0 if pre64[big] > 0 else 1.0                          # a wrong decision at the largest element: left to fail
    mask, n, tau = S.relu_mask_at_discontinuity(pre64, pre32, y)
    assert n == 1 and not bool(mask[0, 0, 0, 0]) and bool(mask[big]) == bool(pre64[big] > 0) and tau < 1e-4
    own = s64["pre"] > 0
    again = S.ref_decoder_level(*args, relu_mask=own)
    for k in r64:
        assert torch.equal(again[k], r64[k]) or S._errors(again[k], r64[k])[0] < 1e-14, k
    other = own.clone()
    other[big] = ~other[big]
    wrong = S.ref_decoder_level(*args, relu_mask=other, dtype=torch.float32)
    assert "din:cat" in caught("dec", wrong, r64, r32)


# ----------------------------------------------------------------------------------------------------------------------
# mutation checks
# ----------------------------------------------------------------------------------------------------------------------
def test_mutation_border_column_with_zero_padding(synth_sd):
    """Column x = 0 of a block's input gradient computed with zero padding where the block pads circularly.  With an
    i.i.d. upstream gradient one column's share falls with the width: 3.8 % at block 2's 160 columns, 3.2 % at block 0's 320 (the
    ground encoder's own widths), under the 3 % bar from about 400 columns on — block 0 at 512 columns here."""
    i = 0
    k, s, e, cin, cout, sched = S.block_schedule()[i]
    bp, params = block_params(synth_sd("vigor", 0), "grd_efficientnet", i)
    x, g = synth.normal((2, cin, 4, 512), 1), synth.normal((2, cout, 4, 512), 2)
    drop = None
    r64, r32 = both(S.ref_mbconv, x, params, bp, i, True, drop, g)
    zero = S.ref_mbconv(x, params, bp, i, False, drop, g, dtype=torch.float32)
    got = dict(r32)
    got["din:x"] = r32["din:x"].clone()
    got["din:x"][..., 0] = zero["din:x"][..., 0]
    moved = rel_l2(got["din:x"], r32["din:x"])
    print("border column: input gradient moved by %.3e" % moved)
    assert 0 < moved < WHOLE_MODEL_BAR
    assert "din:x" in caught("block:%d" % i, got, r64, r32)


def test_mutation_drop_scale_of_a_dropped_sample(synth_sd):
    """The drop-connect scale of one sample taken as 1 / keep although its mask is 0, on block 14 of 16.  One sample's share of
    _bn2.weight's gradient falls with the batch and with that sample's upstream gradient (in the measured CVM_VIGOR B = 4 step
    the per-sample norms at this block spread over 0.5 - 1.0 of the largest, so there the fault moves the tensor by far more
    than 3 %); the shape where it stays under 3 %: B = 16 and a dropped sample whose upstream gradient is 1/16 of the others'."""
    i = 14
    k, s, e, cin, cout, sched = S.block_schedule()[i]
    bp, params = block_params(synth_sd("vigor", 0), "sat_efficientnet", i)
    b = 16
    keep = 1 - 0.2 * i / 16
    x, g = synth.normal((b, cin, 4, 4), 1), synth.normal((b, cout, 4, 4), 2)
    g[3] *= 0.0625
    mask = torch.ones(b)
    mask[3] = 0
    r64, r32 = both(S.ref_mbconv, x, params, bp, i, False, mask / keep, g)
    wrong = S.ref_mbconv(x, params, bp, i, False, torch.ones(b) / keep, g, dtype=torch.float32)
    name = "dp:" + bp + "._bn2.weight"
    moved = rel_l2(wrong[name], r32[name])
    print("drop scale: %s moved by %.3e" % (name, moved))
    assert 0 < moved < WHOLE_MODEL_BAR
    got = dict(r32)
    got[name] = wrong[name]
    assert name in caught("block:%d" % i, got, r64, r32)


class _MeanCut(torch.autograd.Function):
    """x.mean over (H, W) whose backward leaves out a channel group: the SE branch's contribution to dmean is lost there."""

    @staticmethod
    def forward(ctx, x, lo, hi):
        ctx.shape, ctx.lo, ctx.hi = x.shape, lo, hi
        return x.sum(dim=(2, 3), keepdim=True) / (x.shape[2] * x.shape[3])

    @staticmethod
    def backward(ctx, g):
        g = g.clone()
        g[:, ctx.lo:ctx.hi] = 0
        return (g / (ctx.shape[2] * ctx.shape[3])).expand(ctx.shape), None, None


def test_mutation_se_gate_left_out_of_dmean(synth_sd, monkeypatch):
    """The squeeze-excite contribution left out of dmean for one channel group (8 of 480 expanded channels)."""
    i = 6
    k, s, e, cin, cout, sched = S.block_schedule()[i]
    bp, params = block_params(synth_sd("vigor", 0), "sat_efficientnet", i)
    x, g = synth.normal((3, cin, 6, 6), 1), synth.normal((3, cout, 6, 6), 2)
    drop = torch.ones(3) / (1 - 0.2 * i / 16)
    r64, r32 = both(S.ref_mbconv, x, params, bp, i, False, drop, g)
    plain = torch.Tensor.mean

    def mean(self, *a, **kw):
        if self.dim() == 4 and kw.get("dim") == (2, 3) and kw.get("keepdim"):
            return _MeanCut.apply(self, 64, 72)
        return plain(self, *a, **kw)
    monkeypatch.setattr(torch.Tensor, "mean", mean)
    wrong = S.ref_mbconv(x, params, bp, i, False, drop, g, dtype=torch.float32)
    monkeypatch.undo()
    assert torch.equal(wrong["out:x"], r32["out:x"])
    name = "dp:" + bp + "._depthwise_conv.weight"
    moved = max(rel_l2(wrong[n], r32[n]) for n in ("din:x", name))
    print("SE dmean: input gradient moved by %.3e, depthwise weight gradient by %.3e"
          % (rel_l2(wrong["din:x"], r32["din:x"]), rel_l2(wrong[name], r32[name])))
    assert 0 < moved < WHOLE_MODEL_BAR
    got = dict(r32)
    got["din:x"], got[name] = wrong["din:x"], wrong[name]
    text = caught("block:%d" % i, got, r64, r32)
    assert "din:x" in text and name in text


def test_mutation_level1_cat_columns_swapped():
    """Level 1's `cat` gradient with the max-score column and its neighbour swapped.  Two columns of k hold about sqrt(4 / k) of
    the tensor when they are alike: 5.3 % at the model's 1 + 1280 columns (measured in the CVM_VIGOR B = 4 step: the two
    columns hold 2.1 % and 2.6 % of the gradient's norm), under 3 % from about 4 500 columns on — 1 + 8191 here."""
    names = ("deconv6", "conv6")
    params = decoder_params(names, 8192, 8, 4, 8, 8, 300)
    cat = synth.normal((2, 8192, 4, 4), 1, std=8191 ** -0.5)          # L2-normalised features, scores in [-1, 1]
    r64, r32 = both(S.ref_decoder_level, cat, synth.normal((2, 4, 8, 8), 2), params, names, synth.normal((2, 8, 8, 8), 3))
    got = dict(r32)
    d = r32["din:cat"].clone()
    d[:, [0, 1]] = d[:, [1, 0]]
    got["din:cat"] = d
    moved = rel_l2(d, r32["din:cat"])
    print("cat columns: gradient moved by %.3e" % moved)
    assert 0 < moved < WHOLE_MODEL_BAR
    assert "din:cat" in caught("dec_loc:1", got, r64, r32)


def test_mutation_dg_one_descriptor_slot_off():
    """One matching level's dg written one descriptor slot (cd) off inside dgdesc, the tensor the ground-descriptor heads
    receive.  The fault moves dgdesc by about 1.4 x that level's share of its norm (in the measured CVM_VIGOR B = 4 step every
    level holds 16 - 60 % of it, so there the fault is far above 3 %); the shape where it stays under 3 %: level 6 (cd = 2,
    40 of 2 520 entries) with an upstream gradient 1/100 of the other levels'."""
    cds, gw, b = synth.MODEL_SPECS["vigor"]["cd"], 20, 2
    parts64, parts32 = [], []
    for j, cd in enumerate(cds):
        L, c, hw, n = gw * cd, 2 * gw * cd if j else gw * cd, 4, 4
        scale = 1e-2 if j == 5 else 1.0
        args = (synth.normal((b, c, hw, hw), 10 + j), synth.normal((b, L), 20 + j), list(range(n)), n, 0, cd, 0,
                scale * synth.normal((b, n, hw, hw), 30 + j), scale * synth.normal((b, c + 1, hw, hw), 40 + j), None)
        r64, r32 = both(S.ref_match_level, *args)
        S.compare("match:%d" % (j + 1), r32, r64, r32)
        parts64.append(r64["din:g"])
        parts32.append(r32["din:g"])
    want64, want32 = torch.cat(parts64, 1), torch.cat(parts32, 1)
    off = want32.clone()
    lo, cd = gw * sum(cds[:5]), cds[5]
    off[:, lo:] = 0
    off[:, lo + cd:] = want32[:, lo:-cd]               # every entry of level 6 one slot late; the last slot falls off the end
    moved = rel_l2(off, want32)
    print("dg slot: dgdesc moved by %.3e" % moved)
    assert 0 < moved < WHOLE_MODEL_BAR
    assert "din:g" in caught("dgdesc", {"din:g": off}, {"din:g": want64}, {"din:g": want32})


def test_mutation_orientation_skip_gradient_missing():
    """The orientation decoder's skip gradient missing from dfeats[10].  The fault moves dfeats[10] by the orientation decoder's
    share of it (measured in the CVM_VIGOR B = 4 step: 28 % at block 10, 11 - 37 % over the five skips, so there it is far above
    3 %); the shape where it stays under 3 %: an orientation upstream gradient 1/100 of the localisation decoder's."""
    skip = synth.normal((2, 6, 12, 12), 1)
    refs = {}
    for branch, names, scale in (("loc", ("deconv5", "conv5"), 1.0), ("ori", ("deconv5_ori", "conv5_ori"), 1e-2)):
        params = decoder_params(names, 9, 8, 6, 8, 8, 500 if branch == "loc" else 600)
        refs[branch] = both(S.ref_decoder_level, synth.normal((2, 9, 6, 6), 2), skip, params, names,
                            scale * synth.normal((2, 8, 12, 12), 3 if branch == "loc" else 4))
    w64, w32 = (refs["loc"][q]["din:skip"] + refs["ori"][q]["din:skip"] for q in (0, 1))
    S.compare("skipsum:10", {"din:sum": w32}, {"din:sum": w64}, {"din:sum": w32})
    wrong = refs["loc"][1]["din:skip"]
    moved = rel_l2(wrong, w32)
    print("skip sum: dfeats[10] moved by %.3e" % moved)
    assert 0 < moved < WHOLE_MODEL_BAR
    assert "din:sum" in caught("skipsum:10", {"din:sum": wrong}, {"din:sum": w64}, {"din:sum": w32})


# ----------------------------------------------------------------------------------------------------------------------
# hook names
# ----------------------------------------------------------------------------------------------------------------------
def test_recorder_hooks_exist_with_expected_parameters():
    for mname, attrs in S.HOOKS.items():
        mod = importlib.import_module(mname)
        for name, params in attrs.items():
            fn = getattr(mod, name, None)
            assert callable(fn), "%s.%s is gone: the Recorder would record nothing" % (mname, name)
            have = [p.name for p in inspect.signature(fn).parameters.values() if p.kind != p.VAR_KEYWORD]
            assert tuple(have[:len(params)]) == params, "%s.%s%s" % (mname, name, inspect.signature(fn))
            assert hasattr(S.Recorder, "_on_" + name.lstrip("_"))
    src = inspect.getsource(importlib.import_module("ccvpe_amd.train"))
    for name in S.HOOKS["ccvpe_amd.train"]:
        assert ("%s(" % name) in src.replace("def %s(" % name, ""), "train.py no longer calls %s by its module-level name" % name
    for name in S.HOOKS["ccvpe_amd.backward"]:
        assert ("bw.%s(" % name) in src, "train.py no longer calls bw.%s" % name


def test_recorder_clones_inside_the_wrapper_and_restores(monkeypatch):
    from ccvpe_amd import backward as bw, train
    before = train._bn_bwd, bw.match_level_bwd
    with monkeypatch.context() as mp:
        def fake(live, name, grads, x_raw, dv, mean, var, act, **kw):
            dv.mul_(2)                     # a later in-place use of the buffer must not reach the record
            return dv
        mp.setattr(train, "_bn_bwd", fake)
        rec = S.Recorder(mp)
        assert bw.match_level_bwd is not before[1]
        dv = torch.ones(3)
        out = train._bn_bwd(None, "sat_efficientnet._blocks.3._bn2", {}, None, dv, None, None, 0, dc_scale=None)
        assert out is dv and torch.equal(rec.bn["sat_efficientnet._blocks.3._bn2"], torch.ones(3))
        train._bn_bwd(None, "sat_efficientnet._blocks.3._bn0", {}, None, dv, None, None, 0)       # not a block boundary
        train._bn_bwd(None, "sat_efficientnet._bn0", {}, None, dv, None, None, 0)
        assert sorted(rec.bn) == ["sat_efficientnet._blocks.3._bn2", "sat_efficientnet._bn0"]
    assert (train._bn_bwd, bw.match_level_bwd) == before
