"""Teacher-forced stage checks of the training step.  TEST INFRASTRUCTURE ONLY, importable without a GPU.

The training step (ccvpe_amd/train.py) is a chain of stages.  forward_train keeps a tape with the fp32 input of every stage,
and backward_train is a chain of module-level calls.  A Recorder wraps those calls and stores, per stage, the fp32 input,
the fp32 upstream gradient and the input gradient the stage returned.  Each stage is then restated ALONE in float64 from
oracle/ccvpe_oracle.py and differentiated with autograd on the recorded tensors, so a comparison carries no chain
amplification: the reference's own fp32 run of one MBConv block sits ~1e-5 from float64, three orders below the 3 % bar of
the whole-model gradient test.  Each link's output gradient is the next link's recorded input, so nothing hides between links.

Contents: (a) float64 stage references, (b) layout adapters, (c) the Recorder, (d) Report / compare, (e) StepChecker, which
walks a recorded step stage by stage and then checks the joins train.py assembles itself (skip gradients, dgdesc, level 1's
cat gradient); StepChecker.loss_link is the chain's first link: the loss value and the gradients on the nine outputs against the
benched loss mix restated on the recorded outputs.  Besides the calls of the backward chain the Recorder wraps train.backward_train (the gradients arriving on the
nine outputs) and bw.l2norm2_bwd (the raw orientation field, which the tape does not hold).
"""
import math
import time

import torch
import torch.nn.functional as F

from oracle import ccvpe_oracle as O

FLOOR_FWD = 1e-4        # forward outputs and batch statistics: the `close` default of tests/test_ops_gpu.py
FLOOR_GRAD = 2e-4       # gradients: the B = 64 backward-kernel bar of tests/test_fullsize_train_kernels_gpu.py
REF_FACTOR = 4.0        # granted for a different summation order (test_full_backward_vs_reference_autograd)
NOISE_REF = 1e-6        # a parameter gradient whose fp64 reference is below this fraction of the step's largest is zero
NOISE_GOT = 1e-4        # ... and the implementation's must then stay below this fraction (golden_util.compare_grads)
MAX_NOISE_SHARE = 0.10


# ----------------------------------------------------------------------------------------------------------------------
# (a) float64 stage references
# ----------------------------------------------------------------------------------------------------------------------
def _run(fn, inputs, params, gouts, dtype, consts=None):
    """fn(inputs, sd) -> {name: output}.  inputs / params: {name: tensor}, made leaves of `dtype`; gouts: {output name:
    upstream gradient or None}.  Returns {"out:N": output, "din:N": input gradient, "dp:N": parameter gradient}."""
    def leaf(t):
        return t.detach().cpu().to(dtype).clone().requires_grad_(True)
    xin = {k: leaf(v) for k, v in inputs.items() if v is not None}
    sd = {k: leaf(v) for k, v in params.items()}
    for k in list(sd):                       # batch-statistic BatchNorm: fresh running statistics, not differentiated
        if k.endswith(".weight") and sd[k].dim() == 1 and "_bn" in k.rsplit(".", 2)[-2]:
            p = k[:-len(".weight")]
            sd[p + ".running_mean"] = torch.zeros_like(sd[k]).detach()
            sd[p + ".running_var"] = torch.ones_like(sd[k]).detach()
    for k, v in (consts or {}).items():
        xin[k] = None if v is None else v.detach().cpu().to(dtype)
    for k, v in inputs.items():
        if v is None:
            xin[k] = None
    outs = fn(xin, sd)
    res = {"out:" + k: v.detach() for k, v in outs.items()}
    loss = None
    for k, g in gouts.items():
        if g is None:
            continue
        term = (outs[k] * g.detach().cpu().to(dtype).reshape(outs[k].shape)).sum()
        loss = term if loss is None else loss + term
    if loss is None:
        return res
    leaves = [(("din:" + k), v) for k, v in xin.items() if v is not None and v.requires_grad]
    leaves += [(("dp:" + k), v) for k, v in sd.items() if v.requires_grad]
    grads = torch.autograd.grad(loss, [v for _, v in leaves], allow_unused=True)
    for (k, v), g in zip(leaves, grads):
        res[k] = torch.zeros_like(v).detach() if g is None else g.detach()
    return res


def block_schedule():
    """[(k, s, e, cin, cout, sched)] per MBConv block: the static-224 schedule argument as efficientnet_features computes it."""
    sched = math.ceil(O.STATIC_IMAGE_SIZE / 2)
    out = []
    for (k, s, e, cin, cout) in O.B0_BLOCKS:
        out.append((k, s, e, cin, cout, sched))
        sched = math.ceil(sched / s)
    return out


def ref_stem(img, params, prefix, circular, g_out, dtype=torch.float64):
    """stem conv + _bn0 + swish.  The image receives no gradient in the step; only the parameters are differentiated."""
    def fn(x, sd):
        raw = O.same_conv(x["img"], sd[prefix + "._conv_stem.weight"], 3, 2, O.STATIC_IMAGE_SIZE, circular)
        return {"x": O.swish(O.bn_eval(raw, sd, prefix + "._bn0", {}))}
    return _run(fn, {}, params, {"x": g_out}, dtype, consts={"img": img})


def ref_mbconv(x, params, p, i, circular, drop_scale, g_out, dtype=torch.float64):
    """MBConv block i (block 0 without expand; skip blocks with the per-sample drop scale; stride 2 and 5x5 included)."""
    k, s, e, cin, cout, sched = block_schedule()[i]

    def fn(xi, sd):
        return {"x": O.mbconv(xi["x"], sd, p, k, s, e, cin, cout, sched, circular, {}, xi["drop"])}
    return _run(fn, {"x": x}, params, {"x": g_out}, dtype, consts={"drop": drop_scale})


def ref_head(x, params, prefix, g_out, dtype=torch.float64):
    """_conv_head + _bn1 + swish."""
    def fn(xi, sd):
        return {"x": O.swish(O.bn_eval(F.conv2d(xi["x"], sd[prefix + "._conv_head.weight"]), sd, prefix + "._bn1", {}))}
    return _run(fn, {"x": x}, params, {"x": g_out}, dtype)


def ref_ground_descriptors(feat, params, g_out, dtype=torch.float64):
    """All six ground-descriptor heads from gfeat, concatenated in level order ([B, sum_l w * Cd_l])."""
    def fn(xi, sd):
        return {"gdesc": torch.cat([O.ground_descriptor(xi["x"], sd, l) for l in range(1, 7)], dim=1)}
    return _run(fn, {"x": feat}, params, {"gdesc": g_out}, dtype)


def ref_aerial_descriptor(vol, params, g_out, dtype=torch.float64):
    def fn(xi, sd):
        return {"x": O.aerial_descriptor(xi["x"], sd)}
    return _run(fn, {"x": vol}, params, {"x": g_out}, dtype)


def ref_match_level(x, g, shifts, n_max, n_tail, stride, win_off, g_sc, g_cat, g_tail, dtype=torch.float64):
    """One matching level.  Outputs: sc [B,n,H,W]; cat = [max over the first n_max shifts, normalised x] (reference order);
    tail = the last n_tail scores (level 1: what the orientation decoder reads in front of the same normalised x)."""
    def fn(xi, sd):
        sc = O.rotational_matching(xi["x"], xi["g"], shifts, stride, win_off)
        out = {"sc": sc, "cat": O.lmu_input(xi["x"], sc[:, :n_max])}
        if n_tail:
            out["tail"] = sc[:, len(shifts) - n_tail:]
        return out
    gouts = {"sc": g_sc, "cat": g_cat}
    if n_tail:
        gouts["tail"] = g_tail
    return _run(fn, {"x": x, "g": g}, {}, gouts, dtype)


def ref_decoder_level(cat, skip, params, names, g_out, dtype=torch.float64, relu_mask=None, seen=None):
    """deconv k2 s2 -> cat skip -> 3x3 + ReLU -> 3x3 (the last level's second conv is the 16 -> 1 / 16 -> 2 head).
    seen: a dict that receives the pre-activation of the ReLU ("pre").  relu_mask: a boolean tensor that replaces the
    ReLU's own decision v > 0 (see relu_mask_at_discontinuity)."""
    deconv, conv = names

    def relu(v):
        if seen is not None:
            seen["pre"] = v.detach()
        return F.relu(v) if relu_mask is None else v * relu_mask.to(v.dtype)

    def fn(xi, sd):
        u = O.up(xi["cat"], sd, deconv)
        if xi["skip"] is not None:
            u = torch.cat([u, xi["skip"]], dim=1)
        return {"x": O.double_conv(u, sd, conv, relu)}
    return _run(fn, {"cat": cat, "skip": skip}, params, {"x": g_out}, dtype)


def relu_mask_at_discontinuity(pre64, pre32, taped_y):
    """The ReLU's derivative jumps at 0, and a pre-activation smaller than the fp32 round-off of its own accumulation has no
    determined sign in fp32: the fp64 restatement and a correct fp32 implementation may then differentiate two different
    functions.  Elements with |pre64| <= 4 x the largest error of the reference's own fp32 pre-activation are AT the
    discontinuity; where the taped activation's sign decision differs from the fp64 one there, the taped decision is the
    one differentiated (by the fp64 and the fp32 reference alike).  A disagreement anywhere else is left to fail.
    Returns (mask or None when nothing changes, number of elements taken from the tape, tau).

    tau is one value per tensor: the error of an fp32 accumulation at one element is a random draw, its bound is the tensor's.

    Measured (profiles/r08/stage_checks.txt; CVM_VIGOR B = 4, conv6.0, K = 9 x 1344): one element of 655 360, fp64 pre-activation +1.08e-7 (2e-8 of the
    tensor's largest), taped 0; alone it moved conv6.0.bias by 1.1e-3 of its largest entry and the level's input gradients
    by 1.6e-4 relative L2, and with the taped decision conv6.0.bias agrees to 4e-7.  The reference's own fp32 run lands on
    either side of 0 there under a changed summation order, on the CPU: +6.7e-8 as is, +2.1e-7 channels-last, +2.2e-8 with the
    input channels reversed, -1.2e-7 with the input channels permuted."""
    tau = REF_FACTOR * float((pre32.double() - pre64).abs().max())
    want, have = pre64 > 0, taped_y.detach().cpu() > 0
    take = (want != have) & (pre64.abs() <= tau)
    n = int(take.sum())
    return (torch.where(take, have, want) if n else None), n, tau


def ref_softmax_head(logits, g_logits, g_heat, dtype=torch.float64):
    """softmax over the flattened map; gradients may arrive on the logits and on the heat-map."""
    def fn(xi, sd):
        lg = xi["logits"].flatten(1)
        return {"logits": lg, "heat": torch.softmax(lg, dim=-1)}
    return _run(fn, {"logits": logits}, {}, {"logits": g_logits, "heat": g_heat}, dtype)


def ref_normalize_head(raw, g_out, dtype=torch.float64):
    def fn(xi, sd):
        return {"x": F.normalize(xi["raw"], p=2, dim=1)}
    return _run(fn, {"raw": raw}, {}, {"x": g_out}, dtype)


# The first link: the benched loss mix on the nine outputs.  Output index -> tensor name; output 1, the heat-map, is not read.
LOSS_OUTPUTS = {0: "logits", 2: "ori", 3: "scores1", 4: "scores2", 5: "scores3", 6: "scores4", 7: "scores5", 8: "scores6"}
LOSS_DEVICE_MIN_ELEMENTS = 4 * 1024 * 1024    # an output above this is restated where it lives (float64 tensor operations on the device)
LOSS_CROSSCHECK = 1e-12                       # ... and a two-sample sub-batch of it both ways must agree to this


def _loss_term(i, outs, targets, dtype, dev, need_grad, samples=None):
    """The mix's term that reads output i — cross_entropy (0), 1e1 * orientation (2), 1e4 * infoNCE / 6 (3 .. 8), the oracle's
    three functions — in `dtype` on `dev`, on the first `samples` samples if given.  Returns (term, its gradient on output i or
    None).  The infoNCE mask `> 1e-2` is decided identically on a float32 label and on its float64 copy (0.01f < 0.01 <
    nextafter(0.01f))."""
    gt, gt_flat, gt_ori, labels = targets

    def c(t):
        return t.detach()[:samples].to(device=dev, dtype=dtype)
    x = c(outs[i]).clone().requires_grad_(need_grad)
    with torch.set_grad_enabled(need_grad):
        if i == 0:
            term = O.cross_entropy_loss(x.flatten(1), c(gt_flat).flatten(1))
        elif i == 2:
            term = 1e1 * O.orientation_loss(x, c(gt_ori), c(gt))
        else:
            term = 1e4 * O.infonce_loss(x.flatten(1), c(labels[i - 3]).flatten(1)) / 6
    grad = torch.autograd.grad(term, x)[0].detach() if need_grad else None
    return term.detach(), grad


def _loss_device(t):
    return t.device if t.numel() > LOSS_DEVICE_MIN_ELEMENTS else torch.device("cpu")


def ref_loss_mix(outs, targets, outputs=None, dtype=torch.float64):
    """cross_entropy + 1e4 * sum(infoNCE) / 6 + 1e1 * orientation (the benched step's loss) on the recorded outputs, and its
    gradient on every output in `outputs` (default: all eight the mix reads).  targets = (gt, gt_flat, gt_ori, labels) as
    targets.train_targets returns them.  The terms share no input, so each is differentiated alone; an output above
    LOSS_DEVICE_MIN_ELEMENTS elements is restated on its own device.  An output not in `outputs` still enters the value."""
    outputs = sorted(LOSS_OUTPUTS) if outputs is None else outputs
    res, loss = {}, torch.zeros((), dtype=dtype)
    for i in sorted(LOSS_OUTPUTS):
        term, grad = _loss_term(i, outs, targets, dtype, _loss_device(outs[i]), i in outputs)
        loss = loss + term.cpu()
        if grad is not None:
            res["din:" + LOSS_OUTPUTS[i]] = grad
    res["out:loss"] = loss
    return res


def loss_device_crosscheck(outs, targets, i, samples=2):
    """Output i's term and gradient on a `samples`-sample sub-batch, float64, on the CPU and on the output's device: the largest
    difference relative to the CPU result's largest value (term, gradient)."""
    a = _loss_term(i, outs, targets, torch.float64, torch.device("cpu"), True, samples)
    b = _loss_term(i, outs, targets, torch.float64, outs[i].device, True, samples)
    return tuple(float((p - q.cpu()).abs().max()) / (float(p.abs().max()) + 1e-300) for p, q in zip(a, b))


def ref_bn_stats(raw_nchw, dtype=torch.float64):
    """Batch mean and biased variance per channel of a raw (pre-BatchNorm) tensor."""
    x = raw_nchw.detach().cpu().to(dtype)
    return {"stat:mean": x.mean(dim=(0, 2, 3)), "stat:var": x.var(dim=(0, 2, 3), unbiased=False)}


# ----------------------------------------------------------------------------------------------------------------------
# (b) layout adapters
# ----------------------------------------------------------------------------------------------------------------------
def to_nchw(t):
    return None if t is None else t.detach().cpu().permute(0, 3, 1, 2).contiguous()


def to_nhwc(t):
    return None if t is None else t.detach().cpu().permute(0, 2, 3, 1).contiguous()


def cat_to_ref(cat_nhwc, col_map, k_used, must_be_zero="pad"):
    """This implementation's `cat` columns [B,H,W,ld] -> the reference's channel order [B,k_ref,H,W] through the col_map
    (ours first column, reference first channel, count) the real call receives.  Columns from k_used up to ld are padding:
    dropped and asserted zero.  must_be_zero="unmapped": every column the map does not cover must be zero (gradients)."""
    t = cat_nhwc.detach().cpu()
    k_ref = sum(n for _, _, n in col_map)
    out = t.new_zeros(t.shape[:3] + (k_ref,))
    covered = torch.zeros(t.shape[-1], dtype=torch.bool)
    for d0, s0, n in col_map:
        out[..., s0:s0 + n] = t[..., d0:d0 + n]
        covered[d0:d0 + n] = True
    zero = ~covered if must_be_zero == "unmapped" else torch.arange(t.shape[-1]) >= k_used
    if bool(zero.any()):
        assert float(t[..., zero].abs().max()) == 0.0, "non-zero values in columns %s" % zero.nonzero().flatten().tolist()
    return out.permute(0, 3, 1, 2).contiguous()


def match_cat_to_ref(ddst_nhwc, c, n_tail):
    """A matching level's `cat` row, or the gradient arriving on it, [B,H,W,ldo] in this implementation's order
    [x (c), max, tail (n_tail), pad] -> (the reference's [max, x] cat, the tail scores or None).  Pad columns are asserted zero."""
    g_cat = cat_to_ref(ddst_nhwc, [(0, 1, c), (c, 0, 1)], c + 1 + n_tail)
    g_tail = to_nchw(ddst_nhwc[..., c + 1:c + 1 + n_tail]) if n_tail else None
    return g_cat, g_tail


# ----------------------------------------------------------------------------------------------------------------------
# (c) recorder
# ----------------------------------------------------------------------------------------------------------------------
# module -> {attribute: parameter names the recorder relies on}; tests/test_stage_check.py checks them against the code
HOOKS = {
    "ccvpe_amd.train": {
        "forward_train": ("model", "grd", "sat", "drop_masks", "rec"),
        "backward_train": ("model", "tape", "gout", "on_ready"),
        "_bn_bwd": ("live", "name", "grads", "x_raw", "dv", "mean", "var", "act"),
        "_decoder_level_backward": ("live", "lv", "t", "dout", "last", "names", "col_map", "dfeats", "skip_block", "grads",
                                    "bwd", "defer"),
        "encoder_backward": ("e", "live", "prefix", "tape", "dfeat", "dfeats", "circular", "grads", "bwd"),
    },
    "ccvpe_amd.backward": {
        "match_level_bwd": ("x", "g", "L", "shifts", "n_max", "n_tail", "stride", "scores", "dscores", "ddst", "channels",
                            "dg_out", "window_offset"),
        "ground_descriptor_bwd": ("y1", "wh", "cd", "dout"),
        "conv2x2s2_dgrad": ("dy", "w", "wp"),
        "l2norm2_bwd": ("raw", "dout"),
    },
}


def _clone(t):
    return None if t is None else t.detach().clone()


class Recorder(object):
    """Wraps the module-level calls of the backward chain (HOOKS) through a pytest.MonkeyPatch.  Every upstream gradient is
    cloned INSIDE the wrapper, so the copy is enqueued on whatever stream the step uses at that moment; the three-stream
    schedule stays as it is.  keep(stage key) -> bool limits what is cloned (B = 64)."""

    def __init__(self, monkeypatch, keep=None):
        import inspect
        from ccvpe_amd import backward as bw, train
        self.keep = keep or (lambda key: True)
        self.tape, self.outs, self.gout, self.raw_ori = None, None, None, None
        self.bn, self.dec, self.match, self.enc = {}, {}, {}, {}
        self.gd, self.sd = None, None
        mods = {"ccvpe_amd.train": train, "ccvpe_amd.backward": bw}

        for mname, attrs in HOOKS.items():
            for name in attrs:
                orig = getattr(mods[mname], name)
                setattr(self, "_orig_" + name, orig)
                handler = getattr(self, "_on_" + name.lstrip("_"))

                def wrapper(*args, _orig=orig, _name=name, _handler=handler, **kwargs):
                    a = dict(inspect.signature(_orig).bind(*args, **kwargs).arguments)
                    return _handler(a, lambda: _orig(*args, **kwargs))
                monkeypatch.setattr(mods[mname], name, wrapper)

    # -- forward / backward entry ------------------------------------------------------------------------------------
    def _on_forward_train(self, a, call):
        outs, tape = call()
        if tape is not None:
            self.tape, self.outs = tape, outs
            self.bn, self.dec, self.match, self.enc, self.gd, self.sd = {}, {}, {}, {}, None, None
        return outs, tape

    def _on_backward_train(self, a, call):
        self.gout = [_clone(g) for g in a["gout"]]
        return call()

    def _on_l2norm2_bwd(self, a, call):
        self.raw_ori = _clone(a["raw"])
        return call()

    # -- encoder -----------------------------------------------------------------------------------------------------
    def _on_bn_bwd(self, a, call):
        name = a["name"]
        boundary = name.endswith("._bn2") or name.count(".") == 1       # block outputs; prefix._bn0 / prefix._bn1
        if boundary and self.keep(("bn", name)):
            self.bn[name] = _clone(a["dv"])
        return call()

    def _on_encoder_backward(self, a, call):
        p = a["prefix"]
        self.enc[p] = dict(dfeat=_clone(a["dfeat"]), dfeats={i: _clone(t) for i, t in a["dfeats"].items()})
        return call()

    # -- decoders ----------------------------------------------------------------------------------------------------
    def _on_decoder_level_backward(self, a, call):
        branch = "ori" if a["names"][0].endswith("_ori") else "loc"
        lvl = int(a["names"][1][4])                                      # convK / convK_ori
        key = (branch, 6 - lvl)
        sb, dfeats = a["skip_block"], a["dfeats"]
        if not self.keep(("dec",) + key):
            return call()
        r = dict(dout=_clone(a["dout"]), col_map=list(a["col_map"]), last=bool(a["last"]), names=tuple(a["names"]),
                 skip_block=sb, k=a["t"]["k"], skip_before=_clone(dfeats.get(sb)) if sb is not None else None)
        ret = call()
        r["dcat"] = _clone(ret)
        r["skip_after"] = _clone(dfeats.get(sb)) if sb is not None else None
        self.dec[key] = r
        return ret

    # -- matching / descriptors ----------------------------------------------------------------------------------------
    def _on_match_level_bwd(self, a, call):
        j = [mt["x"] is a["x"] for mt in self.tape["match"]].index(True)      # the level whose taped input this call received
        if not self.keep(("match", j)):
            return call()
        r = dict(dscores=_clone(a["dscores"]), ddst=_clone(a["ddst"]))
        ret = call()
        r["dx"], r["dg"] = _clone(ret), _clone(a["dg_out"])
        self.match[j] = r
        return ret

    def _on_ground_descriptor_bwd(self, a, call):
        self.gd = dict(dout=_clone(a["dout"])) if self.keep(("gd",)) else None
        return call()

    def _on_conv2x2s2_dgrad(self, a, call):
        ret = call()
        if self.keep(("sd",)):
            self.sd = dict(dy=_clone(a["dy"]), dx=_clone(ret))
        return ret


# ----------------------------------------------------------------------------------------------------------------------
# (d) comparison
# ----------------------------------------------------------------------------------------------------------------------
def _errors(a, ref):
    a, ref = a.detach().cpu().double().reshape(-1), ref.detach().cpu().double().reshape(-1)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    d = a - ref
    mx, l2 = float(ref.abs().max()), float(ref.norm())
    if mx == 0.0:
        z = float(d.abs().max())
        return (0.0, 0.0) if z == 0.0 else (float("inf"), float("inf"))
    return float(d.abs().max()) / mx, float(d.norm()) / l2


def _floor(name):
    return FLOOR_FWD if name.startswith(("out:", "stat:")) else FLOOR_GRAD


class Report(object):
    """Collects every comparison before asserting, so that one run reports all margins.  Rows are
    (stage, tensor, e_got, e_ref, bar); a tensor gives one row per metric (max-abs error over max |ref64|, relative L2).
    e_ref is the same metric for the reference's own fp32 run and never involves the code under test."""

    def __init__(self):
        self.rows = []
        self._params = []          # (row indices, max |ref64|, max |got|, max |ref32|)
        self.noise = []

    def compare(self, stage, got, ref64, ref32, exceptions=None):
        """got: {tensor name: tensor} (a subset of the references' keys).  exceptions: {tensor name: factor on the bar}, each
        with its CPU evidence written beside the caller's entry."""
        for name, g in got.items():
            if g is None:
                continue
            eg, er = _errors(g, ref64[name]), _errors(ref32[name], ref64[name])
            idx = []
            for metric, e_got, e_ref in (("max", eg[0], er[0]), ("l2", eg[1], er[1])):
                bar = max(_floor(name), REF_FACTOR * e_ref) * (exceptions or {}).get(name, 1.0)
                idx.append(len(self.rows))
                self.rows.append((stage, "%s [%s]" % (name, metric), e_got, e_ref, bar))
            if name.startswith("dp:"):
                self._params.append((idx, float(ref64[name].abs().max()), float(g.detach().abs().max()),
                                     float(ref32[name].abs().max())))
        return self

    def finish(self):
        """Applies the noise-level rule to the parameter gradients: decided by the fp64 reference alone."""
        if self._params:
            top = max(p[1] for p in self._params)
            for idx, m64, mgot, m32 in self._params:
                if m64 < NOISE_REF * top:
                    stage, name = self.rows[idx[0]][0], self.rows[idx[0]][1].rsplit(" [", 1)[0]
                    self.rows[idx[0]] = (stage, name + " [noise]", mgot / top, m32 / top, NOISE_GOT)
                    self.rows[idx[1]] = None
                    self.noise.append((stage, name))
            self.rows = [r for r in self.rows if r is not None]
            self._params = []
        return self

    def failures(self):
        self.finish()
        return [r for r in self.rows if not r[2] <= r[4]]

    def tensors(self):
        self.finish()
        return len(set((r[0], r[1].rsplit(" [", 1)[0]) for r in self.rows))

    def assert_ok(self):
        bad = self.failures()
        assert not bad, "%d comparisons outside their bar:\n%s" % (len(bad), format_rows(bad))
        assert len(self.noise) <= MAX_NOISE_SHARE * self.tensors(), \
            "%d of %d tensors treated as noise-level" % (len(self.noise), self.tensors())

    def worst_by_kind(self):
        """{stage kind: (e_got, e_ref, bar, stage, tensor)} of the row with the largest e_got / bar."""
        self.finish()
        out = {}
        for stage, tensor, e_got, e_ref, bar in self.rows:
            kind = stage_kind(stage)
            if kind not in out or e_got / bar > out[kind][0] / out[kind][2]:
                out[kind] = (e_got, e_ref, bar, stage, tensor)
        return out


def stage_kind(stage):
    s = stage.split(" ")[0]
    return s.split(":")[0]


def format_rows(rows):
    return "\n".join("  %-44s %-52s e_got %.3e  e_ref %.3e  bar %.3e%s" % (r[0], r[1], r[2], r[3], r[4], "" if r[2] <= r[4] else "  <-- FAIL")
                     for r in rows)


def compare(stage, got, ref64, ref32):
    """One stage: collect all comparisons, assert, return the rows."""
    rep = Report().compare(stage, got, ref64, ref32)
    rep.assert_ok()
    return rep.rows


# ----------------------------------------------------------------------------------------------------------------------
# (e) one recorded step, stage by stage
# ----------------------------------------------------------------------------------------------------------------------
def skip_block(i):
    k, s, e, cin, cout = O.B0_BLOCKS[i]
    return s == 1 and cin == cout


def params_under(named, prefix):
    return {n: p for n, p in named.items() if n.startswith(prefix + ".")}


class StepChecker(object):
    """Walks a recorded step.  named: {parameter name: parameter} (values fp32, own layout); grads: {name: .grad}.
    want(stage key) selects the stages (the same predicate the Recorder was given).  Every check goes into self.report;
    self.checked collects the parameter names whose gradient was compared."""

    def __init__(self, rec, named, grads, want=None):
        self.rec, self.tape, self.named, self.grads = rec, rec.tape, named, grads
        self.want = want or (lambda key: True)
        self.report = Report()
        self.checked = set()
        self.relu_taken = []         # (stage, elements whose ReLU decision came from the tape, of, tau)
        self.dg_refs, self.cat_refs = {}, {}    # level -> (fp64, fp32) din:g; branch -> (fp64, fp32) din:cat of level 1
        self.skip_refs = {}          # (branch, skip block) -> fp64 skip gradient of that decoder level
        self.stages = []
        self.loss_left_out, self.loss_crosschecks, self.loss_seconds = [], [], 0.0   # loss_link: outputs not compared; (name, dv, dg); wall time

    def _both(self, fn, *args):
        return fn(*args, dtype=torch.float64), fn(*args, dtype=torch.float32)

    def _pgot(self, params):
        self.checked.update(params)
        return {"dp:" + n: self.grads[n] for n in params}

    def _cmp(self, stage, got, refs):
        self.stages.append(stage)
        self.report.compare(stage, got, refs[0], refs[1])

    def _stats(self, stage, raw_nhwc, mean, var):
        raw = to_nchw(raw_nhwc)
        self.report.compare(stage, {"stat:mean": mean, "stat:var": var}, ref_bn_stats(raw), ref_bn_stats(raw, torch.float32))

    # -- encoders ----------------------------------------------------------------------------------------------------
    def encoder(self, prefix, circular, feat_next):
        """feat_next: the taped tensor the head's output must equal (gfeat / svol)."""
        tp, rec = self.tape["grd" if prefix.startswith("grd") else "sat"], self.rec
        blocks = tp["blocks"]
        dfeats = rec.enc[prefix]["dfeats"] if prefix in rec.enc else {}
        if self.want(("stem", prefix)):
            img, stem_raw, m, v = tp["stem"]
            params = {n: self.named[n] for n in (prefix + "._conv_stem.weight", prefix + "._bn0.weight", prefix + "._bn0.bias")}
            g = to_nchw(rec.bn[prefix + "._bn0"])
            refs = self._both(ref_stem, img, params, prefix, circular, g)
            got = {"out:x": to_nchw(blocks[0]["x_in"])}
            got.update(self._pgot(params))
            self._cmp("stem:%s" % prefix, got, refs)
            self._stats("stem:%s" % prefix, stem_raw, m, v)
        for i, s in enumerate(blocks):
            if not self.want(("block", prefix, i)):
                continue
            bp = "%s._blocks.%d" % (prefix, i)
            params = params_under(self.named, bp)
            g = to_nchw(rec.bn[bp + "._bn2"])
            refs = self._both(ref_mbconv, to_nchw(s["x_in"]), params, bp, i, circular, s["dc"], g)
            nxt = blocks[i + 1]["x_in"] if i + 1 < len(blocks) else tp["head"][0]
            got = {"out:x": to_nchw(nxt)}
            got.update(self._pgot(params))
            stage = "block:%s.%d" % (prefix, i)
            # the gradient at the output of block i-1 is block i's input gradient plus the decoders' skip gradient
            below = rec.bn[bp.rsplit(".", 1)[0] + ".%d._bn2" % (i - 1)] if i else rec.bn[prefix + "._bn0"]
            if i and (i - 1) in dfeats:
                add = to_nchw(dfeats[i - 1]).double()
                refs = tuple(dict(r, **{"din:x": r["din:x"].double() + add}) for r in refs)
            got["din:x"] = to_nchw(below)
            self._cmp(stage, got, refs)
            if "e_raw" in s:
                self._stats(stage + " bn0", s["e_raw"], s["m0"], s["v0"])
            self._stats(stage + " bn1", s["u_raw"], s["m1"], s["v1"])
            self._stats(stage + " bn2", s["p_raw"], s["m2"], s["v2"])
        if self.want(("head", prefix)):
            x_last, h_raw, m, v = tp["head"]
            params = {n: self.named[n] for n in (prefix + "._conv_head.weight", prefix + "._bn1.weight", prefix + "._bn1.bias")}
            refs = self._both(ref_head, to_nchw(x_last), params, prefix, to_nchw(rec.bn[prefix + "._bn1"]))
            if 15 in dfeats:
                add = to_nchw(dfeats[15]).double()
                refs = tuple(dict(r, **{"din:x": r["din:x"].double() + add}) for r in refs)
            got = {"out:x": to_nchw(feat_next), "din:x": to_nchw(rec.bn[prefix + "._blocks.15._bn2"])}
            got.update(self._pgot(params))
            self._cmp("head:%s" % prefix, got, refs)
            self._stats("head:%s" % prefix, h_raw, m, v)

    # -- descriptors -------------------------------------------------------------------------------------------------
    def descriptors(self):
        rec, tape = self.rec, self.tape
        if self.want(("gd",)):
            params = {n: p for n, p in self.named.items() if n.startswith("grd_feature_to_descriptor")}
            refs = self._both(ref_ground_descriptors, to_nchw(tape["gfeat"]), params, rec.gd["dout"])
            got = {"out:gdesc": tape["gdesc"], "din:x": to_nchw(rec.enc["grd_efficientnet"]["dfeat"])}
            got.update(self._pgot(params))
            self._cmp("gdesc", got, refs)
        if self.want(("sd",)):
            params = params_under(self.named, "sat_feature_to_descriptors.1")
            refs = self._both(ref_aerial_descriptor, to_nchw(tape["svol"]), params, to_nchw(rec.sd["dy"]))
            got = {"out:x": to_nchw(tape["match"][0]["x"]), "din:x": to_nchw(rec.sd["dx"])}
            got.update(self._pgot(params))
            self._cmp("sdesc", got, refs)

    # -- matching ----------------------------------------------------------------------------------------------------
    def matching(self, j):
        if not self.want(("match", j)):
            return
        rec, tape = self.rec, self.tape
        mt, r = tape["match"][j], rec.match[j]
        c, n_tail = mt["c"], mt["n_tail"]
        x = to_nchw(mt["x"][..., :c])
        g = tape["gdesc"][:, mt["goff"]:mt["goff"] + mt["L"]]
        g_cat, g_tail = match_cat_to_ref(r["ddst"], c, n_tail)
        refs = self._both(ref_match_level, x, g, list(mt["shifts"]), mt["n_max"], n_tail, mt["stride"], mt["woff"],
                          r["dscores"], g_cat, g_tail)
        cat, tail = match_cat_to_ref(tape["loc"][j]["cat"], c, n_tail)
        got = {"out:sc": mt["sc"], "out:cat": cat, "din:x": to_nchw(r["dx"]), "din:g": r["dg"]}
        if n_tail:
            got["out:tail"] = tail
        self._cmp("match:%d" % (j + 1), got, refs)
        self.dg_refs[j] = (refs[0]["din:g"], refs[1]["din:g"])

    # -- decoders ----------------------------------------------------------------------------------------------------
    def decoder(self, branch, j, out_next):
        """out_next: what the level's forward output must equal (NCHW tensor on any device)."""
        if not self.want(("dec", branch, j)):
            return
        rec = self.rec
        t, r = self.tape[branch][j], rec.dec[(branch, j)]
        deconv, conv = r["names"]
        params = dict(params_under(self.named, deconv))
        params.update(params_under(self.named, conv))
        k_used = max(d0 + n for d0, _, n in r["col_map"])
        cat = cat_to_ref(t["cat"], r["col_map"], max(k_used, self._cat_used(branch, j)))
        dout = r["dout"] if r["last"] else to_nchw(r["dout"])
        seen64, seen32 = {}, {}
        skip = to_nchw(t["skip"])
        refs = (ref_decoder_level(cat, skip, params, (deconv, conv), dout, seen=seen64),
                ref_decoder_level(cat, skip, params, (deconv, conv), dout, dtype=torch.float32, seen=seen32))
        mask, n, tau = relu_mask_at_discontinuity(seen64["pre"], seen32["pre"], to_nchw(t["y"]))
        if mask is not None:
            self.relu_taken.append(("dec_%s:%d" % (branch, j + 1), n, mask.numel(), tau))
            refs = self._both(lambda *a, dtype: ref_decoder_level(*a, dtype=dtype, relu_mask=mask), cat, skip, params, (deconv, conv), dout)
        got = {"out:x": out_next, "din:cat": cat_to_ref(r["dcat"], r["col_map"], k_used, must_be_zero="unmapped")}
        if t["skip"] is not None:
            assert r["skip_before"] is None, "the skip gradient of %s level %d was accumulated into an existing tensor" % (branch, j + 1)
            got["din:skip"] = to_nchw(r["skip_after"])
            self.skip_refs[(branch, r["skip_block"])] = (refs[0]["din:skip"], refs[1]["din:skip"])
        if j == 0:
            self.cat_refs[branch] = (refs[0]["din:cat"], refs[1]["din:cat"])
        got.update(self._pgot(params))
        self._cmp("dec_%s:%d" % (branch, j + 1), got, refs)

    def _cat_used(self, branch, j):
        if j:
            return 0
        mt = self.tape["match"][0]
        return mt["c"] + 1 + mt["n_tail"]

    def skip_sums(self):
        """The captured dfeats[b] equals the sum of the two decoders' skip gradients from their fp64 references."""
        dfeats = self.rec.enc["sat_efficientnet"]["dfeats"]
        for b, t in sorted(dfeats.items()):
            if ("loc", b) in self.skip_refs and ("ori", b) in self.skip_refs:
                w64, w32 = (self.skip_refs[("loc", b)][q] + self.skip_refs[("ori", b)][q] for q in (0, 1))
                self.report.compare("skipsum:%d" % b, {"din:sum": to_nchw(t)}, {"din:sum": w64}, {"din:sum": w32})
                self.stages.append("skipsum:%d" % b)

    def joins(self):
        """The two places where gradients of several links are assembled by train.py itself, compared as assembled:
        dgdesc, which the ground-descriptor heads receive, against the six levels' fp64 dg concatenated at the reference's
        offsets (a `goff` slice one level out moves a level's dg inside it); and the gradient level 1's matching receives on
        its `cat` row against the localisation decoder's fp64 cat gradient plus the orientation decoder's (shared normalised
        features summed, max column from the one, the n_rot tail scores from the other)."""
        if len(self.dg_refs) == 6 and self.rec.gd is not None:
            w64, w32 = (torch.cat([self.dg_refs[j][q] for j in range(6)], dim=1) for q in (0, 1))
            self.report.compare("dgdesc", {"din:g": self.rec.gd["dout"]}, {"din:g": w64}, {"din:g": w32})
            self.stages.append("dgdesc")
        if "loc" in self.cat_refs and "ori" in self.cat_refs and 0 in self.rec.match:
            mt = self.tape["match"][0]
            n = mt["n_tail"]
            got_cat, got_tail = match_cat_to_ref(self.rec.match[0]["ddst"], mt["c"], n)
            want = []
            for q in (0, 1):
                cat = self.cat_refs["loc"][q].clone()
                cat[:, 1:] += self.cat_refs["ori"][q][:, n:]
                want.append({"din:cat": cat, "din:tail": self.cat_refs["ori"][q][:, :n]})
            self.report.compare("catsum:1", {"din:cat": got_cat, "din:tail": got_tail}, want[0], want[1])
            self.stages.append("catsum:1")

    # -- the loss -----------------------------------------------------------------------------------------------------
    def loss_link(self, targets, loss):
        """The first link: rec.gout, the gradients the loss kernels put on the outputs, and the loss value, against the benched
        mix restated on the recorded outputs (ref_loss_mix).  want(("loss", i)) selects the outputs whose gradient is compared;
        the others still enter the value and are listed in self.loss_left_out."""
        if not self.want(("loss",)):
            return
        t0 = time.time()
        rec = self.rec
        outputs = [i for i in sorted(LOSS_OUTPUTS) if self.want(("loss", i))]
        self.loss_left_out = [LOSS_OUTPUTS[i] for i in sorted(LOSS_OUTPUTS) if i not in outputs]
        assert len(rec.gout) == 9 and all(rec.gout[i] is not None for i in LOSS_OUTPUTS), "an output the mix reads received no gradient"
        assert rec.gout[1] is None or float(rec.gout[1].abs().max()) == 0.0, "a gradient arrived on the heat-map, which the mix does not read"
        refs = (ref_loss_mix(rec.outs, targets, outputs), ref_loss_mix(rec.outs, targets, outputs, torch.float32))
        for i in outputs:
            if _loss_device(rec.outs[i]).type != "cpu":
                dv, dg = loss_device_crosscheck(rec.outs, targets, i)
                self.loss_crosschecks.append((LOSS_OUTPUTS[i], dv, dg))
                assert dv <= LOSS_CROSSCHECK and dg <= LOSS_CROSSCHECK, \
                    "float64 on the device and on the CPU disagree on %s: value %.2e, gradient %.2e" % (LOSS_OUTPUTS[i], dv, dg)
        got = {"out:loss": torch.as_tensor(loss, dtype=torch.float64)}
        for i in outputs:
            got["din:" + LOSS_OUTPUTS[i]] = rec.gout[i].reshape(rec.outs[i].shape)
        self._cmp("loss", got, refs)
        self.loss_seconds = time.time() - t0

    # -- output heads ------------------------------------------------------------------------------------------------
    def heads(self):
        if not self.want(("heads",)):
            return
        rec = self.rec
        logits, heat, xo = rec.outs[0], rec.outs[1], rec.outs[2]
        refs = self._both(ref_softmax_head, logits, rec.gout[0], rec.gout[1])
        got = {"out:heat": heat.reshape(heat.shape[0], -1), "din:logits": rec.dec[("loc", 5)]["dout"].reshape(logits.shape)}
        self._cmp("head_softmax", got, refs)
        refs = self._both(ref_normalize_head, rec.raw_ori, rec.gout[2])
        got = {"out:x": xo, "din:raw": rec.dec[("ori", 5)]["dout"]}
        self._cmp("head_normalize", got, refs)

    def decoder_outputs(self, branch, j):
        """The tensor a decoder level's output feeds: the next level's input, the logits or the raw orientation field."""
        if j < 5:
            nxt = self.tape["match"][j + 1]["x"] if branch == "loc" else self.tape["ori"][j + 1]["cat"]
            c = self.tape["match"][j + 1]["c"] if branch == "loc" else nxt.shape[-1]
            return to_nchw(nxt[..., :c])
        if branch == "loc":
            return self.rec.outs[0].reshape(self.tape["heatmap"].shape)
        return self.rec.raw_ori

    def run_all(self, circular, targets=None, loss=None):
        """targets, loss: what the step built and returned; given, the chain starts at the loss (loss_link)."""
        if targets is not None:
            self.loss_link(targets, loss)
        self.encoder("grd_efficientnet", circular, self.tape["gfeat"])
        self.encoder("sat_efficientnet", False, self.tape["svol"])
        self.descriptors()
        for j in range(6):
            self.matching(j)
            for branch in ("loc", "ori"):
                self.decoder(branch, j, self.decoder_outputs(branch, j))
        self.skip_sums()
        self.joins()
        self.heads()
        return self.report
