"""Every stage of the training step against a float64 restatement of that stage alone, teacher-forced (tests/stage_check.py).

Each case runs the PUBLIC path — net.train(), net(grd, sat, drop_masks=...), the benched loss mix, loss.backward() — with the
Recorder installed, so the upstream gradients have the real scale and sparsity and the default three-stream schedule is on.
Per stage: the forward output recomputed in fp64 from the taped input equals the next stage's taped input (and every taped
BatchNorm mean / variance equals the fp64 statistics of the taped raw tensor); the returned input gradient and every parameter
gradient the stage owns (the step's final .grad) equal the fp64 VJP of the recorded upstream gradient.  The bar per tensor is
max(floor, 4 * e_ref), floor 1e-4 (forward, statistics) / 2e-4 (gradients), e_ref = the reference's own fp32 error on the same
inputs.  The full-coverage cases also assert that the parameters checked are exactly the parameters with a gradient.

The chain starts at the loss (StepChecker.loss_link, stage `loss`): the loss value and the gradients the loss kernels put on the
outputs against the benched mix restated on the recorded outputs, so the teacher-forced links below it no longer take `gout` as
given.  The B = 64 case compares every output of at most B64_MAX_ELEMENTS elements, all but level 6's scores (printed; its row
length is covered by tests/test_losses_gpu.py).  Outputs above 4 Mi elements are restated in float64 on the device and a
two-sample sub-batch recomputed on the CPU must agree to 1e-12.  The link adds 0.3 s / 0.04 s / 1.1 s to the B = 4 / B = 3 /
B = 64 case (profiles/r13/loss_checks.txt, with the wall times of every test of this file before and after).

The printed table (worst e_got / e_ref / bar per stage kind and case, and the B = 64 stage set) is kept in
profiles/r08/stage_checks.txt, with the wall times.  Wall-time rule: a test of this file should not be slower than the slowest
test the suite had before (27 s); the two trims provided for that were both taken (ori_prior: matching levels only; the B = 64
threshold halved to 32 Mi elements).  The two full-coverage cases, whose stage sets are fixed, still take 36 s and 27 s and the halved B = 64 case 65 s, nearly
all of it the float64 and float32 references on the CPU.
"""
import os
import time

import pytest
import torch

import stage_check as S
from ccvpe_amd import synth

pytestmark = pytest.mark.gpu

# Largest fp64 activation of a stage kept at B = 64.  64 Mi elements fit in host memory, but that case then took 165 s against 27 s
# of the slowest test of the suite before it (tests/test_bench_torchrun_gpu.py): halved, the second trim of the wall-time rule.
B64_MAX_ELEMENTS = 32 * 1024 * 1024
TABLE = os.environ.get("CCVPE_STAGE_TABLE")  # optional: append the per-case tables to this file


def _step(net, grd, sat, masks, center, angle, n_rot):
    """The benched step (tests/test_fullsize_train_gpu.py::_step)."""
    from ccvpe_amd import losses, targets
    for p in net.parameters():
        p.grad = None
    built = targets.train_targets(center, angle, n_rot)
    gt, gt_flat, gt_ori, labels = built
    out = net(grd, sat, drop_masks=masks)
    nce = 0.0
    for lvl in range(6):
        nce = nce + losses.infoNCELoss(torch.flatten(out[3 + lvl], start_dim=1), torch.flatten(labels[lvl], start_dim=1))
    loss = losses.cross_entropy_loss(out[0], gt_flat) + 1e4 * nce / 6 + 1e1 * losses.orientation_loss(out[2], gt_ori, gt)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}, built


def _drop_masks(batch, seed):
    """Drop-connect draws from synth.uniform thresholds; at least one sample dropped in a skip block of each encoder."""
    masks = {}
    for e, enc in enumerate(("grd_efficientnet", "sat_efficientnet")):
        for i in range(16):
            masks[(enc, i)] = (synth.uniform((batch,), seed + 16 * e + i) > 0.25).float().cuda()
        dropped = [i for i in range(1, 16) if S.skip_block(i) and float(masks[(enc, i)].min()) == 0.0]
        assert dropped, "no sample dropped in any skip block of %s" % enc
    return masks


def _run_case(synth_sd, monkeypatch, label, kind, batch, ori_noise=None, want=None, keep=None, seed=0):
    """want(stage key): the stages to check; keep(stage key): what the Recorder clones (default: what is checked)."""
    from ccvpe_amd import models
    n_rot = synth.MODEL_SPECS[kind]["n_rot"]
    if kind == "kitti":
        net = models.CVM_KITTI("cuda")
    elif ori_noise is not None:
        net = models.CVM_VIGOR_ori_prior("cuda", ori_noise, True)
    else:
        net = models.CVM_VIGOR("cuda", True)
    net.load_state_dict(synth_sd(kind, 0), strict=True)
    net = net.to("cuda:0").train()
    grd, sat = synth.synthetic_pair(batch, kind, 4100 + seed, device="cuda")
    u = synth.uniform((batch, 3), 4200 + seed)
    center, angle = ((u[:, :2] - 0.5) * 384.0).cuda(), (u[:, 2] * 359.99).cuda()
    masks = _drop_masks(batch, 4300 + 100 * seed)
    t0 = time.time()
    with monkeypatch.context() as mp:
        rec = S.Recorder(mp, keep=keep or want)
        loss, grads, built = _step(net, grd, sat, masks, center, angle, n_rot)
    assert loss == loss and rec.tape is not None and rec.gout is not None
    for (enc, i), m in masks.items():
        if S.skip_block(i) and i:
            assert torch.equal(net._last_drop_masks[(enc, i)], m), "drop mask of %s block %d was not the injected one" % (enc, i)
    t1 = time.time()
    named = {n: p.detach() for n, p in net.named_parameters()}
    chk = S.StepChecker(rec, named, grads, want)
    report = chk.run_all(bool(rec.tape["circular"]), built, loss)
    report.finish()
    lines = ["== %s: loss %.6f, %d stages, %d tensors compared (%d noise-level), step %.1f s, references %.1f s"
             % (label, loss, len(set(chk.stages)), report.tensors(), len(report.noise), t1 - t0, time.time() - t1)]
    if "loss" in chk.stages:
        lines.append("  loss link: %.2f s of the references; outputs left out: %s; float64 on the device (cross-checked on two samples "
                     "against the CPU: value, gradient): %s" % (chk.loss_seconds, ", ".join(chk.loss_left_out) or "none",
                                                                ", ".join("%s %.1e %.1e" % c for c in chk.loss_crosschecks) or "none"))
    for kindname, (e_got, e_ref, bar, stage, tensor) in sorted(report.worst_by_kind().items()):
        lines.append("  %-16s worst e_got %.3e  e_ref %.3e  bar %.3e   (%s %s)" % (kindname, e_got, e_ref, bar, stage, tensor))
    if report.noise:
        lines.append("  noise-level (fp64 reference below 1e-6 of the largest gradient): %s" % ", ".join(n[3:] for _, n in report.noise))
    for stage, n, of, tau in chk.relu_taken:
        lines.append("  %s: %d of %d ReLU decisions taken from the tape (|fp64 pre-activation| <= %.1e, stage_check.relu_mask_at_discontinuity)"
                     % (stage, n, of, tau))
    assert sum(n for _, n, _, _ in chk.relu_taken) <= 1e-5 * max(1, sum(of for _, _, of, _ in chk.relu_taken)), chk.relu_taken
    text = "\n".join(lines)
    print(text)
    print(S.format_rows(report.rows))
    if TABLE:
        with open(TABLE, "a") as f:
            f.write(text + "\n")
        with open(TABLE + ".rows", "a") as f:
            f.write("== %s\n%s\n" % (label, S.format_rows(report.rows)))
    return chk, report, grads, rec


def _full_coverage(chk, report, grads):
    report.assert_ok()
    missing, extra = sorted(set(grads) - chk.checked), sorted(chk.checked - set(grads))
    assert not missing and not extra, "parameters with a gradient that no stage checked: %s; checked without a gradient: %s" % (missing, extra)
    kinds = [S.stage_kind(s) for s in set(chk.stages)]
    assert (kinds.count("stem"), kinds.count("block"), kinds.count("head"), kinds.count("match"),
            kinds.count("dec_loc") + kinds.count("dec_ori")) == (2, 32, 2, 6, 12), sorted(set(chk.stages))
    assert {"gdesc", "sdesc", "head_softmax", "head_normalize", "loss"} <= set(chk.stages)
    assert not chk.loss_left_out, chk.loss_left_out
    assert len([s for s in set(chk.stages) if s.startswith("skipsum")]) == 5 and {"dgdesc", "catsum:1"} <= set(chk.stages)


def test_every_stage_vigor_b4(synth_sd, monkeypatch):
    """CVM_VIGOR, circular padding, 320x640 / 512x512, B = 4: every stage of the step."""
    chk, report, grads, rec = _run_case(synth_sd, monkeypatch, "CVM_VIGOR B=4", "vigor", 4)
    _print_premises(rec)
    _full_coverage(chk, report, grads)
    assert len(grads) == 520


def test_every_stage_kitti_b3(synth_sd, monkeypatch):
    """CVM_KITTI, 256x1024, B = 3 (odd batch; partial matching windows L < C; zero padding in both encoders)."""
    chk, report, grads, rec = _run_case(synth_sd, monkeypatch, "CVM_KITTI B=3", "kitti", 3, seed=1)
    _full_coverage(chk, report, grads)
    assert len(grads) == 520


def test_ori_prior_stages_b2(synth_sd, monkeypatch):
    """CVM_VIGOR_ori_prior(36), B = 2: the six matching levels with 5 localisation shifts (level 1 with the 20-shift tail behind
    them), and dgdesc assembled from them.  (Level 1 of both decoders and the output heads, which do not differ in code from
    CVM_VIGOR's, were the first trim the wall-time rule in the module docstring asks for.)"""
    def want(key):
        return key[0] == "match"
    chk, report, grads, rec = _run_case(synth_sd, monkeypatch, "CVM_VIGOR_ori_prior(36) B=2", "vigor", 2, ori_noise=36,
                                        want=want, keep=lambda key: want(key) or key == ("gd",), seed=2)
    assert rec.tape["match"][0]["n_max"] == 5 and rec.tape["match"][0]["n_tail"] == 20 and len(rec.tape["match"][0]["shifts"]) == 25
    report.assert_ok()
    assert sorted(set(chk.stages)) == ["dgdesc"] + ["match:%d" % l for l in range(1, 7)], chk.stages


# ----------------------------------------------------------------------------------------------------------------------
# B = 64: the benched step
# ----------------------------------------------------------------------------------------------------------------------
def b64_stage_set(kind, batch, limit):
    """Stage keys whose largest activation (elements, at this batch) is at most `limit`, from the model's shapes alone."""
    spec = synth.MODEL_SPECS[kind]
    keep, sizes = set(), {}
    for prefix, (h, w) in (("grd_efficientnet", synth.GRD_SHAPES[kind]), ("sat_efficientnet", (512, 512))):
        h, w = (h + 1) // 2, (w + 1) // 2
        sizes[("stem", prefix)] = batch * max(3 * (2 * h + 1) * (2 * w + 1), 32 * h * w)
        for i, (k, s, e, cin, cout) in enumerate(synth.B0_BLOCKS):
            ho, wo = (h + s - 1) // s, (w + s - 1) // s
            pad = k - 1 if s == 1 else k - 2                # SAME padding in front of the depthwise convolution
            sizes[("block", prefix, i)] = batch * max(cin * h * w, cin * e * (h + pad) * (w + pad), cout * ho * wo)
            h, w = ho, wo
        sizes[("head", prefix)] = batch * 1280 * h * w
        if prefix.startswith("grd"):
            sizes[("gd",)] = batch * 1280 * h * w
        else:
            sizes[("sd",)] = batch * 1280 * h * w
    hw = 8
    for j in range(6):
        for branch in ("loc", "ori"):
            k_in, c_up, c_cat, c_out = spec[branch][j]
            sizes[("dec", branch, j)] = batch * max(k_in * hw * hw, max(c_cat, c_out) * 4 * hw * hw)
        sizes[("match", j)] = batch * spec["loc"][j][0] * hw * hw
        hw *= 2
    sizes[("heads",)] = batch * 512 * 512 * 2
    # the loss link: one key per output the mix reads (logits, orientation field, scores of level 1 .. 6), its own elements
    sizes[("loss", 0)], sizes[("loss", 2)] = batch * 512 * 512, batch * 2 * 512 * 512
    for j in range(6):
        sizes[("loss", 3 + j)] = batch * spec["n_rot"] * (8 << j) ** 2
    for key, n in sizes.items():
        if n <= limit:
            keep.add(key)
    if any(k[0] == "loss" for k in keep):
        keep.add(("loss",))
    return keep, sizes


def _describe(keys):
    out = []
    for enc in ("grd_efficientnet", "sat_efficientnet"):
        out.append("%s blocks %s" % (enc, sorted(k[2] for k in keys if k[0] == "block" and k[1] == enc)))
    out.append("stems %s, heads %s" % (sorted(k[1] for k in keys if k[0] == "stem"), sorted(k[1] for k in keys if k[0] == "head")))
    out.append("descriptors %s" % sorted(k[0] for k in keys if k[0] in ("gd", "sd")))
    out.append("matching levels %s" % sorted(k[1] + 1 for k in keys if k[0] == "match"))
    for branch in ("loc", "ori"):
        out.append("%s decoder levels %s" % (branch, sorted(k[2] + 1 for k in keys if k[0] == "dec" and k[1] == branch)))
    out.append("output heads %s" % (("heads",) in keys))
    out.append("loss link on %s (left out: %s)" % (
        [S.LOSS_OUTPUTS[i] for i in sorted(S.LOSS_OUTPUTS) if ("loss", i) in keys],
        [S.LOSS_OUTPUTS[i] for i in sorted(S.LOSS_OUTPUTS) if ("loss", i) not in keys] or "nothing"))
    return "; ".join(out)


def test_b64_stage_set_from_shapes():
    keys, sizes = b64_stage_set("vigor", 64, 64 * 1024 * 1024)           # the set the shapes give at 64 Mi elements
    for enc in ("grd_efficientnet", "sat_efficientnet"):
        assert set(range(5, 16)) <= set(k[2] for k in keys if k[0] == "block" and k[1] == enc)
        assert ("block", enc, 3) not in keys and ("stem", enc) not in keys and ("head", enc) in keys
    assert {("gd",), ("sd",), ("heads",)} <= keys
    for branch in ("loc", "ori"):
        assert sorted(k[2] for k in keys if k[0] == "dec" and k[1] == branch) == [0, 1, 2]
    assert {("match", 0), ("match", 1), ("match", 2)} <= keys and ("match", 5) not in keys
    assert sizes[("loss", 8)] == 64 * 20 * 256 * 256 and ("loss", 8) not in keys and ("loss",) in keys
    keys, sizes = b64_stage_set("vigor", 64, B64_MAX_ELEMENTS)
    # the loss link: every output but level 6's scores (84 Mi elements; its row length is covered by tests/test_losses_gpu.py)
    assert sorted(k[1] for k in keys if k[0] == "loss" and len(k) == 2) == [0, 2, 3, 4, 5, 6, 7] and ("loss",) in keys
    assert sizes[("loss", 2)] == B64_MAX_ELEMENTS
    print("B = 64 stage set (largest activation <= %d elements): %s" % (B64_MAX_ELEMENTS, _describe(keys)))
    assert set(range(12, 16)) <= set(k[2] for k in keys if k[0] == "block" and k[1] == "sat_efficientnet")
    assert {6, 7, 8, 12, 13, 14, 15} <= set(k[2] for k in keys if k[0] == "block" and k[1] == "grd_efficientnet")
    assert {("gd",), ("sd",), ("heads",), ("head", "grd_efficientnet"), ("head", "sat_efficientnet")} <= keys
    for branch in ("loc", "ori"):
        assert sorted(k[2] for k in keys if k[0] == "dec" and k[1] == branch) == [0, 1]
    assert sorted(k[1] for k in keys if k[0] == "match") == [0, 1, 2]


def test_stages_of_the_benched_step_b64(synth_sd, monkeypatch):
    """CVM_VIGOR at B = 64, the benched step: every stage whose largest fp64 activation has at most B64_MAX_ELEMENTS elements."""
    keys, _ = b64_stage_set("vigor", 64, B64_MAX_ELEMENTS)
    print("B = 64 stage set: " + _describe(keys))
    if TABLE:
        with open(TABLE, "a") as f:
            f.write("B = 64 stage set (largest activation <= %d elements): %s\n" % (B64_MAX_ELEMENTS, _describe(keys)))

    def keep(key):                                  # block boundaries below a kept block; level 6's upstream gradient
        return key in keys or key[0] == "bn" or (key[0] == "dec" and key[2] == 5)
    chk, report, grads, rec = _run_case(synth_sd, monkeypatch, "CVM_VIGOR B=64", "vigor", 64, want=lambda key: key in keys,
                                        keep=keep, seed=3)
    report.assert_ok()
    print("B = 64 loss link: outputs left out: %s" % chk.loss_left_out)
    assert "loss" in chk.stages and chk.loss_left_out == ["scores6"]
    assert len(set(chk.stages)) >= len([k for k in keys if k[0] != "loss"]) + 1      # the loss keys are one stage


def _print_premises(rec):
    """Figures of the real step that tests/test_stage_check.py's mutation checks take their scales from."""
    import builtins

    def print(text):
        builtins.print(text)
        if TABLE:
            with open(TABLE, "a") as f:
                f.write("  " + text + "\n")
    tape = rec.tape
    dg = torch.cat([rec.match[j]["dg"] for j in range(6)], 1).double()
    shares = [float(rec.match[j]["dg"].double().norm() / dg.norm()) for j in range(6)]
    print("premises: share of each matching level's dg in |dgdesc|: %s" % ["%.3e" % s for s in shares])
    for b in (15, 10, 4, 2, 0):
        j = (15, 10, 4, 2, 0).index(b)
        lo, orr = rec.dec[("loc", j)]["skip_after"].double(), rec.dec[("ori", j)]["skip_after"].double()
        print("premises: skip block %d: |ori skip gradient| / |loc + ori| = %.3e" % (b, float(orr.norm() / (lo + orr).norm())))
    for name in ("sat_efficientnet._blocks.14._bn2", "grd_efficientnet._blocks.14._bn2", "sat_efficientnet._blocks.6._bn2"):
        dv = rec.bn[name].double()
        per = dv.flatten(1).norm(dim=1)
        print("premises: per-sample |upstream gradient| at %s relative to the largest: %s" % (name, ["%.3e" % float(v / per.max()) for v in per]))
    r = rec.dec[("loc", 0)]
    d = r["dcat"].double()
    c = tape["match"][0]["c"]
    print("premises: level-1 cat gradient (localisation decoder): |max column| / |all| = %.3e, |column c-1| / |all| = %.3e"
          % (float(d[..., c].norm() / d.norm()), float(d[..., c - 1].norm() / d.norm())))
