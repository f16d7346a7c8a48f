"""Elementwise error models for the three loss kernels (csrc/heads.hip, csrc/heads_bwd.hip), the seeded inputs they are applied to
and the float64 references.  TEST INFRASTRUCTURE ONLY, importable without a GPU.

Shared by tests/test_losses_gpu.py (the kernels, on the MI355X) and tests/test_loss_check.py (CPU: the conditions on the constants
and the sentinels, and the same comparison applied to results with one injected fault each).

REFERENCES.  oracle.ccvpe_oracle.infonce_loss / cross_entropy_loss / orientation_loss on float64 copies of the same float32
inputs; gradients from autograd of g * loss for the upstream scalar g.  The label mask `> 1e-2` is decided on the float32 labels
(labels are data; 0.01f < 0.01 < nextafter(0.01f), so the float32 and the float64 comparison agree on every float32 label, and
the builder asserts it).  For infoNCE the per-row statistics the kernel leaves in `rows` are restated too:
    z_b = sum_j exp(s_j / T)     den_b = sum_{lab > 1e-2} lab_j     num_b = sum_{lab > 1e-2} (s_j / T - log z_b) lab_j     D = sum_b den_b
and loss = -sum_b num_b / D is asserted to equal the oracle's value to 1e-12, which ties the restatement to the oracle.

ERROR MODELS.  u = 2^-24; FL = 2^-120 is an absolute term for the subnormal range, where neither torch's float32 nor the kernels
are relatively accurate (gt = uniform ** 8 reaches 1e-40).  Every gradient element: |got_j - ref_j| <= c u model_j + FL with
    infoNCE        model_j = |g| / (D T) (1 + |s_j| / T) (den_b p_j + lab_j [lab_j > 1e-2]),   p = softmax(s / T) of the row
    cross entropy  model_j = |g| / B (ls_b p_j (1 + |r_j| + |logsumexp_b|) + l_j),              ls_b = the row's label sum
    orientation    model_j = |ref_j|
((1 + |s| / T): the rounding of s / T is an absolute error of the exponent.)  Scalars: |got - ref| <= c_v u S, S = the float64
sum of the absolute values of the terms summed: z_b and den_b and D are sums of positive terms (S = the value);
S(num_b) = sum (|s_j / T| + |log z_b|) lab_j over the positives; S(infoNCE loss) = sum_b S(num_b) / D;
S(cross entropy) = sum_j l_j (|r_j| + |logsumexp_b|) / B; the orientation loss is a sum of non-negative terms.

THE CONSTANTS ARE MEASURED per case: c = 4 max(r32, 2), c_v = 4 max(r32_v, 4), r32 = the largest err / (u model) of the float32
oracle (torch on the CPU, autograd included) against float64 on that case's inputs; the floors keep a lucky float32 run from
setting the bar and the factor 4 is the project's allowance for another summation order (stage_check.REF_FACTOR).  r32 <= R32_CAP
= 16 is asserted for every case in tests/test_loss_check.py: were it to fail, the model is wrong, not the cap.  The suite's older
bars stay as a second condition: 1e-5 on values, 1e-4 (orientation: 1e-5) of the tensor's maximum on gradients.

SENTINELS.  A value check sees an omitted element only if the element matters, so every row carries sentinels at element 0 and
n - 1, at the last n % 4 elements (the last 4 when n % 4 == 0) and, for infoNCE, on both sides of every multiple of NCE_CH = 8192.
A sentinel holds: infoNCE score 1.0 and label 0.9 on a background of scores uniform in [-1, 0] and labels uniform ** 6; cross
entropy the row's largest logit (background maximum + 1) and its largest label (0.5 on a background that sums to 1, before the
row is normalised); orientation gt = 4.0, the largest (background uniform ** 8 <= 1), with gt_orientation = -ori there, so the
sentinel's term is 16.  (With gt = 1 a single element of a 512 x 512 row moves the row's term by 70 x the tolerance only; the
condition below asks for 100.)  sentinel_margins() restates the condition tests/test_loss_check.py asserts: leaving any single
sentinel out of a row moves that row's z_b and num_b (cross entropy, orientation: the row's term) by >= 100 x its tolerance.
"""
import collections
import functools

import torch
import torch.nn.functional as F

from ccvpe_amd import synth
from oracle import ccvpe_oracle as O

U = 2.0 ** -24
FL = 2.0 ** -120
REF_FACTOR = 4.0
R32_CAP = 16.0
NCE_CH = 8192                    # csrc/heads.hip
SENTINEL_MARGIN = 100.0
OLD_VALUE_BAR = 1e-5             # tests/test_backward_gpu.py::test_loss_gradients_vs_oracle_autograd
OLD_GRAD_BAR = {"infonce": 1e-4, "ce": 1e-4, "ori": 1e-5}

# ------------------------------------------------------------------------------------------------------------------------------
# cases (tests/test_losses_gpu.py runs every one; the `reaches` text goes into the printed table)
# ------------------------------------------------------------------------------------------------------------------------------
NceCase = collections.namedtuple("NceCase", "name b n t g no_pos edge real reaches")
INFONCE_CASES = [
    NceCase("nce_b3_n5119", 3, 5119, 0.1, 1.0, (), None, False, "scalar path (n % 4 = 3) forward and backward, one ragged chunk"),
    NceCase("nce_b6_n16388", 6, 16388, 0.1, 1e4 / 6, (4,), (1, 8192), False,
            "two full chunks + a 4-element chunk; second pass of the row loop; row 4 without positives; label == 0.01f on a sentinel"),
    NceCase("nce_b70_n1280", 70, 1280, 0.07, 1.0, (3, 67), None, False, "B > 64 (lane-strided batch sum); rows 3 and 67 without positives; T = 0.07"),
    NceCase("nce_b2_66chunks", 2, 8192 * 65 + 8, 0.1, 1.0, (), None, False, "66 chunks: second pass of the chunk merge, 8-element last chunk"),
    NceCase("nce_b2_level6", 2, 20 * 256 * 256, 0.1, 1.0, (), None, False, "level 6's own row length, 160 chunks"),
    NceCase("nce_b5_level3_real", 5, 20 * 32 * 32, 0.1, 1.0, (), None, True, "level-3 labels of the target pyramid: realistic sparsity"),
]
REAL_CENTERS = [[0.0, 0.0], [37.0, -120.0], [-200.0, 55.0], [255.0, 255.0], [-3.0, 1.0]]     # tests/test_train_glue_gpu.py
REAL_ANGLES = [0.0, 7.5, 18.0, 200.25, 359.9]

CeCase = collections.namedtuple("CeCase", "name b n std peak_last normalised reaches")
CE_CASES = [
    CeCase("ce_b5_n262144", 5, 262144, 12.0, True, True, "peaked logits, row maximum at n - 1, 256 strides of 1024"),
    CeCase("ce_b2_n4099", 2, 4099, 12.0, False, True, "n no multiple of the 1024-thread stride (4 strides + 3)"),
    CeCase("ce_b66_n4096", 66, 4096, 2.0, False, False, "B > 64 in loss_finish; label row sums 0.3 .. 3 (the backward's ls)"),
]

OriCase = collections.namedtuple("OriCase", "name b h w reaches")
ORI_CASES = [
    OriCase("ori_b5_512x512", 5, 512, 512, "the model's own map"),
    OriCase("ori_b3_hw1001", 3, 7, 143, "hw = 1001: no multiple of the stride, odd"),
    OriCase("ori_b66_hw1024", 66, 32, 32, "B > 64 in loss_finish"),
]


def _seed(name):
    return 7000 + 37 * sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100000


def sentinel_positions(n, chunk=None):
    pos = {0, n - 1}
    pos.update(range(n - (n % 4 or 4), n))
    if chunk:
        for m in range(chunk, n, chunk):
            pos.update((m - 1, m))
    return sorted(pos)


# ------------------------------------------------------------------------------------------------------------------------------
# inputs (float32, CPU)
# ------------------------------------------------------------------------------------------------------------------------------
def infonce_inputs(case, labels=None, sentinels=True, quiet_tail=False):
    """(scores, labels) [B, n] float32.  labels: for a `real` case, the [B, n] labels to use (default: the oracle's level-3 pyramid;
    the GPU test passes what targets.train_targets built on the device); they get no label sentinels, the scores do.
    quiet_tail: the last n % 4 elements hold score -3 and label 0 (test_loss_check.py: a tail nobody would miss)."""
    seed = _seed(case.name)
    s = synth.uniform((case.b, case.n), seed, -1.0, 0.0)
    if case.real:
        lab = (O.train_targets(REAL_CENTERS, REAL_ANGLES, 20)[3][2] if labels is None else labels).reshape(case.b, case.n).float().clone()
    else:
        lab = synth.uniform((case.b, case.n), seed + 1) ** 6
    if sentinels:
        pos = torch.tensor(sentinel_positions(case.n, NCE_CH))
        s[:, pos] = 1.0
        if not case.real:
            lab[:, pos] = 0.9
    for b in case.no_pos:
        lab[b] *= 1e-3
    if case.edge is not None:
        lab[case.edge[0], case.edge[1]] = torch.tensor(0.01, dtype=torch.float32)
    if quiet_tail:
        k = case.n % 4
        s[:, case.n - k:] = -3.0
        lab[:, case.n - k:] = 0.0
    assert torch.equal(lab > 1e-2, lab.double() > 1e-2)
    return s, lab


def ce_inputs(case):
    """(logits, labels) [B, n] float32; see the module docstring for the sentinels."""
    seed = _seed(case.name)
    lg = synth.normal((case.b, case.n), seed, case.std)
    lab = synth.uniform((case.b, case.n), seed + 1) ** 20
    lab = lab / lab.sum(1, keepdim=True)
    pos = torch.tensor(sentinel_positions(case.n))
    top = lg.max(dim=1, keepdim=True).values
    lg[:, pos] = top + 1.0
    if case.peak_last:
        lg[:, case.n - 1] = top[:, 0] + 2.0
    lab[:, pos] = 0.5
    lab = lab / lab.sum(1, keepdim=True)
    if not case.normalised:
        lab = lab * (0.3 * 10.0 ** (torch.arange(case.b, dtype=torch.float32) / (case.b - 1))).view(-1, 1)
    return lg, lab


def ori_inputs(case):
    """(ori, gt_orientation [B,2,h,w] unit vectors, gt [B,1,h,w]) float32"""
    seed = _seed(case.name)
    shape = (case.b, 2, case.h, case.w)
    ori = F.normalize(synth.normal(shape, seed), dim=1)
    gto = F.normalize(synth.normal(shape, seed + 1), dim=1)
    gt = synth.uniform((case.b, 1, case.h, case.w), seed + 2) ** 8
    pos = torch.tensor(sentinel_positions(case.h * case.w))
    gto.view(case.b, 2, -1)[:, :, pos] = -ori.view(case.b, 2, -1)[:, :, pos]
    gt.view(case.b, -1)[:, pos] = 4.0
    return ori, gto, gt


# ------------------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------------------
def _autograd(fn, x32, others32, g, dtype):
    x = x32.to(dtype).clone().requires_grad_(True)
    loss = fn(x, *[o.to(dtype) for o in others32])
    (g * loss).backward()
    return loss.detach(), x.grad.detach()


def _r32(got32, ref64, model):
    return float(((got32.double() - ref64).abs() / (U * model + FL)).max())


def _constants(r32_grad, r32_val):
    return REF_FACTOR * max(r32_grad, 2.0), REF_FACTOR * max(r32_val, 4.0)


def infonce_stats(s, lab32, t, dtype=torch.float64):
    """(z_b, den_b, num_b, S(num_b), masked labels, s / T) of the rows in `dtype`; the mask from the float32 labels"""
    mask = lab32 > 1e-2
    tt = s.to(dtype) / t
    z = torch.exp(tt).sum(1)
    labm = torch.where(mask, lab32.to(dtype), torch.zeros((), dtype=dtype))
    logz = torch.log(z)
    num = ((tt - logz[:, None]) * labm).sum(1)
    s_num = ((tt.abs() + logz.abs()[:, None]) * labm).sum(1)
    return z, labm.sum(1), num, s_num, labm, tt


def infonce_grad_formula(ref, z=None, den=None, d=None, labm=None):
    """float64 gradient from (possibly faulted) statistics: g / (D T) (den_b exp(s_j / T) / z_b - lab_j [lab_j > 1e-2])"""
    z, den = ref.z if z is None else z, ref.den if den is None else den
    d, labm = ref.d if d is None else d, ref.labm if labm is None else labm
    return ref.g / (d * ref.t) * (den[:, None] * torch.exp(ref.tt) / z[:, None] - labm)


class InfoNCERef(object):
    kind = "infonce"

    def __init__(self, case, s, lab):
        self.case, self.name, self.s, self.lab, self.t, self.g = case, case.name, s, lab, case.t, case.g
        fn = lambda x, l: O.infonce_loss(x, l, case.t)
        self.loss, self.grad = _autograd(fn, s, [lab], case.g, torch.float64)
        self.z, self.den, self.num, self.s_num, self.labm, self.tt = infonce_stats(s, lab, case.t)
        self.d = self.den.sum()
        self.s_loss = self.s_num.sum() / self.d
        assert abs(float(self.loss + self.num.sum() / self.d)) <= 1e-12 * float(self.s_loss), "row statistics do not restate the oracle"
        p = torch.exp(self.tt) / self.z[:, None]
        self.model = abs(case.g) / (self.d * case.t) * (1 + self.tt.abs()) * (self.den[:, None] * p + self.labm)
        loss32, grad32 = _autograd(fn, s, [lab], case.g, torch.float32)
        z32, den32, num32 = infonce_stats(s, lab, case.t, torch.float32)[:3]
        self.r32_grad = _r32(grad32, self.grad, self.model)
        self.r32_val = max(_r32(loss32, self.loss, self.s_loss), _r32(z32, self.z, self.z), _r32(den32, self.den, self.den),
                           _r32(num32, self.num, self.s_num), _r32(den32.sum(), self.d, self.d))
        self.c, self.c_v = _constants(self.r32_grad, self.r32_val)

    def rows(self):
        """what ccvpe_infonce_loss_f32 leaves in `rows`: (num_b, den_b, z_b, 0) per row, then D"""
        r = torch.zeros(4 * self.case.b + 4, dtype=torch.float64)
        r[0:4 * self.case.b:4], r[1:4 * self.case.b:4], r[2:4 * self.case.b:4] = self.num, self.den, self.z
        r[4 * self.case.b] = self.d
        return r

    def scalars(self):
        """{name: (reference, S)}"""
        return {"loss": (self.loss, self.s_loss), "num_b": (self.num, self.s_num), "den_b": (self.den, self.den),
                "z_b": (self.z, self.z), "D": (self.d, self.d)}


def _ce_rows(lg, lab):
    lse = torch.logsumexp(lg, dim=1)
    term = (lab * (lg - lse[:, None])).sum(1)
    s_term = (lab * (lg.abs() + lse.abs()[:, None])).sum(1)
    return lse, term, s_term


class CERef(object):
    kind = "ce"

    def __init__(self, case, lg, lab, g=1.0):
        self.case, self.name, self.lg, self.lab, self.g = case, case.name, lg, lab, g
        self.loss, self.grad = _autograd(O.cross_entropy_loss, lg, [lab], g, torch.float64)
        lg64, lab64 = lg.double(), lab.double()
        self.lse, self.term, self.s_term = _ce_rows(lg64, lab64)
        self.ls = lab64.sum(1)
        self.s_loss = self.s_term.sum() / case.b
        assert abs(float(self.loss + self.term.sum() / case.b)) <= 1e-12 * float(self.s_loss)
        self.p = torch.exp(lg64 - self.lse[:, None])
        self.model = abs(g) / case.b * (self.ls[:, None] * self.p * (1 + lg64.abs() + self.lse.abs()[:, None]) + lab64)
        loss32, grad32 = _autograd(O.cross_entropy_loss, lg, [lab], g, torch.float32)
        self.r32_grad, self.r32_val = _r32(grad32, self.grad, self.model), _r32(loss32, self.loss, self.s_loss)
        self.c, self.c_v = _constants(self.r32_grad, self.r32_val)

    def scalars(self):
        return {"loss": (self.loss, self.s_loss)}


class OriRef(object):
    kind = "ori"

    def __init__(self, case, ori, gto, gt, g=1.0):
        self.case, self.name, self.ori, self.gto, self.gt, self.g = case, case.name, ori, gto, gt, g
        self.loss, self.grad = _autograd(O.orientation_loss, ori, [gto, gt], g, torch.float64)
        self.term = (((gto.double() - ori.double()) ** 2).sum(1, keepdim=True) * gt.double()).flatten(1).sum(1)
        self.s_term = self.term
        self.s_loss = self.term.sum() / case.b
        assert abs(float(self.loss - self.s_loss)) <= 1e-12 * float(self.s_loss)
        self.model = self.grad.abs()
        loss32, grad32 = _autograd(O.orientation_loss, ori, [gto, gt], g, torch.float32)
        self.r32_grad, self.r32_val = _r32(grad32, self.grad, self.model), _r32(loss32, self.loss, self.s_loss)
        self.c, self.c_v = _constants(self.r32_grad, self.r32_val)

    def scalars(self):
        return {"loss": (self.loss, self.s_loss)}


@functools.lru_cache(maxsize=None)
def cached_ref(name):
    """the reference of a table case on its default inputs (computed once per session, never modified)"""
    for case in INFONCE_CASES:
        if case.name == name:
            return InfoNCERef(case, *infonce_inputs(case))
    for case in CE_CASES:
        if case.name == name:
            return CERef(case, *ce_inputs(case))
    for case in ORI_CASES:
        if case.name == name:
            return OriRef(case, *ori_inputs(case))
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------------------------------------
# sentinel condition
# ------------------------------------------------------------------------------------------------------------------------------
def sentinel_margins(ref):
    """{quantity: the smallest |move| / tolerance over every (row, sentinel)} when that one element is left out of the row
    (out of z_b, the masked sums and num_b alike).  infoNCE: z_b for every row, num_b for the rows that have positives.
    Cross entropy / orientation: the row's term."""
    cv = ref.c_v
    if ref.kind == "infonce":
        pos = torch.tensor(sentinel_positions(ref.case.n, NCE_CH))
        e, tt, labm = torch.exp(ref.tt[:, pos]), ref.tt[:, pos], ref.labm[:, pos]
        z1 = ref.z[:, None] - e
        a = (ref.tt * ref.labm).sum(1)
        num1 = (a[:, None] - tt * labm) - torch.log(z1) * (ref.den[:, None] - labm)
        out = {"z_b": float(((ref.z[:, None] - z1).abs() / (cv * U * ref.z[:, None])).min())}
        has = ref.den > 0
        out["num_b"] = float(((ref.num[:, None] - num1).abs() / (cv * U * ref.s_num[:, None]))[has].min())
        return out
    if ref.kind == "ce":
        pos = torch.tensor(sentinel_positions(ref.case.n))
        lg, lab = ref.lg.double(), ref.lab.double()
        lse1 = torch.log(torch.exp(ref.lse)[:, None] - torch.exp(lg[:, pos]))
        term1 = ((lab * lg).sum(1)[:, None] - lab[:, pos] * lg[:, pos]) - lse1 * (ref.ls[:, None] - lab[:, pos])
        return {"term_b": float(((ref.term[:, None] - term1).abs() / (cv * U * ref.s_term[:, None])).min())}
    pos = torch.tensor(sentinel_positions(ref.case.h * ref.case.w))
    d2 = ((ref.gto.double() - ref.ori.double()) ** 2).sum(1).flatten(1)[:, pos] * ref.gt.double().flatten(1)[:, pos]
    return {"term_b": float((d2 / (cv * U * ref.s_term[:, None])).min())}


# ------------------------------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------------------------------
def old_rule_passes(got, ref, tol_of_scale):
    """the rule the loss tests used before: max error relative to the tensor's maximum"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max()) <= tol_of_scale * (float(ref.abs().max()) + 1e-30)


def _check(what, got, ref, tol, old_bar):
    """every element within tol, then the older bar; returns max err / tol"""
    got, ref = got.detach().cpu().double().reshape(ref.shape), ref
    assert bool(torch.isfinite(got).all()), "%s: non-finite values" % what
    err = (got - ref).abs()
    ratio = err / tol
    worst = float(ratio.max())
    if worst > 1.0:
        i = int(ratio.flatten().argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape)) if ratio.dim() else ()
        raise AssertionError("%s: %d of %d elements outside the tolerance; worst at %s: got %.9g want %.9g, err %.3e = %.2f x tol"
                             % (what, int((ratio > 1.0).sum()), ratio.numel(), idx, float(got.flatten()[i]), float(ref.flatten()[i]),
                                float(err.flatten()[i]), worst))
    scale = float(ref.abs().max()) + 1e-30
    assert float(err.max()) <= old_bar * scale, "%s: max err %.3e above %.0e of scale %.3e" % (what, float(err.max()), old_bar, scale)
    return worst


def check(ref, loss=None, grad=None, rows=None):
    """Assert the models of the module docstring for whatever is given (loss: scalar; grad: the input's shape; rows: infoNCE's
    [4B + 4] statistics).  Returns {tensor name: max err / tol}.  A failure names "<case> <tensor>"."""
    out = {}
    scal = ref.scalars()
    if loss is not None:
        out["loss"] = _check("%s loss" % ref.name, loss, scal["loss"][0], ref.c_v * U * scal["loss"][1], OLD_VALUE_BAR)
    if rows is not None:
        b = ref.case.b
        rows = rows.detach().cpu()
        assert rows.numel() == 4 * b + 4, rows.shape
        for k, nm in enumerate(("num_b", "den_b", "z_b")):
            want, s = scal[nm]
            # the older bar on a per-row statistic is relative to S as well: num_b of a row is a difference of two sums of that size
            out[nm] = _check("%s rows.%s" % (ref.name, nm), rows[k:4 * b:4], want, ref.c_v * U * s + FL, float("inf"))
        out["D"] = _check("%s rows.D" % ref.name, rows[4 * b], scal["D"][0], ref.c_v * U * scal["D"][1], OLD_VALUE_BAR)
    if grad is not None:
        out["grad"] = _check("%s grad" % ref.name, grad, ref.grad, ref.c * U * ref.model + FL, OLD_GRAD_BAR[ref.kind])
    return out


def describe(ref, ratios):
    return "%-20s c = %5.1f (r32 %.2f)  c_v = %5.1f (r32 %.2f)   got / tol: %s" % (
        ref.name, ref.c, ref.r32_grad, ref.c_v, ref.r32_val, "  ".join("%s %.3f" % (k, v) for k, v in ratios.items()))
