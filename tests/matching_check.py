"""Float64 reference and elementwise error model for the rotational-matching kernels (csrc/matching.hip: match_kernel in its
vector-ALU and tiled matrix-core forms, match_stream_kernel), and the seeded inputs of tests/matching_kernel_shapes.py's rows.

Shared by tests/test_matching_forms_gpu.py (the kernels, on the MI355X) and tests/test_matching_check.py (CPU: the float32 oracle
must pass, results with one injected fault each must not).

THE REFERENCE.  Written out as oracle.rotational_matching, in float64: per hypothesis i gather the window
window_i[c] = x[(c + window_offset + shift_i stride) mod C], c < L; num_i = <g, window_i>; score_i = num_i / (||window_i|| ||g||), no
eps.  S_i = <|g|, |window_i|> / (||window_i|| ||g||) is the same dot over absolute values.  The normalised copy is
x / max(||x||, 1e-12).  Inputs are seeded synth.normal: no window has zero norm (asserted).

THE MODEL.  u = 2^-24; d, d_w, d_t, d_g = matching_kernel_shapes.match_chain: the longest chain of fp32 additions a term of the dot,
of the window's sum of squares, of the pixel's sum of squares and of ||g||^2 passes through in the kernel form that ran.  Nothing is
tuned to what a kernel gives.
  score:    |err_i| <= (d + 1) u S_i + ((d_w + 1)/2 + (d_g + 1)/2 + 4) u |ref_i|.
            The dot: every product rounded at most once, then at most d additions: (1 + u)^(d+1) - 1 on every term, summed over
            |terms| = S_i in score units.  The sums of squares are sums of positive terms, so the same bound is RELATIVE there, and the
            square root halves it.  4: two square roots, the product of the norms, the quotient — each correctly rounded (the build
            has no fast-math flag; hipcc's default fp32 divide and sqrt are IEEE).
  normalised copy:  ((d_t + 1)/2 + 3) u |ref|      (sqrt, reciprocal, product)
  max column:       the largest score tolerance among the first n_max hypotheses of that pixel (|max a - max b| <= max |a - b|)
  tail columns:     their scores' tolerances
  padding columns:  exactly 0
  bf16 storage: x is rounded to bf16 before the reference is computed; the fp32 score volume keeps the fp32 model; the bf16 output
            columns add 2^-8 |ref|, the project's figure for one output rounding.
  The suite's older bars stay as a second condition: 2e-5 (fp32 scores, max and tail), 1e-5 (fp32 normalised copy), 1e-2 (bf16
  columns) of the tensor's maximum.
Every element is compared: no masks, no sampling.
"""
import functools

import torch
import torch.nn.functional as F

from ccvpe_amd import synth
from oracle import ccvpe_oracle as O

import matching_kernel_shapes as S

U = 2.0 ** -24
BF = torch.bfloat16


def rbf(t):
    """round to nearest bf16 and back: the values a bf16-storage kernel sees"""
    return t.to(BF).float()


def match_inputs(row, bf16):
    """x [B,C,H,W] (bf16-rounded if asked) and g [B,L], float32, seeded by the row's shape"""
    seed = 9100 + 7 * row.c + 3 * row.l + 11 * row.h + row.w + 131 * row.b
    x = synth.normal((row.b, row.c, row.h, row.w), seed)
    g = synth.normal((row.b, row.l), seed + 1)
    return (rbf(x) if bf16 else x), g


def window_index(row, shift, woff=None):
    return (torch.arange(row.l) + (row.woff if woff is None else woff) + shift * row.stride) % row.c


class MatchRef:
    """float64 reference of one call: scores and S [B,n,HW], the window-norm-free pieces the faults need, the normalised copy
    [B,HW,C]; tolerances per kernel form from tol()"""

    def __init__(self, key, bf16):
        self.row = row = S.Row("ref", *key, None, None, bf16, None, None)     # (no ldx / ldo / switch: the values do not depend on them)
        self.x, self.g = x, g = match_inputs(row, bf16)
        b, c, hw = row.b, row.c, row.h * row.w
        xp = x.double().permute(0, 2, 3, 1).reshape(b, hw, c)                  # pixel-major, as the kernels read it
        g64 = g.double()
        gn = g64.norm(dim=1).view(b, 1)
        sc, sa = [], []
        for i in row.shifts:
            win = xp.index_select(2, window_index(row, i))                    # [B,HW,L]  gather the window
            num = torch.einsum("bpl,bl->bp", win, g64)                        # dot
            den = (win * win).sum(dim=2).sqrt() * gn                          # norms
            assert bool((den > 0).all()), "a window with zero norm"
            sc.append(num / den)                                              # divide
            sa.append(torch.einsum("bpl,bl->bp", win.abs(), g64.abs()) / den)
        self.scores = torch.stack(sc, dim=1)                                  # [B,n,HW]
        self.s_abs = torch.stack(sa, dim=1)
        self.xn = xp / (xp * xp).sum(dim=2, keepdim=True).sqrt().clamp_min(1e-12)

    def tol(self, chain):
        """(score tolerances [B,n,HW], normalised-copy tolerances [B,HW,C]) for the chains of one kernel form"""
        ts = (chain.dot + 1) * U * self.s_abs + ((chain.window + 1) / 2 + (chain.g + 1) / 2 + 4) * U * self.scores.abs()
        tn = ((chain.total + 1) / 2 + 3) * U * self.xn.abs()
        return ts, tn


def ref_key(row):
    return (row.b, row.c, row.l, row.h, row.w, row.shifts, row.n_max, row.n_tail, row.stride, row.woff)


@functools.lru_cache(maxsize=2)
def _cached(key, bf16):
    return MatchRef(key, bf16)


def cached_ref(row):
    """rows that differ only in ldx / ldo / the switch share one reference"""
    return _cached(ref_key(row), row.bf16)


def _where(ratio):
    i = ratio.flatten().argmax().item()
    return tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))


def _compare(got, ref, tol, bar, what, where):
    """|got_i - ref_i| <= tol_i for every element and max error <= bar x the tensor's maximum; `where(idx)` words the coordinates"""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: non-finite output" % what
    err = (got - ref).abs()
    ratio = err / tol.clamp_min(1e-300)
    worst = ratio.max().item()
    scale = ref.abs().max().item() + 1e-30
    rel = err.max().item() / scale
    if worst > 1.0:
        idx = _where(ratio)
        raise AssertionError("%s: %d elements outside the elementwise tolerance; worst at %s: got %.9g want %.9g, err %.3e = %.2f x tol"
                             % (what, int((ratio > 1.0).sum()), where(idx), got[idx].item(), ref[idx].item(), err[idx].item(), worst))
    assert rel <= bar, "%s: max err %.3e above %.0e of scale %.3e" % (what, err.max().item(), bar, scale)
    return worst, rel


def match_check(ref, row, claim, scores, dstx, what, cus=256, chain=None):
    """scores [B,n,HW] fp32 and dstx [B,HW,ldo] (fp32 or bf16) of one launch of the form `claim` names, against the model with that
    form's chains (or the given ones).  Returns [(name, err/tol, err/scale)]; prints them."""
    chain = chain or S.match_chain(row, claim)
    ts, tn = ref.tol(chain)
    c, n, nt = row.c, len(row.shifts), row.n_tail
    out8 = 2.0 ** -8 if row.bf16 else 0.0
    bar_s, bar_n = (1e-2, 1e-2) if row.bf16 else (2e-5, 1e-5)
    dstx = dstx.detach().cpu().double()
    assert dstx.shape == (row.b, row.h * row.w, row.ldo), (what, dstx.shape)

    def own(b, p):
        return S.owner(row, claim, b, p, cus)
    res = []
    r = _compare(scores, ref.scores, ts, 2e-5, what + " scores",
                 lambda i: "(b, shift, pixel) = (%d, %d, %d) [%s]" % (i[0], i[1], i[2], own(i[0], i[2])))
    res.append(("scores",) + r)
    r = _compare(dstx[:, :, :c], ref.xn, tn + out8 * ref.xn.abs(), bar_n, what + " normalised copy",
                 lambda i: "(b, pixel, channel) = (%d, %d, %d) [%s]" % (i[0], i[1], i[2], own(i[0], i[1])))
    res.append(("norm",) + r)
    mx = ref.scores[:, :row.n_max].max(dim=1)[0]
    r = _compare(dstx[:, :, c], mx, ts[:, :row.n_max].max(dim=1)[0] + out8 * mx.abs(), bar_s, what + " max column",
                 lambda i: "(b, pixel) = (%d, %d) [%s]" % (i[0], i[1], own(i[0], i[1])))
    res.append(("max",) + r)
    if nt:
        tail = ref.scores[:, n - nt:].permute(0, 2, 1)
        r = _compare(dstx[:, :, c + 1:c + 1 + nt], tail, ts[:, n - nt:].permute(0, 2, 1) + out8 * tail.abs(), bar_s, what + " tail columns",
                     lambda i: "(b, pixel, shift) = (%d, %d, %d) [%s]" % (i[0], i[1], n - nt + i[2], own(i[0], i[1])))
        res.append(("tail",) + r)
    pad = dstx[:, :, c + 1 + nt:]
    assert bool((pad == 0).all()), "%s: %d padding columns are not exactly zero" % (what, int((pad != 0).sum()))
    print("%s: d %s | %s" % (what, tuple(chain), ", ".join("%s err/tol %.3f err/scale %.2e" % t for t in res)))
    return res


# ---- float32 results on the CPU, in the kernels' output layout (tests/test_matching_check.py) ------------------------------------
def oracle_scores(row, x, g, shifts=None):
    """the float32 oracle's scores [B,n,HW]"""
    sc = O.rotational_matching(x, g, list(row.shifts if shifts is None else shifts), row.stride, row.woff)
    return sc.reshape(row.b, -1, row.h * row.w)


def assemble(row, x, scores, n_max=None, tail0=None):
    """the decoder-input rows [x / max(||x||, 1e-12) | max of the first n_max | last n_tail scores | 0] [B,HW,ldo] from float32
    scores, in the row's storage type.  n_max / tail0 override the row's (fault injection)."""
    n, nt = scores.shape[1], row.n_tail
    n_max = row.n_max if n_max is None else n_max
    tail0 = n - nt if tail0 is None else tail0
    out = torch.zeros((row.b, row.h * row.w, row.ldo), dtype=torch.float32)
    out[:, :, :row.c] = F.normalize(x, p=2, dim=1).permute(0, 2, 3, 1).reshape(row.b, -1, row.c)
    out[:, :, row.c] = scores[:, :n_max].max(dim=1)[0]
    if nt:
        out[:, :, row.c + 1:row.c + 1 + nt] = scores[:, tail0:tail0 + nt].permute(0, 2, 1)
    return rbf(out) if row.bf16 else out


def old_rule_passes(got, ref, tol_of_scale):
    """the rule the operator tests use: max error relative to the tensor's maximum"""
    got, ref = got.detach().double(), ref.detach().double()
    return (got - ref).abs().max().item() <= tol_of_scale * (ref.abs().max().item() + 1e-30)
