"""The rows of tests/test_matching_forms_gpu.py: every launched form of the rotational matching (csrc/matching.hip) ALONE, at the
smallest shape that takes each branch, each row naming the instantiation it pins at every position of ccvpe_set_match_mfma.

    match_kernel<TX, NPAD {1,8,16,24,48}, PARTIAL, VEC {4,2,1}>                 the vector-ALU form          ("valu",   form 0)
    match_kernel<TX, NPAD {16,32}, PARTIAL, VEC {4,2}, MFMA>                    the tiled matrix-core form   ("tiled",  form 1)
    match_stream_kernel<TX, MTL {1,2}, PARTIAL, NB {2,3,4,5}>                   the streaming form           ("stream", form 2)

A row's `claims` are three Claim tuples, one per switch position 0 / 1 / 2 (what ccvpe_match_route must answer there);
`switches` are the positions the GPU test launches it at.  The claim of the form a table is about is written out in that table;
the claims of the other positions follow from (n_shifts, PARTIAL, VEC) by valu_claim / tiled_claim, and the tile geometry of a
channel count comes from the literal TILE table.  tests/test_matching_route.py holds all of it against the library's own
host-only query, so a routing or geometry change shows up there, without a GPU, as a stale row.

Also here, restated in plain Python from csrc/matching.hip: match_lpp, the pitches, NPT / KS / the K slices, the LDS bytes, the
streaming form's tiles per wave, runs and workgroups, and match_chain, the longest chain of fp32 additions a term of each
sum passes through (the d of tests/matching_check.py's error model).
"""
import collections

VALU, TILED, STREAM = 0, 1, 2                    # ccvpe_match_route's return value

Claim = collections.namedtuple("Claim", "form npad partial vec nb lpp tp npt ks slices")
Row = collections.namedtuple("Row", "name b c l h w shifts n_max n_tail stride woff ldx ldo bf16 switches claims")


# ---- restated host arithmetic of csrc/matching.hip -------------------------------------------------------------------------------
def match_lpp(c):
    l = 1
    while l < 32 and c > 24 * l:
        l *= 2
    return l


def match_pitch(c, lpp):
    if lpp >= 16:
        return c + 4
    s = c + 4
    while (s // 4) % lpp or ((s // 4) // lpp) % 2 == 0:
        s += 4
    return s


def match_pitch_mfma(c):
    return ((c + 15) & ~15) + 4


def npt_ks(tp):
    npt = tp >> 4 if tp >= 16 else 1
    return npt, (1 if npt >= 4 else 4 // npt)


def k_slices(c, ks):
    """[kb0, kb1) in 16-channel blocks of every K slice of a tile"""
    nb16 = (c + 15) >> 4
    return tuple((s * nb16 // ks, (s + 1) * nb16 // ks) for s in range(ks))


def offsets(shifts, stride, woff, c):
    return [(-(i * stride + woff)) % c for i in shifts]


def vec_of(offs):
    return 1 if any(o % 2 for o in offs) else (2 if any(o % 4 for o in offs) else 4)


def lds_bytes(c, n_shifts, claim):
    """dynamic LDS of a match_kernel launch: tables, the tile, the tile's scores, 1/norm and max, ||g|| partials, K-slice blocks"""
    mfma = claim.form == TILED
    tl = 2 * c + 16 if mfma else 2 * c
    s = match_pitch_mfma(c) if mfma else match_pitch(c, claim.lpp)
    pbuf = 4 * ((2 if claim.partial else 1) * claim.npad + 1) * 16 if mfma and claim.ks > 1 else 0
    return 4 * (tl * (2 if claim.partial else 1) + claim.tp * s + n_shifts * claim.tp + 2 * claim.tp + 4 + pbuf)


StreamGeo = collections.namedtuple("StreamGeo", "tiles tpw run wgs last_tiles straddled")


def stream_geometry(b, hw, cus=256):
    """tiles per wave, tiles per workgroup run, workgroups, tiles of the last workgroup, and the sample boundaries (in tiles) that
    fall INSIDE a run — its waves rebuild their descriptor fragments there"""
    tiles = b * hw // 16
    waves = 2 * cus * 4
    tpw = (tiles + waves - 1) // waves
    run = 4 * tpw
    wgs = ((tiles + tpw - 1) // tpw + 3) // 4
    tps = hw // 16
    straddled = tuple(k * tps for k in range(1, b) if (k * tps) % run)
    return StreamGeo(tiles, tpw, run, wgs, tiles - (wgs - 1) * run, straddled)


Chain = collections.namedtuple("Chain", "dot window total g")


def match_chain(row, claim):
    """The longest chain of fp32 additions a term passes through, per sum, read off the kernel that `claim` names:
    vector-ALU  a lane walks ceil(C/4 / LPP) 4-channel groups (4 fused multiply-adds each) and the LPP lanes of a pixel meet in a
                log2(LPP) butterfly; the window norm and the total norm walk the same groups;
    tiled       a K slice is ceil(nb16 / KS) 16-channel blocks, 4 matrix instructions of 4 channels each per block (16 additions)
                and the KS slices are added in order (KS - 1); the total norm takes 4 additions per block in each of a pixel's four
                k groups, two cross-lane adds and the slices;
    streaming   NB blocks of 16; the total norm 4 per block and two cross-lane adds.
    ||g||^2: the tiled kernels give thread t the entries t, t + 256, ..., then a 6-step wave butterfly and the four waves' sums in
    order; the streaming kernel gives lane l the entries l, l + 64, ... of the L-wide window and the same butterfly."""
    c = row.c
    if claim.form == VALU:
        d = 4 * -(-(c // 4) // claim.lpp) + claim.lpp.bit_length() - 1
        dt = d
        dg = -(-c // 256) + 6 + 3
    elif claim.form == TILED:
        blocks = -(-((c + 15) // 16) // claim.ks)
        d = 16 * blocks + claim.ks - 1
        dt = 4 * blocks + 2 + claim.ks - 1
        dg = -(-c // 256) + 6 + 3
    else:
        d = 16 * claim.nb
        dt = 4 * claim.nb + 2
        dg = -(-row.l // 64) + 6
    return Chain(d, d if claim.partial else dt, dt, dg)


# ---- the tile geometry per channel count: (LPP, TP, NPT, KS, K slices in 16-channel blocks) -------------------------------------
TILE = {
    8: (1, 256, 16, 1, ((0, 1),)),
    24: (1, 256, 16, 1, ((0, 2),)),               # NPT 16; 8 zero-padded channels in the matrix-core form
    32: (2, 128, 8, 1, ((0, 2),)),
    40: (2, 128, 8, 1, ((0, 3),)),                # NPT 8, pad 8
    48: (2, 128, 8, 1, ((0, 3),)),
    56: (4, 64, 4, 1, ((0, 4),)),
    64: (4, 64, 4, 1, ((0, 4),)),
    72: (4, 64, 4, 1, ((0, 5),)),
    80: (4, 64, 4, 1, ((0, 5),)),                 # NPT 4: the last class whose waves own whole tiles
    88: (4, 64, 4, 1, ((0, 6),)),
    104: (8, 32, 2, 2, ((0, 3), (3, 7))),         # KS 2, uneven 3 | 4, pad 8
    160: (8, 32, 2, 2, ((0, 5), (5, 10))),        # KS 2
    200: (16, 16, 1, 4, ((0, 3), (3, 6), (6, 9), (9, 13))),          # KS 4, uneven, pad 8
    320: (16, 16, 1, 4, ((0, 5), (5, 10), (10, 15), (15, 20))),     # KS 4
    392: (32, 8, 1, 4, ((0, 6), (6, 12), (12, 18), (18, 25))),      # TP 8: half a tile is padding; uneven, pad 8
    1280: (32, 8, 1, 4, ((0, 20), (20, 40), (40, 60), (60, 80))),
    2048: (32, 8, 1, 4, ((0, 32), (32, 64), (64, 96), (96, 128))),
}


def valu_claim(c, npad, partial, vec):
    lpp, tp = TILE[c][:2]
    return Claim(VALU, npad, partial, vec, 0, lpp, tp, 0, 0, ())


def tiled_claim(c, npad, partial, vec):
    lpp, tp, npt, ks, slices = TILE[c]
    return Claim(TILED, npad, partial, vec, 0, lpp, tp, npt, ks, slices)


def stream_claim(mtl, partial, nb):
    return Claim(STREAM, 16 * mtl, partial, 0, nb, 0, 0, 0, 0, ())


def valu_npad(n):
    return 1 if n <= 1 else 8 if n <= 8 else 16 if n <= 16 else 24 if n <= 24 else 48


def _up(v, m):
    return (v + m - 1) // m * m


def _centred(n):
    return tuple(range(-(n // 2), n - n // 2))


ORI_PRIOR_180 = tuple(range(-10, 11)) + tuple(range(20))          # 41 hypotheses, n_max 21, n_tail 20
ORI_PRIOR_54 = tuple(range(-3, 4)) + tuple(range(20))             # 27 hypotheses, n_max 7, n_tail 20


def _make(name, c, l, h, w, shifts, stride, claims, switches, bf16, b=2, n_max=None, n_tail=0, woff=0, ldx=None, ldo=None, wide=False):
    """ldo defaults to C + 1 + n_tail rounded up to 4 — `wide`: to 8, the 16-byte bf16 store path (EO = 8) of the tiled kernels"""
    shifts = tuple(shifts)
    ldo = ldo or _up(c + 1 + n_tail, 8 if wide else 4)
    return Row("%s %s" % (name, "bf16" if bf16 else "fp32"), b, c, l, h, w, shifts, n_max or len(shifts), n_tail, stride, woff,
               ldx or c, ldo, bf16, switches, claims)


# ---- the vector-ALU form at default routing ------------------------------------------------------------------------------------------
# (name, C, L, h, w, shifts, stride, (NPAD, PARTIAL, VEC), extras).  One, 2..8 and >= 33 hypotheses always run here; 9..32 only with
# an odd table offset (VEC 1).  Every row runs in both storage types; the bf16 copy of every second row takes the wide output rows.
_VALU = [
    ("valu npad1 C8 3x3, hw < TP", 8, 8, 3, 3, (0,), 2, (1, False, 4), {}),
    ("valu npad1 partial C160 L40 23x23, ragged last workgroup", 160, 40, 23, 23, (0,), 8, (1, True, 4), {}),
    ("valu npad1 vec2 C24", 24, 24, 4, 5, (1,), 2, (1, False, 2), {}),
    ("valu npad1 vec2 partial C24 L12", 24, 12, 4, 5, (1,), 2, (1, True, 2), {}),
    ("valu npad1 vec1 C24", 24, 24, 4, 5, (1,), 3, (1, False, 1), {}),
    ("valu npad1 vec1 partial C24 L10", 24, 10, 4, 5, (1,), 3, (1, True, 1), {}),
    ("valu npad8 vec4 C80 7 shifts, ldx C + 8", 80, 80, 5, 7, range(-3, 4), 4, (8, False, 4), dict(ldx=88)),
    ("valu npad8 vec4 partial C80 L40 7 shifts", 80, 40, 5, 7, range(-3, 4), 4, (8, True, 4), {}),
    ("valu npad8 vec2 C40 8 shifts (8 | 9)", 40, 40, 5, 5, range(8), 2, (8, False, 2), {}),
    ("valu npad8 vec2 partial C40 L20 8 shifts, two workgroups", 40, 20, 9, 15, range(-4, 4), 2, (8, True, 2), {}),
    ("valu npad8 vec1 C40 stride 3", 40, 40, 5, 5, range(5), 3, (8, False, 1), {}),
    ("valu npad8 vec1 partial C40 L20 stride 3", 40, 20, 5, 5, range(-2, 3), 3, (8, True, 1), {}),
    ("valu npad16 vec1 partial centred C40 L14 12 shifts", 40, 14, 7, 7, _centred(12), 2, (16, True, 1), dict(woff=13)),
    ("valu npad16 vec1 C40 9 shifts stride 3 (8 | 9)", 40, 40, 5, 5, range(9), 3, (16, False, 1), {}),
    ("valu npad16 vec1 C48 16 shifts stride 3 (16 | 17)", 48, 48, 5, 5, range(16), 3, (16, False, 1), {}),
    ("valu npad24 vec1 partial centred C80 L30 20 shifts", 80, 30, 5, 5, _centred(20), 4, (24, True, 1), dict(woff=25)),
    ("valu npad24 vec1 C48 17 shifts stride 3 (16 | 17)", 48, 48, 5, 5, range(17), 3, (24, False, 1), {}),
    ("valu npad48 partial ori_prior(180) C1280 L640, second workgroup one pixel", 1280, 640, 3, 3, ORI_PRIOR_180, 64, (48, True, 4),
     dict(n_max=21, n_tail=20)),
    ("valu npad48 ori_prior(180) C1280 L1280", 1280, 1280, 3, 3, ORI_PRIOR_180, 64, (48, False, 4), dict(n_max=21, n_tail=20)),
    ("valu npad48 vec4 C48 33 shifts (32 | 33)", 48, 48, 5, 5, range(33), 4, (48, False, 4), {}),
    ("valu npad48 vec2 C40 33 shifts", 40, 40, 5, 5, range(33), 2, (48, False, 2), {}),
    ("valu npad48 vec2 partial C40 L20 34 shifts", 40, 20, 5, 5, _centred(34), 2, (48, True, 2), {}),
    ("valu npad48 vec1 C48 25 shifts stride 3", 48, 48, 5, 5, range(25), 3, (48, False, 1), {}),
    ("valu npad48 vec1 partial C80 L40 32 shifts stride 3 (32 | 33)", 80, 40, 5, 5, _centred(32), 3, (48, True, 1), {}),
]


def _valu_rows():
    out = []
    for i, (name, c, l, h, w, shifts, stride, (npad, partial, vec), kw) in enumerate(_VALU):
        cl = valu_claim(c, npad, partial, vec)
        for bf16 in (False, True):
            out.append(_make(name, c, l, h, w, shifts, stride, (cl, cl, cl), (2,), bf16, wide=bf16 and i % 2 == 1, **kw))
    return out


# ---- the tiled matrix-core form -----------------------------------------------------------------------------------------------------
# (name, C, L, h, w, shifts, stride, (NPAD, PARTIAL, VEC), switch, extras): 9..32 hypotheses, even table offsets, too few pixels (or
# tail scores, or C > 80) for the streaming form, so positions 1 and 2 launch the same kernel; `switch` says which of the two the
# row runs at.  Every row runs again at position 0: the vector-ALU NPAD 16 / 24 (48 above 24 hypotheses) x VEC 4 / 2 forms.
_TILED = [
    ("tiled C24 npad16 9 shifts (8 | 9), NPT 16 pad 8", 24, 24, 7, 7, range(9), 4, (16, False, 4), 2, {}),
    ("tiled C24 npad32 partial vec2 17 shifts (16 | 17)", 24, 12, 5, 5, _centred(17), 2, (32, True, 2), 1, {}),
    ("tiled C40 npad16 vec2 16 shifts (16 | 17), NPT 8 pad 8", 40, 40, 7, 7, range(16), 2, (16, False, 2), 2, {}),
    ("tiled C40 npad32 partial vec2 32 shifts (32 | 33), two workgroups", 40, 20, 13, 11, _centred(32), 2, (32, True, 2), 2, {}),
    ("tiled C80 npad32 20 shifts, npx < TP", 80, 80, 5, 5, range(20), 4, (32, False, 4), 1, {}),
    ("tiled C80 npad16 partial 12 shifts, ldx C + 8", 80, 40, 9, 9, _centred(12), 4, (16, True, 4), 2, dict(ldx=88)),
    ("tiled C104 npad32 20 shifts, KS 2 slices 3 | 4 pad 8", 104, 104, 7, 7, range(20), 4, (32, False, 4), 2, {}),
    ("tiled C104 npad16 partial vec2 11 shifts", 104, 52, 5, 5, _centred(11), 2, (16, True, 2), 1, {}),
    ("tiled C160 npad32 20 shifts, KS 2", 160, 160, 7, 7, range(20), 8, (32, False, 4), 2, {}),
    ("tiled C160 npad16 partial vec2 12 shifts", 160, 80, 5, 5, _centred(12), 2, (16, True, 2), 2, {}),
    ("tiled C200 npad32 vec2 20 shifts, KS 4 uneven pad 8", 200, 200, 5, 5, range(20), 10, (32, False, 2), 2, {}),
    ("tiled C200 npad16 partial 16 shifts", 200, 100, 7, 7, _centred(16), 4, (16, True, 4), 1, {}),
    ("tiled C320 npad16 9 shifts, KS 4", 320, 320, 5, 5, range(9), 16, (16, False, 4), 2, {}),
    ("tiled C320 npad32 partial 21 shifts, 9 tail scores", 320, 160, 3, 7, _centred(21), 16, (32, True, 4), 2, dict(n_tail=9)),
    ("tiled C392 npad32 20 shifts, TP 8 uneven pad 8", 392, 392, 5, 5, range(20), 4, (32, False, 4), 2, {}),
    ("tiled C392 npad16 partial vec2 16 shifts", 392, 196, 3, 5, _centred(16), 2, (16, True, 2), 1, {}),
    ("tiled C1280 npad32 20 shifts 20 tail scores", 1280, 1280, 3, 3, range(20), 64, (32, False, 4), 2, dict(n_tail=20)),
    ("tiled C2048 L512 npad16 partial 16 shifts 16 tail scores", 2048, 512, 3, 3, range(16), 128, (16, True, 4), 2, dict(n_tail=16)),
    ("tiled C1280 npad32 ori_prior(54) 27 shifts n_max 7 n_tail 20", 1280, 1280, 3, 3, ORI_PRIOR_54, 64, (32, False, 4), 2,
     dict(n_max=7, n_tail=20)),
]


def _tiled_rows():
    out = []
    for i, (name, c, l, h, w, shifts, stride, (npad, partial, vec), switch, kw) in enumerate(_TILED):
        n = len(tuple(shifts))
        t = tiled_claim(c, npad, partial, vec)
        v = valu_claim(c, valu_npad(n), partial, vec)
        for bf16 in (False, True):
            out.append(_make(name, c, l, h, w, shifts, stride, (v, t, t), (switch, 0), bf16, wide=bf16 and i % 2 == 1, **kw))
    return out


# ---- the streaming form ---------------------------------------------------------------------------------------------------------------
# The gate needs B hw >= 65 536, so these are the three geometries at that floor: "1x256" the model's last level, "4x128", and
# "5x16x821" = 4 105 tiles — at 256 CUs three tiles per wave, runs of 12 tiles that straddle every sample boundary, and a last
# workgroup of ONE tile (three of its waves return at once).
GEOS = {"1x256": (1, 256, 256), "4x128": (4, 128, 128), "5x16x821": (5, 16, 821)}
# (bf16, MTL, PARTIAL, NB, C, geometry, n_shifts, stride, VEC at the lower switch positions, extras) — all 32 instantiations
_STREAM = [
    (False, 1, False, 2, 24, "1x256", 9, 2, 2, {}),
    (False, 1, False, 3, 40, "4x128", 12, 2, 2, {}),
    (False, 1, False, 4, 56, "5x16x821", 16, 2, 2, {}),
    (False, 1, False, 5, 72, "1x256", 11, 4, 4, dict(ldo=72 + 64)),
    (False, 1, True, 2, 32, "4x128", 16, 2, 2, {}),
    (False, 1, True, 3, 48, "5x16x821", 9, 4, 4, {}),
    (False, 1, True, 4, 64, "1x256", 12, 3, 1, {}),                        # stride 3: odd offsets
    (False, 1, True, 5, 80, "4x128", 13, 4, 4, {}),
    (False, 2, False, 2, 32, "5x16x821", 17, 2, 2, {}),
    (False, 2, False, 3, 48, "1x256", 32, 4, 4, {}),
    (False, 2, False, 4, 64, "4x128", 20, 4, 4, dict(n_max=7)),
    (False, 2, False, 5, 80, "5x16x821", 21, 4, 4, dict(ldx=88)),
    (False, 2, True, 2, 24, "1x256", 20, 2, 2, {}),
    (False, 2, True, 3, 40, "4x128", 21, 2, 2, {}),
    (False, 2, True, 4, 56, "5x16x821", 32, 2, 2, {}),
    (False, 2, True, 5, 72, "1x256", 17, 4, 4, {}),
    (True, 1, False, 2, 32, "4x128", 16, 4, 4, {}),
    (True, 1, False, 3, 48, "5x16x821", 9, 2, 2, dict(wide=True)),
    (True, 1, False, 4, 64, "1x256", 12, 4, 4, {}),
    (True, 1, False, 5, 80, "4x128", 10, 4, 4, dict(wide=True, ldx=88)),
    (True, 1, True, 2, 24, "5x16x821", 11, 2, 2, {}),
    (True, 1, True, 3, 40, "1x256", 16, 2, 2, dict(wide=True)),
    (True, 1, True, 4, 56, "4x128", 9, 2, 2, {}),
    (True, 1, True, 5, 72, "5x16x821", 14, 2, 2, dict(ldo=72 + 64)),
    (True, 2, False, 2, 24, "1x256", 24, 2, 2, dict(wide=True)),
    (True, 2, False, 3, 40, "4x128", 20, 2, 2, {}),
    (True, 2, False, 4, 56, "5x16x821", 17, 2, 2, dict(n_max=9)),
    (True, 2, False, 5, 72, "1x256", 32, 2, 2, dict(wide=True)),
    (True, 2, True, 2, 32, "4x128", 21, 2, 2, {}),
    (True, 2, True, 3, 48, "5x16x821", 32, 3, 1, dict(wide=True)),         # stride 3
    (True, 2, True, 4, 64, "1x256", 18, 4, 4, {}),
    (True, 2, True, 5, 80, "4x128", 21, 4, 4, dict(wide=True)),
]


def _stream_rows():
    out = []
    for bf16, mtl, partial, nb, c, geo, n, stride, vec, kw in _STREAM:
        b, h, w = GEOS[geo]
        l = c // 2 if partial else c
        shifts = _centred(n) if partial else tuple(range(n))
        v = valu_claim(c, valu_npad(n), partial, vec)
        t = tiled_claim(c, 16 * mtl, partial, vec) if vec >= 2 else v
        name = "stream MTL%d%s NB%d C%d %s %d shifts stride %d" % (mtl, " partial" if partial else "", nb, c, geo, n, stride)
        for k in sorted(kw):
            name += ", %s %s" % (k, kw[k])
        out.append(_make(name, c, l, h, w, shifts, stride, (v, t, stream_claim(mtl, partial, nb)), (2,), bf16, b=b, **kw))
    return out


_ROWS = _valu_rows() + _tiled_rows() + _stream_rows()


def rows():
    return list(_ROWS)


def stream_rows():
    return [r for r in _ROWS if r.claims[2].form == STREAM]


def _find(**want):
    for r in stream_rows():
        if all(getattr(r, k) == v for k, v in want.items()):
            return r
    raise KeyError(want)


def _retarget(row, name, claim2, **changes):
    """the far side of a gate pair: `row` with one argument moved across the gate; only position 2's claim is about the gate"""
    r = row._replace(name=name, **changes)
    n = len(r.shifts)
    vec = vec_of(offsets(r.shifts, r.stride, r.woff, r.c))
    partial = r.l < r.c
    v = valu_claim(r.c, valu_npad(n), partial, vec)
    t = tiled_claim(r.c, 16 if n <= 16 else 32, partial, vec) if 9 <= n <= 32 and vec >= 2 else v
    return r._replace(claims=(v, t, t if claim2 == TILED else v))


def gate_pairs():
    """(launched streaming row, the same call one step across a gate of the streaming form, which the route query alone sees)"""
    a = _find(c=72, ldo=72 + 64, bf16=False)
    b1 = _find(c=24, b=1, bf16=False, n_max=9)
    n9 = b1
    n32 = _find(c=48, bf16=False, n_max=32)
    c80 = _find(c=80, l=80, bf16=False)
    return [
        (a, _retarget(a, "gate ldo - C 64 | 68", TILED, ldo=a.ldo + 4)),
        (b1, _retarget(b1, "gate B hw 65536 | 65520", TILED, h=16, w=4095)),
        (n9, _retarget(n9, "gate n_shifts 9 | 8", VALU, shifts=n9.shifts[:8], n_max=8)),
        (n32, _retarget(n32, "gate n_shifts 32 | 33", VALU, shifts=tuple(range(33)), n_max=33)),
        (n32, _retarget(n32, "gate n_tail 0 | 1", TILED, n_tail=1)),
        (c80, _retarget(c80, "gate C 80 | 88", TILED, c=88, l=88, ldx=96, ldo=92)),
    ]


ROUTE_INTS = 10            # CCVPE_MATCH_ROUTE_INTS


def route_query(lib, row):
    """ccvpe_match_route for the row's call at the current switch position: (form or negative error code, the ten ints)"""
    import ctypes
    sh = (ctypes.c_int * len(row.shifts))(*row.shifts)
    out = (ctypes.c_int * ROUTE_INTS)(*([-7] * ROUTE_INTS))
    rc = lib.ccvpe_match_route(2 if row.bf16 else 4, row.l, sh, len(row.shifts), row.n_max, row.n_tail, row.stride, row.woff,
                               row.ldx, row.ldo, row.b, row.h * row.w, row.c, out)
    return rc, list(out)


def assert_route(lib, row, claim, where=""):
    """the query's answer is exactly the claim, and the restated pitch, LDS bytes and K slices are the launcher's"""
    rc, out = route_query(lib, row)
    what = "%s%s" % (row.name, where)
    assert rc == claim.form, "%s: form %d, the row claims %d" % (what, rc, claim.form)
    assert tuple(out[:8]) == tuple(int(v) for v in claim[1:9]), "%s: (NPAD, PARTIAL, VEC, NB, LPP, TP, NPT, KS) = %s, the row claims %s" % (what, out[:8], tuple(claim[1:9]))
    if claim.form == STREAM:
        assert out[8:] == [0, 0], what
        return
    pitch = match_pitch_mfma(row.c) if claim.form == TILED else match_pitch(row.c, claim.lpp)
    assert out[8] == pitch and out[9] == lds_bytes(row.c, len(row.shifts), claim), "%s: pitch %d LDS %d B, restated %d, %d" % (what, out[8], out[9], pitch, lds_bytes(row.c, len(row.shifts), claim))
    assert out[9] <= 160 * 1024, what
    if claim.form == TILED:
        assert claim.slices == k_slices(row.c, claim.ks), "%s: K slices %s" % (what, k_slices(row.c, claim.ks))


def instantiation(row, claim):
    """the template instance a claim names, as text"""
    tx = "bf16" if row.bf16 else "float"
    if claim.form == STREAM:
        return "match_stream_kernel<%s,%d,%s,%d>" % (tx, claim.npad // 16, "true" if claim.partial else "false", claim.nb)
    return "match_kernel<%s,%d,%s,%d%s>" % (tx, claim.npad, "true" if claim.partial else "false", claim.vec, ",MFMA" if claim.form == TILED else "")


def inst_key(row, claim):
    return (claim.form, row.bf16, claim.npad, claim.partial, claim.nb if claim.form == STREAM else claim.vec)


def owner(row, claim, b, pixel, cus=256):
    """who computes pixel `pixel` of sample b: workgroup (or run), wave, K slices — for a failure message"""
    if claim.form == STREAM:
        g = stream_geometry(row.b, row.h * row.w, cus)
        tile = (b * row.h * row.w + pixel) // 16
        wg = tile // g.run
        return "tile %d of run / workgroup %d (tiles %d..%d), wave %d" % (tile, wg, wg * g.run, min((wg + 1) * g.run, g.tiles) - 1, (tile - wg * g.run) % 4)
    wg, pp = divmod(pixel, claim.tp)
    if claim.form == VALU:
        lane0 = pp * claim.lpp
        return "workgroup (%d, %d), pixel %d of %d, lanes %d..%d of wave %d" % (wg, b, pp, claim.tp, lane0 % 64, lane0 % 64 + claim.lpp - 1, lane0 // 64)
    tile = pp // 16
    if claim.ks == 1:
        return "workgroup (%d, %d), 16-pixel tile %d column %d, wave %d, one K slice" % (wg, b, tile, pp % 16, tile % 4)
    waves = [tile + q * (2 if claim.npt == 2 else 1) for q in range(claim.ks)]
    return "workgroup (%d, %d), 16-pixel tile %d column %d, K slices %s (16-channel blocks) on waves %s" % (wg, b, tile, pp % 16, list(claim.slices), waves)
