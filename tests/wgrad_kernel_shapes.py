"""Weight-gradient shapes that pin every launched form of conv_wgrad_kernel (csrc/conv_wgrad.hip) alone, and the edges of its
launcher — pixel splits that end mid-stage, empty trailing splits, column tiles that span taps and sources, ragged row tiles,
grids that are no multiple of 8, every lane count of the merge kernel — each at the smallest size that still has its property.

Shared by tests/test_wgrad_forms_gpu.py (values against float64, elementwise: tests/wgrad_check.py), tests/test_wgrad_check.py
(the same comparison on CPU float32 results and on faulted ones) and tests/test_abi.py (the restated planner against the expected
columns and against the library's host-only queries ccvpe_conv_wgrad_tile / ccvpe_conv_wgrad_scratch_floats, so that a planner
change shows up as a stale row in a plain `-m "not gpu"` run).

Where the forms come from: conv_wgrad_impl / wgrad_pick / wgrad_splits in csrc/conv_wgrad.hip, launch_sum_parts in csrc/common.h,
and what the committed trace of the real training step lists (profiles/r06/r06_train_kernel_stats.csv) — the literal list below.
"""
from collections import namedtuple

WG_BP = 32          # pixels per stage (csrc/conv_wgrad.hip)

# ------------------------------------------------------------------------------------------------------------------------------
# The launcher's planner, restated.
#   tile rows: the candidate that minimises (padded rows) / (relative efficiency), first candidate on ties; the 128-row tile
#   needs n >= 128 and ncols >= 512 and is 128 columns wide, every other tile 64;
#   S = min(4096 // tiles, ceil(M / 256), 1024), at least 1: the pixel range is cut into S splits of pps = roundup32(ceil(M / S))
#   pixels, so the last non-empty split ends mid-stage and trailing splits can be empty (they still write zero partials);
#   the merge (launch_sum_parts) uses LN lanes per element: LN = 1, times 4 while LN < 64 and S > 8 LN and elements * LN < 256 K.
# ------------------------------------------------------------------------------------------------------------------------------
CAND = (16, 32, 48, 64, 80, 128)
EFF = (0.45, 0.70, 0.75, 0.80, 0.90, 1.00)


def pick(n, ncols):
    best, best_cost = 64, 1e30
    for t, e in zip(CAND, EFF):
        if t == 128 and (n < 128 or ncols < 512):
            continue
        cost = float((n + t - 1) // t * t) / e
        if cost < best_cost:
            best, best_cost = t, cost
    return best


def tile_cols(tile):
    return 128 if tile == 128 else 64


def splits(m, tiles):
    s = min(4096 // max(tiles, 1), (m + WG_BP * 8 - 1) // (WG_BP * 8), 1024)
    return max(s, 1)


def merge_lanes(nparts, n):
    ln = 1
    while ln < 64 and nparts > 8 * ln and n * ln < 256 * 1024:
        ln *= 4
    return ln


Plan = namedtuple("Plan", "tile tiles_n tiles_c s pps last_px empty grid_mod8 ln_dw ln_bias")


def out_dims(h, w, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def plan(row):
    """what conv_wgrad_impl launches for the row"""
    ho, wo = out_dims(row.h, row.w, row.k, row.stride, row.pad)
    m = row.b * ho * wo
    ncols = row.k * row.k * (row.c0 + row.c1)
    tile = pick(row.n, ncols)
    tn, tc = (row.n + tile - 1) // tile, (ncols + tile_cols(tile) - 1) // tile_cols(tile)
    s = splits(m, tn * tc)
    pps = ((m + s - 1) // s + WG_BP - 1) // WG_BP * WG_BP
    nonempty = (m + pps - 1) // pps
    return Plan(tile, tn, tc, s, pps, m - (nonempty - 1) * pps, s - nonempty, (tn * tc * s) % 8, merge_lanes(s, row.n * ncols),
                merge_lanes(s, row.n))


def merge_chain(s, ln):
    """longest chain of fp32 additions a partial passes through in sum_parts_lanes_kernel<LN>: a lane adds every LN-th partial into
    two alternating sums, adds those, and lane 0 adds the LN lane sums in order"""
    per_lane = (s + ln - 1) // ln
    return (per_lane + 1) // 2 + 1 + (ln - 1)


# ------------------------------------------------------------------------------------------------------------------------------
# What the traced training step launches (profiles/r06/r06_train_kernel_stats.csv): (tile rows, tile columns, gated)
# ------------------------------------------------------------------------------------------------------------------------------
TRACED = [(16, 64, False), (32, 64, False), (48, 64, False), (64, 64, False), (80, 64, False), (128, 128, False),
          (16, 64, True), (32, 64, True), (48, 64, True), (64, 64, True), (80, 64, True)]

# num: the row's number;  kind: "plain" (ccvpe_conv_wgrad_f32 and ccvpe_conv_wgrad_bias_f32, backward.conv_wgrad), "deconv" (the
# same with the roles of input and output gradient swapped, backward.deconv_wgrad) or "gated" (ccvpe_conv_wgrad_gated_f32,
# backward.conv1x1_wgrad_gated);  b, h, w: the conv's INPUT plane;  c0 of ld0 floats per pixel from the first source, c1 from the
# second;  n of ldy floats per pixel of dY.
WgRow = namedtuple("WgRow", "num name kind b h w k stride pad c0 ld0 c1 n ldy plan")


def _r(num, name, b, h, w, k, c0, c1, n, plan_, kind="plain", stride=1, pad=None, ld0=None, ldy=None):
    return WgRow(num, "%02d %s" % (num, name), kind, b, h, w, k, stride, k // 2 if pad is None else pad, c0, ld0 or c0, c1, n,
                 ldy or n, Plan(*plan_))


# plane A: 3 x 19 x 23 output pixels, M = 1311: S = 6 splits of 224; the last has 191 px = five stages and one of 31; Wo = 23 < 32
A = (3, 19, 23)
ROWS = [
    #                                                                                tile tn tc   S  pps last empty %8 LNw LNb
    _r(1, "3x3 C16 N16: three taps per column tile, last column tile 16 of 64", *A, 3, 16, 0, 16, (16, 1, 3, 6, 224, 191, 0, 2, 1, 1)),
    _r(2, "3x3 C24+8 N24: two sources, rows 24..31 not stored", *A, 3, 24, 8, 24, (32, 1, 5, 6, 224, 191, 0, 6, 1, 1)),
    _r(3, "3x3 C40 of ld0 48 + C16 N40: wider pixel rows, second dY piece half used", *A, 3, 40, 16, 40,
       (48, 1, 8, 6, 224, 191, 0, 0, 1, 1), ld0=48),
    _r(4, "1x1 C112 N126 ldy 128: ragged N with padding columns, 62-row and 48-column last tiles", *A, 1, 112, 0, 126,
       (64, 2, 2, 6, 224, 191, 0, 0, 1, 1), ldy=128),
    _r(5, "3x3 C24 N64: 32x32 MFMA path, several taps per column tile", *A, 3, 24, 0, 64, (64, 1, 4, 6, 224, 191, 0, 0, 1, 1)),
    _r(6, "3x3 C80+24 N80: conv3.0's form, source seam inside a tile", *A, 3, 80, 24, 80, (80, 1, 15, 6, 224, 191, 0, 2, 1, 1)),
    _r(7, "3x3 C64 N136: second row tile of 56 rows", *A, 3, 64, 0, 136, (80, 2, 9, 6, 224, 191, 0, 4, 1, 1)),
    _r(8, "3x3 C64 N128: big tile with splits, last column tile 64 of 128", *A, 3, 64, 0, 128, (128, 1, 5, 6, 224, 191, 0, 6, 1, 1)),
    _r(9, "3x3 C64 N200: big tile, second row tile of 72 rows", *A, 3, 64, 0, 200, (128, 2, 5, 6, 224, 191, 0, 4, 1, 1)),
    _r(10, "1x1 C520 N640: big tile 5 x 5, last column tile 8 columns", *A, 1, 520, 0, 640, (128, 5, 5, 6, 224, 191, 0, 6, 1, 1)),
    _r(11, "2x2 stride 2 C64 N48: strided taps", 3, 38, 46, 2, 64, 0, 48, (48, 1, 4, 6, 224, 191, 0, 0, 1, 1), stride=2, pad=0),
    _r(12, "deconv: x 19x23x48, dy_hi 38x46x16, one tile", 3, 38, 46, 2, 16, 0, 48, (48, 1, 1, 6, 224, 191, 0, 6, 1, 1),
       kind="deconv", stride=2, pad=0),
    _r(13, "3x3 C24+8 N24 on 61x5: Wo = 5, the cursor carries six to seven times per stage", 3, 61, 5, 3, 24, 8, 24,
       (32, 1, 5, 4, 256, 147, 0, 4, 1, 1)),
    _r(14, "gated C96 N16", *A, 1, 96, 0, 16, (16, 1, 2, 6, 224, 191, 0, 4, 1, 1), kind="gated"),
    _r(15, "gated C144 N24", *A, 1, 144, 0, 24, (32, 1, 3, 6, 224, 191, 0, 2, 1, 1), kind="gated"),
    _r(16, "gated C240 N40", *A, 1, 240, 0, 40, (48, 1, 4, 6, 224, 191, 0, 0, 1, 1), kind="gated"),
    _r(17, "gated C480 N80", *A, 1, 480, 0, 80, (80, 1, 8, 6, 224, 191, 0, 0, 1, 1), kind="gated"),
    _r(18, "gated C672 N112", *A, 1, 672, 0, 112, (64, 2, 11, 6, 224, 191, 0, 4, 1, 1), kind="gated"),
    _r(19, "gated C1152 N320: 4 x 18 tiles", *A, 1, 1152, 0, 320, (80, 4, 18, 6, 224, 191, 0, 0, 1, 1), kind="gated"),
    _r(20, "3x3 C80+24 N80 on 31x33: S = 12, merge with 4 lanes", 3, 31, 33, 3, 80, 24, 80, (80, 1, 15, 12, 256, 253, 0, 4, 4, 4)),
    _r(21, "3x3 C16 N16 on 4x50x50: S = 40, last split 16 px, merge with 16 lanes", 4, 50, 50, 3, 16, 0, 16,
       (16, 1, 3, 40, 256, 16, 0, 0, 16, 16)),
    _r(22, "1x1 C8 N16 on 4x257x256: the 1024-split cap, 110 empty splits, merge with 64 lanes", 4, 257, 256, 1, 8, 0, 16,
       (16, 1, 1, 1024, 288, 224, 110, 0, 64, 64)),
    _r(23, "3x3 C456 N16 on 5x59x57: S limited by 65 column tiles, 4 empty splits, grid 4095", 5, 59, 57, 3, 456, 0, 16,
       (16, 1, 65, 63, 288, 111, 4, 7, 4, 16)),
]


def rows():
    return ROWS


def form(row):
    """the instantiation the row launches: (tile rows, tile columns, gated)"""
    return (row.plan.tile, tile_cols(row.plan.tile), row.kind == "gated")


def dims(row):
    """(Ho, Wo, M, ctot, taps, ncols)"""
    ho, wo = out_dims(row.h, row.w, row.k, row.stride, row.pad)
    ctot = row.c0 + row.c1
    return ho, wo, row.b * ho * wo, ctot, row.k * row.k, row.k * row.k * ctot
