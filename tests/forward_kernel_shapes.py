"""Forward shapes that pin every conv3x3_kernel form and every mbconv_band_kernel instantiation of the B = 64 steps, each at the
smallest size that still selects it.

Shared by tests/test_forward_variants_gpu.py (values against float64, elementwise: tests/forward_variant_check.py), by
tests/test_forward_variant_check.py (the same comparison on faulted CPU results) and by tests/test_abi.py (the host-only queries
ccvpe_conv_igemm_route / ccvpe_conv3x3_variant / ccvpe_mbconv_band_plan over every row, so that a routing change shows up as a
stale row in a plain `-m "not gpu"` run instead of silently moving a row onto an easier path).

Where the forms come from: the dispatchers in csrc/conv3x3_impl.h (conv3x3_variant: nine <MT,NT,WN> tiles x 4 / 8 waves x a row
of taps or one tap per K stage) and csrc/mbconv_plane.hip (mbband_plan), and what the committed traces of the real steps list
(profiles/r06/r06_train_kernel_stats.csv, fwd_trace_fp32.csv, fwd_trace_bf16*.csv) — the literal lists below.
"""
from collections import namedtuple

# ------------------------------------------------------------------------------------------------------------------------------
# conv3x3_kernel<T, MT, NT, WN, NW, TPS> (DMA below is bit 4 of ccvpe_conv3x3_variant: W staged by LDS-DMA, always set).
# A workgroup tile is (16 MT NW / (16 WN)) rows x 16 columns of pixels x 16 NT WN
# output channels: <4,x,2> tiles are 8 rows tall with 4 waves and 16 with 8, <4,x,1> 16 rows, <2,7,1> 8 rows.
#
# Every row has two sources (c1 > 0 keeps bf16 off the narrow c3n route) and K = 9 x 40: 22.5 fp32 stages of 16 channels / 11.25
# bf16 stages of 32, i.e. a partial last K stage in both types, a chunk that straddles the two sources, and fewer than the 24
# stages at which ops.conv_igemm would cut K into slices (that path is the generic gather kernel, not conv3x3_kernel).
#   name, b, h, w, c0, c1, n: the launch;  ld0 / real0: row pitch of source 0 and how many of its c0 channels hold data (the rest
#   are zero with NON-zero weights);  tile: <MT,NT,WN>;  f32 / bf16: (NW, DMA, TPS) the row must select in that type, None = the
#   row is not run in that type.
# ------------------------------------------------------------------------------------------------------------------------------
ConvRow = namedtuple("ConvRow", "name b h w c0 c1 n ld0 real0 tile f32 bf16")


def _c(name, b, h, w, n, tile, f32=(4, True, 3), bf16=(4, True, 3), c0=24, c1=16, ld0=None, real0=None):
    return ConvRow(name, b, h, w, c0, c1, n, ld0 or c0, real0 or c0, tile, f32, bf16)


CONV3X3 = [
    # 128-channel tile, 4 waves: three 8-row tiles with a 3-row tail, two column tiles with a 4-column tail
    _c("<4,4,2> N = 128, 19 x 20", 2, 19, 20, 128, (4, 4, 2)),
    _c("<4,2,2> N = 64, 11 x 20", 2, 11, 20, 64, (4, 2, 2)),
    _c("<4,1,2> N = 32, 11 x 20", 2, 11, 20, 32, (4, 1, 2)),
    # 160-channel tile: two N tiles (a second W panel base), three column tiles with a 4-column tail, a 3-row tail
    _c("<4,5,2> N = 320, 11 x 36", 2, 11, 36, 320, (4, 5, 2)),
    _c("<4,3,2> N = 96, 11 x 20", 2, 11, 20, 96, (4, 3, 2)),
    # 256-pixel tiles (one wave column): 16-row tiles, 19 rows = a second row tile of 3 rows
    _c("<4,3,1> N = 48, 19 x 20", 2, 19, 20, 48, (4, 3, 1)),
    # the 256 x 80 tile keeps one tap per stage (a row of taps measured the same there)
    _c("<4,5,1> N = 80, 11 x 20", 2, 11, 20, 80, (4, 5, 1), f32=(4, True, 1), bf16=(4, True, 1)),
    _c("<4,1,1> N = 16, 11 x 20", 2, 11, 20, 16, (4, 1, 1)),
    _c("<2,7,1> N = 112, 11 x 20", 2, 11, 20, 112, (2, 7, 1)),
    # ragged N inside a tile: Npad = 48, columns 40 .. 47 of the last 16-column group are computed and not stored (store4's
    # scalar tail), their scale / shift are not read
    _c("<4,3,1> N = 40 (ragged N), 11 x 20", 2, 11, 20, 40, (4, 3, 1)),
    # the decoder's concat buffers: rows wider than the channels the conv reads (ld0 = 32 > c0 = 24) and padding channels that are
    # zero in the data but not in the weights (21 real channels)
    _c("<4,2,2> N = 64, ld0 = 32 > c0 = 24, 21 real channels", 2, 11, 20, 64, (4, 2, 2), ld0=32, real0=21),
]

# 8-wave thresholds: (the row that takes NW = 8, the same shape with one image fewer, which takes NW = 4).  The tile doubles to
# 16 rows (H % 16 == 0 is part of the gate); both members are checked against ONE reference (the shared batch prefix).
#   fp32 <4,4,2>: >= 512 workgroups.  64 x 40 x 512: 3 column tiles x 4 row tiles x 4 N tiles = 48 per image; 11 images = 528,
#                 10 = 480.  The 8-wave fp32 form has one tap per stage (128-VGPR cap: no second fragment set).
#   bf16 <4,5,2> / <4,4,2>: >= 256 workgroups and >= 2 N tiles.  64 x 64 x 320 (or 256): 4 x 4 x 2 = 32 per image; 8 images = 256.
CONV3X3_NW8_PAIRS = [
    (_c("fp32 <4,4,2> NW = 8: 11 x 64 x 40, N = 512", 11, 64, 40, 512, (4, 4, 2), f32=(8, True, 1), bf16=None),
     _c("fp32 <4,4,2> NW = 4: 10 x 64 x 40, N = 512", 10, 64, 40, 512, (4, 4, 2), f32=(4, True, 3), bf16=None)),
    (_c("bf16 <4,5,2> NW = 8: 8 x 64 x 64, N = 320", 8, 64, 64, 320, (4, 5, 2), f32=None, bf16=(8, True, 3)),
     _c("bf16 <4,5,2> NW = 4: 7 x 64 x 64, N = 320", 7, 64, 64, 320, (4, 5, 2), f32=None, bf16=(4, True, 3))),
    (_c("bf16 <4,4,2> NW = 8: 8 x 64 x 64, N = 256", 8, 64, 64, 256, (4, 4, 2), f32=None, bf16=(8, True, 3)),
     _c("bf16 <4,4,2> NW = 4: 7 x 64 x 64, N = 256", 7, 64, 64, 256, (4, 4, 2), f32=None, bf16=(4, True, 3))),
]

# What the traced B = 64 steps launch, as (MT, NT, WN, NW, DMA, TPS): tests/test_abi.py asserts that the rows above select every
# one of them.  (DMA is always True: pick_cfg only returns tiles whose width divides Npad — DESIGN.md section 4.)
CONV3X3_TRACED_F32 = [
    (4, 5, 2, 4, True, 3), (4, 4, 2, 8, True, 1), (4, 3, 2, 4, True, 3), (4, 2, 2, 4, True, 3), (4, 1, 2, 4, True, 3),
    (4, 5, 1, 4, True, 1), (4, 3, 1, 4, True, 3), (4, 1, 1, 4, True, 3), (2, 7, 1, 4, True, 3),
]
CONV3X3_TRACED_BF16 = [(4, 4, 2, 4, True, 3), (4, 4, 2, 8, True, 3), (4, 5, 2, 4, True, 3), (4, 5, 2, 8, True, 3)]


def conv_rows():
    """every ConvRow: the single rows, then both members of each threshold pair"""
    return CONV3X3 + [r for pair in CONV3X3_NW8_PAIRS for r in pair]


# ------------------------------------------------------------------------------------------------------------------------------
# mbconv_band_kernel<k, stride, NKK, TPW, RY> (bf16 fused MBConv front of the late blocks, mid = 6 cin).  A workgroup owns a
# (sample, row band) and walks `cpg` 16-channel slices of mid through a producer / consumer pipeline (plane and weight double
# buffers, a triple-buffered weight panel); ngrp = ceil(mid / 16 / cpg) workgroups share a band and the last one may get fewer
# slices.  cpg is chosen so that the launch is about one workgroup per CU: it depends on the batch and on the device's CU count.
#   inst: (k, stride, nkk, tpw, ry);  cpg256 / ngrp256: the grouping for 256 CUs (what the query gives without a GPU, and on the
#   MI355X);  last: slices of the last group;  deep: the GPU test also asserts cpg >= 3 on the device it runs on.
# ------------------------------------------------------------------------------------------------------------------------------
BandRow = namedtuple("BandRow", "name b h w cin k s circ inst cpg256 ngrp256 last deep")

BAND = [
    BandRow("32 x 32 x 112 k5, B = 3: one slice per workgroup", 3, 32, 32, 112, 5, 1, False, (5, 1, 4, 10, 2), 1, 42, 1, False),
    BandRow("16 x 16 x 192 k5, B = 7: two slices (no steady state)", 7, 16, 16, 192, 5, 1, False, (5, 1, 6, 4, 1), 2, 36, 2, False),
    BandRow("32 x 32 x 80 k3, B = 9: three slices, even groups", 9, 32, 32, 80, 3, 1, False, (3, 1, 3, 10, 2), 3, 10, 3, True),
    BandRow("32 x 32 x 112 k5, B = 13: five slices, last group of 2", 13, 32, 32, 112, 5, 1, False, (5, 1, 4, 10, 2), 5, 9, 2, True),
    BandRow("32 x 32 x 112 k5, B = 24: nine slices, last group of 6", 24, 32, 32, 112, 5, 1, False, (5, 1, 4, 10, 2), 9, 5, 6, True),
    BandRow("16 x 16 x 192 k5, B = 64: the benched launch, 18 slices", 64, 16, 16, 192, 5, 1, False, (5, 1, 6, 4, 1), 18, 4, 18, True),
    # the ground planes (circular padding along W), one output row per depthwise thread
    BandRow("20 x 40 x 80 k3 circular, B = 13", 13, 20, 40, 80, 3, 1, True, (3, 1, 3, 10, 1), 4, 8, 2, True),
    BandRow("10 x 20 x 192 k3 circular, B = 15", 15, 10, 20, 192, 3, 1, True, (3, 1, 6, 4, 1), 5, 15, 2, True),
    BandRow("20 x 40 x 80 k5 circular, B = 13", 13, 20, 40, 80, 5, 1, True, (5, 1, 3, 10, 1), 4, 8, 2, True),
    BandRow("20 x 40 x 112 k5 circular, B = 10", 10, 20, 40, 112, 5, 1, True, (5, 1, 4, 10, 1), 4, 11, 2, True),
    # two output rows per depthwise thread (ry = 2) at the third K-piece count
    BandRow("32 x 32 x 80 k5, B = 13", 13, 32, 32, 80, 5, 1, False, (5, 1, 3, 10, 2), 4, 8, 2, True),
    # stride 2: aerial 32 x 32 -> 16 x 16 and ground 20 x 40 -> 10 x 20
    BandRow("32 x 32 x 112 k5 stride 2, B = 10", 10, 32, 32, 112, 5, 2, False, (5, 2, 4, 10, 1), 4, 11, 2, True),
    BandRow("20 x 40 x 112 k5 stride 2 circular, B = 12", 12, 20, 40, 112, 5, 2, True, (5, 2, 4, 10, 1), 5, 9, 2, True),
]

# every mbconv_band_kernel instantiation in profiles/r06/fwd_trace_bf16.csv
BAND_TRACED = [(3, 1, 3, 10, 1), (3, 1, 3, 10, 2), (3, 1, 6, 4, 1), (5, 1, 3, 10, 1), (5, 1, 3, 10, 2), (5, 1, 4, 10, 1),
               (5, 1, 4, 10, 2), (5, 1, 6, 4, 1), (5, 2, 4, 10, 1)]

# A shape inside the plane geometry's limits that passes the band kernel's shape test (8 tiles per wave, 4 K pieces) but needs
# more than 160 KB of LDS for its two 13-row planes of >= 60 pixels: the launcher falls back to the slice-per-workgroup kernel, and
# since the route, the plan query and the launcher share one helper the route says so.  (h, w, cin, k, stride)
BAND_LDS_REFUSED = (9, 56, 112, 5, 1)
