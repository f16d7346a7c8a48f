"""Training-step shapes of the size-dependent reduction kernels, with the geometry each row is there to pin.

Shared by tests/test_fullsize_train_kernels_gpu.py (values against float64 at these shapes) and tests/test_abi.py (the
same geometry queries without a GPU, so a routing change shows up as a stale row in a plain `-m "not gpu"` run).

Where the model rows come from (ccvpe_amd/train.py, synth.MODEL_SPECS, B = 64 as bench.py's training step):
  * EfficientNet-B0 encoders (synth.B0_BLOCKS): VIGOR ground 320 x 640 (stem output 160 x 320), aerial 512 x 512 (stem
    output 256 x 256), KITTI ground 256 x 1024.  Block 0 runs its depthwise conv at the stem resolution, blocks 1-2 at /4,
    blocks 3-4 at /8, blocks 11-15 at /32 (ground 10 x 20, aerial 16 x 16); the head conv is 320 -> 1280.
    BatchNorm rows = B * h * w of the tensor it normalises (encoder_forward: _bn0 / _bn1 / _bn2).
  * Matching levels j = 0..5 (forward_train): C = sat_desc, then loc[j-1][3]; hw = 8 * 2^j; L = (ground width / 32) * cd[j];
    shifts = range(n_rot) (level 0 also carries the n_rot orientation tail), or loc_shifts + range(n_rot) with an
    orientation prior (ori_noise = 180 degrees: k = 10, 21 location shifts).
  * Decoder heads: conv1.2 (16 -> 1) and conv1_ori.2 (16 -> 2) at 512 x 512; the localisation softmax over 512^2 logits.
Rows marked "edge" are not model shapes: they take the branches the geometry has but the model does not reach at B = 64.
"""

# BatchNorm statistics (ccvpe_bn_stats_f32).  (name, rows, C, rpb, nblk_query) with nblk_query = ccvpe_bn_stats_nblk(rows) =
# partial rows + fold groups.  rpb = 32 below 65 536 rows, else 256 * ceil(rows / 2^20).
BN_STATS = [
    ("VIGOR ground _bn0: stem out 64 x 160 x 320", 64 * 160 * 320, 32, 1024, 3200 + 50),
    ("VIGOR aerial block 2 _bn2: 64 x 128 x 128, C = 24", 64 * 128 * 128, 24, 256, 4096 + 64),
    ("VIGOR aerial block 3 _bn2: 64 x 64 x 64, C = 40", 64 * 64 * 64, 40, 256, 1024 + 16),
    ("VIGOR aerial head _bn1: 64 x 16 x 16, C = 1280", 64 * 16 * 16, 1280, 32, 512 + 8),
    ("edge: 2^20 + 1 rows (rpb 512, one-row last block), C = 24", 1048577, 24, 512, 2049 + 33),
    ("edge: C = 1280 above 65 536 rows (cw = 256 loop), ragged", 70001, 1280, 256, 274 + 5),
    ("edge: 65 535 rows (last rpb = 32 size), C = 56", 65535, 56, 32, 2048 + 32),
]

# BatchNorm apply (ccvpe_bn_act_f32) and its backward (ccvpe_bn_act_bwd_f32): both split one sample's rows into
# max(rows_per_sample / 32, 8)-row workgroups, so the geometry depends on rows per sample only and the tests may use fewer
# samples.  (name, batch, rows_per_sample, C, act, with_dcs_and_residual, nblk)   act: 2 swish, 0 none
BN_ACT = [
    ("VIGOR ground stem _bn0: 160 x 320, C = 32, swish", 8, 160 * 320, 32, 2, False, 32),
    ("VIGOR ground block 2 _bn2: 80 x 160, C = 24, drop-connect + residual", 4, 80 * 160, 24, 0, True, 32),
    ("VIGOR ground block 15 _bn0: 10 x 20, C = 1152, swish", 64, 10 * 20, 1152, 2, False, 25),
    ("VIGOR aerial head _bn1: 16 x 16, C = 1280, swish", 64, 16 * 16, 1280, 2, False, 32),
    ("edge: 51 201 rows per sample (ragged last workgroup), C = 40", 2, 51201, 40, 2, True, 33),
]

# BatchNorm + squeeze-excite (bn_act(want_se) -> se_bn_bwd_reduce -> se_bwd -> se_bn_bwd_apply, se_dgate): the MBConv
# _bn1 of a block.  (name, batch, h, w, C, Cs, nblk)  nblk = ccvpe_bn_act_nblk = ccvpe_bn_bwd_nblk (rows per sample)
BN_SE = [
    ("VIGOR ground block 0 _bn1 + SE: 160 x 320, C = 32, Cs = 8", 4, 160, 320, 32, 8, 32),
    ("VIGOR ground block 1 _bn1 + SE: 80 x 160, C = 96, Cs = 4", 4, 80, 160, 96, 4, 32),
    ("VIGOR aerial block 11 _bn1 + SE: 16 x 16, C = 1152, Cs = 48", 64, 16, 16, 1152, 48, 32),
]

# Depthwise weight gradient, all-taps kernel (planes above 1 024 pixels).  (name, batch, H, W, C, k, stride, circular, nblk)
# nblk = ccvpe_dwconv_wgrad_nblk = ceil(Ho / dww_rows(Ho)), dww_rows = 1 / 2 / 4 for Ho <= 64 / <= 128 / above.
DW_WGRAD = [
    ("VIGOR aerial block 0 dw: 256 x 256, C = 32, k3 s1", 16, 256, 256, 32, 3, 1, False, 64),
    ("VIGOR ground block 0 dw: 160 x 320, C = 32, k3 s1 circular", 16, 160, 320, 32, 3, 1, True, 40),
    ("VIGOR ground block 1 dw: 160 x 320, C = 96, k3 s2 circular", 8, 160, 320, 96, 3, 2, True, 40),
    ("VIGOR aerial block 2 dw: 128 x 128, C = 144, k5 s1", 8, 128, 128, 144, 5, 1, False, 64),
    ("VIGOR ground block 3 dw: 80 x 160, C = 144, k5 s2 circular", 8, 80, 160, 144, 5, 2, True, 40),
    ("edge: Ho = 65 (two-row workgroups, one-row last), C = 48, k3 s2", 4, 130, 66, 48, 3, 2, False, 33),
]

# Head 3x3 conv backward (ccvpe_head_conv3x3_bwd_f32): 64 x 4 pixel tiles, at most CCVPE_HEAD_WGRAD_BLOCKS workgroups
# walking them grid-stride.  B = 64 at 512^2 is 65 536 tiles, 64 per workgroup; fewer samples keep > 1 trip per workgroup.
# (name, batch, H, W, cout, ntiles)
HEAD_WGRAD_BLOCKS = 1024                 # include/ccvpe_hip.h
HEAD_BWD = [
    ("conv1.2 (16 -> 1) at 512 x 512", 4, 512, 512, 1, 4096),
    ("conv1_ori.2 (16 -> 2) at 512 x 512", 4, 512, 512, 2, 4096),
    ("edge: 511 x 200, ragged tiles, 1 or 2 trips per workgroup", 3, 511, 200, 2, 1536),
]

# Stem weight gradient (ccvpe_stem_conv_wgrad_f32): 16-row x 256-column output groups per sample.
# (name, batch, H, W, circular, nblk = ccvpe_stem_wgrad_nblk(batch, H, W), partial last column group)
STEM_WGRAD = [
    ("VIGOR ground stem: 320 x 640 circular (Wo = 320: groups of 256 + 64)", 16, 320, 640, True, 16 * 10 * 2, True),
    ("VIGOR aerial stem: 512 x 512", 8, 512, 512, False, 8 * 16 * 1, False),
    ("KITTI ground stem: 256 x 1024 (two full column groups)", 8, 256, 1024, False, 8 * 8 * 2, False),
    ("edge: 40 x 600 zero padding (Wo = 300: 256 + 44)", 4, 40, 600, False, 4 * 2 * 2, True),
]

# Matching backward (ccvpe_match_level_bwd_f32).  (name, batch, C, L, hw_side, shifts, n_max, n_tail, stride, nblk, npad)
# nblk = ccvpe_match_bwd_nblk(hw, batch, C) = pixel workgroups x channel slices; npad = the shift-count instantiation.
ORI_PRIOR_SHIFTS = list(range(-10, 11)) + list(range(20))
MATCH_BWD = [
    ("VIGOR level 1: C = 640, 16 x 16, L = 640 (LDS above 64 KB)", 64, 640, 640, 16, list(range(20)), 20, 0, 32, 1 * 8, 20),
    ("VIGOR level 2: C = 320, 32 x 32, L = 320 (LDS above 64 KB)", 64, 320, 320, 32, list(range(20)), 20, 0, 16, 4 * 2, 20),
    ("VIGOR level 0 with ori_noise = 180: 41 shifts", 64, 1280, 1280, 8, ORI_PRIOR_SHIFTS, 21, 20, 64, 1 * 8, 48),
    ("KITTI level 0: C = 2048, 8 x 8, L = 512 at B = 2 (32 channel slices)", 2, 2048, 512, 8, list(range(16)), 16, 16, 128, 1 * 32, 16),
    ("VIGOR level 5: C = 40, 256 x 256, L = 40 (one sample)", 1, 40, 40, 256, list(range(20)), 20, 0, 2, 256 * 1, 20),
]

# Softmax backward over the flattened heat map and the cross-entropy backward.  (name, rows, n)
SOFTMAX_BWD = [
    ("VIGOR / KITTI heat map: 64 x 512^2", 64, 512 * 512),
    ("edge: n / 4 not a multiple of the 1 024 lanes", 3, 4 * 1023 + 4 * 517),
]

# Bias gradient column sums (ccvpe_colsum_f32): CS_ROWS = 1 024-row workgroups from 256 * 1 024 rows on.
# (name, rows, C, ld)
CS_ROWS = 1024
COLSUM = [
    ("conv1.0 bias (16 ch at 512^2), 4 samples", 4 * 512 * 512, 16, 16),
    ("conv2.0 bias (32 ch at 256^2), 16 samples", 16 * 256 * 256, 32, 32),
    ("edge: 300 001 rows, 6 of 8 columns (scalar path)", 300001, 6, 8),
]


def sum_parts_chain(nparts, n):
    """Longest serial add chain of launch_sum_parts (csrc/common.h) for nparts rows of n elements."""
    ln = 1
    while ln < 64 and nparts > 8 * ln and n * ln < 256 * 1024:
        ln *= 4
    return (nparts + ln - 1) // ln + ln


def match_bwd_lds_bytes(C, L, hw, n_shifts, npad):
    """Dynamic LDS of match_bwd_kernel (csrc/matching_bwd.hip: launch_match_bwd)."""
    tpb = 256 if hw >= 256 else (hw + 63) // 64 * 64
    return 4 * (4 * C + 2 * 16 * (tpb + 4) + n_shifts * (tpb + 4) + 4 * 16 * ((npad + 15) // 16) * 16 + (L + 1) + 4)


def npad_of(n_shifts):
    for p in (8, 16, 20, 24, 48):
        if n_shifts <= p:
            return p
    raise ValueError(n_shifts)
