"""CPU-side checks of the boundary: the C-ABI library loads and exports every symbol that
include/ccvpe_hip.h declares (no compute calls without a GPU), the ctypes table covers the
header, and the drop-in modules keep the reference's state_dict layout."""
import os
import re

import pytest
import torch

from ccvpe_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "ccvpe_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ccvpe_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    names = header_functions()
    assert len(names) >= 14
    for n in names:
        assert hasattr(lib, n), "libccvpe_hip.so does not export %s" % n
    assert sorted(_lib.PROTOTYPES) == names, "ctypes table and header disagree"
    assert lib.ccvpe_abi_version() == 7


def test_ctypes_prototypes_match_header_signatures():
    """Arity and pointer/int/float kind of every ctypes prototype vs the C declaration."""
    import ctypes
    src = open(os.path.join(ROOT, "include", "ccvpe_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decls = re.findall(r"\b(?:int|const char\*)\s+(ccvpe_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)
    assert len(decls) == len(_lib.PROTOTYPES)
    for name, params in decls:
        params = [q.strip() for q in params.split(",") if q.strip() and q.strip() != "void"]
        argtypes = _lib.PROTOTYPES[name][1]
        assert len(params) == len(argtypes), "%s: header has %d params, ctypes %d" % (name, len(params), len(argtypes))
        for q, a in zip(params, argtypes):
            is_ptr = "*" in q
            if is_ptr:
                assert a is ctypes.c_void_p or issubclass(a, ctypes._Pointer), (name, q, a)
            elif q.startswith("float"):
                assert a is ctypes.c_float, (name, q, a)
            elif q.startswith("double"):
                assert a is ctypes.c_double, (name, q, a)
            elif q.startswith("long"):
                assert a is ctypes.c_long, (name, q, a)
            else:
                assert a is ctypes.c_int, (name, q, a)


def test_conv_desc_matches_header_field_order():
    src = open(os.path.join(ROOT, "include", "ccvpe_hip.h")).read()
    body = src[src.index("typedef struct ccvpe_conv_desc"):src.index("} ccvpe_conv_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = decl.split(None, 1)[1] if not decl.startswith("const") else decl.split(None, 2)[2]
        for n in names.split(","):
            fields.append(n.strip().lstrip("*").strip())
    assert fields == [f[0] for f in _lib.ConvDesc._fields_]


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libccvpe_hip.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.load()


@pytest.mark.parametrize("kind", ["vigor", "kitti", "oxford"])
def test_state_dict_layout_and_roundtrip(kind, synth_sd):
    from ccvpe_amd import models
    net = {"kitti": lambda: models.CVM_KITTI("cpu"), "oxford": lambda: models.CVM_OxfordRobotCar("cpu"),
           "vigor": lambda: models.CVM_VIGOR("cpu", True)}[kind]()
    spec = synth.state_dict_spec(kind)
    sd = net.state_dict()
    assert list(sd.keys()) == [k for k, _, _ in spec]
    assert len(sd) == 818
    for k, shape, _ in spec:
        assert tuple(sd[k].shape) == tuple(shape), k
    # dead _fc weights must round-trip
    assert "grd_efficientnet._fc.weight" in sd and sd["sat_efficientnet._fc.weight"].shape == (1000, 1280)
    src = synth_sd(kind, 3 if kind == "vigor" else 4)
    net.load_state_dict(src, strict=True)
    back = net.state_dict()
    for k in src:
        assert torch.equal(back[k], src[k]), k
    # parameters vs buffers as in the reference (BN statistics are buffers)
    pnames = {n for n, _ in net.named_parameters()}
    assert "conv6.0.weight" in pnames and "grd_efficientnet._bn0.running_mean" not in pnames


def test_vigor_and_ori_prior_share_checkpoints(synth_sd):
    from ccvpe_amd import models
    a = models.CVM_VIGOR("cpu", True)
    b = models.CVM_VIGOR_ori_prior("cpu", 72, True)
    b.load_state_dict(a.state_dict(), strict=True)
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())


def test_cpu_inputs_are_rejected_not_emulated():
    from ccvpe_amd import models
    net = models.CVM_VIGOR_ori_prior("cpu", 0).eval()
    grd, sat = synth.synthetic_pair(1, "vigor", 1)
    with pytest.raises(RuntimeError, match="MI355X"):
        net(grd, sat)


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    """Every entry point validates before launching: bad shapes / alignment come back as CCVPE_EINVAL
    with a message (no exception crosses the ABI, nothing is enqueued), so this runs on CPU."""
    import ctypes
    lib = _lib.load()
    EINVAL = -1
    assert lib.ccvpe_conv_igemm_f32(None, None) == EINVAL
    assert b"null desc" in lib.ccvpe_last_error()
    d = _lib.ConvDesc()
    d.src0, d.w, d.dst = 256, 512, 1024            # fake 16-byte aligned "pointers": never dereferenced
    d.c0, d.ld0, d.batch, d.in_h, d.in_w = 12, 12, 1, 4, 4       # c0 not a multiple of 8
    d.kh = d.kw = d.stride = 1
    d.n, d.kpad, d.ldd = 16, 16, 16
    assert lib.ccvpe_conv_igemm_f32(ctypes.byref(d), None) == EINVAL
    assert b"multiples of 8" in lib.ccvpe_last_error()
    d.c0, d.ld0, d.src0 = 16, 16, 260                              # misaligned pointer
    assert lib.ccvpe_conv_igemm_f32(ctypes.byref(d), None) == EINVAL
    assert b"aligned" in lib.ccvpe_last_error()
    d.src0, d.kpad = 256, 8                                        # kpad too small / not a stage multiple
    assert lib.ccvpe_conv_igemm_bf16(ctypes.byref(d), 0, None) == EINVAL
    assert lib.ccvpe_upconv3x3_f32(None, None) == EINVAL
    assert lib.ccvpe_dwconv_f32(256, 256, 256, 256, 256, 256, 1, 8, 8, 6, 3, 1, 0, None) == EINVAL      # C % 4
    assert lib.ccvpe_dwconv_f32(256, 256, 256, 256, 256, 256, 1, 8, 8, 8, 4, 1, 0, None) == EINVAL      # k = 4
    sh = (ctypes.c_int * 2)(0, 1)
    assert lib.ccvpe_match_level_f32(256, 40, 256, 48, 48, sh, 2, 2, 0, 2, 0, 256, 256, 48, 1, 64, 40, None) == EINVAL
    assert b"bad L" in lib.ccvpe_last_error()                                                           # window wider than C
    assert lib.ccvpe_match_level_f32(256, 40, 256, 40, 40, sh, 99, 2, 0, 2, 0, 256, 256, 48, 1, 64, 40, None) == EINVAL
    assert lib.ccvpe_head_conv3x3_f32(256, 256, 256, 256, 1, 8, 8, 3, 0, None) == EINVAL               # cout = 3
    assert lib.ccvpe_softmax_rows_f32(256, 256, 0, 8, None) == EINVAL
    assert lib.ccvpe_mbconv_front_nblk(8, 8, 16, 96, 4, 1) == EINVAL
    assert lib.ccvpe_mbconv_front_nblk(16, 16, 192, 1152, 3, 1) == 1        # late block: csrc/mbconv_plane.hip, the plane is one band
    assert lib.ccvpe_mbconv_front_nblk(32, 32, 112, 672, 5, 1) == 2         # 32 x 32 plane: two bands of 16 rows
    assert lib.ccvpe_mbconv_front_nblk(16, 16, 96, 576, 3, 1) == 0          # valid but unfused shape (Cin not instantiated)
    assert lib.ccvpe_dwconv_nblk(32, 32, 672, 1) == 2 and lib.ccvpe_dwconv_nblk(7, 9, 480, 1) == 1
    assert lib.ccvpe_mbconv_front_nblk(64, 64, 40, 240, 5, 1) == 32         # squeeze-partial rows = 8 x 16 output tiles: 8 x 4
    assert lib.ccvpe_mbconv_front_nblk(256, 256, 16, 96, 3, 2) == 128       # block 1: 128 x 128 outputs in 8 x 16 tiles
    assert lib.ccvpe_mbconv_front_nblk(64, 64, 40, 240, 5, 2) == 0          # k5 s2 with Cin > 32: not instantiated -> unfused


def test_planning_entry_points_without_a_gpu():
    """The size / split planners are pure host code: callable on a box without a GPU."""
    import ctypes
    EINVAL = -1
    lib = _lib.load()
    d = _lib.ConvDesc()
    d.src0 = d.w = d.dst = 256
    d.c0, d.ld0, d.batch, d.in_h, d.in_w = 1344, 1344, 1, 16, 16
    d.kh = d.kw = 3
    d.stride, d.pad, d.n, d.kpad, d.ldd = 1, 1, 640, 9 * 1344, 640
    want = lib.ccvpe_conv_igemm_splitk_floats(ctypes.byref(d), 0)          # B = 1, level-6 3x3: 8 tiles, 756 K stages
    assert want > 0 and want % (256 * 640) == 0 and 2 <= want // (256 * 640) <= 32
    d.batch = 64                                                            # B = 64: 512 tiles -> one pass
    assert lib.ccvpe_conv_igemm_splitk_floats(ctypes.byref(d), 0) == 0
    # bf16 3x3 with >= 128 halo tiles stays UN-split (the LDS-DMA 3x3 kernel wins there); fp32 and smaller batches still split
    d.batch, d.kpad = 32, 9 * 1344
    assert lib.ccvpe_conv_igemm_splitk_floats(ctypes.byref(d), 1) == 0          # 32 x 2 x 1 x 4 = 256 tiles
    assert lib.ccvpe_conv_igemm_splitk_floats(ctypes.byref(d), 0) > 0           # fp32: 256 gather tiles < 320 -> split
    d.batch = 8
    assert lib.ccvpe_conv_igemm_splitk_floats(ctypes.byref(d), 1) > 0           # 64 tiles: split
    d.batch, d.c0 = 1, 1343
    assert lib.ccvpe_conv_igemm_splitk_floats(ctypes.byref(d), 0) == EINVAL
    assert lib.ccvpe_conv_igemm_splitk_f32(ctypes.byref(d), None, None) == EINVAL      # no scratch
    # matching backward: channel slices only when there are few pixel workgroups
    assert lib.ccvpe_match_bwd_nblk(64, 8, 2048) > lib.ccvpe_match_bwd_nblk(64, 8, 64) >= 1
    assert lib.ccvpe_match_bwd_nblk(65536, 64, 32) == 256
    # BatchNorm statistics: partial rows + one group row per 64 partials, bounded for huge tensors
    assert lib.ccvpe_bn_stats_nblk(256) == 8                               # small tensors: 32-row workgroups
    assert 4096 <= lib.ccvpe_bn_stats_nblk(64 * 512 * 512) <= 4096 + 64 + 1
    assert lib.ccvpe_dwconv_wgrad_nblk(64, 64, 3, 1) == 64 and lib.ccvpe_dwconv_wgrad_nblk(256, 256, 3, 2) == 64
    assert lib.ccvpe_dwconv_wgrad_nblk(16, 16, 5, 1) == 4 and lib.ccvpe_dwconv_wgrad_nblk(32, 32, 5, 2) == 4      # planes <= 1 024 px: dw_wgrad_rows_kernel
    assert lib.ccvpe_conv_wgrad_scratch_floats(2, 16, 16, 3, 3, 1, 1, 1344, 640) > 0
    assert lib.ccvpe_adam_chunk_elems() == 4096 and lib.ccvpe_train_targets_nblk(512, 512) == 256


def test_round5_queries_without_a_gpu():
    """Host-only: the fused-stem planner and the pointwise-ring route (csrc/stem_dw.hip, csrc/conv_pw2_impl.h: pw2_supported)."""
    import ctypes
    lib = _lib.load()
    assert lib.ccvpe_stem_dw_nblk(512, 512, 0) == 32 * 8                     # aerial: 256 x 256 outputs in 8 x 32 tiles
    assert lib.ccvpe_stem_dw_nblk(320, 640, 1) == 20 * 10                    # ground, circular padding
    assert lib.ccvpe_stem_dw_nblk(154, 231, 0) == 10 * 4                     # Oxford: 77 x 115 outputs, ragged tiles
    assert lib.ccvpe_stem_dw_nblk(154, 231, 1) == 0                          # circular padding needs an even width: two launches
    assert lib.ccvpe_stem_dw_nblk(2, 2, 0) == 0
    d = _lib.ConvDesc()
    d.src0 = d.w = d.dst = d.scale = d.shift = 256
    d.c0, d.ld0, d.batch, d.in_h, d.in_w = 112, 112, 2, 32, 32
    d.kh = d.kw = 1
    d.stride, d.pad, d.n, d.kpad, d.ldd, d.act = 1, 0, 672, 112, 672, 2     # expand conv of blocks 9-11: BN + swish
    fam = lambda r: r & 0xff
    for bf16 in (0, 1):
        d.kpad = 128 if bf16 else 112                                        # packed K: whole 64-byte pieces of the element type
        assert fam(lib.ccvpe_conv_igemm_route(ctypes.byref(d), bf16, 0)) == 4, "pw_ring expected"
    d.kpad = 112
    prev = lib.ccvpe_set_pw_ring_kernels(0)
    try:
        assert fam(lib.ccvpe_conv_igemm_route(ctypes.byref(d), 0, 0)) == 1  # the switch brings pw_gemm_kernel back
    finally:
        lib.ccvpe_set_pw_ring_kernels(prev)
    d.batch, d.in_h, d.in_w = 3, 19, 23                                      # M = 1311: not a multiple of the 128-row tile
    assert fam(lib.ccvpe_conv_igemm_route(ctypes.byref(d), 0, 0)) == 1
    d.batch, d.in_h, d.in_w, d.gate = 64, 20, 40, 256                        # ground encoder: a gated tile would span two samples
    d.c0, d.ld0, d.kpad, d.n, d.ldd, d.act = 672, 672, 672, 112, 112, 0
    assert fam(lib.ccvpe_conv_igemm_route(ctypes.byref(d), 0, 0)) == 1
    d.in_h, d.in_w = 32, 32                                                  # aerial: 1 024 pixels per sample = 8 tiles
    assert fam(lib.ccvpe_conv_igemm_route(ctypes.byref(d), 0, 0)) == 4
    assert fam(lib.ccvpe_conv_igemm_route(ctypes.byref(d), 1, 0)) == 4
    assert fam(lib.ccvpe_conv_igemm_route(ctypes.byref(d), 1, 1)) == 1      # bf16 storage writing fp32: pw_gemm_kernel


def test_pw_ring_is_never_routed_with_fewer_than_three_k_stages():
    """csrc/conv_pw2_impl.h: the ring's DMA requests run three K stages ahead of the matrix instructions and the per-tile vectors
    (two LDS copies by tile parity) of tile t + 2 must not be requested before every wave is past tile t's epilogue — a hazard that
    is excluded by ROUTING (pw2_supported), so the route is what this pins: a bf16 layer with K = 64 is exactly two 32-channel stages
    and must stay on pw_gemm_kernel, K = 96 (three stages) may take the ring; fp32 needs K >= 64 = four 16-channel stages anyway."""
    import ctypes
    lib = _lib.load()
    fam = lambda r: r & 0xff
    d = _lib.ConvDesc()
    d.src0 = d.w = d.dst = d.scale = d.shift = 256
    d.batch, d.in_h, d.in_w = 4, 32, 32
    d.kh = d.kw = 1
    d.stride, d.pad, d.n, d.ldd, d.act = 1, 0, 384, 384, 2                    # an expand-shaped layer: BN + swish, N = 384
    for c0, want in ((64, 1), (96, 4), (128, 4)):                             # 2, 3, 4 bf16 K stages
        d.c0, d.ld0, d.kpad = c0, c0, c0
        r = lib.ccvpe_conv_igemm_route(ctypes.byref(d), 1, 0)
        assert fam(r) == want, "bf16 K = %d: route %d, expected %d" % (c0, fam(r), want)
    d.c0, d.ld0, d.kpad = 64, 64, 64
    assert fam(lib.ccvpe_conv_igemm_route(ctypes.byref(d), 0, 0)) == 4        # fp32 K = 64: four stages
    d.c0, d.ld0, d.kpad = 48, 48, 48
    assert fam(lib.ccvpe_conv_igemm_route(ctypes.byref(d), 0, 0)) == 1        # fp32 K = 48 (three stages): below the ring's minimum K


def test_fullsize_train_kernel_table_matches_the_geometry_queries():
    """Host-only: every row of tests/train_kernel_shapes.py (the shapes tests/test_fullsize_train_kernels_gpu.py checks against
    float64) still takes the branch it is there for — a routing change fails here, without a GPU, instead of silently moving a
    row onto an easier path."""
    import train_kernel_shapes as S
    lib = _lib.load()
    for name, rows, c, rpb, nblk in S.BN_STATS:
        assert lib.ccvpe_bn_stats_nblk(rows) == nblk, name
        parts = (rows + rpb - 1) // rpb                                     # partial rows, then one fold row per 64
        assert parts + (parts + 63) // 64 == nblk, "%s: rows per workgroup is no longer %d" % (name, rpb)
    for name, b, rps, c, act, dcs, nblk in S.BN_ACT:
        assert lib.ccvpe_bn_act_nblk(rps) == nblk and lib.ccvpe_bn_bwd_nblk(rps) == nblk, name
    for name, b, h, w, c, cs, nblk in S.BN_SE:
        assert lib.ccvpe_bn_act_nblk(h * w) == nblk and lib.ccvpe_bn_bwd_nblk(h * w) == nblk, name
    for name, b, h, w, c, k, s, circ, nblk in S.DW_WGRAD:
        assert h * w > 1024, "%s: not the all-taps kernel" % name
        assert lib.ccvpe_dwconv_wgrad_nblk(h, w, k, s) == nblk, name
    for name, b, h, w, cout, ntiles in S.HEAD_BWD:
        assert ((w + 63) // 64) * ((h + 3) // 4) * b == ntiles > S.HEAD_WGRAD_BLOCKS, name
    for name, b, h, w, circ, nblk, partial in S.STEM_WGRAD:
        assert lib.ccvpe_stem_wgrad_nblk(b, h, w) == nblk, name
        assert ((w // 2) % 256 != 0) == partial, name
    for name, b, c, L, side, shifts, n_max, n_tail, stride, nblk, npad in S.MATCH_BWD:
        assert lib.ccvpe_match_bwd_nblk(side * side, b, c) == nblk, name
        assert S.npad_of(len(shifts)) == npad, name
    lds = {name: S.match_bwd_lds_bytes(c, L, side * side, len(shifts), npad)
           for name, b, c, L, side, shifts, n_max, n_tail, stride, nblk, npad in S.MATCH_BWD}
    assert sum(v > 64 * 1024 for v in lds.values()) >= 2 and max(lds.values()) <= 160 * 1024, lds
    assert any(row[-1] == 48 for row in S.MATCH_BWD) and any(row[-2] == 32 for row in S.MATCH_BWD)   # NPAD 48, 32 slices
    for name, rows, c, ld in S.COLSUM:
        assert rows >= S.CS_ROWS * 256, "%s: not the many-rows branch" % name


def _conv3x3_desc(row, bf16):
    """descriptor of a tests/forward_kernel_shapes.py ConvRow (fake aligned pointers: the queries never dereference them)"""
    sk = 32 if bf16 else 16
    d = _lib.ConvDesc()
    d.src0 = d.src1 = d.w = d.dst = d.shift = 256
    d.c0, d.ld0, d.c1, d.ld1 = row.c0, row.ld0, row.c1, row.c1
    d.batch, d.in_h, d.in_w = row.b, row.h, row.w
    d.kh = d.kw = 3
    d.stride, d.pad, d.act = 1, 1, 1
    d.n, d.ldd = row.n, row.n
    d.kpad = (9 * (row.c0 + row.c1) + sk - 1) // sk * sk
    return d


def test_forward_kernel_table_matches_the_conv3x3_queries():
    """Host-only: every conv3x3 row of tests/forward_kernel_shapes.py routes to conv3x3_kernel with the tile and the form
    (waves, W by LDS-DMA, taps per stage) it is there for, un-split; NW flips between the two members of every threshold pair; and
    the rows reach every instantiation the traced B = 64 steps launch (the literal lists in the table file)."""
    import ctypes
    import forward_kernel_shapes as S
    lib = _lib.load()
    seen = {0: set(), 1: set()}
    for row in S.conv_rows():
        for bf16, want in ((0, row.f32), (1, row.bf16)):
            if want is None:
                continue
            d = _conv3x3_desc(row, bf16)
            r = lib.ccvpe_conv_igemm_route(ctypes.byref(d), bf16, 0)
            assert r & 0xff == 2, "%s (%s): route family %d, not conv3x3_kernel" % (row.name, "bf16" if bf16 else "fp32", r & 0xff)
            assert ((r >> 8) & 0xf, (r >> 12) & 0xf, (r >> 16) & 0xf) == row.tile, row.name
            v = lib.ccvpe_conv3x3_variant(ctypes.byref(d), bf16)
            assert (v & 0xf, bool((v >> 4) & 1), v >> 8) == want, "%s (%s): variant %#x" % (row.name, "bf16" if bf16 else "fp32", v)
            assert lib.ccvpe_conv_igemm_splitk_floats(ctypes.byref(d), bf16) == 0, "%s: would run split-K (generic kernel)" % row.name
            if bf16:
                assert lib.ccvpe_conv_igemm_route(ctypes.byref(d), 1, 1) == r, "%s: out_f32 changes the route" % row.name
            seen[bf16].add(row.tile + want)
    for hi, lo in S.CONV3X3_NW8_PAIRS:
        assert (hi.b - lo.b, hi.h, hi.w, hi.n, hi.tile) == (1, lo.h, lo.w, lo.n, lo.tile), hi.name
        for a, b in ((hi.f32, lo.f32), (hi.bf16, lo.bf16)):
            assert (a is None) == (b is None) and (a is None or (a[0], b[0]) == (8, 4)), "%s: NW does not flip 8 -> 4" % hi.name
    assert set(S.CONV3X3_TRACED_F32) <= seen[0], sorted(set(S.CONV3X3_TRACED_F32) - seen[0])
    assert set(S.CONV3X3_TRACED_BF16) <= seen[1], sorted(set(S.CONV3X3_TRACED_BF16) - seen[1])
    # not a conv3x3_kernel route -> 0: a 1x1 layer, and a single-source bf16 layer the narrow kernel takes when the plane is large
    d = _conv3x3_desc(S.CONV3X3[0], 0)
    d.kh = d.kw = 1
    d.pad, d.kpad = 0, 48
    assert lib.ccvpe_conv3x3_variant(ctypes.byref(d), 0) == 0
    assert lib.ccvpe_conv3x3_variant(None, 0) == -1


def test_conv3x3_w_tile_is_always_staged_by_lds_dma():
    """pick_cfg (csrc/conv_common.h) charges a tile by the columns it computes, and the 16-wide tile computes exactly Npad: the
    cheapest tile always divides Npad, so launch3x3_nw's `Npad % BN != 0` branch — conv3x3_kernel<.., DMA = false, 1>, W through
    registers — is unreachable through ccvpe_conv_igemm_* (DESIGN.md section 4).  Every N the ABI accepts up to twice the model's
    widest layer, both types, a small and a B = 64 launch."""
    import ctypes
    import forward_kernel_shapes as S
    lib = _lib.load()
    for bf16 in (0, 1):
        for b, h, w in ((2, 11, 20), (64, 64, 64)):
            d = _conv3x3_desc(S.CONV3X3[0]._replace(b=b, h=h, w=w), bf16)
            for n in range(8, 1297):
                d.n, d.ldd = n, (n + 7) // 8 * 8
                v = lib.ccvpe_conv3x3_variant(ctypes.byref(d), bf16)
                assert v > 0 and (v >> 4) & 1 == 1, "N = %d (%s): variant %#x" % (n, "bf16" if bf16 else "fp32", v)


def test_forward_kernel_table_matches_the_band_plan_query():
    """Host-only: every band row of tests/forward_kernel_shapes.py is taken by mbconv_band_kernel with the instantiation it is
    there for and — num_cus() falls back to 256 without a GPU, the MI355X's count — the slices per workgroup, the groups and the
    short last group the row's comment promises; the rows reach every traced instantiation; the slice-per-workgroup switch turns
    the plan off; and a shape the launcher refuses for its LDS need is no longer reported as "band"."""
    import torch
    import forward_kernel_shapes as S
    lib = _lib.load()
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the table stores the grouping for 256 CUs")     # (never on the MI355X or on a box without a GPU)
    seen = set()
    for row in S.BAND:
        mid = 6 * row.cin
        assert lib.ccvpe_mbconv_front_route(row.h, row.w, row.cin, mid, row.k, row.s, 1, row.b) == 3, row.name
        assert lib.ccvpe_mbconv_front_route(row.h, row.w, row.cin, mid, row.k, row.s, 0, row.b) == 2, row.name     # fp32: plane kernel
        p = lib.ccvpe_mbconv_band_plan(row.h, row.w, row.cin, mid, row.k, row.s, row.b)
        assert p > 0, row.name
        nkk, tpw, ry, cpg, ngrp = p & 0xf, (p >> 4) & 0xf, (p >> 8) & 0xf, (p >> 12) & 0xff, (p >> 20) & 0xff
        assert (row.k, row.s, nkk, tpw, ry) == row.inst, "%s: instantiation <%d,%d,%d,%d,%d>" % (row.name, row.k, row.s, nkk, tpw, ry)
        assert (cpg, ngrp) == (row.cpg256, row.ngrp256), "%s: cpg %d ngrp %d" % (row.name, cpg, ngrp)
        assert mid // 16 - (ngrp - 1) * cpg == row.last and 0 < row.last <= cpg, row.name
        assert row.deep == (cpg >= 3), row.name
        assert max(row.b * row.h * row.w * row.cin, row.b * row.h * row.w * mid // row.s ** 2) * 2 < 64 << 20, "%s: a tensor above 64 MB" % row.name
        seen.add(row.inst)
    assert set(S.BAND_TRACED) <= seen, sorted(set(S.BAND_TRACED) - seen)
    assert any(r.deep and r.last < r.cpg256 for r in S.BAND) and any(r.cpg256 >= 18 for r in S.BAND)
    row = S.BAND[3]
    prev = lib.ccvpe_set_mbconv_plane_kernels(3)
    try:
        assert lib.ccvpe_mbconv_front_route(row.h, row.w, row.cin, 6 * row.cin, row.k, row.s, 1, row.b) == 2
        assert lib.ccvpe_mbconv_band_plan(row.h, row.w, row.cin, 6 * row.cin, row.k, row.s, row.b) == 0
    finally:
        lib.ccvpe_set_mbconv_plane_kernels(prev)
    h, w, cin, k, s = S.BAND_LDS_REFUSED
    assert lib.ccvpe_mbconv_front_nblk(h, w, cin, 6 * cin, k, s) == 1                # the plane geometry takes it: one band of 9 rows
    ih, tiles = (h - 1) * s + k, (min((h - 1) * s + k, h) * w + 15) // 16            # 13 plane rows; 32 tiles = 8 per wave <= 10, 4 K pieces
    assert (tiles + 3) // 4 <= 10 and (cin + 31) // 32 == 4
    assert 2 * ih * (w + k - 1) * 20 * 4 > 120 * 1024                                 # the two planes alone, before the pitch padding
    assert lib.ccvpe_mbconv_front_route(h, w, cin, 6 * cin, k, s, 1, 3) == 2, "route says band for a shape the launcher refuses"
    assert lib.ccvpe_mbconv_band_plan(h, w, cin, 6 * cin, k, s, 3) == 0
    assert lib.ccvpe_mbconv_band_plan(16, 16, 192, 1152, 5, 1, 0) == 0               # no batch


def test_wgrad_kernel_table_matches_the_planner_queries():
    """Host-only: every row of tests/wgrad_kernel_shapes.py (the shapes tests/test_wgrad_forms_gpu.py checks against float64) still
    gets the tile and the split count it is there for, the restated planner agrees with the row, and the rows reach every
    conv_wgrad_kernel instantiation of the traced training step."""
    import wgrad_kernel_shapes as S
    lib = _lib.load()
    rows = S.rows()
    assert [r.num for r in rows] == list(range(1, 24))
    for r in rows:
        ho, wo, m, ctot, taps, ncols = S.dims(r)
        assert S.plan(r) == r.plan, (r.name, S.plan(r))
        tile = lib.ccvpe_conv_wgrad_tile(r.n, ncols)
        assert (tile >> 16, tile & 0xffff) == (r.plan.tile, S.tile_cols(r.plan.tile)), (r.name, tile >> 16, tile & 0xffff)
        floats = lib.ccvpe_conv_wgrad_scratch_floats(r.b, r.h, r.w, r.k, r.k, r.stride, r.pad, ctot, r.n)
        assert floats == r.plan.s * (r.n * ncols + r.n), (r.name, floats // (r.n * ncols + r.n))
        assert r.ldy % 4 == 0 and r.ldy >= r.n and r.ld0 >= r.c0 and r.c0 % 4 == 0 and r.c1 % 4 == 0, r.name
        assert 4 * max(r.b * r.h * r.w * (r.ld0 + r.c1), m * r.ldy, floats) < 32 << 20, "%s: a tensor above 32 MB" % r.name
        if r.kind == "gated":
            assert r.k == 1 and r.c1 == 0 and r.plan.tile != 128, r.name
    reached = {S.form(r) for r in rows}
    assert len(S.TRACED) == 11 and set(S.TRACED) <= reached, sorted(set(S.TRACED) - reached)
    # the launcher edges the table is there for
    plans = [r.plan for r in rows]
    assert all(p.pps % S.WG_BP == 0 for p in plans) and any(p.last_px % S.WG_BP for p in plans)       # a split that ends mid-stage
    assert any(p.empty for p in plans) and any(p.s == 1024 for p in plans)
    assert any(p.s == 4096 // (p.tiles_n * p.tiles_c) and p.empty for p in plans)                      # S limited by the tile count
    assert {p.ln_dw for p in plans} == {1, 4, 16, 64} and {p.ln_bias for p in plans} == {1, 4, 16, 64}
    assert {p.grid_mod8 for p in plans} >= {0, 2, 6, 7}
    assert any(r.ldy > r.n for r in rows) and any(r.ld0 > r.c0 for r in rows) and any(r.n % 4 for r in rows)
    assert any(r.stride == 2 for r in rows) and any(r.kind == "deconv" for r in rows)
    assert any(S.dims(r)[1] < S.WG_BP // 4 for r in rows)                                             # Wo < 8: several carries per stage
    for p in plans:
        # the model's merge term: at most S roundings (a chain's first addition is to zero and exact)
        assert S.merge_chain(p.s, p.ln_dw) - 1 <= p.s and S.merge_chain(p.s, p.ln_bias) - 1 <= p.s, p
