"""Depthwise shapes that pin every launched form of dwconv_kernel (the strip kernel), dwconv_plane_kernel and dw_dgrad_kernel, and
the geometry edges of their launcher, each at the smallest size that still has its property.

Shared by tests/test_depthwise_forms_gpu.py (values against float64, elementwise: tests/depthwise_check.py) and by
tests/test_depthwise_check.py (the restated geometry against the expected columns and against the host-only query
ccvpe_dwconv_nblk, so that a routing or geometry change shows up as a stale row in a plain `-m "not gpu"` run; the same comparison on
faulted CPU results).

Where the forms come from: dwconv_any in csrc/effnet_ops.hip (dw_use_plane, dw_geometry) and what the committed trace of the real
training step lists (profiles/r06/r06_train_kernel_stats.csv) — the literal lists below.
"""
from collections import namedtuple

DW_TW = 4          # output columns of a strip (csrc/effnet_ops.hip)

# ------------------------------------------------------------------------------------------------------------------------------
# The launcher's geometry, restated.
#   strip kernel: a thread owns 4 channels x one strip of 4 output columns; a workgroup of 256 threads is cgx channel groups x P
#   strips (P = 256 // cgx: 256 - P cgx threads idle); C / 4 channel groups are cut into `ychunks` equal parts of at most 256;
#   the Ho x ceil(Wo / 4) strips of a sample form ceil(strips / P) groups and a workgroup walks RB of them (RB = groups // 32
#   clamped to 1 .. 8), so a sample has nblk = ceil(groups / RB) workgroups per chunk = squeeze-partial rows.
#   plane kernels: one squeeze-partial row from dwconv_plane_kernel; the fused entry points prefer mbconv_plane_kernel's
#   depthwise-only form where its geometry takes the shape and then write one row per row band (DwRow.bands).
# ------------------------------------------------------------------------------------------------------------------------------
Geo = namedtuple("Geo", "ho wo ychunks cgx p strips groups rb nblk")


def use_plane(h, w, c):
    return h * w <= 1024 and c % 16 == 0


def out_dims(h, w, k, stride):
    total_pad = (k - 1) if stride == 1 else (k - 2)
    return (h + total_pad - k) // stride + 1, (w + total_pad - k) // stride + 1


def geometry(h, w, c, k, stride):
    """dw_geometry of csrc/effnet_ops.hip: what the strip kernel is launched with (plane shapes: only ho, wo and one partial row)"""
    ho, wo = out_dims(h, w, k, stride)
    if use_plane(h, w, c):
        return Geo(ho, wo, None, None, None, None, None, None, 1)
    cg = c // 4
    yc = 1
    while cg // yc > 256 or cg % yc:
        yc += 1
    cgx = cg // yc
    p = 256 // cgx
    strips = ho * ((wo + DW_TW - 1) // DW_TW)
    groups = (strips + p - 1) // p
    rb = min(max(groups // 32, 1), 8)
    return Geo(ho, wo, yc, cgx, p, strips, groups, rb, (groups + rb - 1) // rb)


def strip_chain(geo):
    """longest chain of fp32 additions a term of a strip-kernel squeeze partial passes through: 4 outputs per strip and RB strips
    into the thread's sum, then the P - 1 additions of the workgroup's fixed-order reduction"""
    return 4 * geo.rb + geo.p


def plane_chain(ho, wo, bf16):
    """dwconv_plane_kernel: a thread adds 4 outputs per item over ceil(items / LN) items (LN = 256 / CG lanes per channel group,
    CG = 2 four-channel groups per 32-byte chunk in fp32, 4 in bf16), 16 partial sums of LN / 16 lanes each, then those 16"""
    ln = 256 // (4 if bf16 else 2)
    items = ho * ((wo + 3) // 4)
    return 4 * ((items + ln - 1) // ln) + ln // 16 + 16


def band_chain(h, w, c, ho, wo, stride, bands):
    """mbconv_plane_kernel, depthwise-only form: NOUT outputs per item into the thread's sum, a butterfly over the 64 / CG lanes of a
    wave that share a channel group, then the four waves (CH = 32 channels per workgroup on planes of <= 256 pixels, else 16)"""
    cgs = (32 if h * w <= 256 and c % 32 == 0 else 16) // 4
    nout = 4 if stride == 1 else 2
    bh = (ho + bands - 1) // bands
    items = bh * (wo // nout)
    lanes = 256 // cgs
    return nout * ((items + lanes - 1) // lanes) + (64 // cgs).bit_length() - 1 + 3


# ------------------------------------------------------------------------------------------------------------------------------
# What the traced training step launches (profiles/r06/r06_train_kernel_stats.csv), as (kernel, k, stride).  The strip and plane
# kernels appear in their RAW form only (train mode: batch-statistic BN follows in its own kernel; the stride-1 input gradients
# are the same entry with reversed taps); the fused forms are what inference launches.
# ------------------------------------------------------------------------------------------------------------------------------
TRACED = [("dwconv_kernel", 3, 1), ("dwconv_kernel", 3, 2), ("dwconv_kernel", 5, 1), ("dwconv_kernel", 5, 2),
          ("dwconv_plane_kernel", 3, 1), ("dwconv_plane_kernel", 5, 1), ("dwconv_plane_kernel", 5, 2),
          ("dw_dgrad_kernel", 3, 2), ("dw_dgrad_kernel", 5, 2)]

# name, b, h, w, c, k, s, circ: the launch;  family: "strip" or "plane" (dw_use_plane);  geo: the expected geometry;  bands: the
# squeeze-partial rows of the fused entry points with the MBConv plane kernels at their default (plane rows; 1 = the shape is one
# mbp_geometry_compute refuses, or one band)
DwRow = namedtuple("DwRow", "name b h w c k s circ family geo bands")


def _s(name, b, h, w, c, k, s, circ, geo):
    return DwRow(name, b, h, w, c, k, s, circ, "strip", Geo(*geo), None)


def _p(name, b, h, w, c, k, s, circ, ho, wo, bands):
    return DwRow(name, b, h, w, c, k, s, circ, "plane", Geo(ho, wo, None, None, None, None, None, None, 1), bands)


STRIP = [
    #                                                                        ho  wo yc cgx   p strips groups rb nblk
    _s("k3 s1 C32 50x170: P = 32, RB = 2, Wo % 4 = 2", 2, 50, 170, 32, 3, 1, False, (50, 170, 1, 8, 32, 2150, 68, 2, 34)),
    _s("k3 s2 C96 34x38 circular: P = 10 (16 idle threads), Wo = 19", 2, 34, 38, 96, 3, 2, True, (17, 19, 1, 24, 10, 85, 9, 1, 9)),
    _s("k3 s2 C96 67x90: odd H, Wo = 45, 40 groups", 2, 67, 90, 96, 3, 2, False, (33, 45, 1, 24, 10, 396, 40, 1, 40)),
    _s("k3 s1 C144 33x36 circular: P = 7", 2, 33, 36, 144, 3, 1, True, (33, 36, 1, 36, 7, 297, 43, 1, 43)),
    _s("k5 s2 C144 36x41 circular: odd W, wrap meets the (1,2) pad", 2, 36, 41, 144, 5, 2, True, (18, 20, 1, 36, 7, 90, 13, 1, 13)),
    _s("k5 s2 C144 36x41 zero padding", 2, 36, 41, 144, 5, 2, False, (18, 20, 1, 36, 7, 90, 13, 1, 13)),
    _s("k5 s1 C240 64x64: P = 4, RB = 8 (block 4)", 2, 64, 64, 240, 5, 1, False, (64, 64, 1, 60, 4, 1024, 256, 8, 32)),
    _s("k3 s2 C240 35x37 circular: odd H and W", 2, 35, 37, 240, 3, 2, True, (17, 18, 1, 60, 4, 85, 22, 1, 22)),
    _s("k5 s2 C672 33x34: P = 1, RB = 2", 2, 33, 34, 672, 5, 2, False, (16, 17, 1, 168, 1, 80, 80, 2, 40)),
    _s("k3 s1 C1152 33x32: ychunks = 2, RB = 8", 2, 33, 32, 1152, 3, 1, False, (33, 32, 2, 144, 1, 264, 264, 8, 33)),
    _s("k5 s1 C40 6x7 circular: one partly filled workgroup per sample, 2 in all", 2, 6, 7, 40, 5, 1, True, (6, 7, 1, 10, 25, 12, 1, 1, 1)),
    _s("k5 s1 C96 33x33 circular, B = 3: 90 workgroups (90 % 8 = 2), last group of 7", 3, 33, 33, 96, 5, 1, True, (33, 33, 1, 24, 10, 297, 30, 1, 30)),
    # the narrowest circular planes the launcher accepts: W = k // 2 + 1
    _s("k3 s1 C20 7x2 circular: minimum width", 2, 7, 2, 20, 3, 1, True, (7, 2, 1, 5, 51, 7, 1, 1, 1)),
    _s("k5 s1 C40 5x3 circular: minimum width", 2, 5, 3, 40, 5, 1, True, (5, 3, 1, 10, 25, 5, 1, 1, 1)),
    _s("k5 s2 C24 9x3 circular: minimum width, one output column", 2, 9, 3, 24, 5, 2, True, (4, 1, 1, 6, 42, 4, 1, 1, 1)),
]

PLANE = [
    _p("k3 s1 C480 32x32", 2, 32, 32, 480, 3, 1, False, 32, 32, 2),
    _p("k5 s1 C672 32x32", 2, 32, 32, 672, 5, 1, False, 32, 32, 2),
    _p("k5 s2 C672 32x32", 2, 32, 32, 672, 5, 2, False, 16, 16, 2),
    _p("k5 s1 C1152 16x16", 2, 16, 16, 1152, 5, 1, False, 16, 16, 1),
    _p("k3 s1 C1152 16x16", 2, 16, 16, 1152, 3, 1, False, 16, 16, 1),
    _p("k5 s2 C672 20x40 circular", 2, 20, 40, 672, 5, 2, True, 10, 20, 2),
    _p("k3 s1 C1152 10x20 circular", 2, 10, 20, 1152, 3, 1, True, 10, 20, 1),
    # shapes mbp_geometry_compute refuses: the fused call lands on dwconv_plane_kernel
    _p("k5 s1 C1152 5x9 circular: Wo % 4 != 0", 3, 5, 9, 1152, 5, 1, True, 5, 9, 1),
    _p("k3 s2 C96 12x64: W + 4 > 64", 2, 12, 64, 96, 3, 2, False, 6, 32, 1),
    _p("k3 s1 C1152 4x6 circular: H < 5", 3, 4, 6, 1152, 3, 1, True, 4, 6, 1),
    _p("k5 s2 C672 16x16: stride 2 with the 32-channel chunk", 2, 16, 16, 672, 5, 2, False, 8, 8, 1),
]

# plane rows that mbp_geometry_compute refuses: one partial row at the default switch too, and the GPU test requires the two switch
# positions to give the same bits (both are dwconv_plane_kernel)
PLANE_REFUSED = [r.name for r in PLANE[7:]]


def rows():
    return STRIP + PLANE


def forms(row):
    """the (kernel, k, stride) forms a row launches in the GPU test: the forward kernel of its family and the input gradient
    (stride 1: the forward entry with reversed taps; stride 2: dw_dgrad_kernel)"""
    fwd = "dwconv_kernel" if row.family == "strip" else "dwconv_plane_kernel"
    out = [(fwd, row.k, row.s)]
    if row.s == 2:
        out.append(("dw_dgrad_kernel", row.k, 2))
    return out
