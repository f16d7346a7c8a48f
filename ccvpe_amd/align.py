"""KITTI aerial alignment (datasets.py:443-464 training, :577-596 test of the reference) restated without Pillow, and its
device launch.

The reference aligns every aerial map on the host with four Pillow passes over the whole map and keeps the centre crop:

    sat.rotate(-heading)                                      NEAREST   pass 1
    sat.transform(size, AFFINE, (1, 0, tx1, 0, 1, ty1))       BILINEAR  pass 2   (GPS antenna -> camera)
    sat.transform(size, AFFINE, (1, 0, tx2, 0, 1, ty2))       BILINEAR  pass 3   (the sample's shift)
    sat.rotate(ori)                                           NEAREST   pass 4
    center_crop(512)

This module is the written specification of `ccvpe_kitti_align_u8` (csrc/align.hip), which evaluates the chain LAZILY for
the crop window only.  Nothing here imports PIL; tests/test_kitti_align.py runs Pillow itself as the reference and asks
for equal bytes.  `ccvpe_kitti_align_norm_u8_f32` is the same chain over a table of device addresses (maps resident in the device
image cache) that writes the normalised fp32 NCHW batch side itself; `align_norm_spec` is its specification, `kitti_align_norm`
its launch (tests/test_kitti_map_cache*.py).

Pillow's arithmetic (Pillow 12.2: PIL/Image.py `rotate`, src/libImaging/Geometry.c `affine_fixed`, `affine_transform`,
`bilinear_filter32RGB`):

  * `rotate` builds the inverse matrix from cos / sin rounded to 15 decimals about the centre (w / 2, h / 2)
    (`rotate_matrix`); 0 / 180 degrees, and 90 / 270 on a square image, are transposes (`rotate_fixed` restates them as
    exact integer matrices).
  * NEAREST walks the matrix in 16.16 fixed point: FIX(v) = floor(v * 65536 + 0.5), the half-pixel centre folded into the
    constant terms; source index = accumulated value >> 16 (arithmetic); outside the source -> 0.
  * BILINEAR with a pure translation is float64 per pixel: xin = (x + 0.5) + tx, outside [0, w) -> 0, then xin -= 0.5,
    x0 = floor(xin), dx = xin - x0, taps clipped to the image, v = a + (b - a) * d three times, and the byte is v
    TRUNCATED.  Product and sum are rounded separately (no fused multiply-add).

A parameter row (`kitti_align_params`) is ROW_LEN int64 values:

    [0:6]    a0 a1 a2 a3 a4 a5 of pass 1        [6:12]  the same of pass 4
    [12:16]  tx1 ty1 tx2 ty2, the float64 BIT PATTERNS
    [16:20]  w h left top (torchvision's center_crop rule)
"""
import math

import numpy as np

from .preprocess import IMAGENET_MEAN, IMAGENET_STD

ROW_LEN = 20
_IDENT = (65536, 0, 32768, 0, 65536, 32768)


def rotate_matrix(angle_deg, w, h):
    """The inverse affine matrix (m0 .. m5) `Image.rotate(angle_deg)` hands to its transform for a w x h image."""
    angle = angle_deg % 360.0
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = w / 2, h / 2
    x, y = -cx, -cy
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def fix(v):
    """Pillow's FIX(): 16.16 fixed point, round half up."""
    return int(math.floor(v * 65536.0 + 0.5))


def fix_matrix(m):
    """The six integers of `affine_fixed` for matrix m (the pixel centre folded into a2 / a5)."""
    return (fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5),
            fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5))


def rotate_fixed(angle_deg, w, h):
    """Six fixed-point integers that reproduce `Image.rotate(angle_deg)` (NEAREST, no expand) on a w x h image, including
    its transpose shortcuts: copy for 0, ROTATE_180 for 180, ROTATE_90 / ROTATE_270 for 90 / 270 when w == h."""
    angle = angle_deg % 360.0
    if angle == 0:
        return _IDENT
    if angle == 180:                                            # out[y][x] = in[h - 1 - y][w - 1 - x]
        return (-65536, 0, (w << 16) - 32768, 0, -65536, (h << 16) - 32768)
    if angle == 90 and w == h:                                  # out[y][x] = in[x][w - 1 - y]
        return (0, -65536, (w << 16) - 32768, 65536, 0, 32768)
    if angle == 270 and w == h:                                 # out[y][x] = in[h - 1 - x][y]
        return (0, 65536, 32768, -65536, 0, (h << 16) - 32768)
    return fix_matrix(rotate_matrix(angle_deg, w, h))


def center_crop_origin(w, h, crop_w, crop_h):
    """(left, top) of torchvision's center_crop."""
    return int(round((w - crop_w) / 2.0)), int(round((h - crop_h) / 2.0))


def kitti_align_params(heading, cam_shift_px, shift_px, ori, w, h, crop):
    """One parameter row (int64 [ROW_LEN]) for a w x h map: heading in radians (the OXTS record), cam_shift_px = (tx1, ty1)
    and shift_px = (tx2, ty2) the two translations as handed to Pillow, ori in degrees, crop = side or (crop_h, crop_w)."""
    crop_h, crop_w = (crop, crop) if np.isscalar(crop) else crop
    row = np.zeros((ROW_LEN,), dtype=np.int64)
    row[0:6] = rotate_fixed(-heading / np.pi * 180, w, h)
    row[6:12] = rotate_fixed(ori, w, h)
    row[12:16] = np.asarray([cam_shift_px[0], cam_shift_px[1], shift_px[0], shift_px[1]], dtype=np.float64).view(np.int64)
    row[16:20] = (w, h) + center_crop_origin(w, h, crop_w, crop_h)
    return row


# ---- the passes, evaluated at arbitrary integer coordinates ---------------------------------------------------------------
def fixed_walk(a, x, y):
    """Source (column, row) of the fixed-point walk a = (a0 .. a5) at output pixels x, y (int64)."""
    x, y = np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)
    xs = (int(a[2]) + int(a[0]) * x + int(a[1]) * y) >> 16
    ys = (int(a[5]) + int(a[3]) * x + int(a[4]) * y) >> 16
    return xs, ys


def nearest_at(fetch, w, h, a, x, y):
    """NEAREST pass at pixels (x, y): fetch(xs, ys) -> [..., 3] uint8 gives the previous image at in-range coordinates."""
    xs, ys = fixed_walk(a, x, y)
    inside = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
    v = fetch(np.clip(xs, 0, w - 1), np.clip(ys, 0, h - 1))
    return np.where(inside[..., None], v, np.uint8(0))


def bilinear_at(fetch, w, h, tx, ty, x, y):
    """BILINEAR translation pass (1, 0, tx, 0, 1, ty) at pixels (x, y), float64, the byte truncated."""
    tx, ty = np.float64(tx), np.float64(ty)
    xin = (np.asarray(x, dtype=np.float64) + 0.5) + tx
    yin = (np.asarray(y, dtype=np.float64) + 0.5) + ty
    inside = ~((xin < 0) | (xin >= w) | (yin < 0) | (yin >= h))
    xin = xin - 0.5
    yin = yin - 0.5
    xf, yf = np.floor(xin), np.floor(yin)
    dx, dy = (xin - xf)[..., None], (yin - yf)[..., None]
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    xa, xb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1)
    ya, yb = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    p00, p01 = fetch(xa, ya).astype(np.float64), fetch(xb, ya).astype(np.float64)
    p10, p11 = fetch(xa, yb).astype(np.float64), fetch(xb, yb).astype(np.float64)
    v1 = p00 + (p01 - p00) * dx
    v2 = p10 + (p11 - p10) * dx
    v = v1 + (v2 - v1) * dy
    return np.where(inside[..., None], v.astype(np.uint8), np.uint8(0))          # 0 <= v <= 255: astype truncates


def _grid(w, h):
    y, x = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    return x, y


def affine_nearest(src_u8, a):
    """One whole NEAREST pass (output size = source size): `Image.transform(size, AFFINE, m, NEAREST)` for a = fix_matrix(m)."""
    h, w = src_u8.shape[:2]
    x, y = _grid(w, h)
    return nearest_at(lambda xs, ys: src_u8[ys, xs], w, h, a, x, y)


def translate_bilinear(src_u8, tx, ty):
    """One whole BILINEAR pass: `Image.transform(size, AFFINE, (1, 0, tx, 0, 1, ty), BILINEAR)`."""
    h, w = src_u8.shape[:2]
    x, y = _grid(w, h)
    return bilinear_at(lambda xs, ys: src_u8[ys, xs], w, h, tx, ty, x, y)


def align_reference(src_u8, row, crop=512):
    """The lazy chain for the crop window of one sample: src_u8 [h, w, 3] uint8, row from kitti_align_params, crop = side or
    (crop_h, crop_w) of the window whose origin the row holds (KITTI: 512).  Returns [crop_h, crop_w, 3] uint8 — what the
    four Pillow passes and the crop give."""
    row = np.asarray(row, dtype=np.int64)
    r1, r2 = tuple(int(v) for v in row[0:6]), tuple(int(v) for v in row[6:12])
    tx1, ty1, tx2, ty2 = row[12:16].view(np.float64)
    w, h, left, top = (int(v) for v in row[16:20])
    if src_u8.shape != (h, w, 3) or src_u8.dtype != np.uint8:
        raise ValueError("src_u8 must be [%d,%d,3] uint8" % (h, w))
    crop_h, crop_w = (crop, crop) if np.isscalar(crop) else crop
    x, y = _grid(crop_w, crop_h)

    def p1(xs, ys):
        return nearest_at(lambda u, v: src_u8[v, u], w, h, r1, xs, ys)

    def p2(xs, ys):
        return bilinear_at(p1, w, h, tx1, ty1, xs, ys)

    def p3(xs, ys):
        return bilinear_at(p2, w, h, tx2, ty2, xs, ys)

    x, y = x + left, y + top
    in_image = ((x >= 0) & (x < w) & (y >= 0) & (y < h))[..., None]             # a crop past the image is 0, as PIL's crop
    return np.where(in_image, nearest_at(p3, w, h, r2, x, y), np.uint8(0))


def align_norm_spec(src_list, rows, crop, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """What ccvpe_kitti_align_norm_u8_f32 computes, in numpy: src_list = B arrays [h, w, 3] uint8 (repeats allowed; None = the
    all-zero crop of a row whose address is 0), rows [B, ROW_LEN], crop = side or (crop_h, crop_w).  `align_reference` per
    sample, then the fp32 ToTensor / Normalize of cache.gather_spec with roll 0.  Returns [B, 3, crop_h, crop_w] float32."""
    from .cache import gather_spec
    crop_h, crop_w = (crop, crop) if np.isscalar(crop) else crop
    crops = [np.zeros((crop_h, crop_w, 3), dtype=np.uint8) if src is None else align_reference(src, row, (crop_h, crop_w))
             for src, row in zip(src_list, rows)]
    if not crops:
        return np.empty((0, 3, crop_h, crop_w), dtype=np.float32)
    return gather_spec(crops, [0] * len(crops), mean=mean, std=std)


# ---- the device launches ---------------------------------------------------------------------------------------------------
def kitti_align(src_u8, offsets, rows, crop_hw, out=None):
    """ONE launch for a batch: src_u8 = packed uint8 device buffer of decoded [h, w, 3] maps, offsets int64 [B] (device) =
    each sample's first byte in it, rows int64 [B, ROW_LEN] (device).  Returns / writes out [B, crop_h, crop_w, 3] uint8.
    A sample whose w * h * 3 bytes do not fit in the buffer behind its offset is written as zeros, never read."""
    import torch
    from . import _lib, ops
    lib = _lib.load()
    for t, dt, nm in ((src_u8, torch.uint8, "src_u8"), (offsets, torch.int64, "offsets"), (rows, torch.int64, "rows")):
        if not (t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise ValueError("%s must be a contiguous %s device tensor (no CPU fallback)" % (nm, dt))
    b = int(rows.shape[0])
    if rows.dim() != 2 or rows.shape[1] != ROW_LEN or tuple(offsets.shape) != (b,) or src_u8.dim() != 1:
        raise ValueError("rows must be [B,%d], offsets [B], src_u8 one-dimensional" % ROW_LEN)
    crop_h, crop_w = crop_hw
    if out is None:
        out = torch.empty((b, crop_h, crop_w, 3), device=src_u8.device, dtype=torch.uint8)
    if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (b, crop_h, crop_w, 3)):
        raise ValueError("out must be a contiguous [%d,%d,%d,3] uint8 device tensor" % (b, crop_h, crop_w))
    _lib.check(lib.ccvpe_kitti_align_u8(src_u8.data_ptr(), src_u8.numel(), offsets.data_ptr(), rows.data_ptr(), b,
                                        out.data_ptr(), crop_h, crop_w, ops._stream()), "ccvpe_kitti_align_u8")
    return out


def kitti_align_norm(srcs, rows, crop_hw, dst=None, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """ONE launch for a batch side, from maps that already lie on the device: srcs int64 [B] (device) = the device address of
    each sample's decoded [h, w, 3] uint8 map (raw slots of the device image cache, or any live uint8 device memory of that
    size; repeats allowed; 0 = an all-zero crop, never read), rows int64 [B, ROW_LEN] (device).  Writes / returns
    dst [B, 3, crop_h, crop_w] fp32: the aligned crop through ToTensor -> Normalize, bit-identical to `kitti_align` followed by
    `preprocess.gather_norm`, with no uint8 crop in between.  The caller keeps the addressed memory alive."""
    import ctypes

    import torch
    from . import _lib, ops
    lib = _lib.load()
    for t, nm in ((srcs, "srcs"), (rows, "rows")):
        if not (t.is_cuda and t.dtype == torch.int64 and t.is_contiguous()):
            raise ValueError("%s must be a contiguous int64 device tensor (no CPU fallback)" % nm)
    b = int(rows.shape[0])
    if rows.dim() != 2 or rows.shape[1] != ROW_LEN or tuple(srcs.shape) != (b,) or srcs.device != rows.device:
        raise ValueError("rows must be [B,%d] and srcs [B], on one device" % ROW_LEN)
    crop_h, crop_w = crop_hw
    if dst is None:
        dst = torch.empty((b, 3, crop_h, crop_w), device=rows.device, dtype=torch.float32)
    if not (dst.is_cuda and dst.dtype == torch.float32 and dst.is_contiguous() and tuple(dst.shape) == (b, 3, crop_h, crop_w)):
        raise ValueError("dst must be a contiguous [%d,3,%d,%d] fp32 device tensor" % (b, crop_h, crop_w))
    m = (ctypes.c_float * 3)(*mean)
    s = (ctypes.c_float * 3)(*std)
    _lib.check(lib.ccvpe_kitti_align_norm_u8_f32(srcs.data_ptr(), rows.data_ptr(), b, m, s, dst.data_ptr(), crop_h, crop_w,
                                                 ops._stream()), "ccvpe_kitti_align_norm_u8_f32")
    return dst
