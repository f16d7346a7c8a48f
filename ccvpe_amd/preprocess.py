"""Input pipeline after JPEG decoding, on the MI355X: Resize + ToTensor + Normalize + panorama roll +
FoV crop of train_VIGOR.py:57-70,177-178 / datasets.py:98-121 as ccvpe_preprocess_u8_f32 on the decoded uint8 image.

torchvision's `transforms.Resize` on a PIL image is `PIL.Image.resize(size, BILINEAR)`: Pillow's antialiased resampler
in 8-bit fixed point.  `resample_tables` restates its coefficient set-up (src/libImaging/Resample.c: precompute_coeffs()
and normalize_coeffs_8bpc(), Pillow 12.2) in float64, the kernels do the two integer passes; the result equals PIL's
bit for bit (tests/test_preprocess_gpu.py runs PIL itself as the reference).

`window_resize_norm` is the same transform behind a crop, for a whole batch in one launch: the windows are cut out of ONE large
uint8 map resident on the device (the Oxford RobotCar aerial map) at a table of origins; `window_resize_spec` states it in numpy."""
import ctypes
import functools
import math

import numpy as np
import torch

from . import _lib, ops
from ._lib import check

PRECISION_BITS = 32 - 8 - 2
IMAGENET_MEAN = (0.485, 0.456, 0.406)      # train_VIGOR.py:60
IMAGENET_STD = (0.229, 0.224, 0.225)


@functools.lru_cache(maxsize=64)
def resample_tables(in_size, out_size):
    """Pillow's precompute_coeffs() for the BILINEAR filter over the whole axis (box = [0, in_size]) followed by
    normalize_coeffs_8bpc(): returns (bounds int32 [out,2] = (xmin, count), coef int32 [out,ksize], ksize)."""
    scale = float(in_size - 0) / out_size
    filterscale = scale if scale >= 1.0 else 1.0
    support = 1.0 * filterscale                       # bilinear support = 1
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coef = np.zeros((out_size, ksize), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        k = []
        ww = 0.0
        for x in range(xmax):
            a = (x + xmin - center + 0.5) * ss
            a = -a if a < 0.0 else a
            w = 1.0 - a if a < 1.0 else 0.0
            k.append(w)
            ww += w
        for x in range(xmax):
            v = k[x] / ww if ww != 0.0 else k[x]
            coef[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, coef, ksize


_dev_tables = {}


def _tables_on(device, in_size, out_size):
    key = (str(device), in_size, out_size)
    if key not in _dev_tables:
        b, c, k = resample_tables(in_size, out_size)
        _dev_tables[key] = (torch.from_numpy(b).to(device), torch.from_numpy(c).to(device), k)
    return _dev_tables[key]


def preprocess(img_u8, out_hw, dst=None, roll=0, keep_w=None, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """img_u8: decoded image [H,W,3] uint8 on the device.  Writes / returns dst [3, h, keep_w] fp32 (e.g. batch[i]):
    Resize([h, w]) -> ToTensor -> Normalize -> torch.roll(shifts=roll, dims=W) -> [..., :keep_w]."""
    lib = _lib.load()
    if not (img_u8.is_cuda and img_u8.dtype == torch.uint8 and img_u8.is_contiguous() and img_u8.dim() == 3
            and img_u8.shape[2] == 3):
        raise ValueError("img_u8 must be a contiguous [H,W,3] uint8 device tensor (no CPU fallback)")
    h_in, w_in = int(img_u8.shape[0]), int(img_u8.shape[1])
    h, w = out_hw
    keep = w if keep_w is None else int(keep_w)
    if dst is None:
        dst = torch.empty((3, h, keep), device=img_u8.device, dtype=torch.float32)
    ops._chk(dst, "dst")
    if tuple(dst.shape) != (3, h, keep):
        raise ValueError("dst must be [3,%d,%d]" % (h, keep))
    xb, xc, xk = _tables_on(img_u8.device, w_in, w)
    yb, yc, yk = _tables_on(img_u8.device, h_in, h)
    tmp = torch.empty((h_in, w, 3), device=img_u8.device, dtype=torch.uint8)
    m = (ctypes.c_float * 3)(*mean)
    s = (ctypes.c_float * 3)(*std)
    check(lib.ccvpe_preprocess_u8_f32(img_u8.data_ptr(), h_in, w_in, xb.data_ptr(), xc.data_ptr(), xk, yb.data_ptr(),
                                      yc.data_ptr(), yk, tmp.data_ptr(), dst.data_ptr(), h, w, keep, int(roll), m, s,
                                      ops._stream()), "ccvpe_preprocess_u8_f32")
    return dst


def preprocess_batch(images_u8, out_hw, rolls=None, keep_w=None, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """List of decoded [H,W,3] uint8 device images (sizes may differ) -> one NCHW fp32 batch [B,3,h,keep_w], each sample
    written in place by its own pair of launches (no intermediate float image, no host round trip)."""
    h, w = out_hw
    keep = w if keep_w is None else int(keep_w)
    out = torch.empty((len(images_u8), 3, h, keep), device=images_u8[0].device, dtype=torch.float32)
    for i, img in enumerate(images_u8):
        preprocess(img, out_hw, dst=out[i], roll=0 if rolls is None else int(rolls[i]), keep_w=keep, mean=mean, std=std)
    return out


def resize_u8(img_u8, out_hw, dst=None):
    """img_u8: decoded image [H,W,3] uint8 on the device.  Writes / returns dst [h, w, 3] uint8 (e.g. a slot of the device
    image cache): PIL.Image.resize((w, h), BILINEAR) bit for bit — the per-file half of `preprocess`, kept as bytes."""
    lib = _lib.load()
    if not (img_u8.is_cuda and img_u8.dtype == torch.uint8 and img_u8.is_contiguous() and img_u8.dim() == 3
            and img_u8.shape[2] == 3):
        raise ValueError("img_u8 must be a contiguous [H,W,3] uint8 device tensor (no CPU fallback)")
    h_in, w_in = int(img_u8.shape[0]), int(img_u8.shape[1])
    h, w = out_hw
    if dst is None:
        dst = torch.empty((h, w, 3), device=img_u8.device, dtype=torch.uint8)
    ops._chk(dst, "dst", torch.uint8)
    if dst.numel() != h * w * 3:
        raise ValueError("dst must hold [%d,%d,3] bytes" % (h, w))
    xb, xc, xk = _tables_on(img_u8.device, w_in, w)
    yb, yc, yk = _tables_on(img_u8.device, h_in, h)
    tmp = torch.empty((h_in, w, 3), device=img_u8.device, dtype=torch.uint8)
    check(lib.ccvpe_resize_u8(img_u8.data_ptr(), h_in, w_in, xb.data_ptr(), xc.data_ptr(), xk, yb.data_ptr(), yc.data_ptr(), yk,
                              tmp.data_ptr(), dst.data_ptr(), h, w, ops._stream()), "ccvpe_resize_u8")
    return dst


def gather_norm(addresses, rolls, hw, keep_w=None, dst=None, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """ONE launch for a batch side: addresses int64 [B] (device) = device addresses of resized [h, w, 3] uint8 images (slots
    of the device image cache, or any live uint8 device memory of that size), rolls int32 [B] (device).  Writes / returns
    dst [B, 3, h, keep_w] fp32: ToTensor -> Normalize -> torch.roll(shifts=rolls[b], dims=W) -> [..., :keep_w], bit-identical
    to `preprocess` on the image the slot was resized from.  The caller keeps the addressed memory alive."""
    lib = _lib.load()
    ops._chk(addresses, "addresses", torch.int64)
    ops._chk(rolls, "rolls", torch.int32)
    b = int(addresses.shape[0])
    if addresses.dim() != 1 or tuple(rolls.shape) != (b,):
        raise ValueError("addresses and rolls must both be [B]")
    h, w = hw
    keep = w if keep_w is None else int(keep_w)
    if dst is None:
        dst = torch.empty((b, 3, h, keep), device=addresses.device, dtype=torch.float32)
    ops._chk(dst, "dst")
    if tuple(dst.shape) != (b, 3, h, keep):
        raise ValueError("dst must be [%d,3,%d,%d]" % (b, h, keep))
    m = (ctypes.c_float * 3)(*mean)
    s = (ctypes.c_float * 3)(*std)
    check(lib.ccvpe_gather_norm_u8_f32(addresses.data_ptr(), rolls.data_ptr(), b, h, w, keep, m, s, dst.data_ptr(),
                                       ops._stream()), "ccvpe_gather_norm_u8_f32")
    return dst


def _window_args(map_u8, origins, box_hw, out_hw):
    if not (map_u8.is_cuda and map_u8.dtype == torch.uint8 and map_u8.is_contiguous() and map_u8.dim() == 3
            and map_u8.shape[2] == 3):
        raise ValueError("map_u8 must be a contiguous [H,W,3] uint8 device tensor (no CPU fallback)")
    ops._chk(origins, "origins", torch.int32)
    if origins.dim() != 2 or origins.shape[1] != 2 or origins.device != map_u8.device:
        raise ValueError("origins must be [B,2] int32 (x0, y0) on the map's device")
    (bh, bw), (h, w) = box_hw, out_hw
    if min(bh, bw, h, w) <= 0:
        raise ValueError("box_hw and out_hw must be positive")
    return int(origins.shape[0]), int(bh), int(bw), int(h), int(w)


def window_resize_norm(map_u8, origins, box_hw, out_hw, dst=None, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """ONE launch for a batch side served by a device-resident map: map_u8 [H,W,3] uint8 (device), origins int32 [B,2]
    (device) = (x0, y0) of each sample's box_hw window — any sign, the part outside the map reads as 0 like PIL.Image.crop.
    Writes / returns dst [B, 3, h, w] fp32 = crop -> Resize(out_hw) -> ToTensor -> Normalize, bit-identical to `preprocess`
    on the uploaded crop.  Neither the window nor the horizontal intermediate exists in memory."""
    lib = _lib.load()
    b, bh, bw, h, w = _window_args(map_u8, origins, box_hw, out_hw)
    if dst is None:
        dst = torch.empty((b, 3, h, w), device=map_u8.device, dtype=torch.float32)
    ops._chk(dst, "dst")
    if tuple(dst.shape) != (b, 3, h, w):
        raise ValueError("dst must be [%d,3,%d,%d]" % (b, h, w))
    xb, xc, xk = _tables_on(map_u8.device, bw, w)
    yb, yc, yk = _tables_on(map_u8.device, bh, h)
    m = (ctypes.c_float * 3)(*mean)
    s = (ctypes.c_float * 3)(*std)
    check(lib.ccvpe_window_resize_norm_u8_f32(map_u8.data_ptr(), int(map_u8.shape[0]), int(map_u8.shape[1]), origins.data_ptr(),
                                              b, bh, bw, xb.data_ptr(), xc.data_ptr(), xk, yb.data_ptr(), yc.data_ptr(), yk, m, s,
                                              dst.data_ptr(), h, w, ops._stream()), "ccvpe_window_resize_norm_u8_f32")
    return dst


def _resample_axis0(img, bounds, coef):
    """One integer pass of Pillow's resampler along axis 0 of a uint8 array [n, ...]: out[i] = clip8((2^21 + sum_k
    img[min_i + k] * coef[i, k]) >> 22), the sums in int32 as the C code's."""
    out = np.empty((len(bounds),) + img.shape[1:], dtype=np.uint8)
    for i, (lo, n) in enumerate(bounds):
        acc = np.full(img.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int32)
        for k in range(int(n)):
            acc += img[lo + k].astype(np.int32) * np.int32(coef[i, k])
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def window_resize_spec(map_u8, origins, box_hw, out_hw, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """What ccvpe_window_resize_norm_u8_f32 computes, in numpy: map_u8 [H, W, 3] uint8, origins B pairs (x0, y0).  Per sample:
    the zero-filled box_hw window (PIL.Image.crop), Pillow's two BILINEAR integer passes from `resample_tables` (horizontal,
    uint8 intermediate, vertical), then ((float32)v / 255 - mean[c]) / std[c] with every operation rounded to fp32 — the
    arithmetic of cache.gather_spec.  Returns [B, 3, h, w] float32."""
    map_u8 = np.asarray(map_u8)
    if map_u8.ndim != 3 or map_u8.shape[2] != 3 or map_u8.dtype != np.uint8:
        raise ValueError("map_u8 must be [H,W,3] uint8")
    (bh, bw), (h, w) = box_hw, out_hw
    mh, mw = map_u8.shape[:2]
    xb, xc, _ = resample_tables(bw, w)
    yb, yc, _ = resample_tables(bh, h)
    m = np.asarray(mean, dtype=np.float32).reshape(1, 1, 3)
    s = np.asarray(std, dtype=np.float32).reshape(1, 1, 3)
    origins = np.asarray(origins, dtype=np.int64).reshape(-1, 2)
    out = np.empty((len(origins), 3, h, w), dtype=np.float32)
    for b, (x0, y0) in enumerate(origins):
        x0, y0 = int(x0), int(y0)
        win = np.zeros((bh, bw, 3), dtype=np.uint8)
        ys, ye, xs, xe = max(y0, 0), min(y0 + bh, mh), max(x0, 0), min(x0 + bw, mw)
        if ys < ye and xs < xe:
            win[ys - y0:ye - y0, xs - x0:xe - x0] = map_u8[ys:ye, xs:xe]
        tmp = _resample_axis0(win.transpose(1, 0, 2), xb, xc).transpose(1, 0, 2)      # horizontal: [bh, w, 3] uint8
        res = _resample_axis0(tmp, yb, yc)                                              # vertical:   [h, w, 3] uint8
        v = res.astype(np.float32) / np.float32(255.0)
        out[b] = ((v - m) / s).transpose(2, 0, 1)
    return out
