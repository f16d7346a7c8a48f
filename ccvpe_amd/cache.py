"""Device-resident image cache: the per-FILE half of the input pipeline kept in HBM.

Decoding a file and the Pillow-exact resize depend only on the file; the panorama roll, the field-of-view crop and the choice
of aerial tile change per epoch and are all applied after the resize.  `DeviceImageCache` therefore keeps the RESIZED uint8
image of every source file it has seen ([h, w, 3] bytes: 614 KB per VIGOR panorama, 786 KB per aerial tile), filled by
ccvpe_resize_u8, and ccvpe_gather_norm_u8_f32 assembles a whole normalised NCHW batch side from a table of slot addresses in
one launch (ccvpe_amd.preprocess.gather_norm).  From the second epoch on a cached sample costs no file open, no decode, no
upload and no resample.  `ccvpe_amd.datasets.DeviceBatches(..., cache=cache)` drives it; without a cache nothing changes.

Storage: chunks of uint8 per resized shape, allocated lazily; the chunks' total size never exceeds `capacity_bytes`.  There
is NO eviction: when no slot is left, `full` turns true and new images are simply not retained (they go through `scratch`
slots and the same gather launch).  The host table is guarded by a lock: lookups come from DeviceBatches' producer thread,
inserts from the consumer thread.  `device="cpu"` keeps the same books over CPU tensors and launches nothing (tests).

RAW slots (`insert_raw`): the decoded image as it is, for sources a kernel reads whole — KITTI's 1280 x 1280 aerial maps
(4.9 MB each), which ccvpe_kitti_align_norm_u8_f32 aligns and normalises from a table of slot addresses
(KITTIPairs(device_align=True, cache_maps=True); ccvpe_amd.align.kitti_align_norm).  Same chunks per shape, capacity, lock,
counters and `full` rule; `raw_key` keeps a file's raw entry apart from its resized ones.

`gather_spec` is the numpy fp32 specification of the gather kernel.

Not done here: caching only the window of a KITTI map the alignment can reach, eviction policies, pinned
staging for the first epoch's uploads."""
import threading

import numpy as np
import torch

from .preprocess import IMAGENET_MEAN, IMAGENET_STD


def gather_spec(images, rolls, keep_w=None, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """What ccvpe_gather_norm_u8_f32 computes, in numpy fp32: images = B arrays [h, w, 3] uint8 (one per batch row, repeats
    allowed), rolls = B integers (torch.roll shifts: any sign, any magnitude).  Returns [B, 3, h, keep_w] float32 with
    out[b, c, y, x] = ((float32)img_b[y, (x - roll_b) mod w, c] / 255 - mean[c]) / std[c], every operation rounded to fp32."""
    h, w = images[0].shape[:2]
    keep = w if keep_w is None else int(keep_w)
    if not 0 < keep <= w:
        raise ValueError("keep_w must be in 1..%d" % w)
    m = np.asarray(mean, dtype=np.float32).reshape(1, 1, 3)
    s = np.asarray(std, dtype=np.float32).reshape(1, 1, 3)
    out = np.empty((len(images), 3, h, keep), dtype=np.float32)
    for b, (img, roll) in enumerate(zip(images, rolls)):
        if img.shape != (h, w, 3) or img.dtype != np.uint8:
            raise ValueError("images must all be [%d,%d,3] uint8" % (h, w))
        xs = (np.arange(keep, dtype=np.int64) - int(roll)) % w
        v = img[:, xs, :].astype(np.float32) / np.float32(255.0)
        out[b] = ((v - m) / s).transpose(2, 0, 1)
    return out


class _Shape(object):
    """The chunks of one resized shape: [slots, h, w, 3] uint8 tensors and the next free slot of the last one."""
    __slots__ = ("chunks", "free")

    def __init__(self):
        self.chunks, self.free = [], 0


class DeviceImageCache(object):
    """key (str) -> (device address, resized (h, w), raw (h, w)) of a resized uint8 image in `device` memory (a raw entry:
    both sizes are the image's own).

    capacity_bytes bounds the chunks' total size; chunk_bytes is the allocation granule (a chunk holds
    max(1, chunk_bytes // (h * w * 3)) slots, fewer when less capacity is left — a chunk belongs to ONE shape, so keep
    chunk_bytes well below capacity_bytes when several shapes share the cache).  Counters: hits / misses (of `lookup`),
    entries, bytes_used (occupied slots), bytes_allocated (chunks), full."""

    def __init__(self, device, capacity_bytes, chunk_bytes=64 << 20):
        self.device = torch.device(device)
        self.capacity_bytes, self.chunk_bytes = int(capacity_bytes), int(chunk_bytes)
        if self.capacity_bytes < 0 or self.chunk_bytes <= 0:
            raise ValueError("capacity_bytes must be >= 0 and chunk_bytes > 0")
        self._lock = threading.Lock()
        self._scratch = {}
        self.clear()

    def clear(self):
        """Forget every entry and release the chunks and the scratch slots; the counters start again."""
        with self._lock:
            self._table, self._shapes = {}, {}
            self._scratch = {}
            self.hits = self.misses = self.entries = self.bytes_used = self.bytes_allocated = 0
            self.full = False

    def __len__(self):
        return self.entries

    def lookup(self, key):
        """(address, raw (h, w)) of a cached image, or None; counts a hit or a miss."""
        with self._lock:
            e = self._table.get(key)
            if e is None:
                self.misses += 1
                return None
            self.hits += 1
            return e[0], e[2]

    def address(self, key):
        """The address of a cached image or None, without touching the counters (DeviceBatches: a key that another sample of
        the batch, or an earlier batch still in flight at lookup time, has inserted meanwhile)."""
        with self._lock:
            e = self._table.get(key)
            return None if e is None else e[0]

    def resized_hw(self, key):
        with self._lock:
            e = self._table.get(key)
            return None if e is None else e[1]

    def _slot(self, out_hw):
        """A free slot [h, w, 3] of shape out_hw, or None when the capacity does not allow another one.  Lock held."""
        h, w = out_hw
        size = h * w * 3
        sh = self._shapes.setdefault((h, w), _Shape())
        if not sh.chunks or sh.free == sh.chunks[-1].shape[0]:
            slots = min(max(1, self.chunk_bytes // size), (self.capacity_bytes - self.bytes_allocated) // size)
            if slots <= 0:
                self.full = True
                return None
            sh.chunks.append(torch.empty((slots, h, w, 3), device=self.device, dtype=torch.uint8))
            sh.free = 0
            self.bytes_allocated += slots * size
        slot = sh.chunks[-1][sh.free]
        sh.free += 1
        return slot

    def insert(self, key, img_u8_device, out_hw):
        """Resize the decoded [H, W, 3] uint8 image (on `device`) into a free slot and remember it under `key`.  Returns the
        slot's address; the address already stored when `key` is present (a no-op: nothing is resized); None when the cache
        is full (the image is not retained)."""
        out_hw = (int(out_hw[0]), int(out_hw[1]))
        raw_hw = (int(img_u8_device.shape[0]), int(img_u8_device.shape[1]))
        with self._lock:
            e = self._table.get(key)
            if e is not None:
                return e[0]
            slot = self._slot(out_hw)
            if slot is None:
                return None
        if self.device.type != "cpu":                       # stream-ordered: the gather launch that reads the slot comes later
            from . import preprocess
            preprocess.resize_u8(img_u8_device, out_hw, dst=slot)
        with self._lock:                                    # published only now: a lookup never sees a slot nobody has filled
            self._table[key] = (slot.data_ptr(), out_hw, raw_hw)
            self.entries += 1
            self.bytes_used += out_hw[0] * out_hw[1] * 3
        return slot.data_ptr()

    @staticmethod
    def raw_key(key):
        """The key under which `insert_raw` callers keep the UNRESIZED image of source file `key`: resized entries are keyed
        "<file>|<h>x<w>" (DeviceBatches), so a raw entry and a resized entry of one file never collide."""
        return "%s|raw" % key

    def insert_raw(self, key, img_u8):
        """Retain the decoded [h, w, 3] uint8 image AS IT IS (KITTI's aerial maps: the align kernel reads the whole map) in a
        free slot of its own shape and remember it under `key`; chunks per (h, w), capacity, lock, counters and the `full`
        rule are those of `insert`.  img_u8: a tensor on `device` (a view of the batch's staged upload, say), copied into the
        slot on the current stream.  Returns the slot's address; the address already stored when `key` is present (a no-op:
        nothing is copied); None when the cache is full (the image is not retained).  `lookup` returns the raw (h, w)."""
        if len(img_u8.shape) != 3 or img_u8.shape[2] != 3 or min(img_u8.shape) <= 0:
            raise ValueError("img_u8 must be [h,w,3] uint8")
        hw = (int(img_u8.shape[0]), int(img_u8.shape[1]))
        with self._lock:
            e = self._table.get(key)
            if e is not None:
                return e[0]
            slot = self._slot(hw)
            if slot is None:
                return None
        if self.device.type != "cpu":                       # stream-ordered: the align launch that reads the slot comes later
            slot.copy_(img_u8, non_blocking=True)
        with self._lock:                                    # published only now: a lookup never sees a slot nobody has filled
            self._table[key] = (slot.data_ptr(), hw, hw)
            self.entries += 1
            self.bytes_used += hw[0] * hw[1] * 3
        return slot.data_ptr()

    def scratch(self, batch, out_hw):
        """[batch, h, w, 3] uint8 on `device`: non-retained slots for the images of one batch side that are not cached (a full
        cache, a side without a key).  Reused by the next call for the same shape — the gather launch that reads them is
        enqueued before that, on the same stream.  Working memory: not counted against capacity_bytes."""
        h, w = int(out_hw[0]), int(out_hw[1])
        t = self._scratch.get((h, w))
        if t is None or t.shape[0] < batch:
            t = torch.empty((int(batch), h, w, 3), device=self.device, dtype=torch.uint8)
            self._scratch[(h, w)] = t
        return t[:batch]
