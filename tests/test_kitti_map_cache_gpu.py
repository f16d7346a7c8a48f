"""Device-resident KITTI aerial maps on the MI355X: ccvpe_kitti_align_norm_u8_f32 (csrc/align.hip) against LIVE Pillow followed by
the gather's fp32 normalisation (`cache.gather_spec`) on the case table of tests/kitti_align_cases.py — every source its own device
allocation, addressed through the pointer table — and DeviceBatches with KITTIPairs(device_align=True, cache_maps=True) + a cache
against the plain device_align path, two epochs, the second without any image file.  Equal bits everywhere, no tolerance."""
import ctypes
import os

import numpy as np
import pytest
import torch

import kitti_align_cases as K
from ccvpe_amd import _lib, align, cache as C, datasets as DS, ops
from test_datasets import make_kitti_tree

pytestmark = pytest.mark.gpu

EINVAL = -1
FIELDS = ("grd", "sat", "gt", "gt_ori", "labels", "center", "angle_deg")


def pillow_norm(case):
    """Pillow's crop for a case through ToTensor / Normalize in fp32: [3, crop, crop]."""
    return C.gather_spec([K.expected(case)], [0])[0]


def launch_norm(sources, rows, crop_hw, **kw):
    """ONE launch: sources = per row a device tensor (its own allocation, or one shared with another row) or None (address 0)."""
    table = torch.tensor([0 if s is None else s.data_ptr() for s in sources], dtype=torch.int64, device="cuda")
    got = align.kitti_align_norm(table, torch.from_numpy(np.stack(rows)).cuda(), crop_hw, **kw)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def upload(name):
    return torch.from_numpy(K.source(name).copy()).cuda()       # a fresh allocation per call


def test_one_launch_per_crop_from_separate_allocations_equals_pillow():
    K.check_inputs_are_visible(K.CASES)
    by_crop = {}
    for c in K.CASES:
        if c.crop != 512:
            by_crop.setdefault(c.crop, []).append(c)
    assert sorted(by_crop) == [48, 64, 81] and {c.src for cs in by_crop.values() for c in cs} == {"s97x131", "s96x80", "s81"}
    for crop, cases in sorted(by_crop.items()):
        dev = [upload(c.src) for c in cases]                     # one allocation per row ...
        assert len({t.data_ptr() for t in dev}) == len(cases)
        rows = [K.params(c) for c in cases]
        dev.append(dev[0])                                       # ... and one more row that shares row 0's address, with row 1's draw
        rows.append(K.params(cases[1]))
        assert cases[0].src == cases[1].src
        got = launch_norm(dev, rows, (crop, crop))
        assert got.dtype == np.float32 and got.shape == (len(cases) + 1, 3, crop, crop)
        assert np.array_equal(got, launch_norm(dev, rows, (crop, crop))), "crop %d: two runs differ" % crop
        for j, c in enumerate(cases + [cases[1]]):
            want = pillow_norm(c)
            assert np.array_equal(got[j], want), "%s (row %d): %d of %d values differ" % (c.name, j, int((got[j] != want).sum()), want.size)
        spec = align.align_norm_spec([K.source(c.src) for c in cases[:2]], rows[:2], crop)
        assert np.array_equal(got[:2], spec)


def test_real_size_sources_and_crop_equal_pillow():
    cases = [c for c in K.CASES if c.crop == 512] + [K.CASE_1280]
    assert [c.name for c in cases] == ["k1", "k2", "k1280"]
    for c in cases:                                              # Pillow's own result is image, not fill: zeros cannot pass
        assert np.count_nonzero(K.expected(c)) > 0.8 * K.expected(c).size, c.name
    s640 = upload("s640")
    dev = [s640, s640, upload("s1280")]                          # k1 and k2 share one map, as two samples of one frame would
    out = torch.full((3, 3, 512, 512), float("nan"), device="cuda")
    got = launch_norm(dev, [K.params(c) for c in cases], (512, 512), dst=out)
    assert np.array_equal(got, out.cpu().numpy())                # written in place
    for j, c in enumerate(cases):
        want = pillow_norm(c)
        assert np.array_equal(got[j], want), "%s: %d of %d values differ" % (c.name, int((got[j] != want).sum()), want.size)


def test_non_square_crop_and_other_constants_equal_the_spec():
    c = K.CASES[0]
    h, w, _ = K.SOURCES[c.src]
    crop = (40, 72)                                              # crop_h a multiple of 8, crop_w not of 32 — and the reverse
    mean, std = (0.5, 0.25, 0.0), (0.5, 1.0, 2.0)
    for crop_hw in (crop, crop[::-1]):
        row = align.kitti_align_params(c.heading, c.cam, c.shift, c.ori, w, h, crop_hw)
        want = align.align_norm_spec([K.source(c.src)], [row], crop_hw)
        assert np.count_nonzero(align.align_reference(K.source(c.src), row, crop_hw)) > 0.4 * want.size
        got = launch_norm([upload(c.src)], [row], crop_hw)
        assert got.shape == (1, 3) + crop_hw and np.array_equal(got, want)
        got = launch_norm([upload(c.src)], [row], crop_hw, mean=mean, std=std)
        assert np.array_equal(got, align.align_norm_spec([K.source(c.src)], [row], crop_hw, mean, std))


def test_address_zero_and_bad_sizes_are_zero_crops_between_intact_neighbours():
    a, b = [c for c in K.CASES if c.name in ("int", "half")]
    src = upload(a.src)
    bad_w, bad_h = K.params(b).copy(), K.params(b).copy()
    bad_w[16], bad_h[17] = 32768, 0                              # sizes outside 1..32767 with a live address: not dereferenced either
    got = launch_norm([src, None, src, src, src], [K.params(a), K.params(b), bad_w, bad_h, K.params(b)], (48, 48))
    zero = C.gather_spec([np.zeros((48, 48, 3), dtype=np.uint8)], [0])[0]
    assert len({float(zero[ch, 0, 0]) for ch in range(3)}) == 3 and all((zero[ch] == zero[ch, 0, 0]).all() for ch in range(3))
    for j in (1, 2, 3):
        assert np.array_equal(got[j], zero), "row %d" % j
    assert np.array_equal(got[0], pillow_norm(a)) and np.array_equal(got[4], pillow_norm(b))
    assert np.array_equal(got, align.align_norm_spec([K.source(a.src), None, None, None, K.source(a.src)],
                                                     [K.params(a), K.params(b), bad_w, bad_h, K.params(b)], 48))


def test_argument_checks():
    lib = _lib.load()
    c = K.CASES[0]
    src = upload(c.src)
    table = torch.tensor([src.data_ptr()], dtype=torch.int64, device="cuda")
    rows = torch.from_numpy(K.params(c)[None]).cuda()
    dst = torch.empty((1, 3, 64, 64), device="cuda")
    m, s = (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.25, 0.25, 0.25)
    st = ops._stream()
    f = lib.ccvpe_kitti_align_norm_u8_f32
    assert f(table.data_ptr(), rows.data_ptr(), 1, m, s, dst.data_ptr(), 64, 64, st) == 0
    assert f(None, None, 0, m, s, None, 64, 64, st) == 0        # an empty batch: no launch, no tables
    for bad in ((-1, 64, 64), (65536, 64, 64), (1, 0, 64), (1, 64, 0), (1, 32768, 64)):
        assert f(table.data_ptr(), rows.data_ptr(), bad[0], m, s, dst.data_ptr(), bad[1], bad[2], st) == EINVAL, bad
    assert b"kitti_align_norm" in lib.ccvpe_last_error()
    assert f(None, rows.data_ptr(), 1, m, s, dst.data_ptr(), 64, 64, st) == EINVAL
    assert f(table.data_ptr(), rows.data_ptr(), 1, None, s, dst.data_ptr(), 64, 64, st) == EINVAL
    torch.cuda.synchronize()
    assert tuple(align.kitti_align_norm(table[:0], rows[:0], (64, 64)).shape) == (0, 3, 64, 64)
    with pytest.raises(ValueError):
        align.kitti_align_norm(table.cpu(), rows, (64, 64))     # no CPU fallback
    with pytest.raises(ValueError):
        align.kitti_align_norm(table, rows, (64, 64), dst=dst[:, :, :, :32])
    with pytest.raises(ValueError):
        align.kitti_align_norm(table, rows[:, :19].contiguous(), (64, 64))


def test_the_uint8_kernel_still_writes_pillows_bytes():
    by_crop = {}
    for c in K.CASES + [K.CASE_1280]:
        by_crop.setdefault(c.crop, []).append(c)
    for crop, cases in sorted(by_crop.items()):
        srcs = [K.source(c.src) for c in cases]
        offsets = np.concatenate([[0], np.cumsum([s.size for s in srcs])]).astype(np.int64)
        packed = torch.from_numpy(np.concatenate([s.reshape(-1) for s in srcs])).cuda()
        got = align.kitti_align(packed, torch.from_numpy(offsets[:-1].copy()).cuda(),
                                torch.from_numpy(np.stack([K.params(c) for c in cases])).cuda(), (crop, crop)).cpu().numpy()
        for j, c in enumerate(cases):
            assert np.array_equal(got[j], K.expected(c)), c.name


# ---- end to end ------------------------------------------------------------------------------------------------------------
def epoch(it):
    out = []
    for b in it:
        row = {}
        for f in FIELDS:
            v = getattr(b, f)
            row[f] = [t.cpu() for t in v] if isinstance(v, (list, tuple)) else v.cpu()
        row["indices"] = list(b.indices)
        out.append(row)
    return out


def assert_same(got, want):
    assert len(got) == len(want) > 0
    for g, w in zip(got, want):
        assert g["indices"] == w["indices"]
        for f in FIELDS:
            if isinstance(w[f], list):
                assert len(g[f]) == len(w[f]) and all(torch.equal(a, b) for a, b in zip(g[f], w[f])), f
            else:
                assert g[f].dtype == w[f].dtype and torch.equal(g[f], w[f]), f


def remove_images(root):
    n = 0
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith(".png"):
                os.remove(os.path.join(d, f))
                n += 1
    return n


def twins(tmp_path, test, **kw):
    """(plain device_align index on one tree, cache_maps index on an identical tree of its own)."""
    out = []
    for sub, extra in (("plain", {}), ("cached", {"cache_maps": True})):
        root = str(tmp_path / sub)
        os.makedirs(root)
        train_file, test_file, names = make_kitti_tree(root)
        out.append(DS.KITTIPairs(root, test_file if test else train_file, 20, 20, 10, test=test, rng=np.random.default_rng(11),
                                 device_align=True, **extra))
    return out


KW = dict(device="cuda", workers=2, grd_hw=(64, 208), n_bins=16)
MAP, GRD = 640 * 640 * 3, 64 * 208 * 3


@pytest.mark.parametrize("test", [False, True], ids=["train", "test"])
def test_two_epochs_equal_the_plain_path_and_the_second_opens_no_image(tmp_path, test):
    plain, ds = twins(tmp_path, test)
    order = np.array([0, 1, 0, 2, 3, 1])                         # a file twice in one batch, and again in a later batch
    want = [epoch(DS.DeviceBatches(plain, 3, indices=order, **KW)) for _ in range(2)]
    assert want[0][0]["sat"].std() > 0.5                         # an aerial image, not fill
    if not test:
        assert not torch.equal(want[0][0]["sat"], want[1][0]["sat"])         # the draw changes per epoch, the map does not
    cache = C.DeviceImageCache("cuda", 32 << 20, chunk_bytes=2 * MAP)        # several chunks of maps
    it = DS.DeviceBatches(ds, 3, indices=order, cache=cache, **KW)
    assert_same(epoch(it), want[0])
    assert cache.entries == 8 and cache.bytes_used == 4 * MAP + 4 * GRD and not cache.full       # every file retained once
    hits, misses = cache.hits, cache.misses
    assert hits + misses == 12
    assert remove_images(ds.root) == 8                           # every map and every camera image of the cached twin
    assert_same(epoch(it), want[1])
    assert cache.misses == misses and cache.hits == hits + 12    # both sides of every sample
    assert cache.entries == 8
    with pytest.raises(ValueError):
        DS.DeviceBatches(ds, 3, cache=cache, sat_hw=(256, 256), **KW)


def test_cache_too_small_for_the_maps(tmp_path):
    """Room for the four camera images and TWO maps: maps 0 and 1 are retained, 2 and 3 are read from the staged upload each epoch."""
    plain, ds = twins(tmp_path, False)
    want = [epoch(DS.DeviceBatches(plain, 3, **KW)) for _ in range(2)]
    cache = C.DeviceImageCache("cuda", 4 * GRD + 2 * MAP + MAP // 2, chunk_bytes=4 * GRD)
    it = DS.DeviceBatches(ds, 3, cache=cache, **KW)
    assert_same(epoch(it), want[0])
    assert cache.full and cache.entries == 6 and cache.bytes_allocated <= cache.capacity_bytes
    assert (cache.hits, cache.misses) == (0, 8)
    assert_same(epoch(it), want[1])
    assert cache.entries == 6 and (cache.hits, cache.misses) == (6, 10) and cache.bytes_allocated <= cache.capacity_bytes
    names = [ln for ln in ds.lines]
    for n in names[:2]:                                          # the retained maps are not opened again
        os.remove(ds.paths(n)[0])
    epoch(it)
    os.remove(ds.paths(names[2])[0])                             # the overflow IS decoded again: loud when its file is gone
    with pytest.raises(OSError):
        epoch(it)
