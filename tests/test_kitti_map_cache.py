"""Device-resident KITTI aerial maps, host half (no GPU): `align.align_norm_spec` — the written specification of
ccvpe_kitti_align_norm_u8_f32 — against LIVE Pillow followed by the gather's fp32 normalisation, the raw (unresized) slots of
DeviceImageCache on device="cpu" (no kernel runs there), and KITTIPairs(cache_maps=True): `keys()` names the map,
`sample(cached={"sat_src": hw})` opens no map file and builds the same row."""
import os

import numpy as np
import pytest

import kitti_align_cases as K
from ccvpe_amd import align, cache as C, datasets as DS
from test_datasets import make_kitti_tree


def test_align_norm_spec_is_pillow_then_the_gather_normalisation():
    K.check_inputs_are_visible(K.CASES)
    for c in K.CASES:
        got = align.align_norm_spec([K.source(c.src)], [K.params(c)], c.crop)
        want = C.gather_spec([K.expected(c)], [0])
        assert got.dtype == np.float32 and got.shape == (1, 3, c.crop, c.crop)
        assert np.array_equal(got, want), "%s: %d of %d values differ" % (c.name, int((got != want).sum()), want.size)


def test_align_norm_spec_batches_repeats_and_the_zero_row():
    a, b = K.CASES[11], K.CASES[12]                              # two cases of one source and crop
    assert a.src == b.src and a.crop == b.crop
    src = K.source(a.src)
    got = align.align_norm_spec([src, None, src], [K.params(a), K.params(b), K.params(b)], a.crop, mean=(0.5, 0.25, 0.0), std=(0.5, 1.0, 2.0))
    assert np.array_equal(got[0], C.gather_spec([K.expected(a)], [0], mean=(0.5, 0.25, 0.0), std=(0.5, 1.0, 2.0))[0])
    assert np.array_equal(got[2], C.gather_spec([K.expected(b)], [0], mean=(0.5, 0.25, 0.0), std=(0.5, 1.0, 2.0))[0])
    for ch, v in enumerate((-1.0, -0.25, 0.0)):                  # a row without a source: the normalised zero byte
        assert (got[1, ch] == np.float32(v)).all()
    assert align.align_norm_spec([], [], (40, 72)).shape == (0, 3, 40, 72)


class FakeImage(object):
    """What insert_raw() reads of a decoded image on device="cpu": its shape."""

    def __init__(self, h, w):
        self.shape = (h, w, 3)


def test_raw_slots_two_shapes_duplicates_and_full():
    a, b = 7 * 9 * 3, 5 * 5 * 3
    c = C.DeviceImageCache("cpu", capacity_bytes=2 * a + b + b // 2, chunk_bytes=1)      # one slot per chunk
    got = [c.insert_raw("a0", FakeImage(7, 9)), c.insert_raw("b0", FakeImage(5, 5)), c.insert_raw("a1", FakeImage(7, 9))]
    assert None not in got and len(set(got)) == 3 and not c.full
    assert c.entries == 3 and c.bytes_used == c.bytes_allocated == 2 * a + b <= c.capacity_bytes
    # the same key again: a no-op that returns the stored address, whatever image comes with it
    assert c.insert_raw("a0", FakeImage(3, 3)) == got[0] and c.entries == 3 and c.bytes_used == 2 * a + b
    # lookup / address work unchanged and give the raw size
    assert c.lookup("a1") == (got[2], (7, 9)) and c.lookup("b0") == (got[1], (5, 5)) and c.hits == 2
    assert c.address("b0") == got[1] and c.resized_hw("a0") == (7, 9)
    # no room for another map of either shape: not retained, `full` turns true, nothing is allocated
    assert c.insert_raw("b1", FakeImage(5, 5)) is None
    assert c.full and c.entries == 3 and c.bytes_allocated == 2 * a + b <= c.capacity_bytes
    assert c.lookup("b1") is None and c.misses == 1 and c.address("b1") is None
    with pytest.raises(ValueError):
        c.insert_raw("x", FakeImage(0, 4))
    c.clear()
    assert (c.entries, c.bytes_used, c.bytes_allocated, c.full) == (0, 0, 0, False)


def test_raw_and_resized_entries_share_chunk_accounting_and_never_collide():
    path = "/data/satmap/drive/0000000000.png"
    resized_key = "%s|%dx%d" % (path, 4, 6)                     # DeviceBatches._cache_key
    raw_key = C.DeviceImageCache.raw_key(path)
    assert raw_key != resized_key and raw_key != path
    assert raw_key != "%s|%dx%d" % (path, 8, 8) and "|" in raw_key
    c = C.DeviceImageCache("cpu", capacity_bytes=1 << 20, chunk_bytes=4 * 4 * 6 * 3)
    r = c.insert(resized_key, FakeImage(8, 8), (4, 6))
    w = c.insert_raw(raw_key, FakeImage(8, 8))
    assert r is not None and w is not None and r != w and c.entries == 2
    assert c.lookup(resized_key) == (r, (8, 8)) and c.lookup(raw_key) == (w, (8, 8))
    assert c.resized_hw(resized_key) == (4, 6) and c.resized_hw(raw_key) == (8, 8)
    assert c.bytes_used == 4 * 6 * 3 + 8 * 8 * 3 <= c.bytes_allocated <= c.capacity_bytes
    # a raw map whose shape equals a resized shape takes the next slot of that shape's chunk
    w2 = c.insert_raw(C.DeviceImageCache.raw_key("other.png"), FakeImage(4, 6))
    assert w2 - r == 4 * 6 * 3


def test_kitti_keys_name_the_map_only_with_cache_maps(tmp_path):
    train_file, test_file, names = make_kitti_tree(str(tmp_path))
    with pytest.raises(ValueError):
        DS.KITTIPairs(str(tmp_path), train_file, cache_maps=True, device_align=False)
    with pytest.raises(ValueError):
        DS.KITTIPairs(str(tmp_path), train_file, cache_maps=True)
    for file, test in ((train_file, False), (test_file, True)):
        plain = DS.KITTIPairs(str(tmp_path), file, 20, 20, 10, test=test, rng=np.random.default_rng(1), device_align=True)
        ds = DS.KITTIPairs(str(tmp_path), file, 20, 20, 10, test=test, rng=np.random.default_rng(1), device_align=True, cache_maps=True)
        assert plain.cache_maps is False and ds.cache_maps is True
        for i, n in enumerate(names):
            sat, _, grd = ds.paths(n)
            assert plain.keys(i, None) == {"grd": grd, "sat": None}                       # today's, exactly
            assert ds.keys(i, None) == {"grd": grd, "sat": None, "sat_src": sat}


@pytest.mark.parametrize("test", [False, True])
def test_cached_map_is_not_opened_and_the_row_is_the_same(tmp_path, test):
    root, twin_root = str(tmp_path / "a"), str(tmp_path / "b")
    os.makedirs(root), os.makedirs(twin_root)
    files = make_kitti_tree(root)
    twin_files = make_kitti_tree(twin_root)                      # same seed: the same tree
    mk = lambda r, f: DS.KITTIPairs(r, f[1 if test else 0], 20, 20, 10, test=test, rng=np.random.default_rng(3), device_align=True,
                                    cache_maps=True)
    ds, twin = mk(root, files), mk(twin_root, twin_files)
    for n in files[2]:
        os.remove(ds.paths(n)[0])                                # every map PNG of the cached twin
    rows = []
    for i in range(len(ds)):
        s = ds.sample(i, cached={"sat_src": (640, 640)})         # draws from its own generator, as the undeleted twin does
        want = twin.sample(i)
        assert s["sat_src_u8"] is None and want["sat_src_u8"].shape == (640, 640, 3)
        assert s["align"].dtype == np.int64 and np.array_equal(s["align"], want["align"])
        assert s["grd_u8"] is not None and np.array_equal(s["grd_u8"], want["grd_u8"])
        for k in ("center", "angle_deg", "city", "index", "roll"):
            assert s[k] == want[k], k
        assert set(s) == set(want)
        rows.append(s["align"])
    assert len({r.tobytes() for r in rows}) == len(rows)         # the heading (OXTS file) and the draw still reach the row
    # both sides cached: only the OXTS record is read; a non-square cached size reaches the row
    s = ds.sample(0, cached={"sat_src": (600, 700), "grd": (94, 310)})
    assert s["grd_u8"] is None and s["sat_src_u8"] is None and tuple(s["align"][16:20]) == (700, 600, 94, 44)
    with pytest.raises(ValueError):
        ds.sample(0, cached={"sat_src": (640, 500)})             # smaller than the crop: refused as after a decode
    with pytest.raises(OSError):
        ds.sample(0, cached={})                                  # not cached: the map is decoded, and is gone
    # without cache_maps the mapping's "sat_src" means nothing: the map is opened as today
    plain = DS.KITTIPairs(root, files[1 if test else 0], 20, 20, 10, test=test, device_align=True)
    with pytest.raises(OSError):
        plain.sample(0, cached={"sat_src": (640, 640)})
