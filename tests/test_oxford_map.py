"""Device-resident Oxford aerial map, host side: the numpy specification of ccvpe_window_resize_norm_u8_f32 against LIVE
Pillow (equal bits on every case), OxfordPairs(device_map=True) against its device_map=False twin, the map modes, and the C
entry point's argument checks (no device needed)."""
import ctypes
import random

import numpy as np
import pytest

import oxford_map_cases as K
from ccvpe_amd import datasets as DS
from ccvpe_amd import preprocess
from test_datasets import make_oxford_tree

MEAN, STD = preprocess.IMAGENET_MEAN, preprocess.IMAGENET_STD


def test_case_table_covers_what_it_claims():
    names = {c.name for c in K.CASES}
    assert len(names) == len(K.CASES)
    assert any(c.map_hw == (1000, 900) and c.box_hw == (800, 800) and c.out_hw == (512, 512) and (-37, -5) in c.origins
               for c in K.CASES)
    assert any(c.box_hw == (45, 70) and c.out_hw == (29, 37) for c in K.CASES)
    assert any(c.box_hw[0] > c.out_hw[0] and c.box_hw[1] < c.out_hw[1] for c in K.CASES)
    ks = {preprocess.resample_tables(c.box_hw[0], c.out_hw[0])[2] for c in K.CASES}
    assert {3, 5, 9} <= ks
    assert any(len(c.origins) == 1 for c in K.CASES) and any(len(c.origins) == 5 and len(set(c.origins)) < 5 for c in K.CASES)
    assert any(c.out_hw[1] % 4 for c in K.CASES) and any(c.out_hw[1] % 4 and c.out_hw[1] > 128 for c in K.CASES)
    for c in K.CASES:                                   # x0 + box_w == map_w exactly, and a window wholly outside
        if c.name == "borders":
            assert any(x0 + c.box_hw[1] == c.map_hw[1] for x0, _ in c.origins)
            assert any(x0 >= c.map_hw[1] or x0 + c.box_hw[1] <= 0 or y0 >= c.map_hw[0] or y0 + c.box_hw[0] <= 0
                       for x0, y0 in c.origins)


@pytest.mark.parametrize("case", K.CASES, ids=[c.name for c in K.CASES])
def test_spec_equals_live_pillow(case):
    m = K.case_map(case)
    _, resized = K.pillow_windows(m, case)
    want = K.normalise(resized, MEAN, STD)
    got = preprocess.window_resize_spec(m, case.origins, case.box_hw, case.out_hw, MEAN, STD)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got, want), "%s: %d of %d values differ" % (case.name, int((got != want).sum()), want.size)


def test_spec_of_a_window_wholly_outside_is_the_normalised_zero():
    case = next(c for c in K.CASES if c.name == "borders")
    got = preprocess.window_resize_spec(K.case_map(case), [(500, -900)], case.box_hw, case.out_hw, MEAN, STD)
    zero = (np.float32(0.0) - np.asarray(MEAN, np.float32)) / np.asarray(STD, np.float32)
    assert all(np.array_equal(got[0, c], np.full(case.out_hw, zero[c], np.float32)) for c in range(3))


# ---- the loader ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oxford_tree(tmp_path_factory):
    return make_oxford_tree(str(tmp_path_factory.mktemp("oxford_map")))


def _origin_of(pairs, idx, draws):
    """The host path's box origin, restated: datasets.py:296-330 through OxfordPairs' own helpers."""
    col, row = pairs._position(idx)
    if pairs.split == "train":
        drow, dcol = draws
        return int(col + dcol) - 400, int(row + drow) - 400
    return pairs._grid(col)[0] * 400, pairs._grid(row)[0] * 400


@pytest.mark.parametrize("split", ["train", "val", "test"])
def test_device_map_sample_equals_host_sample(oxford_tree, split):
    g, sat_path = oxford_tree
    host = DS.OxfordPairs(g, sat_path, split=split, rng=random.Random(21))
    dev = DS.OxfordPairs(g, sat_path, split=split, rng=random.Random(21), device_map=True)
    probe = random.Random(21)                                  # a third generator in step: the draws themselves
    rgb = dev.map_rgb()
    assert rgb.dtype == np.uint8 and rgb.shape == (2800, 2600, 3)
    for i in list(range(len(host))) + [1, 0]:
        a, b = dev.sample(i), host.sample(i)
        assert list(b) == ["grd_u8", "sat_u8", "roll", "angle_deg", "center", "city", "index"]          # the default dict is unchanged
        assert list(a) == list(b) + ["sat_origin"] and a["sat_u8"] is None
        for k in b:
            if k == "sat_u8":
                continue
            if isinstance(b[k], np.ndarray):
                assert np.array_equal(a[k], b[k]), k
            else:
                assert a[k] == b[k] and type(a[k]) is type(b[k]), k
        draws = None
        if split == "train":                                    # offset(): two draws, alpha then r
            import math
            alpha, r = 2 * math.pi * probe.random(), 200 * np.sqrt(2) * probe.random()
            draws = (int(r * math.cos(alpha)), int(r * math.sin(alpha)))
        x0, y0 = a["sat_origin"]
        assert (x0, y0) == _origin_of(host, i, draws) and type(x0) is int and type(y0) is int
        # the window of the RGB map at that origin is the host path's patch
        win = rgb[y0:y0 + 800, x0:x0 + 800]
        assert win.shape == (800, 800, 3) and np.array_equal(win, b["sat_u8"])
        assert dev.keys(i, draws)["sat"] is None and dev.keys(i, draws)["grd"] == host.keys(i, draws)["grd"]
    assert host._rng.random() == dev._rng.random()                # both generators advanced by the same number of draws
    # draws handed in (as DeviceBatches does) are used as they are
    if split == "train":
        a, b = dev.sample(2, draws=(-150, 77)), host.sample(2, draws=(-150, 77))
        assert a["sat_origin"] == _origin_of(host, 2, (-150, 77)) and a["center"] == b["center"]
        x0, y0 = a["sat_origin"]
        assert np.array_equal(rgb[y0:y0 + 800, x0:x0 + 800], b["sat_u8"])
    assert host.keys(0, None)["sat"] is None if split == "train" else host.keys(0, None)["sat"] is not None


def _zero_filled(rgb, x0, y0, bh, bw):
    win = np.zeros((bh, bw, 3), np.uint8)
    ys, ye, xs, xe = max(y0, 0), min(y0 + bh, rgb.shape[0]), max(x0, 0), min(x0 + bw, rgb.shape[1])
    if ys < ye and xs < xe:
        win[ys - y0:ye - y0, xs - x0:xe - x0] = rgb[ys:ye, xs:xe]
    return win


def test_map_modes(oxford_tree, tmp_path):
    """P raises; L and RGBA give the windows of their RGB conversion — also across the map's border, where Pillow's crop fills
    with the mode's zero."""
    from PIL import Image
    g, sat_path = oxford_tree
    with Image.open(sat_path) as im:
        small = im.crop((0, 0, 1500, 1600))                     # the vehicles (columns ~1500-1820) make windows cross its edges
        small.load()
    rng = np.random.RandomState(3)
    alpha = Image.fromarray(rng.randint(0, 256, size=(1600, 1500)).astype(np.uint8), "L")
    rgba = small.copy()
    rgba.putalpha(alpha)
    variants = {"L": small.convert("L"), "RGBA": rgba}
    for mode, im in variants.items():
        path = str(tmp_path / ("map_%s.png" % mode))
        im.save(path)
        host = DS.OxfordPairs(g, path, split="train", rng=random.Random(2))
        dev = DS.OxfordPairs(g, path, split="train", rng=random.Random(2), device_map=True)
        assert dev.map.mode == mode
        rgb = dev.map_rgb()
        assert np.array_equal(rgb, np.array(im.convert("RGB")))
        crossed = 0
        for i in range(len(host)):
            a, b = dev.sample(i), host.sample(i)
            x0, y0 = a["sat_origin"]
            crossed += x0 + 800 > 1500 or y0 + 800 > 1600
            assert np.array_equal(_zero_filled(rgb, x0, y0, 800, 800), b["sat_u8"]), (mode, i)
        assert crossed
    path = str(tmp_path / "map_P.png")
    small.convert("P").save(path)
    assert DS.OxfordPairs(g, path, split="val").map.mode == "P"          # the default path takes it as before
    with pytest.raises(ValueError, match="mode"):
        DS.OxfordPairs(g, path, split="val", device_map=True)


# ---- the C entry point's checks (host only: nothing is enqueued) ------------------------------------------------------------
def _call(lib, map_=256, map_h=100, map_w=100, origins=256, batch=1, box=(800, 800), xb=256, xc=256, xk=5, yb=256, yc=256,
          yk=5, mean=MEAN, std=STD, dst=256, out=(512, 512)):
    m = None if mean is None else (ctypes.c_float * 3)(*mean)
    s = None if std is None else (ctypes.c_float * 3)(*std)
    return lib.ccvpe_window_resize_norm_u8_f32(map_, map_h, map_w, origins, batch, box[0], box[1], xb, xc, xk, yb, yc, yk, m, s,
                                               dst, out[0], out[1], None)


def test_c_entry_validates_before_launching():
    """Bad shapes, null pointers and unsupported geometries come back as CCVPE_EINVAL with a message; an empty batch succeeds
    even with null tables.  Every pointer here is a small integer that a launch would fault on: nothing is enqueued."""
    from ccvpe_amd import _lib
    lib = _lib.load()
    for null in ("map_", "origins", "xb", "xc", "yb", "yc", "dst", "mean", "std"):
        assert _call(lib, **{null: None}) == -1 and b"null pointer" in lib.ccvpe_last_error(), null
    assert _call(lib, batch=0) == 0
    assert _call(lib, batch=0, map_=None, origins=None, xb=None, xc=None, yb=None, yc=None, dst=None) == 0
    for bad in (dict(batch=-1), dict(batch=65536), dict(map_h=0), dict(map_w=-3), dict(box=(0, 800)), dict(box=(800, -1)),
                dict(out=(0, 512)), dict(out=(512, 0))):
        assert _call(lib, **bad) == -1 and b"bad shape" in lib.ccvpe_last_error(), bad
    # tables that are not Pillow's for the geometry (ksize 5 is 800 -> 512's)
    assert _call(lib, xk=3) == -1 and b"ksize" in lib.ccvpe_last_error()
    assert _call(lib, yk=0) == -1 and b"ksize" in lib.ccvpe_last_error()
    assert _call(lib, box=(128, 128), out=(32, 32)) == -1 and b"ksize" in lib.ccvpe_last_error()
    # a vertical reduction whose staged tile is above 64 KB of LDS: 15 * 12 + 25 + 1 = 206 rows of 384 bytes
    assert _call(lib, box=(6144, 800), out=(512, 512), yk=25) == -1 and b"unsupported geometry" in lib.ccvpe_last_error()


def test_wrapper_has_no_cpu_path():
    import torch
    with pytest.raises(ValueError, match="device tensor"):
        preprocess.window_resize_norm(torch.zeros((8, 8, 3), dtype=torch.uint8), torch.zeros((1, 2), dtype=torch.int32), (4, 4),
                                      (4, 4))
