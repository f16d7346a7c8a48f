"""Device-resident Oxford aerial map on the MI355X: ccvpe_window_resize_norm_u8_f32 against its numpy specification (which
test_oxford_map.py pins to live Pillow) on every case of the table — torch.equal, no tolerance, no excluded element — 64-bit
map offsets on a 2.7 GB map, and DeviceBatches(OxfordPairs(device_map=True)) against the host-crop path batch by batch."""
import functools
import os
import random

import numpy as np
import pytest
import torch

import oxford_map_cases as K
from ccvpe_amd import cache as C, datasets as DS, preprocess
from test_datasets import make_oxford_tree

pytestmark = pytest.mark.gpu

MEAN, STD = preprocess.IMAGENET_MEAN, preprocess.IMAGENET_STD
BY_NAME = {c.name: c for c in K.CASES}


@functools.lru_cache(maxsize=None)
def spec_of(name):
    case = BY_NAME[name]
    return preprocess.window_resize_spec(K.case_map(case), case.origins, case.box_hw, case.out_hw, MEAN, STD)


def run(map_u8, origins, box_hw, out_hw, **kw):
    o = torch.tensor(origins, dtype=torch.int32, device="cuda").reshape(-1, 2)
    out = preprocess.window_resize_norm(map_u8, o, box_hw, out_hw, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", [c.name for c in K.CASES])
def test_kernel_equals_the_specification(name):
    case = BY_NAME[name]
    m = K.case_map(case)
    got = run(torch.from_numpy(m).cuda(), case.origins, case.box_hw, case.out_hw)
    want = torch.from_numpy(spec_of(name))
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape)
    got = got.cpu()
    assert torch.equal(got, want), "%s: %d of %d values differ" % (name, int((got != want).sum()), want.numel())


def test_workload_geometry_equals_preprocess_of_the_uploaded_pillow_crop():
    case = BY_NAME["workload"]
    m = K.case_map(case)
    crops, _ = K.pillow_windows(m, case)
    got = run(torch.from_numpy(m).cuda(), case.origins, case.box_hw, case.out_hw)
    for b in range(len(case.origins)):
        want = preprocess.preprocess(torch.from_numpy(crops[b]).cuda(), case.out_hw)
        assert torch.equal(got[b], want), b


def test_writes_into_a_given_batch_and_takes_other_statistics():
    case = BY_NAME["ragged_29x37"]
    m = K.case_map(case)
    mean, std = (0.5, 0.25, 0.125), (0.5, 2.0, 0.3)
    dst = torch.full((len(case.origins), 3) + case.out_hw, float("nan"), device="cuda")
    assert run(torch.from_numpy(m).cuda(), case.origins, case.box_hw, case.out_hw, dst=dst, mean=mean, std=std) is dst
    want = preprocess.window_resize_spec(m, case.origins, case.box_hw, case.out_hw, mean, std)
    assert torch.equal(dst.cpu(), torch.from_numpy(want))
    empty = run(torch.from_numpy(m).cuda(), np.zeros((0, 2)), case.box_hw, case.out_hw)
    assert tuple(empty.shape) == (0, 3) + case.out_hw
    with pytest.raises(ValueError):
        run(torch.from_numpy(m).cuda(), case.origins, case.box_hw, case.out_hw, dst=dst[:1])


def test_map_offsets_are_64_bit():
    """A 30000 x 30000 x 3 byte map (2.7 GB): only its last 900 rows x 900 columns hold data, 2.6e9 bytes into the buffer —
    one window inside that corner, one across the map's bottom-right edge.  The specification runs on the corner alone."""
    n, c = 30000, 900
    corner = np.random.RandomState(77).randint(0, 256, size=(c, c, 3)).astype(np.uint8)
    big = torch.zeros((n, n, 3), dtype=torch.uint8, device="cuda")
    big[n - c:, n - c:] = torch.from_numpy(corner).cuda()
    local = ((50, 70), (400, 600))                                 # (x0, y0) inside the corner; 400 + 800 > 900: across the edge
    got = run(big, [(x + n - c, y + n - c) for x, y in local], (800, 800), (512, 512)).cpu()
    del big
    want = torch.from_numpy(preprocess.window_resize_spec(corner, local, (800, 800), (512, 512), MEAN, STD))
    assert torch.equal(got, want), "%d values differ" % int((got != want).sum())
    zero = (np.float32(0.0) - np.float32(MEAN[0])) / np.float32(STD[0])
    assert float(got[1, 0, -1, -1]) == float(zero) and got[0].unique().numel() > 300


# ---- through the loader -------------------------------------------------------------------------------------------------
FIELDS = ("grd", "sat", "center", "angle_deg", "heading_deg", "gt", "gt_flat", "gt_ori", "labels")
KW = dict(device="cuda", workers=2, grd_hw=(154, 231), n_bins=20, ascending_bins=True)


def epoch(it):
    out = []
    for b in it:
        row = {}
        for f in FIELDS:
            v = getattr(b, f)
            row[f] = None if v is None else [t.cpu() for t in v] if isinstance(v, (list, tuple)) else v.cpu()
        row["indices"] = list(b.indices)
        out.append(row)
    return out


def assert_same(got, want):
    assert len(got) == len(want) > 0
    for g, w in zip(got, want):
        assert g["indices"] == w["indices"]
        for f in FIELDS:
            if w[f] is None:
                assert g[f] is None, f
            elif isinstance(w[f], list):
                assert len(g[f]) == len(w[f]) and all(torch.equal(a, b) for a, b in zip(g[f], w[f])), f
            else:
                assert g[f].dtype == w[f].dtype and torch.equal(g[f], w[f]), f


def pairs(tree, split, device_map, seed=5):
    g, sat_path = tree
    return DS.OxfordPairs(g, sat_path, split=split, rng=random.Random(seed), device_map=device_map)


@pytest.fixture(scope="module")
def oxford_tree(tmp_path_factory):
    return make_oxford_tree(str(tmp_path_factory.mktemp("oxford_map_gpu")))


@pytest.mark.parametrize("split", ["train", "val", "test"])
def test_loader_equals_the_host_crop_path(oxford_tree, split):
    want = epoch(DS.DeviceBatches(pairs(oxford_tree, split, False), 4, **KW))
    ds = pairs(oxford_tree, split, True)
    got = epoch(DS.DeviceBatches(ds, 4, **KW))
    assert_same(got, want)
    assert sum(len(r["indices"]) for r in got) == len(ds) and got[0]["sat"].shape[1:] == (3, 512, 512)
    resident = ds.map_on("cuda")
    assert resident is ds.map_on(torch.device("cuda", torch.cuda.current_device()))        # uploaded once per device
    assert resident.dtype == torch.uint8 and tuple(resident.shape) == (2800, 2600, 3)


@pytest.mark.parametrize("split", ["train", "test"])
def test_loader_with_a_ground_cache_second_epoch_without_camera_files(tmp_path, split):
    tree = make_oxford_tree(str(tmp_path))
    host = DS.DeviceBatches(pairs(tree, split, False), 4, **KW)
    want = [epoch(host), epoch(host)]                               # training: the second epoch's draws differ from the first's
    ds = pairs(tree, split, True)
    cache = C.DeviceImageCache("cuda", 64 << 20, chunk_bytes=4 << 20)

    def no_scratch(*a, **k):
        raise AssertionError("the aerial side must not take a scratch slot")

    cache.scratch = no_scratch
    it = DS.DeviceBatches(ds, 4, cache=cache, **KW)
    assert_same(epoch(it), want[0])
    assert (cache.entries, cache.hits, cache.misses) == (len(ds), 0, len(ds))       # the camera images and nothing else
    n = 0
    for f in os.listdir(tree[0]):
        if f.endswith(".png"):
            os.remove(os.path.join(tree[0], f))
            n += 1
    assert n >= len(ds)
    assert_same(epoch(it), want[1])
    assert (cache.entries, cache.hits, cache.misses) == (len(ds), len(ds), len(ds))


def test_loader_windows_across_the_right_and_bottom_edges(oxford_tree, tmp_path):
    """The map cropped to 1900 x 1950: the vehicles sit at columns 1500-1820 and rows 1550-1870, so training windows (and the
    grid patches at 1200 / 1600 + 800) reach past the right and bottom edges."""
    from PIL import Image
    g, sat_path = oxford_tree
    small = str(tmp_path / "satellite_map_small.png")
    with Image.open(sat_path) as im:
        im.crop((0, 0, 1900, 1950)).save(small)
    crossed = 0
    for split in ("train", "val"):
        probe = DS.OxfordPairs(g, small, split=split, rng=random.Random(5), device_map=True)
        for i in range(len(probe)):
            x0, y0 = probe.sample(i)["sat_origin"]
            crossed += x0 + 800 > 1900 or y0 + 800 > 1950
        want = epoch(DS.DeviceBatches(DS.OxfordPairs(g, small, split=split, rng=random.Random(5)), 4, **KW))
        got = epoch(DS.DeviceBatches(DS.OxfordPairs(g, small, split=split, rng=random.Random(5), device_map=True), 4, **KW))
        assert_same(got, want)
    assert crossed >= 3


def test_loader_with_another_aerial_size(oxford_tree):
    kw = dict(KW, sat_hw=(256, 256))
    want = epoch(DS.DeviceBatches(pairs(oxford_tree, "train", False), 4, **kw))
    got = epoch(DS.DeviceBatches(pairs(oxford_tree, "train", True), 4, **kw))
    assert_same(got, want)
    assert got[0]["sat"].shape[1:] == (3, 256, 256)
