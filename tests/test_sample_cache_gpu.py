"""Device image cache on the MI355X: ccvpe_gather_norm_u8_f32 against its numpy specification (`cache.gather_spec`), ccvpe_resize_u8
against live Pillow — both bit for bit — and DeviceBatches with a cache against DeviceBatches without one: identical batches in
the first epoch (the fill) and in the second (all hits, the image files DELETED), with a cache too small for the set, and for
the KITTI and Oxford loaders."""
import ctypes
import os

import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, cache as C, datasets as DS, preprocess
from test_datasets import make_kitti_tree, make_oxford_tree, make_vigor_tree

pytestmark = pytest.mark.gpu

MEAN, STD = preprocess.IMAGENET_MEAN, preprocess.IMAGENET_STD
FIELDS = ("grd", "sat", "gt", "gt_ori", "center", "angle_deg", "heading_deg", "labels")
EINVAL = -1


def run_gather(chunks, order, rolls, hw, keep_w):
    """chunks: uint8 numpy arrays [n_k, h, w, 3]; image i of their concatenation is addressed inside ITS chunk's device tensor."""
    h, w = hw
    dev = [torch.from_numpy(c).cuda() for c in chunks]
    addr = [t.data_ptr() + j * h * w * 3 for t in dev for j in range(t.shape[0])]
    table = torch.tensor([addr[i] for i in order], dtype=torch.int64, device="cuda")
    got = preprocess.gather_norm(table, torch.tensor(rolls, dtype=torch.int32, device="cuda"), hw, keep_w=keep_w)
    torch.cuda.synchronize()
    imgs = np.concatenate(chunks)
    return got.cpu().numpy(), C.gather_spec([imgs[i] for i in order], rolls, keep_w, MEAN, STD)


@pytest.mark.parametrize("keep_w,split", [(8, (5,)), (8, (3, 2)), (7, (5,)), (10, (5,))],
                         ids=["vec_one_chunk", "vec_two_chunks", "scalar_7", "scalar_10"])
def test_gather_small_images_vector_and_scalar_forms(keep_w, split):
    """keep_w = 8: four columns per lane, and with w = 10 the wrap of rolls 3 / -13 falls inside a group; 7 and 10: the scalar
    form (10 % 4 != 0).  Row 1 and row 2 read the same source."""
    imgs = np.random.RandomState(11).randint(0, 256, size=(5, 6, 10, 3)).astype(np.uint8)
    chunks = [imgs[sum(split[:k]):sum(split[:k + 1])].copy() for k in range(len(split))]
    got, want = run_gather(chunks, [4, 0, 0, 2], [0, 3, -13, 10], (6, 10), keep_w)
    assert got.shape == (4, 3, 6, keep_w) and np.array_equal(got, want)


def test_gather_single_group_and_model_shapes():
    rng = np.random.RandomState(12)
    for n, hw, keep_w, order, rolls in ((1, (3, 4), 4, [0], [5]),
                                        (1, (320, 640), 320, [0], [417]),
                                        (2, (512, 512), 512, [0, 1], [0, 0])):
        imgs = rng.randint(0, 256, size=(n,) + hw + (3,)).astype(np.uint8)
        got, want = run_gather([imgs], order, rolls, hw, keep_w)
        assert np.array_equal(got, want), "%r keep %d" % (hw, keep_w)


def test_gather_argument_checks():
    lib = _lib.load()
    m, s = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    img = torch.zeros((6, 10, 3), dtype=torch.uint8, device="cuda")
    table = torch.tensor([img.data_ptr()], dtype=torch.int64, device="cuda")
    rolls = torch.zeros((1,), dtype=torch.int32, device="cuda")
    dst = torch.empty((1, 3, 6, 10), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    good = (table.data_ptr(), rolls.data_ptr(), 1, 6, 10, 10, m, s, dst.data_ptr(), st)
    assert lib.ccvpe_gather_norm_u8_f32(*good) == 0
    assert lib.ccvpe_gather_norm_u8_f32(table.data_ptr(), rolls.data_ptr(), 0, 6, 10, 10, m, s, dst.data_ptr(), st) == 0
    assert lib.ccvpe_gather_norm_u8_f32(None, None, 0, 6, 10, 10, m, s, None, st) == 0       # an empty batch: no launch, no tables
    assert lib.ccvpe_gather_norm_u8_f32(table.data_ptr(), rolls.data_ptr(), 1, 6, 10, 11, m, s, dst.data_ptr(), st) == EINVAL
    assert b"gather_norm" in lib.ccvpe_last_error()
    for k in (0, 1, 6, 7, 8):                                   # each pointer in turn
        bad = list(good)
        bad[k] = None
        assert lib.ccvpe_gather_norm_u8_f32(*bad) == EINVAL, k
        assert b"null" in lib.ccvpe_last_error()
    for k in (3, 4, 5):                                         # h, w, keep_w
        bad = list(good)
        bad[k] = 0
        assert lib.ccvpe_gather_norm_u8_f32(*bad) == EINVAL, k
    assert lib.ccvpe_gather_norm_u8_f32(table.data_ptr(), rolls.data_ptr(), -1, 6, 10, 10, m, s, dst.data_ptr(), st) == EINVAL
    assert lib.ccvpe_resize_u8(None, 4, 4, 256, 256, 3, 256, 256, 3, 256, 256, 2, 2, st) == EINVAL
    assert lib.ccvpe_resize_u8(256, 4, 4, 256, 256, 3, 256, 256, 3, 256, 256, 0, 2, st) == EINVAL
    torch.cuda.synchronize()


@pytest.mark.parametrize("src_hw,out_hw", [((96, 192), (40, 80)), ((64, 64), (80, 72)), ((7, 5), (3, 9))])
def test_resize_u8_equals_pillow(src_hw, out_hw):
    from PIL import Image
    img = np.random.RandomState(src_hw[0]).randint(0, 256, size=src_hw + (3,)).astype(np.uint8)
    want = np.asarray(Image.fromarray(img, "RGB").resize((out_hw[1], out_hw[0]), Image.BILINEAR))
    got = preprocess.resize_u8(torch.from_numpy(img).cuda(), out_hw)
    assert got.dtype == torch.uint8 and tuple(got.shape) == out_hw + (3,)
    assert np.array_equal(got.cpu().numpy(), want)


def epoch(it):
    """Every batch of one pass, on the host: {field: tensor, list of tensors or None} + the indices."""
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


def remove_images(root, only=None):
    n = 0
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            if f.endswith((".jpg", ".png")) and (only is None or p in only):
                os.remove(p)
                n += 1
    assert n


# sat_hw = (48, 48) cannot carry ground truth (ccvpe_train_targets_* takes multiples of 64), so those cases compare the images and
# the scalars (gt / gt_ori / labels are None on both sides); the (64, 64) case adds the ground truth.
@pytest.mark.parametrize("fov,sat_hw,targets", [(360, (48, 48), False), (100, (48, 48), False), (360, (64, 64), True)])
def test_vigor_two_epochs_with_a_cache_equal_the_uncached_batches(tmp_path, fov, sat_hw, targets):
    make_vigor_tree(str(tmp_path))
    kw = dict(device="cuda", workers=3, grd_hw=(40, 80), sat_hw=sat_hw, fov=fov, targets=targets)
    plain = DS.VIGORPairs(str(tmp_path), split="samearea", train=True, seed=4)           # random rolls, seeded
    want = [epoch(DS.DeviceBatches(plain, 4, **kw)) for _ in range(2)]       # the draws run on from epoch to epoch
    assert want[0][0]["grd"].shape[-1] == int(80 * fov / 360) and not torch.equal(want[0][0]["grd"], want[1][0]["grd"])
    ds = DS.VIGORPairs(str(tmp_path), split="samearea", train=True, seed=4)
    cache = C.DeviceImageCache("cuda", 64 << 20, chunk_bytes=5 * 40 * 80 * 3)        # several chunks per shape
    it = DS.DeviceBatches(ds, 4, cache=cache, **kw)
    assert_same(epoch(it), want[0])
    n_tiles = len({ds.sat_paths[ds.labels[i, 0]] for i in range(12)})
    assert cache.entries == 12 + n_tiles and not cache.full and cache.bytes_allocated <= cache.capacity_bytes
    hits, misses = cache.hits, cache.misses
    assert hits + misses == 24
    remove_images(str(tmp_path))
    assert_same(epoch(it), want[1])
    assert cache.misses == misses and cache.hits == hits + 24


def test_vigor_random_tile_choice_draws_in_the_same_order(tmp_path):
    """pos_only=False: the tile is a draw too, and epoch 2 may pick one epoch 1 never used — the tile files stay, every panorama
    is deleted; the batches equal the uncached ones, so the generator was consumed in the same order."""
    make_vigor_tree(str(tmp_path))
    kw = dict(device="cuda", workers=3, grd_hw=(40, 80), sat_hw=(48, 48), targets=False)
    plain = DS.VIGORPairs(str(tmp_path), split="samearea", train=True, pos_only=False, seed=4)
    want = [epoch(DS.DeviceBatches(plain, 4, **kw)) for _ in range(2)]
    ds = DS.VIGORPairs(str(tmp_path), split="samearea", train=True, pos_only=False, seed=4)
    cache = C.DeviceImageCache("cuda", 64 << 20, chunk_bytes=4 << 20)
    it = DS.DeviceBatches(ds, 4, cache=cache, **kw)
    assert_same(epoch(it), want[0])
    hits, misses, entries = cache.hits, cache.misses, cache.entries
    remove_images(str(tmp_path), only=set(ds.grd_paths))
    assert_same(epoch(it), want[1])
    assert cache.hits - hits >= 12 and (cache.hits - hits) + (cache.misses - misses) == 24
    assert cache.entries - entries <= cache.misses - misses


def test_vigor_second_epoch_runs_without_any_image_file(tmp_path):
    """pos_only: both sides of every sample are in the cache after one pass — delete every image, then pass again."""
    make_vigor_tree(str(tmp_path))
    orient = np.linspace(-400.0, 700.0, 12)                     # rolls of either sign, beyond a whole turn
    kw = dict(device="cuda", workers=3, grd_hw=(40, 80), sat_hw=(48, 48), targets=False)
    plain = DS.VIGORPairs(str(tmp_path), split="samearea", train=True, random_orientation=orient)
    want = epoch(DS.DeviceBatches(plain, 4, **kw))
    cache = C.DeviceImageCache("cuda", 64 << 20, chunk_bytes=4 << 20)
    it = DS.DeviceBatches(DS.VIGORPairs(str(tmp_path), split="samearea", train=True, random_orientation=orient), 4, cache=cache, **kw)
    assert_same(epoch(it), want)
    n_tiles = len({plain.sat_paths[plain.labels[i, 0]] for i in range(12)})
    assert cache.entries == 12 + n_tiles and cache.bytes_used == 12 * 40 * 80 * 3 + n_tiles * 48 * 48 * 3
    hits, misses = cache.hits, cache.misses
    assert hits + misses == 24
    remove_images(str(tmp_path))
    assert_same(epoch(it), want)
    assert cache.misses == misses and cache.hits == hits + 24
    cache.clear()
    assert cache.entries == 0 and cache.bytes_allocated == 0
    with pytest.raises(OSError):                                # nothing is cached any more: the tiles are decoded again, and are gone
        epoch(it)


def test_cache_too_small_for_the_set(tmp_path):
    """Room for 3 panoramas, 6 samples: panoramas 0-2 are retained, everything else goes through the scratch slots each epoch."""
    make_vigor_tree(str(tmp_path))
    orient = np.linspace(10.0, 300.0, 12)
    kw = dict(device="cuda", workers=2, grd_hw=(40, 80), sat_hw=(48, 48), targets=False, indices=np.arange(6))
    plain = DS.VIGORPairs(str(tmp_path), split="samearea", train=True, random_orientation=orient)
    want = epoch(DS.DeviceBatches(plain, 4, **kw))
    cache = C.DeviceImageCache("cuda", 3 * 40 * 80 * 3)
    ds = DS.VIGORPairs(str(tmp_path), split="samearea", train=True, random_orientation=orient)
    it = DS.DeviceBatches(ds, 4, cache=cache, **kw)
    assert_same(epoch(it), want)
    assert cache.full and cache.entries == 3 and cache.bytes_allocated <= cache.capacity_bytes
    assert (cache.hits, cache.misses) == (0, 12)
    assert_same(epoch(it), want)
    assert (cache.hits, cache.misses) == (3, 21) and cache.entries == 3
    remove_images(str(tmp_path), only=set(ds.grd_paths[:3]))    # the retained panoramas are not opened again
    assert_same(epoch(it), want)
    remove_images(str(tmp_path), only=set(ds.sat_paths))        # the overflow IS decoded again: loud when its files are gone
    with pytest.raises(OSError):
        epoch(it)


@pytest.mark.parametrize("device_align,sat_hw", [(False, (512, 512)), (True, (512, 512)), (True, (64, 64))])
def test_kitti_ground_side_is_cached_aerial_side_is_not(tmp_path, device_align, sat_hw):
    train_file, _, names = make_kitti_tree(str(tmp_path))
    kw = dict(device="cuda", workers=2, grd_hw=(64, 208), sat_hw=sat_hw, n_bins=16)
    mk = lambda: DS.KITTIPairs(str(tmp_path), train_file, 20, 20, 10, rng=np.random.default_rng(6), device_align=device_align)
    plain = mk()
    want = [epoch(DS.DeviceBatches(plain, 3, **kw)) for _ in range(2)]
    assert not torch.equal(want[0][0]["sat"], want[1][0]["sat"])                  # the perturbation really changes per epoch
    cache = C.DeviceImageCache("cuda", 16 << 20, chunk_bytes=4 << 20)
    ds = mk()
    it = DS.DeviceBatches(ds, 3, cache=cache, **kw)
    assert_same(epoch(it), want[0])
    assert (cache.entries, cache.hits, cache.misses) == (4, 0, 4) and cache.bytes_used == 4 * 64 * 208 * 3
    remove_images(str(tmp_path), only={ds.paths(n)[2] for n in names})            # the camera images; the maps stay
    assert_same(epoch(it), want[1])
    assert (cache.entries, cache.hits, cache.misses) == (4, 4, 4)


def test_oxford_test_split_second_pass_opens_no_file(tmp_path):
    g, sat_path = make_oxford_tree(str(tmp_path))
    kw = dict(device="cuda", workers=2, grd_hw=(154, 231), n_bins=20, ascending_bins=True)
    want = epoch(DS.DeviceBatches(DS.OxfordPairs(g, sat_path, split="test"), 4, **kw))
    ds = DS.OxfordPairs(g, sat_path, split="test")
    cache = C.DeviceImageCache("cuda", 64 << 20, chunk_bytes=4 << 20)
    it = DS.DeviceBatches(ds, 4, cache=cache, **kw)
    assert_same(epoch(it), want)
    patches = {ds.keys(i, None)["sat"] for i in range(len(ds))}
    assert cache.entries == 9 + len(patches) and cache.hits + cache.misses == 18
    hits, misses = cache.hits, cache.misses
    remove_images(g)
    ds.map = None                                               # the second pass cuts no patch either
    assert_same(epoch(it), want)
    assert cache.misses == misses and cache.hits == hits + 18
