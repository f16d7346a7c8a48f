"""Device image cache, host half (no GPU): `gather_spec` — the written specification of ccvpe_gather_norm_u8_f32 — against
torch.roll + ToTensor / Normalize in torch fp32, the bookkeeping of DeviceImageCache on device="cpu" (no kernel runs there), and
the index classes' `keys()` / `sample(cached=...)`: same dict apart from the images, no file access for a cached side, same draws."""
import os

import numpy as np
import pytest
import torch

from ccvpe_amd import cache as C, datasets as DS
from test_datasets import make_kitti_tree, make_oxford_tree, make_vigor_tree

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def torch_pipeline(img, roll, keep_w):
    """ToTensor -> Normalize -> torch.roll -> crop, as the oracle's preprocess_reference does after its resize."""
    t = torch.from_numpy(img.copy()).permute(2, 0, 1).float().div(255)
    t = (t - torch.tensor(MEAN).view(3, 1, 1)) / torch.tensor(STD).view(3, 1, 1)
    return torch.roll(t, int(roll), dims=2)[:, :, :keep_w]


@pytest.mark.parametrize("h,w,keep_w", [(6, 10, 10), (6, 10, 8), (6, 10, 7), (3, 4, 4), (5, 33, 1)])
def test_gather_spec_is_roll_totensor_normalize_in_fp32(h, w, keep_w):
    rng = np.random.RandomState(h * 100 + w)
    imgs = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for _ in range(3)]
    imgs[0][0, 0] = (0, 255, 128)
    order = [2, 0, 0, 1, 2, 1]
    rolls = [0, 3, -13, w, -w - 1, 5 * w + 2]                   # negative, |roll| > w, a whole turn
    got = C.gather_spec([imgs[i] for i in order], rolls, keep_w, MEAN, STD)
    assert got.dtype == np.float32 and got.shape == (6, 3, h, keep_w)
    for b, (i, r) in enumerate(zip(order, rolls)):
        assert torch.equal(torch.from_numpy(got[b]), torch_pipeline(imgs[i], r, keep_w)), "row %d (roll %d)" % (b, r)
    with pytest.raises(ValueError):
        C.gather_spec(imgs, [0, 0, 0], w + 1)


def test_every_byte_value_normalises_as_torch_does():
    img = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, axis=2)
    assert torch.equal(torch.from_numpy(C.gather_spec([img], [-7], 256)[0]), torch_pipeline(img, -7, 256))


class FakeImage(object):
    """What insert() reads of a decoded image on device="cpu": its shape."""

    def __init__(self, h, w):
        self.shape = (h, w, 3)


def test_bookkeeping_capacity_full_duplicates_and_counters():
    slot = 4 * 6 * 3
    c = C.DeviceImageCache("cpu", capacity_bytes=5 * slot + slot // 2, chunk_bytes=2 * slot)
    assert (c.entries, c.bytes_used, c.bytes_allocated, c.full, c.hits, c.misses) == (0, 0, 0, False, 0, 0)
    assert c.lookup("a") is None and c.misses == 1
    addrs = []
    for k in range(5):
        a = c.insert("k%d" % k, FakeImage(10 + k, 20), (4, 6))
        assert a is not None and not c.full
        assert c.bytes_allocated <= c.capacity_bytes and c.bytes_used == (k + 1) * slot <= c.bytes_allocated
        addrs.append(a)
    assert len(set(addrs)) == 5 and c.entries == 5 == len(c)
    assert c.bytes_allocated == 5 * slot                        # chunks of 2, 2 and — what the capacity leaves — 1 slot
    assert addrs[1] - addrs[0] == slot and addrs[3] - addrs[2] == slot
    # a duplicate insert is a no-op that returns the stored address
    assert c.insert("k1", FakeImage(99, 99), (4, 6)) == addrs[1] and c.entries == 5 and c.bytes_used == 5 * slot
    assert c.lookup("k1") == (addrs[1], (11, 20)) and c.hits == 1
    # the sixth image finds no slot: `full` turns true exactly here, nothing is retained, nothing is allocated
    assert c.insert("k5", FakeImage(8, 8), (4, 6)) is None
    assert c.full and c.entries == 5 and c.bytes_allocated == 5 * slot and c.lookup("k5") is None
    assert c.address("k5") is None and c.address("k0") == addrs[0]
    assert (c.hits, c.misses) == (1, 2)                         # address() counts nothing
    assert c.resized_hw("k0") == (4, 6)
    c.clear()
    assert (c.entries, c.bytes_used, c.bytes_allocated, c.full, c.hits, c.misses) == (0, 0, 0, False, 0, 0)
    assert c.lookup("k0") is None and c.insert("k0", FakeImage(3, 3), (4, 6)) is not None


def test_two_shapes_coexist_and_share_the_capacity():
    a, b = 4 * 6 * 3, 5 * 5 * 3
    c = C.DeviceImageCache("cpu", capacity_bytes=2 * a + 2 * b, chunk_bytes=1)        # chunk_bytes below a slot: one slot per chunk
    got = [c.insert("a0", FakeImage(9, 9), (4, 6)), c.insert("b0", FakeImage(7, 7), (5, 5)),
           c.insert("a1", FakeImage(9, 9), (4, 6)), c.insert("b1", FakeImage(7, 7), (5, 5))]
    assert None not in got and len(set(got)) == 4 and not c.full
    assert c.bytes_used == c.bytes_allocated == c.capacity_bytes
    assert c.resized_hw("a1") == (4, 6) and c.resized_hw("b1") == (5, 5)
    assert c.insert("b2", FakeImage(7, 7), (5, 5)) is None and c.full
    s = c.scratch(3, (5, 5))
    assert tuple(s.shape) == (3, 5, 5, 3) and s.dtype == torch.uint8 and c.bytes_allocated == c.capacity_bytes
    assert c.scratch(2, (5, 5)).data_ptr() == s.data_ptr()      # reused
    with pytest.raises(ValueError):
        C.DeviceImageCache("cpu", -1)


def same_but_images(a, b):
    assert set(a) == set(b)
    for k in a:
        if not k.endswith("_u8"):
            assert type(a[k]) is type(b[k]) and np.array_equal(a[k], b[k]), k


def remove_images(root):
    n = 0
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith((".jpg", ".png")):
                os.remove(os.path.join(d, f))
                n += 1
    assert n


def test_vigor_keys_and_cached_samples(tmp_path):
    make_vigor_tree(str(tmp_path))
    ds = DS.VIGORPairs(str(tmp_path), split="samearea", train=True, pos_only=False, seed=5)
    twin = DS.VIGORPairs(str(tmp_path), split="samearea", train=True, pos_only=False, seed=5)
    draws = [ds.draw(i) for i in range(len(ds))]
    assert draws == [twin.draw(i) for i in range(len(ds))]
    assert len({d[1][0] for d in draws}) > 1                   # the draw really picks different tiles
    plain = [ds.sample(i, (48, 48), (40, 80), draws=d) for i, d in enumerate(draws)]
    keys = [ds.keys(i, d) for i, d in enumerate(draws)]
    for i, (k, d) in enumerate(zip(keys, draws)):
        assert k == {"grd": ds.grd_paths[i], "sat": ds.sat_paths[ds.labels[i, d[1][0]]]}
    half = ds.sample(0, (48, 48), (40, 80), draws=draws[0], cached={"sat": (64, 64)})       # one side only
    assert half["sat_u8"] is None and np.array_equal(half["grd_u8"], plain[0]["grd_u8"])
    same_but_images(half, plain[0])
    assert "nocache" not in ds.sample(0, (48, 48), (40, 80), draws=draws[0], cached={})
    remove_images(str(tmp_path))
    for i, d in enumerate(draws):
        s = ds.sample(i, (48, 48), (40, 80), draws=d, cached={"grd": (96, 192), "sat": (64, 64)})
        assert s["grd_u8"] is None and s["sat_u8"] is None
        same_but_images(s, plain[i])
    # a non-square raw tile size reaches `center`
    s = ds.sample(0, (48, 48), (40, 80), draws=draws[0], cached={"grd": (96, 192), "sat": (32, 128)})
    (k, drow, dcol) = draws[0][1]
    assert s["center"] == (float(np.round(dcol / 128 * 48)), float(-np.round(drow / 32 * 48)))
    # an unreadable panorama still gives the blank image, marked as not cacheable; an unreadable tile still raises
    s = ds.sample(1, (48, 48), (40, 80), draws=draws[1], cached={"sat": (64, 64)})
    assert s["grd_u8"].shape == (40, 80, 3) and not s["grd_u8"].any() and s["nocache"] == ("grd",)
    with pytest.raises(OSError):
        ds.sample(1, (48, 48), (40, 80), draws=draws[1], cached={"grd": (96, 192)})
    # without draws=, a cached call consumes the generator exactly as an uncached one does
    a = DS.VIGORPairs(str(tmp_path), split="samearea", train=True, pos_only=False, seed=9)
    b = DS.VIGORPairs(str(tmp_path), split="samearea", train=True, pos_only=False, seed=9)
    both = {"grd": (96, 192), "sat": (64, 64)}
    got = [a.sample(i, cached=both) for i in range(len(a))]
    want = [b.draw(i) for i in range(len(b))]
    assert [(s["angle_deg"] / 360.0) for s in got] == pytest.approx([w[0] for w in want], abs=0, rel=1e-15)
    assert [s["roll"] for s in got] == [int(torch.round(torch.as_tensor(w[0]) * 640).int().item()) for w in want]


def test_kitti_keys_and_cached_samples(tmp_path):
    train_file, test_file, names = make_kitti_tree(str(tmp_path))
    for device_align in (False, True):
        ds = DS.KITTIPairs(str(tmp_path), train_file, 20, 20, 10, rng=np.random.default_rng(2), device_align=device_align)
        draws = [ds.draw(i) for i in range(len(ds))]
        for i, d in enumerate(draws):
            assert ds.keys(i, d) == {"grd": ds.paths(names[i])[2], "sat": None}
            plain = ds.sample(i, draws=d)
            s = ds.sample(i, draws=d, cached={"grd": (94, 310)})
            assert s["grd_u8"] is None
            same_but_images(s, plain)
            aerial = "sat_src_u8" if device_align else "sat_u8"
            assert np.array_equal(s[aerial], plain[aerial])
    te = DS.KITTIPairs(str(tmp_path), test_file, 20, 20, 10, test=True)
    assert te.keys(1, te.draw(1)) == {"grd": te.paths(names[1])[2], "sat": None}
    for n in names:                                             # the cached side does not touch the file system
        os.remove(te.paths(n)[2])
    plain_keys = set(te.sample(0, cached={"grd": (94, 310)}))
    assert plain_keys == {"grd_u8", "sat_u8", "roll", "angle_deg", "center", "city", "index"}
    with pytest.raises(OSError):
        te.sample(0)


def test_oxford_keys_and_cached_samples(tmp_path):
    import random
    g, sat_path = make_oxford_tree(str(tmp_path))
    te = DS.OxfordPairs(g, sat_path, split="test")
    plain = [te.sample(i) for i in range(len(te))]
    keys = [te.keys(i, te.draw(i)) for i in range(len(te))]
    for i, k in enumerate(keys):
        assert k["grd"] == os.path.join(g, te.rows[i][0])
        path, at = k["sat"].rsplit("@", 1)
        kc, kr = (int(v) for v in at.split(","))
        assert path == sat_path
        patch = np.array(te.map.crop((kc * 400, kr * 400, kc * 400 + 800, kr * 400 + 800)).convert("RGB"))
        assert np.array_equal(patch, plain[i]["sat_u8"])        # the key names exactly the patch the sample cuts
    remove_images(g)
    for i in range(len(te)):
        s = te.sample(i, cached={"grd": (60, 90), "sat": (800, 800)})
        assert s["grd_u8"] is None and s["sat_u8"] is None
        same_but_images(s, plain[i])
    tr = DS.OxfordPairs(g, sat_path, split="train", rng=random.Random(4))
    twin = DS.OxfordPairs(g, sat_path, split="train", rng=random.Random(4))
    d = tr.draw(0)
    assert tr.keys(0, d) == {"grd": os.path.join(g, tr.rows[0][0]), "sat": None}
    s = tr.sample(0, draws=d, cached={"grd": (60, 90)})
    assert s["grd_u8"] is None and s["sat_u8"].shape == (800, 800, 3)
    assert twin.sample(0, cached={"grd": (60, 90)})["center"] == s["center"]      # the draw is made either way
