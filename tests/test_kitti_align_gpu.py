"""ccvpe_kitti_align_u8 (csrc/align.hip) against LIVE Pillow on the case table of tests/kitti_align_cases.py — ONE launch of
mixed sizes, packed with per-sample offsets — and DeviceBatches with KITTIPairs(device_align=True) against the host path.
Equal bytes everywhere, no tolerance."""
import numpy as np
import pytest
import torch

import kitti_align_cases as K
from ccvpe_amd import align
from ccvpe_amd import datasets as DS

pytestmark = pytest.mark.gpu


def launch(cases, crop):
    """One launch for `cases` (all with the same crop): sources packed back to back in case order, unaligned offsets included."""
    srcs = [K.source(c.src) for c in cases]
    sizes = [s.size for s in srcs]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    packed = np.concatenate([s.reshape(-1) for s in srcs])
    rows = np.stack([K.params(c) for c in cases])
    return align.kitti_align(torch.from_numpy(packed).cuda(), torch.from_numpy(offsets[:-1].copy()).cuda(),
                             torch.from_numpy(rows).cuda(), (crop, crop))


def test_one_mixed_launch_per_crop_equals_pillow_and_repeats():
    table = K.CASES + [K.CASE_1280]
    K.check_inputs_are_visible(table)
    by_crop = {}
    for c in table:
        by_crop.setdefault(c.crop, []).append(c)
    # the crop is a launch parameter: the 512 launch mixes the 640 and 1280 sources, the 64 launch is all of one size,
    # so one more launch mixes EVERY source size (B = 25) at crop 48 — smaller than every source — against Pillow's same chain
    for crop, cases in sorted(by_crop.items()):
        got = launch(cases, crop)
        again = launch(cases, crop)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (len(cases), crop, crop, 3)
        assert torch.equal(got, again), "crop %d: two runs differ" % crop
        got = got.cpu().numpy()
        for j, c in enumerate(cases):
            want = K.expected(c)
            assert np.array_equal(got[j], want), "%s: %d of %d bytes differ" % (c.name, int((got[j] != want).sum()), want.size)
    mixed = [c._replace(name=c.name + "@48", crop=48) for c in table]
    assert len(mixed) >= 5 and len({c.src for c in mixed}) == 5
    K.check_inputs_are_visible(mixed)
    got = launch(mixed, 48)
    assert torch.equal(got, launch(mixed, 48))
    got = got.cpu().numpy()
    for j, c in enumerate(mixed):
        want = K.expected(c)
        assert np.array_equal(got[j], want), "%s: %d of %d bytes differ" % (c.name, int((got[j] != want).sum()), want.size)


def test_a_sample_that_does_not_fit_the_buffer_is_zeros_not_read():
    c = K.CASES[0]
    src = torch.from_numpy(K.source(c.src).reshape(-1).copy()).cuda()
    rows = torch.from_numpy(np.stack([K.params(c), K.params(c)])).cuda()
    offsets = torch.tensor([0, 3], dtype=torch.int64).cuda()                  # the second sample would end 3 bytes past the buffer
    got = align.kitti_align(src, offsets, rows, (c.crop, c.crop)).cpu().numpy()
    assert np.array_equal(got[0], K.expected(c)) and not got[1].any()
    with pytest.raises(ValueError):
        align.kitti_align(src.cpu(), offsets, rows, (c.crop, c.crop))         # no CPU fallback


def _batches(pairs, **kw):
    return list(DS.DeviceBatches(pairs, 3, device="cuda", workers=2, grd_hw=(256, 1024), n_bins=16, **kw))


def _same_batches(dev, host):
    assert len(dev) == len(host) == 2
    for a, b in zip(dev, host):
        assert a.indices == b.indices and a.cities == b.cities
        assert tuple(a.sat.shape) == (len(a.indices), 3, 512, 512)
        for k in ("sat", "grd", "angle_deg", "center", "gt", "gt_flat", "gt_ori"):
            assert torch.equal(getattr(a, k), getattr(b, k)), k
        assert len(a.labels) == len(b.labels) and all(torch.equal(x, y) for x, y in zip(a.labels, b.labels))


def test_device_batches_with_device_align_equal_the_host_path(tmp_path, synth_sd):
    from ccvpe_amd import models
    from test_datasets import make_kitti_tree
    root = str(tmp_path)
    train_file, test_file, names = make_kitti_tree(root)
    dev = _batches(DS.KITTIPairs(root, test_file, 20, 20, 10, test=True, device_align=True))
    host = _batches(DS.KITTIPairs(root, test_file, 20, 20, 10, test=True))
    _same_batches(dev, host)
    assert dev[0].sat.std() > 0.5                                             # an aerial image, not fill
    # a seeded training file, shuffled: draws are made on the producer thread in index order on both paths
    dev_tr = _batches(DS.KITTIPairs(root, train_file, 20, 20, 10, rng=np.random.default_rng(7), device_align=True), shuffle=True, seed=3)
    host_tr = _batches(DS.KITTIPairs(root, train_file, 20, 20, 10, rng=np.random.default_rng(7)), shuffle=True, seed=3)
    _same_batches(dev_tr, host_tr)
    assert not torch.equal(dev_tr[0].sat, dev[0].sat)
    net = models.CVM_KITTI("cuda")
    net.load_state_dict(synth_sd("kitti", 0), strict=True)
    net = net.to("cuda:0").eval()
    out = net(dev[1].grd, dev[1].sat)                                         # the short last batch: one sample
    assert tuple(out[0].shape) == (1, 512 * 512) and torch.isfinite(out[0]).all()
