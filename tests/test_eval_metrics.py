"""The reference test protocols on the host (ccvpe_amd/evaluate.py: metrics_spec, summarise, format_report) against the
reference's loop and prints restated in tests/eval_metrics_cases.py.  metrics_spec is the specification that
tests/test_eval_metrics_gpu.py holds the kernel to, so it is pinned here, without a GPU, to 1e-12 relative: both sides are
float64."""
import numpy as np
import pytest

import eval_metrics_cases as C
from ccvpe_amd import evaluate as E


@pytest.fixture(scope="module")
def cases():
    batch = C.case_batch()
    return batch, C.restate(*batch)


def _close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= 1e-12 * np.abs(want[ok])), (got, want)


def test_case_list_covers_what_it_claims(cases):
    """The inputs do what the case names say, and no longitudinal / lateral / orientation value lies within 1e-6 of a recall
    threshold: a last-place difference (host libm against the device's) can then never flip a count."""
    batch, ref = cases
    heat, ori, gt, gt_ori, heading, mpp = batch
    assert len(C.CASES) == 12 and heat.shape == (12, 1, C.H, C.W)
    by = {c.name: i for i, c in enumerate(C.CASES)}
    for i, c in enumerate(C.CASES):
        assert ref.pred[i] == c.pred and ref.truth[i] == c.gt, c.name                  # ties: the FIRST index
    assert C.CASES[by["tie in the heat-map"]].also_pred is not None and C.CASES[10].pred < C.CASES[10].also_pred
    i = by["tie in the heat-map"]
    assert heat[i, 0][C.CASES[i].also_pred] == heat[i, 0][C.CASES[i].pred] == heat[i].max()
    i = by["tie in the GT map, sin<0 on both sides"]
    assert gt[i, 0][C.CASES[i].also_gt] == gt[i, 0][C.CASES[i].gt] == gt[i].max() and C.CASES[i].gt < C.CASES[i].also_gt
    assert C.CASES[by["sin<0 on the predicted side"]].pred_cs[1] < 0 < C.CASES[by["sin<0 on the predicted side"]].gt_cs[1]
    assert C.CASES[by["sin<0 on the GT side"]].gt_cs[1] < 0 < C.CASES[by["sin<0 on the GT side"]].pred_cs[1]
    nan_rows = [i for i, a in enumerate(ref.pred_angle) if a is None]
    assert nan_rows == [by["|cos| > 1: NaN row"], by["|sin| > 1: NaN row"]] and len(ref.angle_errors) == 10
    assert ref.pixels[by["pred == gt: distance 0, atan2(0, 0)"]] == 0.0
    assert {0.0, 90.0, 135.5, 360.0} <= set(heading.tolist())
    rows = C.rows_of(ref)
    assert abs(rows[by["wrap: GT 359, prediction 1 -> 2"], 9] - 2.0) < 1e-4
    vals = np.concatenate([ref.along, ref.across, ref.angle_errors])
    for t in E.THRESHOLDS:
        assert np.all(np.abs(vals - t) > 1e-6), (t, vals)
    # the recall counts are not all 0 or all 1: the thresholds cut through the data
    for x in (ref.across, ref.along, ref.angle_errors):
        assert 0 < np.sum(np.array(x) < 1) < np.sum(np.array(x) < 5) <= len(x)


def test_metrics_spec_matches_the_reference_loop(cases):
    batch, ref = cases
    got = E.metrics_spec(*batch)
    want = C.rows_of(ref)
    assert got.shape == (12, 12) and got.dtype == np.float64
    assert np.array_equal(got[:, [0, 1, 2, 3, 10, 11]], want[:, [0, 1, 2, 3, 10, 11]])
    _close(got[:, 4:10], want[:, 4:10])


def test_metrics_spec_on_seeded_maps():
    """maxima wherever the generator put them (no hand-placed pixels), host tensors as well as arrays"""
    import torch
    batch = C.random_batch(6, C.H, C.W, 31)
    want = C.rows_of(C.restate(*batch))
    got = E.metrics_spec(*[torch.from_numpy(a) for a in batch])
    assert np.array_equal(got[:, [0, 1, 2, 3, 10, 11]], want[:, [0, 1, 2, 3, 10, 11]])
    _close(got[:, 4:10], want[:, 4:10])


def _printed(r):
    """the quantities the reference's three test scripts print after the loop (train_KITTI.py:347-360,
    train_OxfordRobotCar.py:249-266, train_VIGOR.py:329-338)"""
    lat, lon = np.array(r.across), np.array(r.along)
    oe = np.array(r.angle_errors)
    return {
        "n": len(r.pixels),
        "mean_metre_error": np.mean(r.metres), "median_metre_error": np.median(r.metres),
        "mean_longitudinal_error": np.mean(lon), "median_longitudinal_error": np.median(lon),
        "mean_lateral_error": np.mean(lat), "median_lateral_error": np.median(lat),
        "mean_orientation_error": np.mean(oe), "median_orientation_error": np.median(oe),
        "mean_probability_at_gt": np.mean(r.p_truth), "median_probability_at_gt": np.median(r.p_truth),
        "mean_probability": np.mean(r.p_pred), "median_probability": np.median(r.p_pred),
        "lateral_within": tuple(np.sum(lat < t) / len(lat) for t in (1, 3, 5)),
        "longitudinal_within": tuple(np.sum(lon < t) / len(lon) for t in (1, 3, 5)),
        "orientation_within": tuple(np.sum(oe < t) / len(oe) for t in (1, 3, 5)),
    }


def _assert_summary(got, want):
    assert got["n"] == want["n"]
    for k, v in want.items():
        if k.endswith("_within"):
            assert tuple(got[k][t] for t in (1, 3, 5)) == v, k                           # counts / length: exact
        elif "probability" in k:
            assert v.dtype == np.float32 and got[k] == float(v), k                       # float32 statistics of float32 entries: exact
        elif k != "n":
            assert abs(got[k] - v) <= 1e-12 * abs(v), (k, got[k], v)


def test_summarise_matches_the_printed_quantities(cases):
    """whole run + three sets of unequal length (5, 4, 3 samples; the first holds both NaN rows: its orientation list has 3
    entries for 5 distances), as index arrays, a slice and a boolean mask"""
    batch, ref = cases
    rows = E.metrics_spec(*batch)
    sets = {"test1": np.arange(0, 5), "test2": slice(5, 9), "test3": np.arange(12) >= 9}
    got = E.summarise(rows, sets)
    _assert_summary(got, _printed(ref))
    assert len(ref.angle_errors) == 10 < len(ref.pixels) == 12
    assert list(got["sets"]) == ["test1", "test2", "test3"]
    for name, sel in (("test1", range(0, 5)), ("test2", range(5, 9)), ("test3", range(9, 12))):
        part = C.restate(*batch, select=sel)
        _assert_summary(got["sets"][name], _printed(part))
    assert got["sets"]["test1"]["n"] == 5 and len(C.restate(*batch, select=range(5)).angle_errors) == 3
    assert "sets" not in E.summarise(rows)
    # no valid orientation at all: NaN statistics, no exception, no warning-as-value
    only_nan = E.summarise(rows[2:4])
    assert only_nan["n"] == 2 and np.isnan(only_nan["mean_orientation_error"]) and np.isnan(only_nan["orientation_within"][3])


SUMMARY = {
    "n": 4, "mean_metre_error": 1.5, "median_metre_error": 1.25, "mean_longitudinal_error": 0.75,
    "median_longitudinal_error": 0.5, "mean_lateral_error": 1.125, "median_lateral_error": 1.0,
    "mean_orientation_error": 2.5, "median_orientation_error": 2.0, "mean_probability_at_gt": 0.001953125,
    "median_probability_at_gt": 0.0009765625, "mean_probability": 0.0625, "median_probability": 0.03125,
    "lateral_within": {1: 0.25, 3: 0.75, 5: 1.0}, "longitudinal_within": {1: 0.5, 3: 1.0, 5: 1.0},
    "orientation_within": {1: 0.0, 3: 0.5, 5: 0.75},
}

VIGOR_REPORT = """mean localization error (m):  1.5
median localization error (m):  1.25
---------------------------------------
mean orientation error (degrees):  2.5
median orientation error (degrees):  2.0
---------------------------------------
mean probability at gt 0.001953125
median probability at gt 0.0009765625"""

KITTI_REPORT = """---------------------------------------
mean localization error (m):  1.5
median localization error (m):  1.25
---------------------------------------
mean orientation error (degrees):  2.5
median orientation error (degrees):  2.0
---------------------------------------
percentage of samples with lateral localization error under 1m, 3m, and 5m:  0.25 0.75 1.0
percentage of samples with longitudinal localization error under 1m, 3m, and 5m:  0.5 1.0 1.0
percentage of samples with orientation error under 1 degree, 3 degrees, and 5 degrees:  0.0 0.5 0.75"""

OXFORD_BLOCK = """mean error (m):  1.5
median error (m):  1.25
mean longitudinal error (m):  0.75
median longitudinal error (m):  0.5
mean lateral error (m):  1.125
median lateral error (m):  1.0
mean orientation error (deg):  2.5
median orientation error (deg):  2.0
percentage of samples with longitudinal localization error under 1m, 3m, and 5m:  0.5 1.0 1.0
percentage of samples with lateral localization error under 1m, 3m, and 5m:  0.25 0.75 1.0
percentage of samples with orientation error under 1 degree, 3 degrees, and 5 degrees:  0.0 0.5 0.75"""


def test_format_report_snapshots():
    assert E.format_report(SUMMARY, "vigor") == VIGOR_REPORT
    assert E.format_report(SUMMARY, "kitti") == KITTI_REPORT
    assert E.format_report(SUMMARY, "oxford") == OXFORD_BLOCK
    with_sets = dict(SUMMARY, sets={"test1": SUMMARY, "test2": dict(SUMMARY, mean_metre_error=2.5)})
    bar = "-" * 70
    assert E.format_report(with_sets, "oxford") == (
        "test1\n" + OXFORD_BLOCK + "\n" + bar + "\ntest2\n" + OXFORD_BLOCK.replace("mean error (m):  1.5", "mean error (m):  2.5"))
    kitti_sets = dict(SUMMARY, sets={"Test 1 set": SUMMARY})
    first, rest = KITTI_REPORT.split("\n", 1)
    assert E.format_report(kitti_sets, "kitti") == first + "\nTest 1 set\n" + rest
    with pytest.raises(ValueError):
        E.format_report(SUMMARY, "elsewhere")


def test_defaults_for_resolution_and_sets():
    """metres per pixel and the Oxford traversals, from the index objects (no files needed: bare instances)"""
    from ccvpe_amd import datasets as DS
    ox = DS.OxfordPairs.__new__(DS.OxfordPairs)
    ox.split, ox.list_lengths = "test", [3, 1, 2]
    sets = E.default_sets(ox)
    assert list(sets) == ["test1", "test2", "test3"]
    assert [s.tolist() for s in sets.values()] == [[0, 1, 2], [3], [4, 5]]
    assert E.default_metres_per_pixel(ox) == 0.09240351462361521 / 512 * 800
    ox.split = "val"
    assert E.default_sets(ox) is None
    ki = DS.KITTIPairs.__new__(DS.KITTIPairs)
    ki.meter_per_pixel = DS.kitti_meter_per_pixel()
    assert E.default_metres_per_pixel(ki) == ki.meter_per_pixel and E.default_sets(ki) is None
    vi = DS.VIGORPairs.__new__(DS.VIGORPairs)
    table = E.default_metres_per_pixel(vi)
    assert table == {"NewYork": 0.113248 / 512 * 640, "Seattle": 0.100817 / 512 * 640,
                     "SanFrancisco": 0.118141 / 512 * 640, "Chicago": 0.111262 / 512 * 640}
    with pytest.raises(ValueError):
        E.default_metres_per_pixel(object())


def test_c_entry_point_validates_before_launching():
    """ccvpe_eval_metrics_f32 rejects bad shapes, null pointers and a misaligned table with CCVPE_EINVAL and a message; nothing
    is enqueued, so this runs without a GPU (fake aligned "pointers", never dereferenced)."""
    from ccvpe_amd import _lib
    lib = _lib.load()
    EINVAL = -1
    ok = [256, 512, 768, 1024, 2048, 4096, 8192]                 # heatmap, ori, gt, gt_ori, heading_deg, metres_per_pixel, rows
    assert lib.ccvpe_eval_metrics_f32(*ok, 0, 8, 12, None) == EINVAL and b"bad shape" in lib.ccvpe_last_error()
    assert lib.ccvpe_eval_metrics_f32(*ok, 2, 0, 12, None) == EINVAL and b"bad shape" in lib.ccvpe_last_error()
    assert lib.ccvpe_eval_metrics_f32(*ok, 2, 8, -1, None) == EINVAL
    assert lib.ccvpe_eval_metrics_f32(*ok, 1, 65536, 65536, None) == EINVAL                # h * w does not fit an int
    for k in range(7):
        args = list(ok)
        args[k] = None
        assert lib.ccvpe_eval_metrics_f32(*args, 2, 8, 12, None) == EINVAL and b"null" in lib.ccvpe_last_error(), k
    for k in (4, 5, 6):
        args = list(ok)
        args[k] += 4
        assert lib.ccvpe_eval_metrics_f32(*args, 2, 8, 12, None) == EINVAL and b"8-byte" in lib.ccvpe_last_error(), k
    args = list(ok)
    args[0] += 2
    assert lib.ccvpe_eval_metrics_f32(*args, 2, 8, 12, None) == EINVAL and b"4-byte" in lib.ccvpe_last_error()
    with pytest.raises(_lib.CcvpeError, match="ccvpe_eval_metrics_f32 failed"):
        _lib.check(lib.ccvpe_eval_metrics_f32(*ok, 0, 8, 12, None), "ccvpe_eval_metrics_f32")


# ---- the driver without a GPU: a stand-in for DeviceBatches and for the launch (metrics_spec writes the slice) ----------------
class _FakeBatch(object):
    pass


class _FakeBatches(object):
    """what evaluate_batches reads of a DeviceBatches: pairs, batch_size, device, targets, indices (this rank's shard) and the
    batches; `sat` carries the heat-map and `grd` the orientation field, so that forward(grd, sat) = (None, sat, grd)"""

    def __init__(self, pairs, data, batch_size, rank=0, world=1, cities=None):
        import torch
        from ccvpe_amd import harness
        self.pairs, self.batch_size, self.device, self.targets = pairs, batch_size, torch.device("cpu"), True
        self.shard = "exact"
        self.indices = np.asarray(harness.shard_indices(len(data[0]), world, rank))[::-1].copy()     # out of order on purpose
        self.data, self.cities = data, cities

    def __iter__(self):
        import torch
        heat, ori, gt, gt_ori, heading, _ = self.data
        for k in range(0, len(self.indices), self.batch_size):
            idx = self.indices[k:k + self.batch_size]
            b = _FakeBatch()
            b.sat, b.grd, b.gt, b.gt_ori = (torch.from_numpy(a[idx]) for a in (heat, ori, gt, gt_ori))
            b.heading_deg = torch.from_numpy(heading[idx])
            b.indices = [int(i) for i in idx]
            b.cities = [self.cities[i] for i in idx] if self.cities else ["oxford"] * len(idx)
            yield b


def _spec_launch(heatmap, ori, gt, gt_ori, heading_deg, metres_per_pixel, out=None):
    import torch
    out.copy_(torch.from_numpy(E.metrics_spec(heatmap, ori, gt, gt_ori, heading_deg.numpy(), metres_per_pixel.numpy())))
    return out


def _oxford_pairs():
    from ccvpe_amd import datasets as DS
    ox = DS.OxfordPairs.__new__(DS.OxfordPairs)
    ox.split, ox.list_lengths = "test", [3, 2, 2]
    return ox


def _forward(grd, sat):
    return (None, sat, grd)


def _driver_worker(rank, world, port, out):
    import os
    import sys
    import torch
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ccvpe_amd import evaluate, ops
    ops.eval_metrics = _spec_launch
    batches = _FakeBatches(_oxford_pairs(), C.random_batch(7, C.H, C.W, 77), 2, rank, world)
    batches.shard = "pad"                       # a padded shard repeats samples over the ranks: refused, not counted twice
    try:
        evaluate.evaluate_batches(_forward, batches)
        raise AssertionError("a padded shard was accepted on two ranks")
    except ValueError as ex:
        assert "shard='exact'" in str(ex)
    batches.shard = "exact"
    res = evaluate.evaluate_batches(_forward, batches)
    if rank == 1:
        torch.save(res, out)
    dist.barrier()
    dist.destroy_process_group()


def test_evaluate_batches_driver_on_the_host(monkeypatch, tmp_path):
    """evaluate_batches over a stand-in for DeviceBatches (7 samples, batches of 2, iterated out of order), the launch replaced
    by its specification: rows ordered by sample index, Oxford's three traversals from list_lengths, the reference's Oxford
    resolution, a caller's sets and resolution table; and two gloo ranks with shards of 4 and 3 give the single-process result."""
    import socket
    import torch
    import torch.multiprocessing as mp
    from ccvpe_amd import ops
    monkeypatch.setattr(ops, "eval_metrics", _spec_launch)
    data = C.random_batch(7, C.H, C.W, 77)
    res = E.evaluate_batches(_forward, _FakeBatches(_oxford_pairs(), data, 2))
    want = E.metrics_spec(*data[:5], np.full(7, 0.09240351462361521 / 512 * 800))
    assert res["n"] == 7 and res["indices"].tolist() == list(range(7))
    assert np.array_equal(res["rows"].view(np.int64), want.view(np.int64))
    spec = E.summarise(want, {"test1": slice(0, 3), "test2": slice(3, 5), "test3": slice(5, 7)})
    assert list(res["sets"]) == ["test1", "test2", "test3"] and [s["n"] for s in res["sets"].values()] == [3, 2, 2]
    for name in spec["sets"]:
        assert res["sets"][name] == spec["sets"][name], name
    assert {k: v for k, v in res.items() if k not in ("rows", "indices")} == spec
    # a caller's resolution table (looked up through batch.cities) and sets (by sample index)
    cities = ["Seattle", "Chicago", "NewYork", "Seattle", "SanFrancisco", "Chicago", "NewYork"]
    vi = _FakeBatches(object(), data, 3, cities=cities)
    res2 = E.evaluate_batches(_forward, vi, metres_per_pixel=E.VIGOR_METRES_PER_PIXEL, sets={"odd": [1, 3, 5]})
    want2 = E.metrics_spec(*data[:5], np.array([E.VIGOR_METRES_PER_PIXEL[c] for c in cities]))
    assert np.array_equal(res2["rows"].view(np.int64), want2.view(np.int64))
    assert res2["sets"]["odd"] == E.summarise(want2[[1, 3, 5]])
    with pytest.raises(ValueError):
        E.evaluate_batches(_forward, vi)                                   # no default resolution for an unknown index object
    vi.targets = False
    with pytest.raises(ValueError, match="targets=True"):
        E.evaluate_batches(_forward, vi, metres_per_pixel=0.2)
    # two ranks
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "r.pt")
    mp.spawn(_driver_worker, args=(2, port, out), nprocs=2, join=True)
    multi = torch.load(out, weights_only=False)
    assert multi["n"] == 7 and multi["indices"].tolist() == list(range(7))
    assert np.array_equal(multi["rows"].view(np.int64), want.view(np.int64))
    assert multi["sets"]["test2"] == res["sets"]["test2"]
