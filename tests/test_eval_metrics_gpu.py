"""ccvpe_eval_metrics_f32 (csrc/heads.hip: eval_metrics_kernel) through ccvpe_amd.ops.eval_metrics against its specification
ccvpe_amd.evaluate.metrics_spec (pinned to the reference's loop on the CPU by tests/test_eval_metrics.py), and
evaluate_batches end to end on a synthetic KITTI test tree.

The bound (eval_metrics_cases.assert_rows_close): indices and values read bit-equal; the double-precision tail within 1e-9
absolute + 1e-9 relative, NaN positions identical."""
import ctypes

import numpy as np
import pytest
import torch

import eval_metrics_cases as C
from ccvpe_amd import _lib, evaluate as E

pytestmark = pytest.mark.gpu


def _dev(batch):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in batch]


def _run(batch, **kw):
    from ccvpe_amd import ops
    return ops.eval_metrics(*_dev(batch), **kw).cpu().numpy()


@pytest.mark.parametrize("b,h,w", [(3, 8, 12),        # non-square, n < 1024: most threads idle
                                   (2, 5, 7),         # n % 4 != 0: the scalar path
                                   (2, 64, 64),       # 4 elements (one 16-byte load) per thread
                                   (2, 512, 512)])    # the real row length
def test_kernel_matches_the_spec(b, h, w):
    batch = C.random_batch(b, h, w, 1000 + h)
    want = E.metrics_spec(*batch)
    got = _run(batch)
    assert got.dtype == np.float64 and got.shape == (b, 12)
    C.assert_rows_close(got, want, (b, h, w))
    assert np.array_equal(got.view(np.int64), _run(batch).view(np.int64))               # run to run: bit-identical


def test_case_list_on_the_device():
    """the twelve CPU cases (sin < 0 on either side, NaN rows, the 359 / 1 wrap, distance 0, headings 0 / 90 / 135.5 / 360, ties)"""
    batch = C.case_batch()
    got = _run(batch)
    C.assert_rows_close(got, E.metrics_spec(*batch), "cases")
    for i, c in enumerate(C.CASES):
        assert (got[i, 0], got[i, 1], got[i, 2], got[i, 3]) == c.pred + c.gt, c.name
    assert np.isnan(got[[2, 3], 8:10]).all() and not np.isnan(np.delete(got, [2, 3], axis=0)).any()


def test_scan_edges():
    """The maximum in the LAST element (vector path at 8 x 12, scalar path at 5 x 7, both maps); a row base that is not 16-byte
    aligned although n % 4 == 0 (scalar path by alignment); 1024 x 201 elements with a tie in two elements of one thread
    (7 and 7 + 1024 * 200) in the heat-map and in the GT map: the smaller index wins."""
    from ccvpe_amd import ops
    for h, w in ((8, 12), (5, 7)):
        batch = list(C.random_batch(2, h, w, 5))
        batch[0][0, 0, h - 1, w - 1] = 2.0
        batch[2][1, 0, h - 1, w - 1] = 2.0
        got = _run(batch)
        C.assert_rows_close(got, E.metrics_spec(*batch), ("last", h, w))
        assert tuple(got[0, 0:2]) == (h - 1, w - 1) and tuple(got[1, 2:4]) == (h - 1, w - 1)
    batch = C.random_batch(2, 8, 12, 6)
    dev = _dev(batch)
    for k in (0, 2):                                  # heat-map and GT map one float into a larger buffer
        buf = torch.zeros((dev[k].numel() + 4,), device="cuda")
        buf[1:1 + dev[k].numel()] = dev[k].reshape(-1)
        dev[k] = buf[1:1 + dev[k].numel()].reshape(dev[k].shape)
        assert dev[k].data_ptr() % 16 == 4 and dev[k].is_contiguous()
    C.assert_rows_close(ops.eval_metrics(*dev).cpu().numpy(), E.metrics_spec(*batch), "unaligned")
    h, w = 201, 1024
    batch = list(C.random_batch(2, h, w, 7))
    first, second = 7, 7 + 1024 * 200
    batch[0].reshape(2, -1)[0, [first, second]] = 2.0
    batch[2].reshape(2, -1)[1, [first, second]] = 2.0
    got = _run(batch)
    C.assert_rows_close(got, E.metrics_spec(*batch), "tie in one thread")
    assert tuple(got[0, 0:2]) == (0, 7) and tuple(got[1, 2:4]) == (0, 7)


@pytest.mark.parametrize("h,w", [(8, 1024),       # n % 4 == 0: thread = (index / 4) % 1024
                                 (7, 1023)])      # scalar path: thread = index % 1024
def test_ties_across_waves(h, w):
    """The (value, smaller index) rule of the merge over the 16 per-wave slots, in both maps: index 1023 against 2048 and 3072
    against 1023 + 5 * 1024 (the pairs of test_losses_gpu.test_eval_postprocess_scan_edges).  Vector path: 1023 sits in wave 3,
    2048 in wave 8 (the later wave holds the larger index and must not win); 3072 in wave 12, 6143 in wave 7 (the later wave
    holds the smaller index and must win).  Scalar path: 1023 in wave 15 against 2048 in wave 0; 3072 in wave 0 against 6143 in
    wave 15."""
    pairs = ((1023, 2048), (3072, 1023 + 5 * 1024))
    assert pairs[1][1] < h * w
    batch = list(C.random_batch(4, h, w, 11))
    for k, (lo, hi) in enumerate(pairs):
        batch[0].reshape(4, -1)[k, [lo, hi]] = 2.0               # heat-map ties in samples 0, 1
        batch[2].reshape(4, -1)[2 + k, [lo, hi]] = 2.0           # GT-map ties in samples 2, 3
    got = _run(batch)
    C.assert_rows_close(got, E.metrics_spec(*batch), ("ties", h, w))
    for k, (lo, hi) in enumerate(pairs):
        assert tuple(got[k, 0:2]) == divmod(lo, w) and tuple(got[2 + k, 2:4]) == divmod(lo, w)


def test_out_slice_of_a_larger_table():
    from ccvpe_amd import ops
    batch = C.random_batch(3, 8, 12, 8)
    dev = _dev(batch)
    whole = ops.eval_metrics(*dev).cpu()
    table = torch.full((5, 12), -7.0, device="cuda", dtype=torch.float64)
    r0 = ops.eval_metrics(*[t[0:2] for t in dev], out=table[0:2])
    ops.eval_metrics(*[t[2:3] for t in dev], out=table[2:3])
    assert r0.data_ptr() == table.data_ptr()
    host = table.cpu()
    assert torch.equal(host[3:], torch.full((2, 12), -7.0, dtype=torch.float64))
    assert torch.equal(host[:3].view(torch.int64), whole.view(torch.int64))
    with pytest.raises(ValueError):
        ops.eval_metrics(*dev, out=table[0:2])                                            # [2,12] for B = 3


def test_argument_checks():
    from ccvpe_amd import ops
    lib = _lib.load()
    for b, h in ((0, 8), (2, 0)):
        heat = torch.zeros((b, 1, h, 12), device="cuda")
        ori = torch.zeros((b, 2, h, 12), device="cuda")
        hd = torch.zeros((b,), device="cuda", dtype=torch.float64)
        with pytest.raises(_lib.CcvpeError, match="bad shape"):
            ops.eval_metrics(heat, ori, heat, ori, hd, hd)
    dev = _dev(C.random_batch(2, 8, 12, 9))
    rows = torch.full((2 * 12 + 1,), -7.0, device="cuda", dtype=torch.float64)
    ptr = [ctypes.c_void_p(t.data_ptr()) for t in dev]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    with pytest.raises(_lib.CcvpeError, match="null"):
        _lib.check(lib.ccvpe_eval_metrics_f32(ptr[0], ptr[1], None, ptr[3], ptr[4], ptr[5], ctypes.c_void_p(rows.data_ptr()),
                                              2, 8, 12, stream), "ccvpe_eval_metrics_f32")
    with pytest.raises(_lib.CcvpeError, match="8-byte aligned"):
        _lib.check(lib.ccvpe_eval_metrics_f32(ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], ptr[5],
                                              ctypes.c_void_p(rows.data_ptr() + 4), 2, 8, 12, stream), "ccvpe_eval_metrics_f32")
    torch.cuda.synchronize()
    assert bool((rows.cpu() == -7.0).all())                                               # nothing was launched
    with pytest.raises(ValueError):
        ops.eval_metrics(dev[0], dev[1], dev[2], dev[3], dev[4].float(), dev[5])          # heading must be float64


def test_evaluate_batches_end_to_end(tmp_path, synth_sd, monkeypatch):
    """5 KITTI test samples in batches of 2 through CVM_KITTI: evaluate_batches' rows against metrics_spec applied to the same
    forward's outputs and the same batches' ground truth (recorded on the device, copied to the host afterwards, batch by batch);
    n, order, recall counts; and ONE read-back — the table's — after the last forward."""
    from ccvpe_amd import datasets as DS, models
    from test_datasets import make_kitti_tree
    train_file, test_file, names = make_kitti_tree(str(tmp_path), per_drive=3)
    with open(test_file) as f:
        lines = f.readlines()
    with open(test_file, "w") as f:
        f.write("".join(lines[:5]))
    ds = DS.KITTIPairs(str(tmp_path), test_file, 20, 20, 10, test=True)
    assert len(ds) == 5
    net = models.CVM_KITTI("cuda")
    net.load_state_dict(synth_sd("kitti", 0), strict=True)
    net = net.to("cuda:0").eval()
    log, outputs, seen = [], [], []

    def forward(grd, sat):
        out = net(grd, sat)
        outputs.append((out[1], out[2]))
        log.append("forward")
        return out

    class Recording(DS.DeviceBatches):
        def __iter__(self):
            for batch in super().__iter__():
                seen.append(batch)
                yield batch

    real_cpu = torch.Tensor.cpu

    def counting_cpu(self, *a, **kw):
        if self.is_cuda and self.dtype == torch.float64 and self.dim() == 2 and self.shape[1] == 12:
            log.append("table.cpu")
        return real_cpu(self, *a, **kw)

    batches = Recording(ds, batch_size=2, device="cuda", workers=2, targets=True, n_bins=16, grd_hw=(256, 1024))
    monkeypatch.setattr(torch.Tensor, "cpu", counting_cpu)
    res = E.evaluate_batches(forward, batches)
    monkeypatch.setattr(torch.Tensor, "cpu", real_cpu)
    assert log == ["forward"] * 3 + ["table.cpu"], log
    assert res["n"] == 5 and res["indices"].tolist() == [0, 1, 2, 3, 4] and res["rows"].shape == (5, 12)
    want = []
    for batch, (heat, ori) in zip(seen, outputs):
        heading = batch.heading_deg.cpu().numpy()
        assert heading.dtype == np.float64 and heading.tolist() == [ds.sample(i)["angle_deg"] for i in batch.indices]
        want.append(E.metrics_spec(heat.cpu(), ori.cpu(), batch.gt.cpu(), batch.gt_ori.cpu(), heading,
                                   np.full(len(batch.indices), ds.meter_per_pixel)))
    want = np.concatenate(want)
    C.assert_rows_close(res["rows"], want, "end to end")
    spec = E.summarise(want)
    for key in ("lateral_within", "longitudinal_within", "orientation_within"):
        assert res[key] == spec[key], key
    assert res["lateral_within"] == {t: float(np.sum(want[:, 7] < t) / 5) for t in (1, 3, 5)}
    assert abs(res["mean_metre_error"] - float(np.mean(want[:, 5]))) < 1e-9
    assert "sets" not in res
    print(E.format_report(res, "kitti"))
