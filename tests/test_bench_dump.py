"""`bench.py --dump-outputs DIR`: what the timed path returned in its last step goes to DIR/<name>.npy in float32 — the same
seeded subset of the batch for every output, at most 64 MB in all — so that two builds can be compared file by file."""
import os

import numpy as np
import torch

import bench


def _outs(batch):
    g = torch.Generator().manual_seed(0)
    shapes = [(batch, 262144), (batch, 1, 512, 512), (batch, 2, 512, 512), (batch, 20, 8, 8), (batch, 5, 16, 16),
              (batch, 5, 32, 32), (batch, 5, 64, 64), (batch, 5, 128, 128), (batch, 5, 256, 256)]
    return tuple(torch.randn(s, generator=g) for s in shapes)


def test_dump_is_a_seeded_batch_subset_within_the_budget(tmp_path):
    outs = _outs(64)
    names = bench.dump_outputs(str(tmp_path / "a"), outs)
    assert names == sorted(["batch_index", "logits", "heatmap", "orientation"] + ["score%d" % i for i in range(1, 7)])
    total = sum(os.path.getsize(str(tmp_path / "a" / (n + ".npy"))) for n in names)
    assert total <= bench.DUMP_BUDGET_BYTES
    idx = np.load(str(tmp_path / "a" / "batch_index.npy"))
    assert idx.dtype == np.float64 and len(idx) == 8 and len(set(idx.tolist())) == 8 and idx.max() < 64
    for name, t in zip(["logits", "heatmap", "orientation"] + ["score%d" % i for i in range(1, 7)], outs):
        a = np.load(str(tmp_path / "a" / (name + ".npy")))
        assert a.dtype == np.float32 and np.array_equal(a, t[torch.as_tensor(idx.astype(np.int64))].numpy())
    bench.dump_outputs(str(tmp_path / "b"), outs)
    for n in names:
        assert np.array_equal(np.load(str(tmp_path / "a" / (n + ".npy"))), np.load(str(tmp_path / "b" / (n + ".npy"))))


def test_dump_of_a_small_batch_and_of_extras(tmp_path):
    outs = _outs(2)
    names = bench.dump_outputs(str(tmp_path), outs, {"loss": torch.tensor([1.5], dtype=torch.float64)})
    assert "loss" in names and np.load(str(tmp_path / "loss.npy")).tolist() == [1.5]
    assert np.load(str(tmp_path / "batch_index.npy")).tolist() == [0.0, 1.0]
    assert np.load(str(tmp_path / "logits.npy")).shape == (2, 262144)
