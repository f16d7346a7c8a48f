"""The frozen-BatchNorm fixtures (tools/make_golden_frozen.py: the reference in .train() with every BatchNorm2d in .eval())
pinned to the CPU oracle in fp32, so that they stay checked where the reference is not present: one oracle run with
train_stats=None (running statistics) and the injected drop_connect scales reproduces fwd_vigor_frozenbn, and its autograd
gradients of golden_util.train_loss pass compare_grads against grad_vigor_frozenbn.  Forward tolerance: 2e-5 (+ 2e-5 relative)
on O(1) logits, 2e-6 on the scores — fp32 round-off of two implementations of the same eval-mode BatchNorm arithmetic (the
generator measured the reference's logits 6.4e-7 of their scale from the float64 oracle's); tests/test_oracle_golden.py allows
the batch-statistic forward ten times the relative part."""
import os

import numpy as np
import pytest
import torch

import frozen_bn_util as FZ
import golden_util as G
from ccvpe_amd import synth
from oracle import ccvpe_oracle as O

RTOL, ATOL = 2e-5, 2e-5


@pytest.fixture(scope="module")
def oracle_frozen_step():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    c = G.TRAIN_CASE
    sd = synth.synthetic_state_dict(c["kind"], c["wseed"])
    params = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running_" not in k else v.clone())
              for k, v in sd.items()}
    grd, sat = synth.synthetic_pair(c["batch"], c["grd"], c["pseed"])
    _, scales, _ = G.train_drop_masks(c["batch"])
    out = O.forward(params, grd, sat, c["kind"], c["circular"], None, train_stats=None, drop_scales=scales)
    G.train_loss(out).backward()
    return [t.detach() for t in out], params


def test_oracle_reproduces_the_frozen_forward_fixture(oracle_frozen_step):
    out, _ = oracle_frozen_step
    want = G.load("fwd_vigor_frozenbn")
    got = G.summarize_forward(out)
    assert (got["top4_idx"][:, 0] == want["top4_idx"][:, 0]).all()
    G.assert_close(got["logits_s4"], want["logits_s4"], RTOL, ATOL, "frozen logits")
    for i in range(1, 7):
        G.assert_close(got["score%d" % i], want["score%d" % i], RTOL, 2e-6, "frozen score%d" % i)
    # not the batch-statistic forward: the two fixtures differ by far more than the tolerance
    other = G.load("fwd_vigor_trainmode")
    assert np.abs(other["logits_s4"] - want["logits_s4"]).max() > 100 * ATOL


def test_oracle_gradients_match_the_frozen_gradient_fixtures(oracle_frozen_step):
    _, params = oracle_frozen_step
    want = FZ.load_grads("grad_vigor_frozenbn")
    names = set(str(n) for n in want["names"])
    assert len(names) == 520
    got = G.summarize_grads([(k, v.grad) for k, v in params.items() if k in names])
    bad, med = G.compare_grads(got, want)
    assert not bad, bad[:10]
    assert med < 6e-3, med
    # the float64 fixture is the same gradient without the round-off
    truth = FZ.load_grads("grad_vigor_frozenbn_f64")
    bad64, med64 = G.compare_grads(want, truth)
    assert not bad64, bad64[:10]
    assert med64 < 6e-3, med64


def test_fixture_files_fit_the_committed_file_limit():
    for f in os.listdir(G.GOLDEN_DIR):
        if "frozenbn" in f:
            assert os.path.getsize(os.path.join(G.GOLDEN_DIR, f)) < FZ.MAX_FILE_BYTES, f
