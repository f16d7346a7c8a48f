"""Inputs shared by tests/test_eval_metrics.py (CPU) and tests/test_eval_metrics_gpu.py: the twelve hand-placed cases of the
reference test protocols' per-sample loop, seeded random batches, and `restate` — what that loop (train_KITTI.py:309-343,
train_OxfordRobotCar.py:218-246, train_VIGOR.py:294-326) computes per sample, restated in this file's own words from the column
table of the kernel's contract, independently of ccvpe_amd.evaluate.metrics_spec."""
import math
from collections import namedtuple

import numpy as np

H, W = 8, 12
SEED = 20
KITTI_MPP = 0.19582850865
Case = namedtuple("Case", "name pred gt pred_cs gt_cs heading mpp also_pred also_gt")


def cs(deg):
    """(cos, sin) of an angle in degrees, rounded to float32 as a network output / a ground-truth map holds them"""
    return (np.float32(math.cos(math.radians(deg))), np.float32(math.sin(math.radians(deg))))


# pred / gt: (y, x) of the maximum; also_pred / also_gt: a LATER pixel holding the same value (a tie: the first index wins)
CASES = (
    Case("sin<0 on the predicted side", (1, 2), (6, 9), cs(250.0), cs(40.0), 12.25, KITTI_MPP, None, None),
    Case("sin<0 on the GT side", (5, 3), (2, 10), cs(75.0), cs(290.0), 301.5, 0.75, None, None),
    Case("|cos| > 1: NaN row", (3, 3), (4, 8), (np.float32(1.0000001), np.float32(0.0)), cs(10.0), 45.0, 0.6, None, None),
    Case("|sin| > 1: NaN row", (7, 0), (0, 11), (np.float32(0.0), np.float32(-1.0000001)), cs(200.0), 200.0, 0.5, None, None),
    Case("wrap: GT 359, prediction 1 -> 2", (2, 2), (3, 6), cs(1.0), cs(359.0), 77.0, 0.14156, None, None),
    Case("pred == gt: distance 0, atan2(0, 0)", (4, 5), (4, 5), cs(100.0), cs(103.5), 33.0, 0.9, None, None),
    Case("heading 0", (0, 0), (7, 11), cs(181.0), cs(179.0), 0.0, 0.7, None, None),
    Case("heading 90", (6, 1), (1, 7), cs(0.0), cs(0.5), 90.0, 0.8, None, None),
    Case("heading 135.5", (2, 9), (5, 1), cs(300.0), cs(20.0), 135.5, 0.65, None, None),
    Case("heading 360 (no wrap)", (1, 10), (6, 4), cs(45.0), cs(52.0), 360.0, 0.55, None, None),
    Case("tie in the heat-map", (3, 7), (5, 2), cs(90.0), cs(94.0), 250.0, 0.45, (6, 1), None),
    Case("tie in the GT map, sin<0 on both sides", (6, 6), (0, 3), cs(270.0), cs(190.0), 18.0, 0.85, None, (0, 4)),
)


def _maps(rng, b, h, w):
    """seeded float32 inputs: a softmax-like heat-map, a blob-like GT map, unit orientation fields"""
    heat = rng.random((b, 1, h, w)).astype(np.float32)
    heat /= heat.sum(axis=(2, 3), keepdims=True)
    gt = rng.random((b, 1, h, w)).astype(np.float32)
    ang = rng.random((2, b, h, w)) * 2 * math.pi
    ori = np.stack([np.cos(ang[0]), np.sin(ang[0])], axis=1).astype(np.float32)
    gt_ori = np.stack([np.cos(ang[1]), np.sin(ang[1])], axis=1).astype(np.float32)
    return heat, ori, gt, gt_ori


def case_batch(cases=CASES, h=H, w=W, seed=SEED):
    """(heatmap, ori, gt, gt_ori, heading, mpp) with one sample per case"""
    rng = np.random.default_rng(seed)
    heat, ori, gt, gt_ori = _maps(rng, len(cases), h, w)
    for i, c in enumerate(cases):
        top, gtop = np.float32(heat[i].max() * 2), np.float32(gt[i].max() + 0.5)
        for p in (c.pred, c.also_pred):
            if p is not None:
                heat[i, 0, p[0], p[1]] = top
        for p in (c.gt, c.also_gt):
            if p is not None:
                gt[i, 0, p[0], p[1]] = gtop
        ori[i, :, c.pred[0], c.pred[1]] = c.pred_cs
        gt_ori[i, :, c.gt[0], c.gt[1]] = c.gt_cs
    heading = np.array([c.heading for c in cases], dtype=np.float64)
    mpp = np.array([c.mpp for c in cases], dtype=np.float64)
    return heat, ori, gt, gt_ori, heading, mpp


def random_batch(b, h, w, seed):
    """seeded maps with their maxima wherever the generator put them; headings in [0, 360), KITTI-like resolutions"""
    rng = np.random.default_rng(seed)
    heat, ori, gt, gt_ori = _maps(rng, b, h, w)
    return heat, ori, gt, gt_ori, rng.random(b) * 360.0, 0.1 + rng.random(b) * 0.2


class Restated(object):
    """What the test protocols keep per sample, as parallel lists.  `pred_angle` has one entry per sample (None where the
    orientation vector at the arg-max is not a valid cosine / sine pair); `angle_errors` has entries for the valid samples only,
    so it may be shorter than the other lists — the statistics of the protocols run over exactly that shorter list."""

    def __init__(self):
        self.pred, self.truth = [], []                      # (y, x) of the two arg-max pixels
        self.pixels, self.metres = [], []                   # distance between them
        self.along, self.across = [], []                    # metres along / across the vehicle's heading
        self.pred_angle, self.angle_errors = [], []         # degrees
        self.p_pred, self.p_truth = [], []                  # heat-map values (float32 scalars, as read)


def _first_max_yx(plane):
    """(y, x) of the first maximum of a 2-D map in row-major order"""
    k = int(np.argmax(plane.reshape(-1)))
    return divmod(k, plane.shape[1])


def _unit_to_degrees(c, s, clamp):
    """angle in degrees of a (cos, sin) pair read from a float32 map: acos of the cosine (widened to double), mirrored to the
    lower half circle when the sine is negative — Python's `-angle % 360`, which maps -0.0 to 0.0"""
    c = float(c)
    if clamp:
        c = min(1.0, max(-1.0, c))
    up = math.degrees(math.acos(c))
    return up if not s < 0 else (-up) % 360


def restate(heat, ori, truth, truth_ori, heading, mpp, select=None):
    """The twelve columns of the issue's table, sample by sample in plain Python floats and ints, written from that table and
    not from ccvpe_amd.evaluate.metrics_spec.  heat, truth [B,1,h,w]; ori, truth_ori [B,2,h,w] float32; heading (degrees, used
    as given) and mpp (metres per pixel) [B].  select: the samples to visit (all by default)."""
    out = Restated()
    for n in (range(heat.shape[0]) if select is None else select):
        py, px = _first_max_yx(heat[n, 0])
        ty, tx = _first_max_yx(truth[n, 0])
        dy, dx = ty - py, tx - px                                               # Python ints
        d = math.sqrt(dy * dy + dx * dx)
        off_heading = abs(float(heading[n]) - math.atan2(abs(dx), abs(dy)) * 180 / math.pi)     # atan2(0, 0) = 0
        turn = off_heading * math.pi / 180
        out.pred.append((py, px))
        out.truth.append((ty, tx))
        out.pixels.append(d)
        out.metres.append(d * float(mpp[n]))
        out.along.append(abs(math.cos(turn) * d) * float(mpp[n]))
        out.across.append(abs(math.sin(turn) * d) * float(mpp[n]))
        c, s = ori[n, 0, py, px], ori[n, 1, py, px]
        valid = bool(abs(c) <= np.float32(1) and abs(s) <= np.float32(1))      # decided in float32, where the maps live
        out.pred_angle.append(_unit_to_degrees(c, s, clamp=False) if valid else None)
        if valid:
            gap = abs(_unit_to_degrees(truth_ori[n, 0, ty, tx], truth_ori[n, 1, ty, tx], clamp=True) - out.pred_angle[-1])
            out.angle_errors.append(min(gap, 360 - gap))
        out.p_pred.append(heat[n, 0, py, px])
        out.p_truth.append(heat[n, 0, ty, tx])
    return out


def rows_of(r):
    """[n,12] float64 in ccvpe_eval_metrics_f32's column order from a Restated (NaN in columns 8, 9 of an invalid sample)"""
    rows = np.full((len(r.pixels), 12), np.nan)
    errors = iter(r.angle_errors)
    for i in range(rows.shape[0]):
        rows[i, 0:2], rows[i, 2:4] = r.pred[i], r.truth[i]
        rows[i, 4:8] = r.pixels[i], r.metres[i], r.along[i], r.across[i]
        if r.pred_angle[i] is not None:
            rows[i, 8], rows[i, 9] = r.pred_angle[i], next(errors)
        rows[i, 10], rows[i, 11] = r.p_pred[i], r.p_truth[i]
    return rows


def assert_rows_close(got, want, what=""):
    """The kernel's bound: columns 0-3, 10, 11 (indices, values read) bit-equal; columns 4-9 within 1e-9 absolute + 1e-9 relative
    with identical NaN positions.  Derived, not measured: the values are <= 1e3 and a handful of double roundings apart
    (~1e-13); a tail computed in float32 sits at ~1e-5 and fails."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    exact = [0, 1, 2, 3, 10, 11]
    assert np.array_equal(got[:, exact].view(np.int64), want[:, exact].view(np.int64)), (what, got[:, exact], want[:, exact])
    g, w_ = got[:, 4:10], want[:, 4:10]
    assert np.array_equal(np.isnan(g), np.isnan(w_)), (what, g, w_)
    ok = ~np.isnan(w_)
    err = np.abs(g[ok] - w_[ok])
    assert np.all(err <= 1e-9 + 1e-9 * np.abs(w_[ok])), (what, float(err.max()))
