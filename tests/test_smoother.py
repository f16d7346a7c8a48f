"""The forward-backward smoother on the CPU: the specifications (tracking.smooth_step_spec, smooth_step_rigid_spec,
invert_motion) against first principles, and the argument checks of the C entry points and of SequenceSmoother."""
import numpy as np
import pytest

import smoother_cases as SC
import test_tracking_gpu as G
from ccvpe_amd import _lib, tracking as T

U24 = 2.0 ** -24


def test_the_back_predict_is_the_exact_adjoint_of_the_predict():
    """<g, predict(p)> = <B'(g), p> for random non-negative p, g on 23 x 31, R = 4, a fractional shift, within 1e-13 relative.
    B' is read out of smooth_step_spec as V with alpha = 1 and beta = 1; g enters as the heat-map with outlier = 0, so that
    M = g (with outlier = 1 the measurement would be the constant 1 / (h w) and g would not enter at all)."""
    rng = np.random.default_rng(0)
    h, w, radius = 23, 31, 4
    p, g = rng.random((1, h, w)).astype(np.float32), rng.random((1, h, w)).astype(np.float32)
    offsets, taps = T.motion_taps_spec([[2.3, -3.6]], 1.3, radius)
    assert offsets.tolist() == [[2, -4]]
    q = T._predict_spec(p[0].astype(np.float64), offsets[0, 0], offsets[0, 1], taps[0, 0], taps[0, 1])
    ones = np.ones((1, h, w), np.float32)
    _, _, rows, v = T.smooth_step_spec(ones, g, ones, G.unit_ori(rng, 1, h, w), offsets, taps, outlier=0.0, return_v=True)
    lhs, rhs = float((g[0].astype(np.float64) * q).sum()), float((v[0] * p[0].astype(np.float64)).sum())
    assert lhs > 0 and abs(lhs - rhs) <= 1e-13 * lhs, (lhs, rhs)
    assert rows[0, T.RESET] == 0 and rows[0, T.SURVIVED] == pytest.approx(float(v[0].sum()), rel=1e-14)


def test_the_chain_gives_the_exact_smoothed_marginals():
    """5 x 6 grid, 4 frames, R = 1, one start (frame 0): the dense transition matrices are built by applying _predict_spec to
    one-hot maps, the smoothed marginals by a dense float64 forward-backward; the chain step_spec -> smooth_step_spec must
    match them.

    Bound.  u = 2^-24.  Both computations are sums and products of non-negative numbers, so a relative perturbation of the
    inputs of a step passes through it without growing, and common scale factors (the fp32 casts of 1 / Z and 1 / S) drop out
    at the next normalisation.  The chain departs from exact arithmetic only where it stores fp32: each posterior (+ u per
    frame: alpha_s carries (s + 1) u), each message (+ u per step: the message read at frame s carries (T - 1 - s) u), and
    the smoothed map itself (the cast of 1 / Z and the store: 2 u).  Per pixel before normalisation that is (T + 2) u; the
    normalised ratio at most doubles it: 2 (T + 2) u = 12 u for T = 4.  float64 rounding (1e-16) is far below."""
    h, w, n, radius, outlier = 5, 6, 4, 1, 0.05
    rng = np.random.default_rng(1)
    heat, ori = G.softmax_maps(rng, n, h, w), G.unit_ori(rng, n, h, w)
    offsets, taps = T.motion_taps_spec([[0, 0], [1.3, -0.6], [-0.8, 1.2], [0.4, 0.7]], 0.7, radius)
    hw = h * w
    trans = np.zeros((n, hw, hw))                                               # trans[t][:, k] = predict of the one-hot map k
    for t in range(1, n):
        for k in range(hw):
            e = np.zeros(hw)
            e[k] = 1.0
            trans[t][:, k] = T._predict_spec(e.reshape(h, w), offsets[t, 0], offsets[t, 1], taps[t, 0], taps[t, 1]).reshape(-1)
    m = (1 - np.float64(np.float32(outlier))) * heat.reshape(n, hw).astype(np.float64) + np.float64(np.float32(outlier)) / hw
    alpha = np.zeros((n, hw))
    alpha[0] = m[0] / m[0].sum()
    for t in range(1, n):
        a = m[t] * (trans[t] @ alpha[t - 1])
        alpha[t] = a / a.sum()
    beta = np.ones((n, hw))
    for t in range(n - 2, -1, -1):
        b = trans[t + 1].T @ (m[t + 1] * beta[t + 1])
        beta[t] = b / b.sum()
    want = alpha * beta
    want /= want.sum(axis=1, keepdims=True)
    # the chain
    posts = np.zeros((n, h, w), np.float32)
    for t in range(n):
        prior = posts[t - 1:t] if t else np.zeros((1, h, w), np.float32)
        posts[t] = T.step_spec(prior, heat[t:t + 1], ori[t:t + 1], offsets[t:t + 1], taps[t:t + 1], outlier, reset=[int(t == 0)])[0][0]
    msg = np.ones((1, h, w), np.float32)
    bound = 2 * (n + 2) * U24
    for t in range(n - 1, -1, -1):
        nxt = min(t + 1, n - 1)
        sm, msg, rows = T.smooth_step_spec(msg, heat[nxt:nxt + 1], posts[t:t + 1], ori[t:t + 1], offsets[nxt:nxt + 1],
                                           taps[nxt:nxt + 1], outlier, cut=[int(t == n - 1)])
        assert rows[0, T.RESET] == int(t == n - 1)
        err = np.abs(sm[0].reshape(-1).astype(np.float64) - want[t]) / want[t]
        print("frame %d: max relative error %.2f u" % (t, err.max() / U24))
        assert np.all(err <= bound), (t, err.max() / U24)


def test_states():
    h, w, radius = 12, 14, 1
    rng = np.random.default_rng(2)
    beta, heat, alpha, ori = G.softmax_maps(rng, 1, h, w), G.softmax_maps(rng, 1, h, w), G.softmax_maps(rng, 1, h, w), G.unit_ori(rng, 1, h, w)
    offsets, taps = T.motion_taps_spec([[2.0, -1.0]], 0.6, radius)
    fallback = (alpha[0].astype(np.float64) * np.float64(np.float32(1.0 / float(alpha[0].astype(np.float64).sum())))).astype(np.float32)
    uniform = np.full((h, w), np.float32(1.0 / (h * w)), np.float32)
    # cut: alpha renormalised, a uniform message, S = 0
    sm, msg, rows = T.smooth_step_spec(beta, heat, alpha, ori, offsets, taps, 0.1, cut=[1])
    assert np.array_equal(sm[0], fallback) and np.array_equal(msg[0], uniform)
    assert rows[0, T.RESET] == 1 and rows[0, T.SURVIVED] == 0 and rows[0, T.EVIDENCE] == float(alpha[0].astype(np.float64).sum())
    assert (rows[0, T.PRED_Y], rows[0, T.PRED_X]) == np.unravel_index(np.argmax(alpha[0]), (h, w))
    # a message that is zero where the back-predicted mass would meet alpha: a one-hot alpha at (5, 6) reads G around (7, 5)
    hot = np.zeros((1, h, w), np.float32)
    hot[0, 5, 6] = 1.0
    holed = beta.copy()
    holed[0, 6:9, 4:7] = 0.0
    sm, msg, rows = T.smooth_step_spec(holed, heat, hot, ori, offsets, taps, 0.1)
    assert rows[0, T.RESET] == 2 and rows[0, T.SURVIVED] > 0 and rows[0, T.EVIDENCE] == 1.0
    assert np.array_equal(sm[0], hot[0]) and np.array_equal(msg[0], uniform)
    filled = T.smooth_step_spec(beta, heat, hot, ori, offsets, taps, 0.1)[2]
    assert filled[0, T.RESET] == 0                                              # the hole is what made it state 2
    # an offset beyond the grid: nothing comes back, S = 0
    sm, msg, rows = T.smooth_step_spec(beta, heat, alpha, ori, [[h + 5, 0]], taps, 0.1)
    assert rows[0, T.RESET] == 2 and rows[0, T.SURVIVED] == 0
    assert np.array_equal(sm[0], fallback) and np.array_equal(msg[0], uniform)
    # INT_MIN offsets are negated in Python integers, not in int32
    rows = T.smooth_step_spec(beta, heat, alpha, ori, np.array([[-2 ** 31, -2 ** 31]], np.int32), taps, 0.1)[2]
    assert rows[0, T.RESET] == 2 and rows[0, T.SURVIVED] == 0


def _compose(a, b):
    """the row of (y, x) -> a(b(y, x))"""
    la, lb = np.array([[a[0], a[1]], [a[3], a[4]]]), np.array([[b[0], b[1]], [b[3], b[4]]])
    lin = la @ lb
    tr = la @ np.array([b[2], b[5]]) + np.array([a[2], a[5]])
    return np.array([lin[0, 0], lin[0, 1], tr[0], lin[1, 0], lin[1, 1], tr[1]])


IDENTITY = np.array([1.0, 0, 0, 0, 1.0, 0])


def test_invert_motion():
    hw = (48, 48)
    for angle in (0.0, 90.0, 180.0, 270.0, 33.3):
        for shift in ([0.0, 0.0], [7.0, -40.0], [-12.25, 3.7], [40.0, 40.0]):
            m = T.rigid_motion([shift], angle, hw)
            inv = T.invert_motion(m)
            assert inv.shape == (1, 6) and inv.dtype == np.float64
            for c in (_compose(inv[0], m[0]), _compose(m[0], inv[0])):
                assert np.all(np.abs(c - IDENTITY) <= 1e-12), (angle, shift, c)
            if angle != 33.3 and shift in ([0.0, 0.0], [7.0, -40.0], [40.0, 40.0]):
                assert np.array_equal(_compose(inv[0], m[0]), IDENTITY) and np.array_equal(T.invert_motion(inv), m)
    bad = T.invert_motion([[1, 2, 0, 2, 4, 0], [np.nan, 0, 0, 0, 1, 0], [1, 0, np.inf, 0, 1, 0], [0, 0, 0, 0, 0, 0], [2, 0, 1, 0, 4, 3]])
    assert np.isnan(bad[:4]).all() and np.array_equal(bad[4], [0.5, 0, -0.5, 0, 0.25, -0.75])


def test_rigid_specification_equals_the_translate_one_for_exact_motions():
    """Angle 0 with whole-pixel shifts: the translate specification with those offsets.  Quarter turns with whole-pixel
    shifts on a square grid: the translate specification on the maps of frame t turned back (rot90 by -k) with the shift
    brought into the turned frame, o = A s (A the linear part of the forward row).  Centred taps; value for value."""
    rng = np.random.default_rng(3)
    h, w, radius = 37, 53, 3
    beta, heat, alpha, ori = [G.softmax_maps(rng, 3, h, w) for _ in range(3)] + [G.unit_ori(rng, 3, h, w)]
    _, taps = T.motion_taps_spec(np.zeros((3, 2)), [1.0, 0.5, 1.2], radius)
    shifts = np.array([[3, -7], [-30, 20], [0, 0]])
    for cut in (None, [0, 1, 0]):
        a = T.smooth_step_rigid_spec(beta, heat, alpha, ori, T.rigid_motion(shifts, 0.0, (h, w)), taps, 0.03125, cut=cut, return_v=True)
        b = T.smooth_step_spec(beta, heat, alpha, ori, shifts.astype(np.int32), taps, 0.03125, cut=cut, return_v=True)
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True)
    n = 48
    beta, heat, alpha, ori = [G.softmax_maps(rng, 2, n, n) for _ in range(3)] + [G.unit_ori(rng, 2, n, n)]
    _, taps = T.motion_taps_spec(np.zeros((2, 2)), [1.0, 0.7], radius)
    for k in (1, 2, 3):
        shifts = np.array([[0, 0], [5, -9]])
        motion = T.rigid_motion(shifts, 90.0 * k, (n, n))
        offsets = np.stack([motion[:, 0] * shifts[:, 0] + motion[:, 1] * shifts[:, 1],
                            motion[:, 3] * shifts[:, 0] + motion[:, 4] * shifts[:, 1]], 1).astype(np.int32)
        back = lambda x: np.ascontiguousarray(np.rot90(x, -k, axes=(1, 2)))
        a = T.smooth_step_rigid_spec(beta, heat, alpha, ori, motion, taps, 0.03125, return_v=True)
        b = T.smooth_step_spec(back(beta), back(heat), alpha, ori, offsets, taps, 0.03125, return_v=True)
        assert a[2][:, T.RESET].tolist() == [0, 0]
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True), k
    # a singular row samples nothing: state 2
    rows = T.smooth_step_rigid_spec(beta, heat, alpha, ori, [[1, 1, 0, 1, 1, 0], [np.nan] * 6], taps, 0.03125)[2]
    assert rows[:, T.RESET].tolist() == [2, 2] and rows[:, T.SURVIVED].tolist() == [0, 0]


def test_smoothing_the_moved_distractor_track_beats_the_filter():
    """Generator seed 3, the stronger distractor in the frames t % 3 == 0, starts at frames 0 and 12: the filter has nothing
    but one ambiguous heat-map at a start; the smoother brings the later frames back.  A float64 prototype of the
    specification gave 0.42 px against 1.90 px mean arg-max error, 0.0 / 0.4 px at the two starts (the filter: 26.4 / 8.9 px),
    and a smallest top-2 margin of V of 3.7e-2."""
    s = SC.moved_scenario()
    radius = SC.TRK["radius"]
    offsets, taps = T.motion_taps_spec(s["odo"], SC.TRK["sigma"], radius)
    c = SC.spec_chain(offsets, taps)
    G.assert_margin(c["vs"], radius, "moved track")
    assert c["rows"][:, T.RESET].tolist() == [float(t in SC.STARTS) for t in range(24)]
    assert c["srows"][:, T.RESET].tolist() == [float(t in (11, 23)) for t in range(24)]
    fil = np.hypot(c["rows"][:, T.PRED_Y] - s["pos"][:, 0], c["rows"][:, T.PRED_X] - s["pos"][:, 1])
    smo = np.hypot(c["srows"][:, T.PRED_Y] - s["pos"][:, 0], c["srows"][:, T.PRED_X] - s["pos"][:, 1])
    print("moved track: filtered %.3f px, smoothed %.3f px; starts: filtered %s, smoothed %s"
          % (fil.mean(), smo.mean(), fil[list(SC.STARTS)], smo[list(SC.STARTS)]))
    assert smo.mean() < fil.mean()
    assert np.all(smo[list(SC.STARTS)] <= 1.5)


def _fake():
    return dict(beta=0x100000, heat=0x200000, alpha=0x300000, ori=0x400000, move=0x600000, taps=0x700000, beta_out=0x800000,
                smooth=0x900000, scratch=0xa00000, rows=0xb00000)


@pytest.mark.parametrize("entry", ["ccvpe_belief_smooth_step_f32", "ccvpe_belief_smooth_step_rigid_f32"])
def test_smooth_step_rejects_bad_arguments_without_a_gpu(entry):
    """Both entry points validate before they launch (fake aligned pointers that are never dereferenced): CCVPE_EINVAL and a
    message, nothing enqueued."""
    lib = _lib.load()
    fn = getattr(lib, entry)
    EINVAL = -1
    n = 64 * 64 * 4                                                             # bytes of one map; B = 2

    def call(radius=8, outlier=0.1, batch=2, h=64, w=64, **kw):
        a = dict(_fake(), **kw)
        return fn(a["beta"], a["heat"], a["alpha"], a["ori"], a["move"], a["taps"], radius, outlier, None, a["beta_out"], a["smooth"],
                  a["scratch"], a["rows"], batch, h, w, None)

    f = _fake()
    assert call(radius=33) == EINVAL and b"radius" in lib.ccvpe_last_error()
    assert call(radius=-1) == EINVAL and b"radius" in lib.ccvpe_last_error()
    assert call(outlier=1.5) == EINVAL and b"outlier" in lib.ccvpe_last_error()
    assert call(outlier=float("nan")) == EINVAL and b"outlier" in lib.ccvpe_last_error()
    for name in ("beta", "heat", "alpha", "ori", "move", "taps", "beta_out", "smooth", "scratch", "rows"):
        assert call(**{name: None}) == EINVAL and b"null" in lib.ccvpe_last_error(), name
    assert call(rows=f["rows"] + 4) == EINVAL and b"8-byte" in lib.ccvpe_last_error()
    assert call(scratch=f["scratch"] + 4) == EINVAL and b"8-byte" in lib.ccvpe_last_error()
    for name in ("beta", "alpha", "beta_out", "smooth"):
        assert call(**{name: f[name] + 2}) == EINVAL and b"4-byte" in lib.ccvpe_last_error(), name
    if entry.endswith("rigid_f32"):
        assert call(move=f["move"] + 4) == EINVAL and b"motion must be 8-byte" in lib.ccvpe_last_error()
    # neither output may share memory with the other or with an input map: the first and the last float of either side
    for out in ("beta_out", "smooth"):
        for name, maps in (("beta", 1), ("heat", 1), ("alpha", 1), ("ori", 2)):
            assert call(**{out: f[name]}) == EINVAL and b"overlap" in lib.ccvpe_last_error(), (out, name)
            assert call(**{out: f[name] + 2 * maps * n - 4}) == EINVAL and b"overlap" in lib.ccvpe_last_error(), (out, name)
            assert call(**{out: f[name] - 2 * n + 4}) == EINVAL and b"overlap" in lib.ccvpe_last_error(), (out, name)
    assert call(beta_out=f["smooth"] + 2 * n - 4) == EINVAL and b"smooth and beta_out overlap" in lib.ccvpe_last_error()
    assert call(smooth=f["beta_out"] + 2 * n - 4) == EINVAL and b"smooth and beta_out overlap" in lib.ccvpe_last_error()
    assert call(h=0) == EINVAL and b"shape" in lib.ccvpe_last_error()
    assert call(batch=0) == EINVAL and b"shape" in lib.ccvpe_last_error()
    assert call(h=65536, w=65536) == EINVAL


def test_sequence_smoother_refuses_bad_settings():
    for kw in (dict(sigma_px=-1.0), dict(sigma_px=float("nan")), dict(sigma_px=20.0), dict(radius=33), dict(radius=-1),
               dict(outlier=1.5), dict(outlier=-0.1), dict(hw=(0, 5))):
        with pytest.raises(ValueError):
            T.SequenceSmoother(device="cpu", **kw)
    sm = T.SequenceSmoother((96, 80), sigma_px=1.5, outlier=0.05, device="cpu")
    assert sm.radius == 6 and sm.hw == (96, 80)
    import torch
    heat, ori = torch.zeros((3, 1, 96, 80)), torch.zeros((3, 2, 96, 80))
    with pytest.raises(ValueError):
        sm.run(heat, ori)                                                       # neither shift_px nor motion
    with pytest.raises(ValueError):
        sm.run(heat, ori, shift_px=np.zeros((3, 2)), motion=np.zeros((3, 6)))
    with pytest.raises(ValueError):
        sm.run(heat[:, :, :50], ori, shift_px=np.zeros((3, 2)))
    with pytest.raises(ValueError):
        sm.run(heat, ori, shift_px=np.zeros((2, 2)))
    with pytest.raises(ValueError):
        sm.run(heat, ori, motion=np.zeros((2, 6)))
    with pytest.raises(ValueError):
        sm.run(heat, ori, shift_px=np.zeros((3, 2)), starts=[1, 0])
