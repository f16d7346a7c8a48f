"""Shared, read-only inputs of test_smoother.py (CPU) and test_smoother_gpu.py: the 24-frame track of test_tracking_gpu.py with
the stronger distractor moved to the frames t % 3 == 0 — so frame 0 and every start carry one — and starts at frames 0 and 12;
the specification's forward-backward chain over it, computed once."""
import numpy as np

import test_tracking_gpu as G
from ccvpe_amd import tracking as T

TRK = G.TRK
STARTS = (0, 12)
_MOVED = {}
_CHAIN = {}


def moved_scenario():
    """test_tracking_gpu.track_scenario with `t % 3 == 1` replaced by `t % 3 == 0` (same generator seed 3, same draws)."""
    if _MOVED:
        return _MOVED
    h, w, n = TRK["h"], TRK["w"], TRK["frames"]
    rng = np.random.default_rng(3)
    pos = np.array([40.0, 30.0])
    heats, odos, poss = [], [], []
    for t in range(n):
        step = rng.uniform(-3, 3, 2) if t else np.zeros(2)
        pos = np.clip(pos + step, 8, [h - 9, w - 9])
        logit = 0.3 * rng.standard_normal((h, w)) + 6 * G._gauss(h, w, pos[0], pos[1], 2.0)
        if t % 3 == 0:
            d = rng.uniform(10, [h - 10, w - 10])
            logit += 8 * G._gauss(h, w, d[0], d[1], 2.0)
        p = np.exp(logit - logit.max())
        heats.append((p / p.sum()).astype(np.float32))
        odos.append(step + rng.normal(0, 0.5, 2) if t else np.zeros(2))
        poss.append(pos.copy())
    starts = np.zeros(n, dtype=bool)
    starts[list(STARTS)] = True
    _MOVED.update(heat=np.stack(heats), odo=np.stack(odos), pos=np.stack(poss), ori=G.unit_ori(np.random.default_rng(4), n, h, w),
                  starts=starts)
    for a in _MOVED.values():
        a.setflags(write=False)
    return _MOVED


def spec_chain(offsets, taps):
    """The specification over the moved scenario with the given motion inputs.  Forward: priors, posts, rows.  Backward, frame
    t: beta_in[t] (the message of frame t + 1 that the step of frame t reads), smooth[t], beta[t] (the message it writes),
    srows[t], V[t]; cut[t].  Cached per motion input (the arrays are read-only)."""
    key = (offsets.tobytes(), taps.tobytes())
    if key in _CHAIN:
        return _CHAIN[key]
    s = moved_scenario()
    h, w, n = TRK["h"], TRK["w"], TRK["frames"]
    posts, rows = np.zeros((n, h, w), np.float32), np.zeros((n, 14))
    priors = np.zeros((n, h, w), np.float32)
    for t in range(n):
        if t:
            priors[t] = posts[t - 1]
        p, r = T.step_spec(priors[t:t + 1], s["heat"][t:t + 1], s["ori"][t:t + 1], offsets[t:t + 1], taps[t:t + 1], TRK["outlier"],
                           reset=[int(s["starts"][t])])
        posts[t], rows[t] = p[0], r[0]
    cut = np.ones(n, np.int32)
    cut[:-1] = (s["starts"][1:] | (rows[1:, T.RESET] != 0)).astype(np.int32)
    smooth, beta, beta_in = np.zeros((n, h, w), np.float32), np.zeros((n, h, w), np.float32), np.ones((n, h, w), np.float32)
    srows, vs = np.zeros((n, 14)), np.zeros((n, h, w))
    for t in range(n - 1, -1, -1):
        nxt = min(t + 1, n - 1)
        if t < n - 1:
            beta_in[t] = beta[t + 1]
        sm, bo, r, v = T.smooth_step_spec(beta_in[t:t + 1], s["heat"][nxt:nxt + 1], posts[t:t + 1], s["ori"][t:t + 1],
                                          offsets[nxt:nxt + 1], taps[nxt:nxt + 1], TRK["outlier"], cut=cut[t:t + 1], return_v=True)
        smooth[t], beta[t], srows[t], vs[t] = sm[0], bo[0], r[0], v[0]
    out = dict(priors=priors, posts=posts, rows=rows, cut=cut, beta_in=beta_in, smooth=smooth, beta=beta, srows=srows, vs=vs)
    for a in out.values():
        a.setflags(write=False)
    _CHAIN[key] = out
    return out
