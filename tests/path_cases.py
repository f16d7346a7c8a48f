"""Shared, read-only inputs of test_path.py (CPU) and test_path_gpu.py: the step cases, the six-frame backtrack drives, the
exact-tie drive and the specification's free-running chain over the two 24-frame scenarios, each computed once.

Bounds — derived, not tuned.  u = 2^-24.  The max-product predict is a maximum of products ky (kx prev): rounding is monotone,
so the device's max of rounded products is the rounded product at the winner — two roundings whatever R is, delta_P <= 2 u.
M = fma(1 - a, heat, a / (h w)) with both constants rounded once and the product P M add 4 u (test_tracking_gpu.py's terms):
delta_U = (2 + 4) u.  Z is a double sum of non-negative terms and inherits delta_U; post = U * (float)(1 / Z) adds the cast,
the product and the specification's own fp32 store: TOL_MAX = 2 delta_U + 4 u = 16 u relative, plus the suite's 2^-100
absolute.  An arg-max is compared only where the specification's own best value exceeds the second by more than 2 delta_U
relative.  A link of the backtrack is compared only where the specification's own margin exceeds LINK_MARGIN = 8 u: the
device's candidate values carry two roundings each (2 u), the two competitors 4 u together, doubled."""
import numpy as np

import smoother_cases as SC
import test_tracking_gpu as G
from ccvpe_amd import tracking as T

U24 = 2.0 ** -24
ABS = 2.0 ** -100
DELTA_U = 6 * U24
TOL_MAX = 16 * U24
LINK_MARGIN = 8 * U24
SIZES = [(37, 53), (70, 45), (16, 64)]
RADII = [0, 1, 5, 32]
FRAMES = 6
_CACHE = {}


def frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def assert_argmax_margin(u, rel, what):
    """the specification's own top-2 margin of every map of u [..., h, w] leaves room for `rel`"""
    flat = u.reshape(-1, u.shape[-2] * u.shape[-1])
    for k in range(flat.shape[0]):
        top = np.partition(flat[k], -2)[-2:]
        assert top[1] > 0 and (top[1] - top[0]) / top[1] > rel, (what, k, top)


def assert_link_margins(path, margin, rel, what):
    """every LINK 0 decision has a margin, and it exceeds `rel`: no link is excused"""
    chained = path[..., T.PATH_LINK] == 0
    assert np.array_equal(chained, ~np.isnan(margin)), what
    assert np.all(margin[chained] > rel), (what, float(margin[chained].min()) / U24)


def sigmas(radius):
    return np.zeros(3) if radius == 0 else np.array([radius / 3.0, radius / 2.5, radius / 4.0])


def step_case(h, w, radius):
    """test_tracking_gpu.three_tracks (a negative offset, (30, -40), one beyond the grid) with NaN planted in the previous map
    of tracks 0 and 1, inside the part the predict reads."""
    key = ("step", h, w, radius)
    if key not in _CACHE:
        prior, heat, ori, offsets, taps = G.three_tracks(h, w, radius, seed=300 + radius)
        prior = prior.copy()
        prior[0, h // 2, w // 3] = np.nan
        prior[0, 0, 0] = np.nan
        prior[1, 2, w - 3] = np.nan                                           # (30, -40) moves it to (32, w - 43) or off the grid
        _CACHE[key] = frozen(dict(prior=prior, heat=heat, ori=ori, offsets=offsets, taps=taps))
    return _CACHE[key]


def drive_case(h, w, radius):
    """T = 6, B = 3: random softmax maps and shifts; track 0 ends at a lone peak one pixel from the corner (its last
    windows are cut by the grid edge); track 1 restarts at frame 3; track 2 has a shift beyond the grid into frame 2 (the
    forward pass resets there: RESET 2).  The specification's forward chain (each frame from its own fp32 map), path and link
    margins."""
    key = ("drive", h, w, radius)
    if key in _CACHE:
        return _CACHE[key]
    n, b = FRAMES, 3
    rng = np.random.default_rng(1000 + 37 * radius + h)
    z = rng.standard_normal((n, b, h, w)) * 1.5
    z[:, 0] *= 0.2                                                              # track 0: shallow maps, so that its lone last peak wins
    heat = (np.exp(z) / np.exp(z).sum(axis=(2, 3), keepdims=True)).astype(np.float32)
    heat[n - 1, 0] = 0                                                          # only the outlier floor elsewhere
    heat[n - 1, 0, 0, 1] = 0.75
    ori = G.unit_ori(rng, n * b, h, w).reshape(n, b, 2, h, w)
    shifts = rng.uniform(-3.0, 3.0, (n, b, 2))
    shifts[:, 0] = rng.uniform(-0.45, 0.45, (n, 2))                             # offsets 0: no empty border moves in, the corner keeps mass
    shifts[2, 2] = (h + radius + 12.0, 3.0)
    reset = np.zeros((n, b), np.int32)
    reset[0] = 1
    reset[3, 1] = 1
    offsets, taps = T.motion_taps_spec(shifts.reshape(-1, 2), np.tile(sigmas(radius), n), radius)
    offsets, taps = offsets.reshape(n, b, 2), taps.reshape(n, b, 2, -1)
    deltas, rows, us = np.zeros((n, b, h, w), np.float32), np.zeros((n, b, 14)), np.zeros((n, b, h, w))
    for t in range(n):
        prev = deltas[t - 1] if t else np.zeros((b, h, w), np.float32)
        deltas[t], rows[t], us[t] = T.viterbi_step_spec(prev, heat[t], ori[t], offsets[t], taps[t], 0.03125, reset=reset[t],
                                                        return_u=True)
    path, margin = T.backtrack_spec(deltas, ori, offsets, taps, rows, reset, return_margin=True)
    _CACHE[key] = frozen(dict(heat=heat, ori=ori, offsets=offsets, taps=taps, reset=reset, deltas=deltas, rows=rows, us=us,
                              path=path, margin=margin, outlier=0.03125))
    return _CACHE[key]


def window_is_cut(case, radius):
    """some LINK 0 decision of the drive had candidates outside the grid"""
    p, o = case["path"], case["offsets"]
    h, w = case["deltas"].shape[-2:]
    for t in range(1, p.shape[0]):
        for k in range(p.shape[1]):
            if p[t - 1, k, T.PATH_LINK] == 0:
                cy, cx = p[t, k, T.PATH_Y] - o[t, k, 0], p[t, k, T.PATH_X] - o[t, k, 1]
                if cy - radius < 0 or cx - radius < 0 or cy + radius >= h or cx + radius >= w:
                    return True
    return False


def tie_case():
    """Two frames, one track, 9 x 11, R = 2, a zero shift (so the taps are symmetric bit for bit): the previous map holds two
    equal values left and right of the target pixel (4, 5), and a smaller one above it.  The two give equal products in any
    arithmetic; the smaller flat index, (4, 4), wins."""
    if "tie" in _CACHE:
        return _CACHE["tie"]
    h, w, radius = 9, 11, 2
    offsets, taps = T.motion_taps_spec([[0.0, 0.0], [0.0, 0.0]], 1.0, radius)
    assert np.array_equal(taps[:, :, ::-1].view(np.int32), taps.view(np.int32)) and offsets.tolist() == [[0, 0], [0, 0]]
    deltas = np.zeros((2, 1, h, w), np.float32)
    deltas[0, 0, 4, 4] = deltas[0, 0, 4, 6] = 0.25
    deltas[0, 0, 3, 5] = 0.125
    deltas[1, 0, 4, 5] = 1.0
    rows = np.zeros((2, 1, 14))
    rows[1, 0, T.PRED_Y], rows[1, 0, T.PRED_X] = 4, 5
    rows[0, 0, T.PRED_Y], rows[0, 0, T.PRED_X] = 3, 5
    ori = G.unit_ori(np.random.default_rng(8), 2, h, w).reshape(2, 1, 2, h, w)
    path, margin = T.backtrack_spec(deltas, ori, offsets.reshape(2, 1, 2), taps.reshape(2, 1, 2, -1), rows, None, return_margin=True)
    _CACHE["tie"] = frozen(dict(deltas=deltas, ori=ori, offsets=offsets.reshape(2, 1, 2), taps=taps.reshape(2, 1, 2, -1), rows=rows,
                                path=path, margin=margin))
    return _CACHE["tie"]


def scenarios():
    """The two 24-frame scenarios as B = 2 tracks of one drive: track 0 test_tracking_gpu.track_scenario (one start), track 1
    smoother_cases.moved_scenario (starts at frames 0 and 12).  heat [24,2,h,w], ori [24,2,2,h,w], odo [24,2,2], pos [24,2,2],
    starts [24,2]."""
    if "scen" not in _CACHE:
        a, m = G.track_scenario(), SC.moved_scenario()
        starts = np.zeros((G.TRK["frames"], 2), np.int32)
        starts[0] = 1
        starts[:, 1] = m["starts"]
        _CACHE["scen"] = frozen(dict(heat=np.stack([a["heat"], m["heat"]], 1), ori=np.stack([a["ori"], m["ori"]], 1),
                                     odo=np.stack([a["odo"], m["odo"]], 1), pos=np.stack([a["pos"], m["pos"]], 1), starts=starts))
    return _CACHE["scen"]


def spec_run(offsets, taps):
    """The specification free-running over scenarios() with the given motion inputs [24,2,2] / [24,2,2,2R+1]: deltas, rows, U,
    path, margin.  Cached per motion input."""
    key = ("run", offsets.tobytes(), taps.tobytes())
    if key in _CACHE:
        return _CACHE[key]
    s = scenarios()
    n, b, h, w = s["heat"].shape
    deltas, rows, us = np.zeros((n, b, h, w), np.float32), np.zeros((n, b, 14)), np.zeros((n, b, h, w))
    for t in range(n):
        prev = deltas[t - 1] if t else np.zeros((b, h, w), np.float32)
        deltas[t], rows[t], us[t] = T.viterbi_step_spec(prev, s["heat"][t], s["ori"][t], offsets[t], taps[t], G.TRK["outlier"],
                                                        reset=s["starts"][t], return_u=True)
    path, margin = T.backtrack_spec(deltas, s["ori"], offsets, taps, rows, s["starts"], return_margin=True)
    _CACHE[key] = frozen(dict(deltas=deltas, rows=rows, us=us, path=path, margin=margin))
    return _CACHE[key]


def path_errors(path, pos):
    """distance of every path pixel [T,B,8] from the rounded true position [T,B,2]"""
    return np.hypot(path[..., T.PATH_Y] - np.rint(pos[..., 0]), path[..., T.PATH_X] - np.rint(pos[..., 1]))
