"""The most likely path on the CPU: the specifications (tracking.viterbi_step_spec, backtrack_spec) against first principles,
the margins of every case test_path_gpu.py compares on the device (path_cases.py), and the argument checks of the C entry
points, of MostLikelyPath and of evaluate_sequence's new keyword."""
import inspect

import numpy as np
import pytest

import path_cases as PC
import test_tracking_gpu as G
from ccvpe_amd import _lib, evaluate as E, tracking as T


def test_the_separable_max_equals_the_brute_force_2d_max():
    """9 x 11, R = 2, an offset of (1, -2), fractional taps: P[y,x] = max_ij ky[i] kx[j] prev[y - oy - i, x - ox - j] (0 outside
    the grid, 0 at least) to 1e-15 relative; SURVIVED is its sum; a NaN and a negative value in prev count as nothing."""
    rng = np.random.default_rng(0)
    h, w, radius = 9, 11, 2
    prev = rng.random((1, h, w)).astype(np.float32)
    prev[0, 3, 4], prev[0, 6, 7] = np.nan, -2.0
    heat, ori = G.softmax_maps(rng, 1, h, w), G.unit_ori(rng, 1, h, w)
    offsets, taps = T.motion_taps_spec([[1.3, -2.4]], 0.9, radius)
    assert offsets.tolist() == [[1, -2]]
    _, rows, u = T.viterbi_step_spec(prev, heat, ori, offsets, taps, 0.0, return_u=True)
    want = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            for i in range(-radius, radius + 1):
                for j in range(-radius, radius + 1):
                    sy, sx = y - 1 - i, x + 2 - j
                    if 0 <= sy < h and 0 <= sx < w and prev[0, sy, sx] > 0:
                        want[y, x] = max(want[y, x], float(taps[0, 0, i + radius]) * float(taps[0, 1, j + radius]) * float(prev[0, sy, sx]))
    got = u[0] / heat[0].astype(np.float64)
    assert np.all(np.abs(got - want) <= 1e-15 * want) and want.min() > 0
    assert rows[0, T.RESET] == 0 and rows[0, T.SURVIVED] == pytest.approx(want.sum(), rel=1e-14)
    # the sum form is a different map: the max never exceeds it
    _, _, us = T.step_spec(np.nan_to_num(np.maximum(prev, 0)), heat, ori, offsets, taps, 0.0, return_u=True)
    assert np.all(u[0] <= us[0] * (1 + 1e-15)) and np.any(u[0] < 0.9 * us[0])


def _random_drive(h, w, radius, seed, frames=5):
    rng = np.random.default_rng(seed)
    heat, ori = G.softmax_maps(rng, frames, h, w).reshape(frames, 1, h, w), G.unit_ori(rng, frames, h, w).reshape(frames, 1, 2, h, w)
    offsets, taps = T.motion_taps_spec(rng.uniform(-4, 4, (frames, 2)), 0.0 if radius == 0 else radius / 2.0, radius)
    offsets, taps = offsets.reshape(frames, 1, 2), taps.reshape(frames, 1, 2, -1)
    deltas, rows = np.zeros((frames, 1, h, w), np.float32), np.zeros((frames, 1, 14))
    for t in range(frames):
        deltas[t], rows[t] = T.viterbi_step_spec(deltas[t - 1], heat[t], ori[t], offsets[t], taps[t], 0.05, reset=[int(t == 0)])
    return deltas, ori, offsets, taps, rows


def test_radius_zero_follows_the_offsets_exactly():
    deltas, ori, offsets, taps, rows = _random_drive(37, 53, 0, seed=1)
    path = T.backtrack_spec(deltas, ori, offsets, taps, rows)
    assert np.all(rows[1:, 0, T.RESET] == 0) and np.all(path[:-1, 0, T.PATH_LINK] == 0) and path[-1, 0, T.PATH_LINK] == 1
    yx = path[:, 0, [T.PATH_Y, T.PATH_X]]
    assert np.array_equal(yx[:-1], yx[1:] - offsets[1:, 0])
    assert np.array_equal(yx[-1], rows[-1, 0, [T.PRED_Y, T.PRED_X]])


@pytest.mark.parametrize("radius", [1, 3, 6])
def test_a_link_never_exceeds_the_radius(radius):
    """random maps at 37 x 53: within a segment |path[t] - path[t-1] - offset| <= R on each axis, SCORE is the forward map's
    predict at the path pixel (the link's value IS P there) and PROB is the map there."""
    deltas, ori, offsets, taps, rows = _random_drive(37, 53, radius, seed=10 + radius)
    path = T.backtrack_spec(deltas, ori, offsets, taps, rows)
    assert np.all(path[:-1, 0, T.PATH_LINK] == 0)
    yx = path[:, 0, [T.PATH_Y, T.PATH_X]]
    assert np.all(np.abs(yx[1:] - yx[:-1] - offsets[1:, 0]) <= radius)
    for t in range(1, len(path)):
        y, x = int(yx[t, 0]), int(yx[t, 1])
        pad = T._moved_spec(deltas[t - 1, 0].astype(np.float64), offsets[t, 0, 0], offsets[t, 0, 1], radius)
        p = T._maxblur_spec(pad, taps[t, 0, 0], taps[t, 0, 1])
        assert path[t - 1, 0, T.PATH_SCORE] == pytest.approx(p[y, x], rel=1e-15)
        assert path[t, 0, T.PATH_PROB] == deltas[t, 0, y, x]


def test_an_exact_tie_takes_the_smaller_flat_index():
    c = PC.tie_case()
    assert c["path"][1, 0, [T.PATH_Y, T.PATH_X, T.PATH_LINK]].tolist() == [4, 5, 1]
    assert c["path"][0, 0, [T.PATH_Y, T.PATH_X, T.PATH_LINK]].tolist() == [4, 4, 0]
    k = c["taps"][1, 0]
    assert c["path"][0, 0, T.PATH_SCORE] == float(k[0, 2]) * (float(k[1, 3]) * 0.25)
    # the margin is taken against the best candidate with OTHER factors: the value above the target
    second = float(k[0, 3]) * (float(k[1, 2]) * 0.125)
    assert c["margin"][0, 0] == (c["path"][0, 0, T.PATH_SCORE] - second) / c["path"][0, 0, T.PATH_SCORE] > PC.LINK_MARGIN


def test_segment_starts_and_dead_links():
    """reset[t] or rows[t, RESET] end a segment (LINK 1 on the frame before); a window without mass gives LINK 2."""
    deltas, ori, offsets, taps, rows = _random_drive(16, 20, 1, seed=4)
    reset = np.zeros((5, 1), np.int32)
    reset[2] = 1
    rows = rows.copy()
    rows[4, 0, T.RESET] = 2
    deltas = deltas.copy()
    deltas[0] = 0                                                               # frame 1's window finds nothing
    path = T.backtrack_spec(deltas, ori, offsets, taps, rows, reset)
    assert path[:, 0, T.PATH_LINK].tolist() == [2, 1, 0, 1, 1]
    for t in (0, 1, 3, 4):
        assert np.array_equal(path[t, 0, [T.PATH_Y, T.PATH_X]], rows[t, 0, [T.PRED_Y, T.PRED_X]]) and path[t, 0, T.PATH_SCORE] == 0


def test_a_rows_pixel_off_the_grid_is_clamped():
    """+inf clamps to the last row, NaN (and anything negative) gives 0, as the kernel does; nothing lies there: LINK 2."""
    c = PC.tie_case()
    rows = c["rows"].copy()
    rows[1, 0, T.PRED_Y], rows[1, 0, T.PRED_X] = np.inf, np.nan
    path = T.backtrack_spec(c["deltas"], c["ori"], c["offsets"], c["taps"], rows)
    assert path[:, 0, [T.PATH_Y, T.PATH_X, T.PATH_LINK]].tolist() == [[3, 5, 2], [8, 0, 1]]


@pytest.mark.parametrize("h,w", PC.SIZES)
@pytest.mark.parametrize("radius", PC.RADII)
def test_the_device_cases_have_room(h, w, radius):
    """What test_path_gpu.py compares exactly must be decided by the specification alone: the arg-max margins of the step
    cases, and EVERY link of the drives."""
    c = PC.step_case(h, w, radius)
    for outlier, reset in ((0.0, None), (0.125, [1, 0, 1])):
        _, rows, u = T.viterbi_step_spec(c["prior"], c["heat"], c["ori"], c["offsets"], c["taps"], outlier, reset=reset, return_u=True)
        PC.assert_argmax_margin(u, 2 * PC.DELTA_U, ("step", h, w, radius))
        assert rows[:, T.RESET].tolist() == ([0, 0 if h + radius > 30 else 2, 2] if reset is None else [1, 0 if h + radius > 30 else 2, 1])
    d = PC.drive_case(h, w, radius)
    PC.assert_link_margins(d["path"], d["margin"], PC.LINK_MARGIN, ("drive", h, w, radius))
    assert d["rows"][2, 2, T.RESET] == 2 and d["rows"][3, 1, T.RESET] == 1
    link = d["path"][..., T.PATH_LINK]
    assert link[1, 2] == 1 and link[2, 1] == 1 and np.all(link[-1] == 1) and np.count_nonzero(link == 0) >= 10
    if radius:
        assert PC.window_is_cut(d, radius)


def test_the_scenarios_have_room():
    """Every link of the free-running specification over the two 24-frame scenarios leaves room for 24 steps of drift on the
    device (both competitors carry up to k TOL_MAX each at step k) plus the backtrack's own 8 u.  Prints the path's and the
    filter's mean error against the rounded true position; test_path_gpu.py asserts on them."""
    s = PC.scenarios()
    n, b = s["heat"].shape[:2]
    offsets, taps = T.motion_taps_spec(s["odo"].reshape(-1, 2), G.TRK["sigma"], G.TRK["radius"])
    offsets, taps = offsets.reshape(n, b, 2), taps.reshape(n, b, 2, -1)
    r = PC.spec_run(offsets, taps)
    PC.assert_link_margins(r["path"], r["margin"], 2 * n * PC.TOL_MAX + PC.LINK_MARGIN, "scenarios")
    err = PC.path_errors(r["path"], s["pos"])
    fil = np.zeros((n, b))
    for k in range(b):
        post = np.zeros((1,) + s["heat"].shape[2:], np.float32)
        for t in range(n):
            post, row = T.step_spec(post, s["heat"][t, k:k + 1], s["ori"][t, k:k + 1], offsets[t, k:k + 1], taps[t, k:k + 1],
                                    G.TRK["outlier"], reset=[int(s["starts"][t, k])])
            fil[t, k] = np.hypot(row[0, T.PRED_Y] - np.rint(s["pos"][t, k, 0]), row[0, T.PRED_X] - np.rint(s["pos"][t, k, 1]))
    print("path: mean error %s px (filter %s px), at the starts %s, smallest link margin %.3g u"
          % (err.mean(0), fil.mean(0), err[[0, 0, 12], [0, 1, 1]], np.nanmin(r["margin"]) / PC.U24))
    assert np.all(err[[0, 0, 12], [0, 1, 1]] == 0)


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    """Both new entry points validate before they launch (fake aligned pointers that are never dereferenced)."""
    lib = _lib.load()
    EINVAL = -1
    f = dict(prior=0x100000, heat=0x200000, ori=0x400000, move=0x600000, taps=0x700000, post=0x800000, scratch=0xa00000,
             rows=0xb00000)
    n = 64 * 64 * 4

    def step(radius=8, outlier=0.1, batch=2, h=64, w=64, **kw):
        a = dict(f, **kw)
        return lib.ccvpe_belief_viterbi_step_f32(a["prior"], a["heat"], a["ori"], a["move"], a["taps"], radius, outlier, None, a["post"],
                                                 a["scratch"], a["rows"], batch, h, w, None)

    assert step(radius=33) == EINVAL and b"belief_viterbi_step: radius" in lib.ccvpe_last_error()
    assert step(radius=-1) == EINVAL and step(outlier=1.5) == EINVAL and b"outlier" in lib.ccvpe_last_error()
    for name in f:
        assert step(**{name: None}) == EINVAL and b"null" in lib.ccvpe_last_error(), name
    assert step(rows=f["rows"] + 4) == EINVAL and b"8-byte" in lib.ccvpe_last_error()
    assert step(prior=f["prior"] + 2) == EINVAL and b"4-byte" in lib.ccvpe_last_error()
    for name, maps in (("prior", 1), ("heat", 1), ("ori", 2)):
        assert step(post=f[name] + 2 * maps * n - 4) == EINVAL and b"overlap" in lib.ccvpe_last_error(), name
    assert step(h=0) == EINVAL and step(batch=0) == EINVAL and step(h=65536, w=65536) == EINVAL

    g = dict(deltas=0x1000000, ori=0x2000000, offsets=0x3000000, taps=0x3100000, rows=0x3200000, reset=0x3300000, path=0x3400000)

    def back(radius=8, frames=3, batch=2, h=64, w=64, **kw):
        a = dict(g, **kw)
        return lib.ccvpe_belief_backtrack_f32(a["deltas"], a["ori"], a["offsets"], a["taps"], radius, a["rows"], a["reset"], a["path"],
                                              frames, batch, h, w, None)

    assert back(radius=33) == EINVAL and b"belief_backtrack: radius" in lib.ccvpe_last_error()
    assert back(radius=-1) == EINVAL
    for name in ("deltas", "ori", "offsets", "taps", "rows", "path"):
        assert back(**{name: None}) == EINVAL and b"null" in lib.ccvpe_last_error(), name
    assert back(path=g["path"] + 4) == EINVAL and b"8-byte" in lib.ccvpe_last_error()
    assert back(rows=g["rows"] + 4) == EINVAL and b"8-byte" in lib.ccvpe_last_error()
    assert back(deltas=g["deltas"] + 2) == EINVAL and b"4-byte" in lib.ccvpe_last_error()
    sizes = dict(deltas=6 * n, ori=12 * n, offsets=6 * 2 * 4, taps=6 * 2 * 17 * 4, rows=6 * 14 * 8, reset=6 * 4)
    for name, size in sizes.items():
        assert back(path=g[name]) == EINVAL and b"overlap" in lib.ccvpe_last_error(), name
        assert back(path=g[name] + size - 8) == EINVAL and b"overlap" in lib.ccvpe_last_error(), name
    assert back(frames=0) == EINVAL and b"shape" in lib.ccvpe_last_error()
    assert back(batch=0) == EINVAL and back(h=0) == EINVAL and back(h=65536, w=65536) == EINVAL


def test_most_likely_path_refuses_bad_settings():
    for kw in (dict(sigma_px=-1.0), dict(sigma_px=float("nan")), dict(sigma_px=20.0), dict(radius=33), dict(radius=-1),
               dict(outlier=1.5), dict(outlier=-0.1), dict(hw=(0, 5))):
        with pytest.raises(ValueError):
            T.MostLikelyPath(device="cpu", **kw)
    p = T.MostLikelyPath(hw=(8, 8), sigma_px=2.0, device="cpu")
    assert p.radius == 7


def test_evaluate_sequence_path_keyword_is_off_by_default_and_refuses_motion():
    """path is a keyword with default False, and the rigid form is refused before anything runs.  That the returned keys
    without the keyword are the earlier ones needs a device: test_path_gpu.py compares them."""
    sig = inspect.signature(E.evaluate_sequence)
    assert sig.parameters["path"].default is False and sig.parameters["smooth"].default is False
    with pytest.raises(ValueError, match="out of scope"):
        E.evaluate_sequence(None, None, None, None, [True], motion=np.zeros((1, 6)), path=True)
