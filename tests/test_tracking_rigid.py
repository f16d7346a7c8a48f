"""CPU-side checks of the rigid-motion predict of the histogram filter (ccvpe_amd/tracking.py: rigid_motion, step_rigid_spec,
kitti_frame_motion, kitti_motions): the sign convention, the cases in which the rigid step must equal the translate step value
for value, the KITTI geometry against live Pillow on a synthetic tree, and a synthetic drive whose patch frame turns.

The scenario builders (`rigid_scenario`, `make_rigid_kitti_tree`) are shared with tests/test_tracking_rigid_gpu.py.

The warp's rounding, counted for the device tolerance of that file: the specification and the kernel apply the SAME fp32 weights
(the coordinates are equal doubles), the kernel combines in fp32 — top = fma(wx1, v01, wx0 v00), bot likewise,
W = fma(wy1, bot, wy0 top): each combine is one rounded product and one rounded fma of non-negative terms, at most 2 u relative;
two levels: delta_W <= 4 u (u = 2^-24).  test_fp32_warp_emulation_stays_within_four_u measures it on an fp32 emulation."""
import os

import numpy as np
import pytest

from ccvpe_amd import datasets as DS, tracking as T

U24 = 2.0 ** -24
WARP_U = 4                                                       # delta_W in units of u, derived above


def softmax_maps(rng, b, h, w):
    z = rng.standard_normal((b, h, w)) * 4
    p = np.exp(z - z.max(axis=(1, 2), keepdims=True))
    return (p / p.sum(axis=(1, 2), keepdims=True)).astype(np.float32)


def unit_ori(rng, b, h, w):
    a = rng.uniform(0, 2 * np.pi, (b, h, w))
    return np.stack([np.cos(a), np.sin(a)], 1).astype(np.float32)


def forward_point(row, p):
    """the forward motion of point p = (y, x) under an inverse-map row: solve A q + a = p"""
    a = np.array([[row[0], row[1]], [row[3], row[4]]])
    return np.linalg.solve(a, np.asarray(p, dtype=np.float64) - np.array([row[2], row[5]]))


def centred_taps(b, sigma, radius):
    return T.motion_taps_spec(np.zeros((b, 2)), sigma, radius)[1]


# ---- 1. sign convention ---------------------------------------------------------------------------------------------------------
def test_rigid_motion_and_step_rigid_spec_pin_the_sign_convention():
    h = w = 41
    cy = cx = 20
    prior = np.zeros((1, h, w), np.float32)
    prior[0, cy, cx + 10] = 1.0                                   # 10 px right of the centre
    heat = np.full((1, h, w), 1.0 / (h * w), np.float32)
    ori = unit_ori(np.random.default_rng(0), 1, h, w)
    one = np.ones((1, 2, 1), np.float32)
    m = T.rigid_motion([0.0, 0.0], 90.0, (h, w))
    assert m.shape == (1, 6) and m.dtype == np.float64
    post, rows, u = T.step_rigid_spec(prior, heat, ori, m, one, return_u=True)
    assert np.count_nonzero(u[0]) == 1 and u[0, cy - 10, cx] > 0   # counter-clockwise in the image: 10 px ABOVE the centre
    assert rows[0, T.PRED_Y] == cy - 10 and rows[0, T.PRED_X] == cx and rows[0, T.SURVIVED] == 1.0 and rows[0, T.RESET] == 0
    y0, x0 = 14, 30
    prior = np.zeros((1, h, w), np.float32)
    prior[0, y0, x0] = 1.0
    post, rows, u = T.step_rigid_spec(prior, heat, ori, T.rigid_motion([3, -5], 0.0, (h, w)), one, return_u=True)
    assert np.count_nonzero(u[0]) == 1 and u[0, y0 + 3, x0 - 5] > 0
    assert rows[0, T.PRED_Y] == y0 + 3 and rows[0, T.PRED_X] == x0 - 5
    # the rows are the inverse map; forward_point inverts them: the centre stays under a pure rotation, an own centre too
    assert np.allclose(forward_point(T.rigid_motion([0, 0], 37.0, (h, w))[0], (20, 20)), (20, 20), atol=1e-12)
    assert np.allclose(forward_point(T.rigid_motion([1, 2], 171.0, (h, w), centre=(5.0, 7.5))[0], (5.0, 7.5)), (6.0, 9.5), atol=1e-12)
    # multiples of 90 degrees: exact 0 / +-1, also far from the first turn
    for ang in (0, 90, 180, 270, -90, 360, 450, -630, 90 * 41):
        r = T.rigid_motion([0, 0], float(ang), (h, w))[0]
        assert set(np.abs(r[[0, 1, 3, 4]]).tolist()) == {0.0, 1.0}, (ang, r)
    assert T.rigid_motion(np.zeros((3, 2)), [0.0, 10.0, 20.0], (h, w)).shape == (3, 6)


# ---- 2. / 3. where the rigid step must equal the translate step ------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0, 3])
def test_angle_zero_with_integer_shifts_equals_step_spec(radius):
    h, w = 37, 53
    rng = np.random.default_rng(10 + radius)
    prior, heat, ori = softmax_maps(rng, 3, h, w), softmax_maps(rng, 3, h, w), unit_ori(rng, 3, h, w)
    shifts = np.array([[-3, 2], [30, -40], [h + 40, -7]])
    taps = centred_taps(3, [0.0, 0.0, 0.0] if radius == 0 else [1.0, 0.8, 1.2], radius)
    for outlier, reset in ((0.0, None), (0.125, [1, 0, 1])):
        a = T.step_rigid_spec(prior, heat, ori, T.rigid_motion(shifts, 0.0, (h, w)), taps, outlier, reset=reset, return_u=True)
        b = T.step_spec(prior, heat, ori, shifts, taps, outlier, reset=reset, return_u=True)
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True)
    assert b[1][:, T.RESET].tolist() == [1, 0, 1]


@pytest.mark.parametrize("quarter", [1, 2, 3])
def test_quarter_turns_on_a_square_grid_equal_step_spec_on_rot90(quarter):
    n = 48
    rng = np.random.default_rng(20 + quarter)
    prior, heat, ori = softmax_maps(rng, 2, n, n), softmax_maps(rng, 2, n, n), unit_ori(rng, 2, n, n)
    taps = centred_taps(2, [1.0, 0.7], 3)
    a = T.step_rigid_spec(prior, heat, ori, T.rigid_motion(np.zeros((2, 2)), 90.0 * quarter, (n, n)), taps, 0.03125, return_u=True)
    turned = np.ascontiguousarray(np.rot90(prior, quarter, axes=(1, 2)))
    b = T.step_spec(turned, heat, ori, np.zeros((2, 2), np.int32), taps, 0.03125, return_u=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)


def test_wild_motion_rows_sample_nothing():
    """NaN, inf and a motion wholly off the grid: W = 0 everywhere, the step falls back to the measurement (RESET 2)."""
    h, w = 20, 24
    rng = np.random.default_rng(3)
    prior, heat, ori = softmax_maps(rng, 4, h, w), softmax_maps(rng, 4, h, w), unit_ori(rng, 4, h, w)
    m = T.rigid_motion(np.zeros((4, 2)), [5.0, 5.0, 5.0, 5.0], (h, w))
    m[0, 2] = np.nan
    m[1, 5] = np.inf
    m[2] = T.rigid_motion([3 * h, 0], 12.0, (h, w))[0]
    post, rows = T.step_rigid_spec(prior, heat, ori, m, centred_taps(4, 1.0, 2), 0.0)
    assert rows[:, T.RESET].tolist() == [2, 2, 2, 0] and rows[:3, T.SURVIVED].tolist() == [0, 0, 0]
    assert 0.5 < rows[3, T.SURVIVED] <= 1.0 + 1e-6


def test_fp32_warp_emulation_stays_within_four_u():
    """The count of the module docstring, measured: the kernel's three fp32 combines (a rounded product, then an fma computed
    exactly and rounded once) against the specification's float64 combines of the same weights."""
    h, w, r = 70, 45, 5
    rng = np.random.default_rng(7)
    worst = 0.0
    for ang, shift in ((7.3, (-3.3, 2.45)), (-33.0, (30.2, -39.6)), (171.0, (2.0, 1.0)), (45.0, (0.25, -0.75))):
        prior = softmax_maps(rng, 1, h, w)[0].astype(np.float64)
        m = T.rigid_motion(shift, ang, (h, w))[0]
        want = T._warp_spec(prior, m, r)
        ys = np.arange(-r, h + r, dtype=np.float64).reshape(-1, 1)
        xs = np.arange(-r, w + r, dtype=np.float64).reshape(1, -1)
        sy, sx = (m[0] * ys + m[1] * xs) + m[2], (m[3] * ys + m[4] * xs) + m[5]
        ok = (sy > -1) & (sy < h) & (sx > -1) & (sx < w)
        sy, sx = np.where(ok, sy, 0.0), np.where(ok, sx, 0.0)
        fy, fx = sy - np.floor(sy), sx - np.floor(sx)
        f32 = np.float32
        wy1, wy0, wx1, wx0 = fy.astype(f32), (1 - fy).astype(f32), fx.astype(f32), (1 - fx).astype(f32)
        pad = np.zeros((h + 2, w + 2), f32)
        pad[1:-1, 1:-1] = prior.astype(f32)
        iy, ix = np.floor(sy).astype(np.int64) + 1, np.floor(sx).astype(np.int64) + 1
        fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)
        top = fma(wx1, pad[iy, ix + 1], wx0 * pad[iy, ix])
        bot = fma(wx1, pad[iy + 1, ix + 1], wx0 * pad[iy + 1, ix])
        got = np.where(ok, fma(wy1, bot, wy0 * top), f32(0)).astype(np.float64)
        big = want > 2.0 ** -100
        assert big.sum() > 500
        worst = max(worst, float((np.abs(got - want)[big] / want[big]).max()) / U24)
    print("fp32 warp emulation: worst relative error %.2f u" % worst)
    assert 0 < worst <= WARP_U


# ---- 4. KITTI geometry against live Pillow --------------------------------------------------------------------------------------
KITTI_DRIVES = ("2011_09_26/2011_09_26_drive_0001_sync/", "2011_09_26/2011_09_26_drive_0002_sync/")
# (drive, frame number): drive 0 runs four frames; drive 1 two frames and then a frame number that goes back
KITTI_FRAMES = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 5), (1, 6), (1, 2))
KITTI_STARTS = [True, False, False, False, True, False, True]
KITTI_BLOB_SIGMA = 3.0
_LAT0, _LON0 = 49.01, 8.43


def kitti_world_px(lat, lon):
    """the test's own world: map pixels east / north of (_LAT0, _LON0) on the tangent plane there"""
    mpp = DS.kitti_meter_per_pixel()
    return np.array([T.EARTH_RADIUS_M * np.cos(np.radians(_LAT0)) * np.radians(lon - _LON0),
                     T.EARTH_RADIUS_M * np.radians(lat - _LAT0)]) / mpp


def make_rigid_kitti_tree(root, sat_size=640, seed=9):
    """A KITTI tree (the layout of tests/test_datasets.py::make_kitti_tree) of one short synthetic drive: the vehicle moves about
    1.5 m and turns about 4 degrees per frame, so latitude, longitude and heading all vary; every frame's 640 x 640 north-up
    map is cut from ONE synthetic world — black with a single bright Gaussian blob at a world-fixed point — centred on the
    frame's GPS position.  Test perturbations are moderate (shifts within 0.3 of the range, theta within +-1 x rotation_range)
    so the blob stays inside every 512 x 512 patch.  Returns (train file, test file, blob world position [px])."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    mpp = DS.kitti_meter_per_pixel()
    names, gps = [], []
    lat, lon, heading = _LAT0 + 2e-5, _LON0 - 3e-5, 0.6
    for d in KITTI_DRIVES:
        assert len(d) == 38
        os.makedirs(os.path.join(root, "satmap", d))
        os.makedirs(os.path.join(root, "raw_data", d, "oxts/data"))
        os.makedirs(os.path.join(root, "raw_data", d, "image_02/data"))
    for d, k in KITTI_FRAMES:
        step = 1.5 + 0.3 * rng.uniform(-1, 1)
        lat += step * np.sin(heading) / T.EARTH_RADIUS_M * 180 / np.pi
        lon += step * np.cos(heading) / (T.EARTH_RADIUS_M * np.cos(np.radians(lat))) * 180 / np.pi
        heading += np.radians(4.0 + rng.uniform(-1, 1))
        names.append(KITTI_DRIVES[d] + "%010d.png" % k)
        gps.append((lat, lon, heading))
    blob = kitti_world_px(*gps[3][:2]) + np.array([25.0, -18.0])
    jj, ii = np.meshgrid(np.arange(sat_size) + 0.5 - sat_size / 2.0, -(np.arange(sat_size) + 0.5 - sat_size / 2.0))
    for name, (lat, lon, heading) in zip(names, gps):
        g = kitti_world_px(lat, lon)
        img = 255.0 * np.exp(-((g[0] + jj - blob[0]) ** 2 + (g[1] + ii - blob[1]) ** 2) / (2 * KITTI_BLOB_SIGMA ** 2))
        Image.fromarray(np.repeat(np.round(img).astype(np.uint8)[:, :, None], 3, axis=2), "RGB").save(os.path.join(root, "satmap", name))
        Image.fromarray((rng.rand(94, 310, 3) * 255).astype(np.uint8), "RGB").save(
            os.path.join(root, "raw_data", name[:38], "image_02/data", name[38:]))
        with open(os.path.join(root, "raw_data", name[:38], "oxts/data", name[38:].replace(".png", ".txt")), "w") as f:
            f.write("%.12f %.12f 112.0 0.02 0.01 %.12f 1.0 2.0\n" % (lat, lon, heading))
    train_file, test_file = os.path.join(root, "train_files.txt"), os.path.join(root, "test1_files.txt")
    with open(train_file, "w") as f:
        f.write("".join(n + "\n" for n in names))
    with open(test_file, "w") as f:
        f.write("".join("%s %.4f %.4f %.4f\n" % (n, rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-1, 1)) for n in names))
    return train_file, test_file, blob


def kitti_exact_gt(pairs, i):
    """(y, x) of the camera in the 512 x 512 patch of test sample i: the loader's own offsets (KITTIPairs.sample: x_off, y_off)
    BEFORE its int(), taken from the patch centre (255.5, 255.5) — where targets.train_targets centres the Gaussian (256 - center
    on its grid) up to the loader's truncation."""
    sx, sy, ori = pairs.perturbation(i)
    c, s = np.cos(ori / 180 * np.pi), np.sin(ori / 180 * np.pi)
    x_off = sx * pairs.shift_px_lon * c - sy * pairs.shift_px_lat * s
    y_off = -sy * pairs.shift_px_lat * c - sx * pairs.shift_px_lon * s
    return np.array([255.5 - y_off, 255.5 - x_off])


def blob_centroid(img):
    a = img[:, :, 0].astype(np.float64)
    a = np.where(a >= 8, a, 0.0)
    assert a.sum() > 2000, "the blob left the patch"
    yy, xx = np.mgrid[0:a.shape[0], 0:a.shape[1]]
    return np.array([(a * yy).sum(), (a * xx).sum()]) / a.sum()


def test_kitti_motions_against_live_pillow(tmp_path):
    train_file, test_file, blob = make_rigid_kitti_tree(str(tmp_path))
    pairs = DS.KITTIPairs(str(tmp_path), test_file, rotation_range=10.0, test=True)
    n = len(pairs)
    assert n == len(KITTI_FRAMES)
    motion, starts = T.kitti_motions(pairs)
    assert motion.shape == (n, 6) and motion.dtype == np.float64 and starts.tolist() == KITTI_STARTS
    assert np.array_equal(motion[starts], np.tile([1.0, 0, 0, 0, 1.0, 0], (int(starts.sum()), 1)))
    samples = [pairs.sample(i) for i in range(n)]
    seen = [blob_centroid(s["sat_u8"]) for s in samples]
    gts = [kitti_exact_gt(pairs, i) for i in range(n)]
    turned = far = 0
    for t in range(n):
        # the loader's own ground truth is this point, truncated: 256 - center on the Gaussian's grid
        cx, cy = samples[t]["center"]
        assert abs(gts[t][0] - (256 - cy)) < 1.5 and abs(gts[t][1] - (256 - cx)) < 1.5
        if starts[t]:
            continue
        # the frame change alone carries the world-fixed blob of frame t-1 onto where Pillow put it in frame t
        fm = T.kitti_frame_motion(pairs, t - 1, t)
        carried = forward_point(fm, seen[t - 1])
        err = float(np.hypot(*(carried - seen[t])))
        moved = float(np.hypot(*(seen[t - 1] - seen[t])))
        print("frame %d: blob moved %.2f px, carried to within %.3f px" % (t, moved, err))
        assert err <= 1.5, (t, carried, seen[t], seen[t - 1])
        far += moved > 5.0
        # with the camera's displacement the exact ground truth of t-1 lands on that of t
        got = forward_point(motion[t], gts[t - 1])
        assert np.all(np.abs(got - gts[t]) <= 1e-6), (t, got, gts[t])
        ang = np.degrees(np.arctan2(motion[t, 1], motion[t, 0]))
        turned += abs(ang) > 1.0
        assert abs(motion[t, 0] ** 2 + motion[t, 1] ** 2 - 1) < 1e-12 and motion[t, 3] == -motion[t, 1] and motion[t, 4] == motion[t, 0]
    assert turned >= 3 and far >= 2                               # the drive does turn the patch frame and move the blob
    # a subset restarts where it begins
    m2, s2 = T.kitti_motions(pairs, indices=[2, 3])
    assert s2.tolist() == [True, False] and np.array_equal(m2[1], motion[3])
    train = DS.KITTIPairs(str(tmp_path), train_file)
    with pytest.raises(ValueError):
        T.kitti_motions(train)
    with pytest.raises(ValueError):
        T.kitti_frame_motion(train, 0, 1)


# ---- 5. a drive whose patch frame turns -----------------------------------------------------------------------------------------
RIG = dict(h=96, w=80, frames=24, radius=6, sigma=1.5, outlier=0.05)
_RIGID = {}


def _gauss(h, w, cy, cx, s):
    y, x = np.mgrid[0:h, 0:w]
    return np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))


def rigid_scenario():
    """Fixed seeds; computed once and shared (read-only).  The patch frame turns 4 to 8 degrees about the grid centre and shifts
    up to 1.5 px per frame; the vehicle sits about 26 px from the centre, so the turn alone moves it 2 to 4.5 px per frame.  Every
    third frame carries a stronger distractor a few pixels from the vehicle.  The odometry is the motion plus noise: `motion`
    (rigid_motion rows) for the rigid filter, `shift` alone for a filter that cannot turn."""
    if _RIGID:
        return _RIGID
    h, w, n = RIG["h"], RIG["w"], RIG["frames"]
    rng = np.random.default_rng(12)
    pos = np.array([30.0, 20.0])
    heats, motions, shifts, poss = [], [], [], []
    for t in range(n):
        ang, shift = (rng.uniform(4, 8), rng.uniform(-1.5, 1.5, 2)) if t else (0.0, np.zeros(2))
        if t:
            pos = forward_point(T.rigid_motion(shift, ang, (h, w))[0], pos) + rng.normal(0, 0.3, 2)
        assert 10 <= pos[0] <= h - 11 and 10 <= pos[1] <= w - 11
        logit = 0.3 * rng.standard_normal((h, w)) + 6 * _gauss(h, w, pos[0], pos[1], 2.0)
        if t % 3 == 1:
            a = rng.uniform(0, 2 * np.pi)
            d = pos + rng.uniform(7, 9) * np.array([np.sin(a), np.cos(a)])
            logit += 8 * _gauss(h, w, d[0], d[1], 2.0)
        p = np.exp(logit - logit.max())
        heats.append((p / p.sum()).astype(np.float32))
        odo_ang, odo_shift = (ang + rng.normal(0, 0.3), shift + rng.normal(0, 0.3, 2)) if t else (0.0, np.zeros(2))
        motions.append(T.rigid_motion(odo_shift, odo_ang, (h, w))[0])
        shifts.append(odo_shift)
        poss.append(pos.copy())
    _RIGID.update(heat=np.stack(heats), motion=np.stack(motions), shift=np.stack(shifts), pos=np.stack(poss),
                  ori=unit_ori(np.random.default_rng(13), n, h, w), taps=centred_taps(n, RIG["sigma"], RIG["radius"]))
    for a in _RIGID.values():
        a.setflags(write=False)
    return _RIGID


def spec_rigid_track(motion, taps):
    """step_rigid_spec run over the scenario: per frame (prior used, post, row, U)."""
    s = rigid_scenario()
    h, w, n = RIG["h"], RIG["w"], RIG["frames"]
    priors, posts, rows, us = np.zeros((n, h, w), np.float32), np.zeros((n, h, w), np.float32), np.zeros((n, 14)), np.zeros((n, h, w))
    for t in range(n):
        if t:
            priors[t] = posts[t - 1]
        p, r, u = T.step_rigid_spec(priors[t:t + 1], s["heat"][t:t + 1], s["ori"][t:t + 1], motion[t:t + 1], taps[t:t + 1],
                                    RIG["outlier"], reset=[int(t == 0)], return_u=True)
        posts[t], rows[t], us[t] = p[0], r[0], u[0]
    return priors, posts, rows, us


def rigid_track_errors():
    """mean arg-max error [px] of (the raw heat-maps, the rigid filter, a filter fed the translation part alone)"""
    s = rigid_scenario()
    h, w, n = RIG["h"], RIG["w"], RIG["frames"]
    _, _, rows, _ = spec_rigid_track(s["motion"], s["taps"])
    offsets, shifted_taps = T.motion_taps_spec(s["shift"], RIG["sigma"], RIG["radius"])
    post, trans = np.zeros((1, h, w), np.float32), np.zeros((n, 14))
    for t in range(n):
        post, r = T.step_spec(post, s["heat"][t:t + 1], s["ori"][t:t + 1], offsets[t:t + 1], shifted_taps[t:t + 1], RIG["outlier"],
                              reset=[int(t == 0)])
        trans[t] = r[0]
    raw = [np.hypot(*(np.array(np.unravel_index(np.argmax(s["heat"][t]), (h, w))) - s["pos"][t])) for t in range(n)]
    err = lambda rr: [np.hypot(rr[t, T.PRED_Y] - s["pos"][t, 0], rr[t, T.PRED_X] - s["pos"][t, 1]) for t in range(n)]
    return float(np.mean(raw)), float(np.mean(err(rows))), float(np.mean(err(trans)))


def test_rigid_filter_beats_the_raw_arg_max_and_a_translation_only_filter():
    raw, rigid, trans = rigid_track_errors()
    print("rotating drive: raw mean error %.3f px, rigid filter %.3f px, translation-only filter %.3f px" % (raw, rigid, trans))
    assert rigid < raw and rigid < trans


def test_rigid_step_rejects_bad_arguments_without_a_gpu():
    """ccvpe_belief_step_rigid_f32 validates before it launches, as ccvpe_belief_step_f32 does (fake aligned pointers that are
    never dereferenced), plus its own: motion non-null and 8-byte aligned."""
    from ccvpe_amd import _lib
    lib = _lib.load()
    EINVAL = -1
    prior, heat, ori, mot, taps, post, scratch, rows = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000, 0x800000

    def call(motion=mot, radius=8, outlier=0.1, post=post, rows=rows, batch=2, h=64, w=64):
        return lib.ccvpe_belief_step_rigid_f32(prior, heat, ori, motion, taps, radius, outlier, None, post, scratch, rows, batch, h, w, None)

    assert call(motion=None) == EINVAL and b"null" in lib.ccvpe_last_error()
    assert call(motion=mot + 4) == EINVAL and b"motion must be 8-byte aligned" in lib.ccvpe_last_error()
    assert call(motion=mot + 2) == EINVAL
    assert call(radius=33) == EINVAL and b"radius" in lib.ccvpe_last_error()
    assert call(outlier=float("nan")) == EINVAL and b"outlier" in lib.ccvpe_last_error()
    assert call(post=prior) == EINVAL and b"overlap" in lib.ccvpe_last_error()
    assert call(post=heat) == EINVAL and b"heat and post overlap" in lib.ccvpe_last_error()
    assert call(rows=rows + 4) == EINVAL and b"8-byte" in lib.ccvpe_last_error()
    assert call(batch=0) == EINVAL and call(h=0) == EINVAL
    # the ops wrapper checks the motion tensor before anything reaches the library
    import torch
    from ccvpe_amd import ops
    with pytest.raises(ValueError, match="motion"):
        ops.belief_step_rigid(None, None, None, torch.zeros((1, 6), dtype=torch.float64), None)
