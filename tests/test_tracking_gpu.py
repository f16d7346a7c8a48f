"""The histogram-filter step on the device (csrc/belief.hip through ops.belief_step) against its specification
(tracking.step_spec, numpy float64) from the same inputs.

Tolerances — derived, not tuned.  u = 2^-24.  The kernel's predict is two passes of 2R+1 non-negative fp32 terms (fma chains,
no cancellation): delta_Q <= 2 (2R+3) u relative per pixel (an fp32 emulation on the CPU measured at most 9 u at R = 32).
M = fma(1 - a, heat, a / (h w)) with both constants rounded once and the product Q M add 4 u: delta_U = (2 (2R+3) + 4) u.
Z and S are sums of non-negative terms accumulated in double, so they inherit delta_U / delta_Q relative; post = U * (float)(1/Z)
adds the cast, the product and the specification's own fp32 store: 2 delta_U + 3 u <= tol := (4 (2R+3) + 12) u.  post, PROB,
EVIDENCE and SURVIVED are held to tol relative + 2^-100 absolute; the moments are ratios of such sums over coordinates below
max(h, w): MEAN_* within 2 tol max(h,w), VAR_* and COV_YX within 4 tol max(h,w)^2; ANGLE (double on both sides) within 1e-9;
PRED_Y, PRED_X, COS, SIN and RESET are equal.  Arg-max equality needs inputs with room: every case first asserts, on the
specification's own U, that the best value exceeds the second by more than 2 delta_U relative.
Free-running over k steps the belief's error compounds linearly: k tol at step k."""
import numpy as np
import pytest
import torch

from ccvpe_amd import evaluate as E, tracking as T

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
ABS = 2.0 ** -100


def tol_of(radius):
    return (4 * (2 * radius + 3) + 12) * U24


def delta_u(radius):
    return (2 * (2 * radius + 3) + 4) * U24


def softmax_maps(rng, b, h, w):
    z = rng.standard_normal((b, h, w)) * 4                           # N(0, 4^2) logits
    p = np.exp(z - z.max(axis=(1, 2), keepdims=True))
    return (p / p.sum(axis=(1, 2), keepdims=True)).astype(np.float32)


def unit_ori(rng, b, h, w):
    a = rng.uniform(0, 2 * np.pi, (b, h, w))
    return np.stack([np.cos(a), np.sin(a)], 1).astype(np.float32)


def assert_margin(u, radius, what):
    """the specification's own top-2 margin leaves room for the kernel's rounding"""
    for b in range(u.shape[0]):
        top = np.sort(u[b].reshape(-1))[-2:]
        assert top[1] > 0 and (top[1] - top[0]) / top[1] > 2 * delta_u(radius), (what, b, top)


def assert_step_close(got_post, got_rows, want_post, want_rows, radius, h, w, what, scale=1.0):
    tol = np.asarray(scale, dtype=np.float64) * tol_of(radius)       # a scalar, or one factor per track
    got_post, want_post = np.asarray(got_post, np.float64), np.asarray(want_post, np.float64)
    b = want_post.shape[0]
    tb = np.broadcast_to(tol, (b,))
    err = np.abs(got_post.reshape(b, -1) - want_post.reshape(b, -1))
    lim = tb[:, None] * np.abs(want_post.reshape(b, -1)) + ABS
    assert np.all(err <= lim), (what, "post", float((err / lim).max()))
    exact = [T.PRED_Y, T.PRED_X, T.COS, T.SIN, T.RESET]
    assert np.array_equal(got_rows[:, exact], want_rows[:, exact]), (what, got_rows[:, exact], want_rows[:, exact])
    for c in (T.PROB, T.EVIDENCE, T.SURVIVED):
        assert np.all(np.abs(got_rows[:, c] - want_rows[:, c]) <= tb * np.abs(want_rows[:, c]) + ABS), (what, c, got_rows[:, c], want_rows[:, c])
    m = max(h, w)
    for c in (T.MEAN_Y, T.MEAN_X):
        assert np.all(np.abs(got_rows[:, c] - want_rows[:, c]) <= 2 * tb * m), (what, c, got_rows[:, c], want_rows[:, c])
    for c in (T.VAR_YY, T.VAR_XX, T.COV_YX):
        assert np.all(np.abs(got_rows[:, c] - want_rows[:, c]) <= 4 * tb * m * m), (what, c, got_rows[:, c], want_rows[:, c])
    ga, wa = got_rows[:, T.ANGLE], want_rows[:, T.ANGLE]
    assert np.array_equal(np.isnan(ga), np.isnan(wa)) and np.all(np.abs(ga - wa)[~np.isnan(wa)] <= 1e-9), (what, ga, wa)


def run_step(prior, heat, ori, offsets, taps, outlier, reset=None):
    from ccvpe_amd import ops
    b, h, w = heat.shape
    dev = lambda a, dt: torch.as_tensor(np.array(a), dtype=dt).cuda()              # a copy: the shared scenario is read-only
    rows, post = ops.belief_step(dev(prior, torch.float32).reshape(b, 1, h, w), dev(heat, torch.float32).reshape(b, 1, h, w),
                                 dev(ori, torch.float32), dev(offsets, torch.int32), dev(taps, torch.float32), outlier=outlier,
                                 reset=None if reset is None else dev(reset, torch.int32))
    return post.cpu().numpy().reshape(b, h, w), rows.cpu().numpy()


def three_tracks(h, w, radius, seed):
    """B = 3 with a different offset and different taps per track: a negative offset, (30, -40), and one beyond the grid."""
    rng = np.random.default_rng(seed)
    prior, heat, ori = softmax_maps(rng, 3, h, w), softmax_maps(rng, 3, h, w), unit_ori(rng, 3, h, w)
    shifts = np.array([[-3.3, 2.45], [30.2, -39.6], [h + 40.0, -7.5]])
    sigma = np.array([0.0, 0.0, 0.0]) if radius == 0 else np.array([radius / 3.0, radius / 2.5, radius / 4.0])
    offsets, taps = T.motion_taps_spec(shifts, sigma, radius)
    assert offsets.tolist() == [[-3, 2], [30, -40], [h + 40, -7]]
    return prior, heat, ori, offsets, taps


@pytest.mark.parametrize("h,w,radius", [(37, 53, 0), (37, 53, 1), (70, 45, 32), (64, 64, 7)])
def test_belief_step_matches_the_specification(h, w, radius):
    """Odd sizes, the smallest and the largest radius, tiles that straddle the edge (16 x 64 tiles: 37 x 53 is 3 x 1 ragged
    tiles, 70 x 45 is 5 x 1, 64 x 64 exactly 4 x 1); w % 4 != 0 takes the scalar staging, 64 x 64 the 16-byte one.  Three tracks
    with their own offsets and taps, without reset flags (the third leaves the grid: RESET 2) and with flags (1, 0, 1)."""
    prior, heat, ori, offsets, taps = three_tracks(h, w, radius, seed=100 + radius)
    for outlier, reset in ((0.0, None), (0.125, [1, 0, 1])):
        want_post, want_rows, u = T.step_spec(prior, heat, ori, offsets, taps, outlier, reset=reset, return_u=True)
        assert_margin(u, radius, (h, w, radius))
        assert want_rows[:, T.RESET].tolist() == ([0, 0, 2] if reset is None else [1, 0, 1])
        assert 0 < want_rows[1, T.SURVIVED] < 1                                                # (30, -40) keeps part of the mass
        got_post, got_rows = run_step(prior, heat, ori, offsets, taps, outlier, reset)
        assert_step_close(got_post, got_rows, want_post, want_rows, radius, h, w, (h, w, radius, outlier))


def test_belief_step_translation_on_the_device():
    """The sign convention of the specification, on the kernel: one-hot prior, R = 0, offset (3, -5)."""
    h, w, y0, x0 = 40, 72, 14, 66
    prior = np.zeros((1, h, w), np.float32)
    prior[0, y0, x0] = 1.0
    heat = softmax_maps(np.random.default_rng(5), 1, h, w)
    ori = unit_ori(np.random.default_rng(6), 1, h, w)
    post, rows = run_step(prior, heat, ori, [[3, -5]], np.ones((1, 2, 1), np.float32), 0.0)
    assert np.count_nonzero(post[0]) == 1 and abs(float(post[0, y0 + 3, x0 - 5]) - 1.0) <= 2 * U24      # m * (float)(1 / m)
    assert rows[0, T.PRED_Y] == y0 + 3 and rows[0, T.PRED_X] == x0 - 5 and rows[0, T.SURVIVED] == 1.0 and rows[0, T.RESET] == 0


def test_belief_step_full_size():
    """512 x 512, R = 8, B = 2: 256 tiles per track (several workgroups per record merge), the 16-byte paths, an offset of a whole
    Oxford patch change (256 px) on one track."""
    h = w = 512
    rng = np.random.default_rng(11)
    prior, heat, ori = softmax_maps(rng, 2, h, w), softmax_maps(rng, 2, h, w), unit_ori(rng, 2, h, w)
    offsets, taps = T.motion_taps_spec([[4.3, -6.8], [-256.4, 3.5]], [2.5, 1.7], 8)
    want_post, want_rows, u = T.step_spec(prior, heat, ori, offsets, taps, 0.03125, return_u=True)
    assert_margin(u, 8, "full size")
    assert want_rows[:, T.RESET].tolist() == [0, 0]
    got_post, got_rows = run_step(prior, heat, ori, offsets, taps, 0.03125)
    assert_step_close(got_post, got_rows, want_post, want_rows, 8, h, w, "full size")


def test_two_identical_calls_are_bit_identical():
    prior, heat, ori, offsets, taps = three_tracks(70, 45, 5, seed=21)
    a_post, a_rows = run_step(prior, heat, ori, offsets, taps, 0.0625, [0, 1, 0])
    b_post, b_rows = run_step(prior, heat, ori, offsets, taps, 0.0625, [0, 1, 0])
    assert np.array_equal(a_post.view(np.int32), b_post.view(np.int32))
    assert np.array_equal(a_rows.view(np.int64), b_rows.view(np.int64))


# ---- the 24-frame track: 96 x 80, a stronger distractor peak in every third frame ---------------------------------------------
TRK = dict(h=96, w=80, frames=24, radius=6, sigma=1.5, outlier=0.05)
_TRACK = {}


def _gauss(h, w, cy, cx, s):
    y, x = np.mgrid[0:h, 0:w]
    return np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))


def track_scenario():
    """Fixed seeds; computed once and shared (read-only): positions, heat-maps, orientation fields and noisy odometry."""
    if _TRACK:
        return _TRACK
    h, w, n = TRK["h"], TRK["w"], TRK["frames"]
    rng = np.random.default_rng(3)
    pos = np.array([40.0, 30.0])
    heats, odos, poss = [], [], []
    for t in range(n):
        step = rng.uniform(-3, 3, 2) if t else np.zeros(2)
        pos = np.clip(pos + step, 8, [h - 9, w - 9])
        logit = 0.3 * rng.standard_normal((h, w)) + 6 * _gauss(h, w, pos[0], pos[1], 2.0)
        if t % 3 == 1:
            d = rng.uniform(10, [h - 10, w - 10])
            logit += 8 * _gauss(h, w, d[0], d[1], 2.0)
        p = np.exp(logit - logit.max())
        heats.append((p / p.sum()).astype(np.float32))
        odos.append(step + rng.normal(0, 0.5, 2) if t else np.zeros(2))
        poss.append(pos.copy())
    _TRACK.update(heat=np.stack(heats), odo=np.stack(odos), pos=np.stack(poss), ori=unit_ori(np.random.default_rng(4), n, h, w))
    for a in _TRACK.values():
        a.setflags(write=False)
    return _TRACK


def spec_track(offsets, taps):
    """The specification run over the scenario with the given motion inputs: per frame (prior used, post, row, U)."""
    s = track_scenario()
    h, w, n = TRK["h"], TRK["w"], TRK["frames"]
    priors, posts, rows, us = np.zeros((n, h, w), np.float32), np.zeros((n, h, w), np.float32), np.zeros((n, 14)), np.zeros((n, h, w))
    for t in range(n):
        if t:
            priors[t] = posts[t - 1]
        p, r, u = T.step_spec(priors[t:t + 1], s["heat"][t:t + 1], s["ori"][t:t + 1], offsets[t:t + 1], taps[t:t + 1], TRK["outlier"],
                              reset=[int(t == 0)], return_u=True)
        posts[t], rows[t], us[t] = p[0], r[0], u[0]
    return priors, posts, rows, us


def test_track_filtering_beats_the_raw_arg_max_and_teacher_forced_steps_match():
    s = track_scenario()
    h, w, n, radius = TRK["h"], TRK["w"], TRK["frames"], TRK["radius"]
    offsets, taps = T.motion_taps_spec(s["odo"], TRK["sigma"], radius)
    priors, posts, rows, us = spec_track(offsets, taps)
    # on the specification alone: the filter helps
    raw = [np.hypot(*(np.array(np.unravel_index(np.argmax(s["heat"][t]), (h, w))) - s["pos"][t])) for t in range(n)]
    fil = [np.hypot(rows[t, T.PRED_Y] - s["pos"][t, 0], rows[t, T.PRED_X] - s["pos"][t, 1]) for t in range(n)]
    print("track: raw mean error %.3f px, filtered %.3f px" % (np.mean(raw), np.mean(fil)))
    assert np.mean(fil) < np.mean(raw)
    assert_margin(us, radius, "track")
    assert rows[:, T.RESET].tolist() == [1] + [0] * (n - 1)
    # teacher-forced: every step from the specification's previous posterior — 24 independent tracks of one call
    reset = [1] + [0] * (n - 1)
    got_post, got_rows = run_step(priors, s["heat"], s["ori"], offsets, taps, TRK["outlier"], reset)
    assert_step_close(got_post, got_rows, posts, rows, radius, h, w, "teacher-forced")


def _capture_steps(monkeypatch):
    """record the motion inputs a HistogramFilter hands to ops.belief_step (device tensors, cloned), so that the specification
    runs on the very same taps"""
    from ccvpe_amd import ops
    real, seen = ops.belief_step, []

    def recording(prior, heatmap, ori, offsets, taps, **kw):
        seen.append((offsets.clone(), taps.clone()))
        return real(prior, heatmap, ori, offsets, taps, **kw)

    monkeypatch.setattr(ops, "belief_step", recording)
    return seen


def test_track_free_running_through_the_filter(monkeypatch):
    """HistogramFilter over the 24 frames, never corrected: tolerance k tol at step k, arg-max equal in every frame; the taps it
    computes on the device are within 1 fp32 ulp of the numpy twin's."""
    s = track_scenario()
    h, w, n, radius = TRK["h"], TRK["w"], TRK["frames"], TRK["radius"]
    seen = _capture_steps(monkeypatch)
    filt = T.HistogramFilter(1, hw=(h, w), sigma_px=TRK["sigma"], radius=radius, outlier=TRK["outlier"])
    heat, ori = torch.from_numpy(s["heat"].copy()).cuda().unsqueeze(1), torch.from_numpy(s["ori"].copy()).cuda()
    odo = torch.from_numpy(s["odo"].copy()).cuda()
    table = torch.zeros((n, 14), device="cuda", dtype=torch.float64)
    beliefs = []
    for t in range(n):
        filt.step(heat[t:t + 1], ori[t:t + 1], odo[t:t + 1], rows_out=table[t:t + 1])
        beliefs.append(filt.belief.clone())
    got_post = torch.cat(beliefs).cpu().numpy().reshape(n, h, w)
    got_rows = table.cpu().numpy()
    offsets = torch.cat([o for o, _ in seen]).cpu().numpy()
    taps = torch.cat([k for _, k in seen]).cpu().numpy()
    want_o, want_k = T.motion_taps_spec(s["odo"], TRK["sigma"], radius)
    assert np.array_equal(offsets, want_o) and np.all(np.abs(taps.astype(np.float64) - want_k) <= np.spacing(want_k))
    priors, posts, rows, us = spec_track(offsets, taps)
    assert_margin(us, radius, "free-running")
    assert np.array_equal(got_rows[:, [T.PRED_Y, T.PRED_X]], rows[:, [T.PRED_Y, T.PRED_X]])
    assert_step_close(got_post, got_rows, posts, rows, radius, h, w, "free-running", scale=np.arange(1, n + 1))


def test_a_reset_track_equals_a_fresh_filter():
    h, w = 48, 72
    rng = np.random.default_rng(31)
    heat = torch.from_numpy(softmax_maps(rng, 8, h, w)).cuda().reshape(4, 2, 1, h, w)
    ori = torch.from_numpy(unit_ori(rng, 8, h, w)).cuda().reshape(4, 2, 2, h, w)
    shift = torch.tensor([[1.3, -2.2], [-0.7, 4.1]], dtype=torch.float64)
    used = T.HistogramFilter(2, hw=(h, w), sigma_px=1.0, outlier=0.02)
    for t in range(3):
        used.step(heat[t], ori[t], shift)
    mid_rows = used.rows.clone()
    assert mid_rows[:, T.RESET].tolist() == [0, 0]
    used.reset()
    fresh = T.HistogramFilter(2, hw=(h, w), sigma_px=1.0, outlier=0.02)
    a = used.step(heat[3], ori[3], shift).cpu().numpy()
    b = fresh.step(heat[3], ori[3], shift).cpu().numpy()
    assert a[:, T.RESET].tolist() == [1, 1] and np.array_equal(a.view(np.int64), b.view(np.int64))
    assert torch.equal(used.belief, fresh.belief)
    # one track of two: the other goes on from its belief
    used.reset(tracks=[1])
    c = used.step(heat[0], ori[0], shift).cpu().numpy()
    assert c[:, T.RESET].tolist() == [0, 1]
    fresh2 = T.HistogramFilter(2, hw=(h, w), sigma_px=1.0, outlier=0.02)
    d = fresh2.step(heat[0], ori[0], shift).cpu().numpy()
    assert np.array_equal(c[1].view(np.int64), d[1].view(np.int64)) and not np.array_equal(c[0], d[0])
    assert torch.equal(used.belief[1], fresh2.belief[1])


def test_evaluate_sequence_on_a_synthetic_oxford_tree(tmp_path, monkeypatch):
    """Nine frames (three traversals) with a stub forward that returns planted heat-maps — a bump at the vehicle and, in every
    second frame, a stronger bump elsewhere: "raw" equals evaluate_batches on the same stub; "filtered" equals metrics_spec
    applied to the specification's beliefs (positions, errors and angles as eval_metrics' own bound, the probabilities read from
    the belief within k tol); one read-back."""
    import eval_metrics_cases as C
    from ccvpe_amd import datasets as DS
    from test_datasets import make_oxford_tree
    g, sat_path = make_oxford_tree(str(tmp_path))
    ds = DS.OxfordPairs(g, sat_path, split="test")
    n = len(ds)
    shift, starts = T.oxford_shifts(ds)
    gt_px = np.array([[256 - ds.sample(i)["center"][1], 256 - ds.sample(i)["center"][0]] for i in range(n)])
    yy, xx = torch.meshgrid(torch.arange(512, device="cuda", dtype=torch.float32), torch.arange(512, device="cuda", dtype=torch.float32),
                            indexing="ij")
    gen = torch.Generator(device="cuda").manual_seed(7)
    heats, oris = [], []
    for i in range(n):
        logit = 0.2 * torch.randn((512, 512), device="cuda", generator=gen)
        logit += 6 * torch.exp(-((yy - float(gt_px[i, 0])) ** 2 + (xx - float(gt_px[i, 1])) ** 2) / 18)
        if i % 2 == 1:
            logit += 8 * torch.exp(-((yy - 40.0 - 37 * i) ** 2 + (xx - 470.0 + 41 * i) ** 2) / 18)
        heats.append(torch.softmax(logit.reshape(-1), 0).reshape(1, 512, 512))
        ang = torch.rand((512, 512), device="cuda", generator=gen) * 6.2831853
        oris.append(torch.stack([torch.cos(ang), torch.sin(ang)]))
    heats, oris = torch.stack(heats), torch.stack(oris)

    def stub_for():
        state = {"k": 0, "forwards": 0}

        def forward(grd, sat):
            k, b = state["k"], grd.shape[0]
            state["k"], state["forwards"] = k + b, state["forwards"] + 1
            return (None, heats[k:k + b].contiguous(), oris[k:k + b].contiguous())
        return forward, state

    seen_batches = []

    class Recording(DS.DeviceBatches):
        def __iter__(self):
            for batch in super().__iter__():
                seen_batches.append(batch)
                yield batch

    kw = dict(batch_size=4, device="cuda", workers=2, targets=True, grd_hw=(154, 231), ascending_bins=True)
    fwd, _ = stub_for()
    base = E.evaluate_batches(fwd, DS.DeviceBatches(ds, **kw))
    seen = _capture_steps(monkeypatch)
    filt = T.HistogramFilter(1, sigma_px=2.0, outlier=0.02)
    assert filt.radius == 7
    fwd, state = stub_for()
    real_cpu, reads = torch.Tensor.cpu, []

    def counting_cpu(self, *a, **k):
        if self.is_cuda and self.dtype == torch.float64 and self.dim() == 2:
            reads.append(tuple(self.shape))
        return real_cpu(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "cpu", counting_cpu)
    res = E.evaluate_sequence(fwd, Recording(ds, **kw), filt, shift, starts)
    monkeypatch.setattr(torch.Tensor, "cpu", real_cpu)
    assert reads == [(n, 38)] and state["forwards"] == 3 and len(seen) == n
    # raw: the very rows and numbers of evaluate_batches
    assert np.array_equal(res["raw_rows"].view(np.int64), base["rows"].view(np.int64)) and res["indices"].tolist() == list(range(n))
    for key, val in base.items():
        if key not in ("rows", "indices"):
            assert res["raw"][key] == val or (val != val and res["raw"][key] != res["raw"][key]), key
    assert sorted(res["raw"]["sets"]) == ["test1", "test2", "test3"]
    # filtered: the specification's beliefs through metrics_spec
    offsets = torch.cat([o for o, _ in seen]).cpu().numpy()
    taps = torch.cat([k for _, k in seen]).cpu().numpy()
    want_o, want_k = T.motion_taps_spec(shift, 2.0, 7)
    assert np.array_equal(offsets, want_o) and np.all(np.abs(taps.astype(np.float64) - want_k) <= np.spacing(want_k))
    h_heat, h_ori = heats.cpu().numpy(), oris.cpu().numpy()
    gt = np.concatenate([b.gt.cpu().numpy() for b in seen_batches])
    gt_ori = np.concatenate([b.gt_ori.cpu().numpy() for b in seen_batches])
    heading = np.concatenate([b.heading_deg.cpu().numpy() for b in seen_batches])
    beliefs, rows = np.zeros((n, 1, 512, 512), np.float32), np.zeros((n, 14))
    depth, k = np.zeros(n), 0
    for i in range(n):
        k = 1 if starts[i] else k + 1
        depth[i] = k
        prior = np.zeros((1, 512, 512), np.float32) if starts[i] else beliefs[i - 1]
        p, r, u = T.step_spec(prior, h_heat[i], h_ori[i:i + 1], offsets[i:i + 1], taps[i:i + 1], 0.02, reset=[int(starts[i])],
                              return_u=True)
        assert_margin(u, 7, ("sequence", i))
        beliefs[i, 0], rows[i] = p[0], r[0]
    want = E.metrics_spec(beliefs, h_ori, gt, gt_ori, heading, np.full(n, E.OXFORD_METRES_PER_PIXEL))
    got = res["filtered_rows"]
    assert np.array_equal(got[:, :4], want[:, :4])
    a, b = got[:, 4:10], want[:, 4:10]
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.all(np.abs(a - b)[~np.isnan(b)] <= 1e-9 + 1e-9 * np.abs(b[~np.isnan(b)]))
    for c in (E.PROB, E.PROB_AT_GT):
        assert np.all(np.abs(got[:, c] - want[:, c]) <= depth * tol_of(7) * np.abs(want[:, c]) + ABS), (c, got[:, c], want[:, c])
    assert_step_close(np.zeros((n, 1)), res["tracks"], np.zeros((n, 1)), rows, 7, 512, 512, "sequence tracks", scale=depth)
    assert res["filtered"]["n"] == n and res["filtered"]["mean_pixel_error"] == float(np.mean(want[:, E.PIXEL]))
    # the planted distractors fool the raw arg-max in frames that follow a start; the belief stays on the vehicle there
    follow = [i for i in range(n) if i % 2 == 1 and not starts[i]]
    assert follow and np.all(res["raw_rows"][follow, E.PIXEL] > 20) and np.all(got[follow, E.PIXEL] <= 2)
    with pytest.raises(ValueError):
        E.evaluate_sequence(fwd, DS.DeviceBatches(ds, shuffle=True, seed=1, **kw), filt, shift, starts)
    with pytest.raises(ValueError):
        E.evaluate_sequence(fwd, DS.DeviceBatches(ds, **dict(kw, targets=False)), filt, shift, starts)
    # the loader's own settings decide: a shard of a two-rank world is ascending, a shuffle of one frame too
    half = DS.DeviceBatches(ds, rank=0, world=2, **kw)
    with pytest.raises(ValueError):
        E.evaluate_sequence(fwd, half, filt, shift[:len(half.indices)], starts[:len(half.indices)])
    with pytest.raises(ValueError):
        E.evaluate_sequence(fwd, DS.DeviceBatches(ds, indices=[0], shuffle=True, **kw), filt, shift[:1], starts[:1])
