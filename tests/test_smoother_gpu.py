"""The backward step of the forward-backward smoother on the device (belief_smooth_kernel / belief_smooth_rigid_kernel in
csrc/belief.hip through ops.belief_smooth_step / ops.belief_smooth_step_rigid) against its specification
(tracking.smooth_step_spec / smooth_step_rigid_spec, numpy float64) from the same inputs, and SequenceSmoother /
evaluate_sequence(smooth=True) on top of it.

Tolerances — the derivation of tests/test_tracking_gpu.py, applied to the backward step.  u = 2^-24.  G = fma(1 - a, heat,
floor) beta costs 3 u (the two rounded constants and the fma as there, one product); the two passes of 2R+1 non-negative fp32
terms add 2 (2R+3) u: delta_B' = (2 (2R+3) + 3) u; V = alpha B' costs one more product: delta_V = (2 (2R+3) + 4) u, the forward
step's delta_U.  Z and S are sums of non-negative terms in double and inherit delta_V / delta_B'; each normalised map adds the
cast of 1 / Z (1 / S), the product and the specification's own fp32 store: 2 delta + 3 u <= tol_of(R) = (4 (2R+3) + 12) u — the
forward step's tolerance, for smooth AND for beta_out, relative + 2^-100 absolute (messages reach fp32 denormals in the far
field, legitimately).  Rows as assert_step_close of that file.  The rigid form adds the forward rigid test's 2 WARP_U u = 8 u
(tests/test_tracking_rigid_gpu.py: the three fp32 bilinear combines; the inverted row is computed operation for operation as
tracking.invert_motion, so the coordinates are the specification's doubles).  Arg-max equality is conditional: every case first
asserts, on the specification's own V, a top-2 margin above 2 delta_V.  Free-running, step k from the end: k tol."""
import numpy as np
import pytest
import torch

import smoother_cases as SC
import test_tracking_gpu as G
import test_tracking_rigid as RG
import test_tracking_rigid_gpu as GR
from ccvpe_amd import evaluate as E, tracking as T

pytestmark = pytest.mark.gpu


def _dev(a, dt):
    return torch.as_tensor(np.array(a), dtype=dt).cuda()                        # a copy: shared scenarios are read-only


def run_smooth(beta, heat, alpha, ori, move, taps, outlier, cut=None, rigid=False):
    from ccvpe_amd import ops
    b, h, w = heat.shape
    fn = ops.belief_smooth_step_rigid if rigid else ops.belief_smooth_step
    m4 = lambda a: _dev(a, torch.float32).reshape(b, 1, h, w)
    rows, smooth, beta_out = fn(m4(beta), m4(heat), m4(alpha), _dev(ori, torch.float32), _dev(move, torch.float64 if rigid else torch.int32),
                                _dev(taps, torch.float32), outlier=outlier, cut=None if cut is None else _dev(cut, torch.int32))
    return smooth.cpu().numpy().reshape(b, h, w), beta_out.cpu().numpy().reshape(b, h, w), rows.cpu().numpy()


def assert_smooth_close(got, want, radius, h, w, what, scale=1.0, rigid=False):
    """got, want: (smooth, beta_out, rows).  smooth and the rows as the forward step's post and rows; beta_out within the same
    tolerance per pixel."""
    scale = np.asarray(scale, dtype=np.float64) * (GR.tol_rigid(radius) / G.tol_of(radius) if rigid else 1.0)
    G.assert_step_close(got[0], got[2], want[0], want[2], radius, h, w, what, scale=scale)
    b = want[1].shape[0]
    tb = np.broadcast_to(scale * G.tol_of(radius), (b,))
    gm, wm = np.asarray(got[1], np.float64).reshape(b, -1), np.asarray(want[1], np.float64).reshape(b, -1)
    err, lim = np.abs(gm - wm), tb[:, None] * np.abs(wm) + G.ABS
    assert np.all(err <= lim), (what, "beta_out", float((err / lim).max()))
    uniform = want[2][:, T.RESET] != 0                                          # the fallback message is one constant: equal
    assert np.array_equal(got[1][uniform], want[1][uniform]), (what, "uniform message")


def _margin(v, radius, what, rigid=False):
    (GR.assert_margin if rigid else G.assert_margin)(v, radius, what)


def three_tracks(h, w, radius, seed):
    """test_tracking_gpu.three_tracks (a negative offset, (30, -40), one beyond the grid; own taps) with its prior as alpha and
    a message from a generator of its own."""
    alpha, heat, ori, offsets, taps = G.three_tracks(h, w, radius, seed)
    return G.softmax_maps(np.random.default_rng(seed + 1000), 3, h, w), heat, alpha, ori, offsets, taps


@pytest.mark.parametrize("h,w,radius", [(37, 53, 0), (37, 53, 1), (70, 45, 32), (64, 64, 7)])
def test_smooth_step_matches_the_specification(h, w, radius):
    """The forward test's shapes: w % 4 != 0 takes the scalar staging, 64 x 64 the 16-byte one (two quads per LDS quad); ragged
    tiles; both radius extremes.  Three tracks with their own offsets and taps; without cut flags the third brings nothing back
    (state 2), with flags (1, 0, 1) the first and the third are cut."""
    beta, heat, alpha, ori, offsets, taps = three_tracks(h, w, radius, seed=300 + radius)
    for outlier, cut in ((0.0, None), (0.125, [1, 0, 1])):
        want = T.smooth_step_spec(beta, heat, alpha, ori, offsets, taps, outlier, cut=cut, return_v=True)
        _margin(want[3], radius, (h, w, radius))
        assert want[2][:, T.RESET].tolist() == ([0, 0, 2] if cut is None else [1, 0, 1])
        assert want[2][1, T.SURVIVED] > 0 and want[2][2, T.SURVIVED] == 0
        got = run_smooth(beta, heat, alpha, ori, offsets, taps, outlier, cut)
        assert_smooth_close(got, want, radius, h, w, (h, w, radius, outlier))


def test_smooth_step_full_size_and_repeat():
    """512 x 512, R = 8, B = 2: 256 tiles per track, the 16-byte paths, a 256-px offset (an Oxford patch change) on one track;
    two identical calls give the same bits in both maps and the rows."""
    h = w = 512
    rng = np.random.default_rng(12)
    beta, heat, alpha, ori = G.softmax_maps(rng, 2, h, w), G.softmax_maps(rng, 2, h, w), G.softmax_maps(rng, 2, h, w), G.unit_ori(rng, 2, h, w)
    offsets, taps = T.motion_taps_spec([[4.3, -6.8], [-256.4, 3.5]], [2.5, 1.7], 8)
    want = T.smooth_step_spec(beta, heat, alpha, ori, offsets, taps, 0.03125, return_v=True)
    _margin(want[3], 8, "full size")
    assert want[2][:, T.RESET].tolist() == [0, 0]
    a = run_smooth(beta, heat, alpha, ori, offsets, taps, 0.03125)
    b = run_smooth(beta, heat, alpha, ori, offsets, taps, 0.03125)
    assert_smooth_close(a, want, 8, h, w, "full size")
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    assert np.array_equal(a[2].view(np.int64), b[2].view(np.int64))


def rigid_tracks(h, w, radius, seed):
    """B = 3: a small turn with a fractional shift; a quarter turn with a whole-pixel shift; a motion that leaves the grid."""
    rng = np.random.default_rng(seed)
    beta, heat, alpha, ori = G.softmax_maps(rng, 3, h, w), G.softmax_maps(rng, 3, h, w), G.softmax_maps(rng, 3, h, w), G.unit_ori(rng, 3, h, w)
    motion = np.concatenate([T.rigid_motion([-3.3, 2.45], 7.3, (h, w)), T.rigid_motion([4.0, -6.0], 90.0, (h, w)),
                             T.rigid_motion([3.0 * h, -2.0 * w], 12.0, (h, w))])
    sigma = np.zeros(3) if radius == 0 else np.array([radius / 3.0, radius / 2.5, radius / 4.0])
    return beta, heat, alpha, ori, motion, RG.centred_taps(3, sigma, radius)


@pytest.mark.parametrize("h,w,radius", [(37, 53, 0), (37, 53, 1), (70, 45, 32), (64, 64, 7)])
def test_rigid_smooth_step_matches_the_specification(h, w, radius):
    beta, heat, alpha, ori, motion, taps = rigid_tracks(h, w, radius, seed=400 + radius)
    for outlier, cut in ((0.0, None), (0.125, [1, 0, 1])):
        want = T.smooth_step_rigid_spec(beta, heat, alpha, ori, motion, taps, outlier, cut=cut, return_v=True)
        _margin(want[3], radius, (h, w, radius), rigid=True)
        assert want[2][:, T.RESET].tolist() == ([0, 0, 2] if cut is None else [1, 0, 1])
        got = run_smooth(beta, heat, alpha, ori, motion, taps, outlier, cut, rigid=True)
        assert_smooth_close(got, want, radius, h, w, (h, w, radius, outlier), rigid=True)


def test_rigid_smooth_step_nan_row_and_bit_identity_with_the_translate_form():
    """A NaN row and a singular row sample nothing (state 2) beside an ordinary track.  Angle 0 with whole-pixel shifts gives
    the bits of ops.belief_smooth_step with those offsets; quarter turns on 64 x 64 the bits of ops.belief_smooth_step on the
    maps of frame t turned back, the shift brought into the turned frame."""
    h, w, radius = 37, 53, 1
    beta, heat, alpha, ori, motion, taps = rigid_tracks(h, w, radius, seed=51)
    motion = motion.copy()
    motion[1, 4] = np.nan
    motion[2] = [1, 1, 0, 1, 1, 0]
    want = T.smooth_step_rigid_spec(beta, heat, alpha, ori, motion, taps, 0.0, return_v=True)
    _margin(want[3], radius, "nan row", rigid=True)
    assert want[2][:, T.RESET].tolist() == [0, 2, 2] and want[2][1:, T.SURVIVED].tolist() == [0, 0]
    got = run_smooth(beta, heat, alpha, ori, motion, taps, 0.0, rigid=True)
    assert_smooth_close(got, want, radius, h, w, "nan row", rigid=True)
    bits = lambda r: (r[0].view(np.int32), r[1].view(np.int32), r[2].view(np.int64))
    h, w, radius = 70, 45, 5
    beta, heat, alpha, ori, _, taps = rigid_tracks(h, w, radius, seed=52)
    shifts = np.array([[3, -7], [-30, 20], [0, 0]])
    for cut in (None, [0, 1, 0]):
        a = run_smooth(beta, heat, alpha, ori, T.rigid_motion(shifts, 0.0, (h, w)), taps, 0.03125, cut, rigid=True)
        b = run_smooth(beta, heat, alpha, ori, shifts, taps, 0.03125, cut)
        for x, y in zip(bits(a), bits(b)):
            assert np.array_equal(x, y)
    n, radius = 64, 7
    beta, heat, alpha, ori, _, taps = rigid_tracks(n, n, radius, seed=53)
    shifts = np.array([[0, 0], [5, -9], [-2, 11]])
    motion = np.concatenate([T.rigid_motion(shifts[k], 90.0 * (k + 1), (n, n)) for k in range(3)])
    offsets = np.stack([motion[:, 0] * shifts[:, 0] + motion[:, 1] * shifts[:, 1],
                        motion[:, 3] * shifts[:, 0] + motion[:, 4] * shifts[:, 1]], 1).astype(np.int32)
    back = lambda x: np.stack([np.rot90(x[k], -(k + 1)) for k in range(3)])
    a = run_smooth(beta, heat, alpha, ori, motion, taps, 0.03125, rigid=True)
    b = run_smooth(back(beta), back(heat), alpha, ori, offsets, taps, 0.03125)
    assert a[2][:, T.RESET].tolist() == [0, 0, 0]
    for x, y in zip(bits(a), bits(b)):
        assert np.array_equal(x, y)


def test_moved_distractor_track_through_the_sequence_smoother(monkeypatch):
    """SequenceSmoother.run over the 24 frames with starts at 0 and 12.  The forward rows are HistogramFilter's, bit for bit.
    Teacher-forced: the 24 backward steps as 24 tracks of one call, each fed the specification's posterior and message, within
    tol.  Free-running (the device's own posteriors and messages): step k from the end within k tol, arg-max equal."""
    s = SC.moved_scenario()
    h, w, n, radius = SC.TRK["h"], SC.TRK["w"], SC.TRK["frames"], SC.TRK["radius"]
    heat, ori = torch.from_numpy(s["heat"].copy()).cuda().unsqueeze(1), torch.from_numpy(s["ori"].copy()).cuda()
    odo = torch.from_numpy(s["odo"].copy()).cuda()
    seen = G._capture_steps(monkeypatch)
    sm = T.SequenceSmoother((h, w), sigma_px=SC.TRK["sigma"], radius=radius, outlier=SC.TRK["outlier"])
    out = sm.run(heat, ori, shift_px=odo, starts=s["starts"], keep_beliefs=True)
    assert len(seen) == n and out["beliefs"].shape == (n, 1, h, w)
    offsets = torch.cat([o for o, _ in seen]).cpu().numpy()
    taps = torch.cat([k for _, k in seen]).cpu().numpy()
    want_o, want_k = T.motion_taps_spec(s["odo"], SC.TRK["sigma"], radius)
    assert np.array_equal(offsets, want_o) and np.all(np.abs(taps.astype(np.float64) - want_k) <= np.spacing(want_k))
    filt = T.HistogramFilter(1, hw=(h, w), sigma_px=SC.TRK["sigma"], radius=radius, outlier=SC.TRK["outlier"])
    table = torch.zeros((n, 14), device="cuda", dtype=torch.float64)
    for t in range(n):
        if s["starts"][t]:
            filt.reset()
        filt.step(heat[t:t + 1], ori[t:t + 1], odo[t:t + 1], rows_out=table[t:t + 1])
    assert torch.equal(out["filtered"].view(torch.int64), table.view(torch.int64))
    c = SC.spec_chain(offsets, taps)
    G.assert_margin(c["vs"], radius, "moved track")
    want = (c["smooth"], c["beta"], c["srows"])
    nxt = np.minimum(np.arange(n) + 1, n - 1)
    got = run_smooth(c["beta_in"], s["heat"][nxt], c["posts"], s["ori"], offsets[nxt], taps[nxt], SC.TRK["outlier"], c["cut"])
    assert_smooth_close(got, want, radius, h, w, "teacher-forced")
    got_rows = out["smoothed"].cpu().numpy()
    assert np.array_equal(got_rows[:, [T.PRED_Y, T.PRED_X, T.RESET]], c["srows"][:, [T.PRED_Y, T.PRED_X, T.RESET]])
    G.assert_step_close(out["beliefs"].cpu().numpy().reshape(n, h, w), got_rows, c["smooth"], c["srows"], radius, h, w, "free-running",
                        scale=np.arange(n, 0, -1))
    err = np.hypot(got_rows[:, T.PRED_Y] - s["pos"][:, 0], got_rows[:, T.PRED_X] - s["pos"][:, 1])
    assert np.all(err[list(SC.STARTS)] <= 1.5)
    # without keep_beliefs: the same rows, no table
    again = sm.run(heat, ori, shift_px=odo, starts=s["starts"])
    assert again["beliefs"] is None and torch.equal(again["smoothed"].view(torch.int64), out["smoothed"].view(torch.int64))


def test_evaluate_sequence_with_smoothing_on_a_synthetic_oxford_tree(tmp_path):
    """The nine-frame synthetic Oxford tree of the existing sequence test with planted heat-maps: with smooth=True "raw" and
    "filtered" are the smooth=False call's, bit for bit; "smoothed_tracks" equals SequenceSmoother.run on the same frames, and
    "smoothed_rows" the protocol rows of its beliefs."""
    from ccvpe_amd import datasets as DS, ops
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
        state = {"k": 0}

        def forward(grd, sat):
            k, b = state["k"], grd.shape[0]
            state["k"] = k + b
            return (None, heats[k:k + b].contiguous(), oris[k:k + b].contiguous())
        return forward

    seen = []

    class Recording(DS.DeviceBatches):
        def __iter__(self):
            for batch in super().__iter__():
                seen.append(batch)
                yield batch

    kw = dict(batch_size=4, device="cuda", workers=2, targets=True, grd_hw=(154, 231), ascending_bins=True)
    plain = E.evaluate_sequence(stub_for(), DS.DeviceBatches(ds, **kw), T.HistogramFilter(1, sigma_px=2.0, outlier=0.02), shift, starts)
    assert "smoothed" not in plain and sorted(plain) == ["filtered", "filtered_rows", "indices", "raw", "raw_rows", "tracks"]
    res = E.evaluate_sequence(stub_for(), Recording(ds, **kw), T.HistogramFilter(1, sigma_px=2.0, outlier=0.02), shift, starts, smooth=True)
    for key in ("raw_rows", "filtered_rows", "tracks"):
        assert np.array_equal(res[key].view(np.int64), plain[key].view(np.int64)), key
    for key in ("raw", "filtered"):
        for name, val in plain[key].items():
            assert repr(res[key][name]) == repr(val), (key, name)
    run = T.SequenceSmoother((512, 512), sigma_px=2.0, outlier=0.02).run(heats, oris, shift_px=shift, starts=starts, keep_beliefs=True)
    assert run["smoothed"].shape == (n, 14) and res["smoothed_tracks"].shape == (n, 14)
    assert np.array_equal(res["smoothed_tracks"].view(np.int64), run["smoothed"].cpu().numpy().view(np.int64))
    assert np.array_equal(res["tracks"].view(np.int64), run["filtered"].cpu().numpy().view(np.int64))
    cat = lambda name: torch.cat([getattr(b, name) for b in seen])
    mpp = torch.full((n,), E.OXFORD_METRES_PER_PIXEL, device="cuda", dtype=torch.float64)
    rows = ops.eval_metrics(run["beliefs"], oris, cat("gt"), cat("gt_ori"), cat("heading_deg"), mpp).cpu().numpy()
    assert np.array_equal(res["smoothed_rows"].view(np.int64), rows.view(np.int64))
    assert res["smoothed"]["n"] == n and res["smoothed"]["mean_pixel_error"] == float(np.mean(rows[:, E.PIXEL]))
    # every segment's last frame is cut; a frame at a start that carries a distractor is brought back by the frames after it
    last = [i for i in range(n) if i == n - 1 or starts[i + 1]]
    assert res["smoothed_tracks"][:, T.RESET].tolist() == [float(i in last) for i in range(n)]
    fooled = [i for i in range(n) if i % 2 == 1 and starts[i] and i not in last]
    assert np.all(res["smoothed_rows"][fooled, E.PIXEL] <= 2) and np.all(res["filtered_rows"][fooled, E.PIXEL] > 20)
