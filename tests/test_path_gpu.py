"""The most likely path on the device (csrc/belief.hip through ops.belief_viterbi_step, ops.belief_backtrack and
tracking.MostLikelyPath) against its specification (tracking.viterbi_step_spec, backtrack_spec; numpy float64).

Tolerances — derived, not tuned; path_cases.py carries the derivation.  u = 2^-24.  A maximum of products carries two roundings
whatever R is (rounding is monotone: the max of the rounded products is the rounded product at the winner), so delta_U =
(2 + 4) u and TOL_MAX = 2 delta_U + 4 u = 16 u relative plus 2^-100 absolute on post, PROB, EVIDENCE and SURVIVED; the moments,
ANGLE and the exact columns as test_tracking_gpu.py holds them.  Steps are teacher-forced from the specification's fp32 map; a
free-running step k gets k TOL_MAX.  Row indices are compared where the specification's own top-2 margin exceeds 2 delta_U
(asserted first).  The backtrack is teacher-forced on the specification's maps and rows: PATH_Y, PATH_X, PATH_LINK, COS, SIN
and PROB (a value read from the input) are equal, SCORE within 2 u (two products rounded once each), and EVERY chained link
must first show a margin above 8 u on the specification alone (test_path.py checks that on the CPU as well)."""
import numpy as np
import pytest
import torch

import path_cases as PC
import test_tracking_gpu as G
from ccvpe_amd import evaluate as E, tracking as T

pytestmark = pytest.mark.gpu


def dev(a, dt):
    return torch.as_tensor(np.array(a), dtype=dt).cuda()                       # a copy: the shared cases are read-only


def run_step(prior, heat, ori, offsets, taps, outlier, reset=None):
    from ccvpe_amd import ops
    b, h, w = heat.shape
    rows, post = ops.belief_viterbi_step(dev(prior, torch.float32).reshape(b, 1, h, w), dev(heat, torch.float32).reshape(b, 1, h, w),
                                         dev(ori, torch.float32), dev(offsets, torch.int32), dev(taps, torch.float32),
                                         outlier=outlier, reset=None if reset is None else dev(reset, torch.int32))
    return post.cpu().numpy().reshape(b, h, w), rows.cpu().numpy()


def assert_step_close(got_post, got_rows, want_post, want_rows, radius, h, w, what, scale=1.0):
    """test_tracking_gpu.assert_step_close at TOL_MAX instead of the sum form's tol_of(radius)"""
    G.assert_step_close(got_post, got_rows, want_post, want_rows, radius, h, w, what,
                        scale=np.asarray(scale, dtype=np.float64) * (PC.TOL_MAX / G.tol_of(radius)))


def run_backtrack(c, reset):
    from ccvpe_amd import ops
    path = ops.belief_backtrack(dev(c["deltas"], torch.float32), dev(c["ori"], torch.float32), dev(c["offsets"], torch.int32),
                                dev(c["taps"], torch.float32), dev(c["rows"], torch.float64),
                                None if reset is None else dev(reset, torch.int32))
    return path.cpu().numpy()


def assert_path_equal(got, want, what):
    exact = [T.PATH_Y, T.PATH_X, T.PATH_LINK, T.PATH_COS, T.PATH_SIN]
    assert np.array_equal(got[..., exact], want[..., exact]), (what, got[..., exact], want[..., exact])
    assert np.array_equal(got[..., T.PATH_PROB].view(np.int64), want[..., T.PATH_PROB].view(np.int64)), what
    gs, ws = got[..., T.PATH_SCORE], want[..., T.PATH_SCORE]
    assert np.all(np.abs(gs - ws) <= 2 * PC.U24 * ws), (what, gs, ws)
    ga, wa = got[..., T.PATH_ANGLE], want[..., T.PATH_ANGLE]
    assert np.array_equal(np.isnan(ga), np.isnan(wa)) and np.all(np.abs(ga - wa)[~np.isnan(wa)] <= 1e-9), what


@pytest.mark.parametrize("h,w", PC.SIZES)
@pytest.mark.parametrize("radius", PC.RADII)
def test_viterbi_step_matches_the_specification(h, w, radius):
    """Ragged tiles (37 x 53: 3 x 1, 70 x 45: 5 x 1), one exact tile (16 x 64, the 16-byte staging), the smallest and the largest
    radius; three tracks with their own offsets and taps, one beyond the grid (Z = 0: RESET 2); NaN planted in the previous
    maps; without reset flags and with (1, 0, 1)."""
    c = PC.step_case(h, w, radius)
    for outlier, reset in ((0.0, None), (0.125, [1, 0, 1])):
        want_post, want_rows, u = T.viterbi_step_spec(c["prior"], c["heat"], c["ori"], c["offsets"], c["taps"], outlier, reset=reset,
                                                      return_u=True)
        PC.assert_argmax_margin(u, 2 * PC.DELTA_U, (h, w, radius))
        assert want_rows[2, T.RESET] == (2 if reset is None else 1) and want_rows[0, T.RESET] == (0 if reset is None else 1)
        got_post, got_rows = run_step(c["prior"], c["heat"], c["ori"], c["offsets"], c["taps"], outlier, reset)
        assert_step_close(got_post, got_rows, want_post, want_rows, radius, h, w, (h, w, radius, outlier))


def test_viterbi_step_with_an_infinite_value():
    """inf in the previous map: P is inf around it, Z is inf, the track resets from the measurement (RESET 2), on both sides."""
    c = PC.step_case(37, 53, 1)
    prior = c["prior"].copy()
    prior[0, 20, 20] = np.inf
    want_post, want_rows = T.viterbi_step_spec(prior, c["heat"], c["ori"], c["offsets"], c["taps"], 0.0625)
    assert want_rows[:, T.RESET].tolist() == [2, 0, 2] and want_rows[0, T.SURVIVED] == np.inf
    got_post, got_rows = run_step(prior, c["heat"], c["ori"], c["offsets"], c["taps"], 0.0625)
    assert got_rows[0, T.SURVIVED] == np.inf
    got, want = got_rows.copy(), want_rows.copy()
    got[0, T.SURVIVED] = want[0, T.SURVIVED] = 0.0                             # compared above: inf - inf has no distance
    assert_step_close(got_post, got, want_post, want, 1, 37, 53, "inf")


def test_viterbi_step_full_size_and_bit_identical_calls():
    """512 x 512, R = 8, B = 2: 256 tiles per track, the 16-byte paths, an offset of a whole tile plus one on each axis."""
    h = w = 512
    rng = np.random.default_rng(12)
    prior, heat, ori = G.softmax_maps(rng, 2, h, w), G.softmax_maps(rng, 2, h, w), G.unit_ori(rng, 2, h, w)
    offsets, taps = T.motion_taps_spec([[17.3, -65.2], [-3.6, 2.5]], [2.5, 1.7], 8)
    assert offsets.tolist() == [[17, -65], [-4, 3]]
    want_post, want_rows, u = T.viterbi_step_spec(prior, heat, ori, offsets, taps, 0.03125, return_u=True)
    PC.assert_argmax_margin(u, 2 * PC.DELTA_U, "full size")
    assert want_rows[:, T.RESET].tolist() == [0, 0]
    got_post, got_rows = run_step(prior, heat, ori, offsets, taps, 0.03125)
    assert_step_close(got_post, got_rows, want_post, want_rows, 8, h, w, "full size")
    again_post, again_rows = run_step(prior, heat, ori, offsets, taps, 0.03125)
    assert np.array_equal(got_post.view(np.int32), again_post.view(np.int32))
    assert np.array_equal(got_rows.view(np.int64), again_rows.view(np.int64))


@pytest.mark.parametrize("h,w", PC.SIZES)
@pytest.mark.parametrize("radius", PC.RADII)
def test_backtrack_matches_the_specification(h, w, radius):
    """T = 6, B = 3, teacher-forced on the specification's maps and rows: a start in mid-drive (track 1, frame 3), a frame with
    RESET 2 (track 2, frame 2), windows cut by the grid edge (track 0 ends one pixel from the corner).  Two launches are
    bit-identical."""
    c = PC.drive_case(h, w, radius)
    PC.assert_link_margins(c["path"], c["margin"], PC.LINK_MARGIN, (h, w, radius))
    assert c["rows"][2, 2, T.RESET] == 2 and c["path"][1, 2, T.PATH_LINK] == 1 and c["path"][2, 1, T.PATH_LINK] == 1
    assert radius == 0 or PC.window_is_cut(c, radius)
    got = run_backtrack(c, c["reset"])
    assert_path_equal(got, c["path"], (h, w, radius))
    assert np.array_equal(got.view(np.int64), run_backtrack(c, c["reset"]).view(np.int64))
    # without the flags the rows' own RESET column still ends the segments of frame 0 (state 1) and of track 2's frame 2
    bare = T.backtrack_spec(c["deltas"], c["ori"], c["offsets"], c["taps"], c["rows"], None, return_margin=True)
    PC.assert_link_margins(bare[0], bare[1], PC.LINK_MARGIN, (h, w, radius, "no flags"))
    assert_path_equal(run_backtrack(c, None), bare[0], (h, w, radius, "no flags"))


def test_backtrack_resolves_an_exact_tie_to_the_smaller_index():
    c = PC.tie_case()
    PC.assert_link_margins(c["path"], c["margin"], PC.LINK_MARGIN, "tie")
    got = run_backtrack(c, None)
    assert got[0, 0, [T.PATH_Y, T.PATH_X, T.PATH_LINK]].tolist() == [4, 4, 0]
    assert_path_equal(got, c["path"], "tie")


def test_backtrack_clamps_a_rows_pixel_off_the_grid():
    """PRED_Y = +inf and PRED_X = NaN in the last row: the kernel starts at (h - 1, 0) as the specification does, finds no mass
    in that window (LINK 2, no decision to compare) and takes frame 0's own arg-max."""
    c = dict(PC.tie_case())
    rows = c["rows"].copy()
    rows[1, 0, T.PRED_Y], rows[1, 0, T.PRED_X] = np.inf, np.nan
    c["rows"] = rows
    want = T.backtrack_spec(c["deltas"], c["ori"], c["offsets"], c["taps"], rows)
    assert want[:, 0, [T.PATH_Y, T.PATH_X, T.PATH_LINK]].tolist() == [[3, 5, 2], [8, 0, 1]]
    assert_path_equal(run_backtrack(c, None), want, "clamped")


def test_backtrack_full_size():
    """512 x 512, T = 3, B = 2, R = 8: flat indices up to 2^18, the chain through two links per track."""
    h = w = 512
    n, b, radius = 3, 2, 8
    rng = np.random.default_rng(13)
    heat, ori = G.softmax_maps(rng, n * b, h, w).reshape(n, b, h, w), G.unit_ori(rng, n * b, h, w).reshape(n, b, 2, h, w)
    offsets, taps = T.motion_taps_spec(rng.uniform(-70, 70, (n * b, 2)), 2.5, radius)
    offsets, taps = offsets.reshape(n, b, 2), taps.reshape(n, b, 2, -1)
    deltas, rows = np.zeros((n, b, h, w), np.float32), np.zeros((n, b, 14))
    for t in range(n):
        deltas[t], rows[t] = T.viterbi_step_spec(deltas[t - 1], heat[t], ori[t], offsets[t], taps[t], 0.03125, reset=[int(t == 0)] * b)
    want, margin = T.backtrack_spec(deltas, ori, offsets, taps, rows, None, return_margin=True)
    PC.assert_link_margins(want, margin, PC.LINK_MARGIN, "full size")
    assert want[:, :, T.PATH_LINK].tolist() == [[0, 0], [0, 0], [1, 1]]
    got = run_backtrack(dict(deltas=deltas, ori=ori, offsets=offsets, taps=taps, rows=rows), None)
    assert_path_equal(got, want, "full size")


def _record_backtrack(monkeypatch):
    """record the motion inputs MostLikelyPath hands to ops.belief_backtrack, so that the specification runs on the same taps"""
    from ccvpe_amd import ops
    real, seen = ops.belief_backtrack, []

    def recording(deltas, ori, offsets, taps, rows, reset=None, out=None):
        seen.append((offsets.clone(), taps.clone()))
        return real(deltas, ori, offsets, taps, rows, reset, out)

    monkeypatch.setattr(ops, "belief_backtrack", recording)
    return seen


_RUN = {}


def scenario_run(monkeypatch):
    """MostLikelyPath.run free-running over the two 24-frame scenarios as B = 2 tracks with their own shifts and starts; the
    specification on the very taps the device computed.  Run once, shared (read-only)."""
    if _RUN:
        return _RUN
    s = PC.scenarios()
    n, b, h, w = s["heat"].shape
    seen = _record_backtrack(monkeypatch)
    mlp = T.MostLikelyPath((h, w), sigma_px=G.TRK["sigma"], radius=G.TRK["radius"], outlier=G.TRK["outlier"])
    out = mlp.run(dev(s["heat"], torch.float32), dev(s["ori"], torch.float32), dev(s["odo"], torch.float64), starts=s["starts"])
    assert len(seen) == 1
    offsets, taps = seen[0][0].cpu().numpy(), seen[0][1].cpu().numpy()
    want_o, want_k = T.motion_taps_spec(s["odo"].reshape(-1, 2), G.TRK["sigma"], G.TRK["radius"])
    assert np.array_equal(offsets.reshape(-1, 2), want_o)
    assert np.all(np.abs(taps.reshape(want_k.shape).astype(np.float64) - want_k) <= np.spacing(want_k))
    _RUN.update(out={k: v.cpu().numpy() for k, v in out.items()}, spec=PC.spec_run(offsets, taps), mlp=mlp)
    return _RUN


def test_most_likely_path_free_running(monkeypatch):
    """24 frames, never corrected: maps within k TOL_MAX at step k, the rows' arg-max and the PATH equal to the specification's
    in every frame of both tracks; every link's margin on the specification exceeds 2 * 24 TOL_MAX + 8 u first."""
    s, r = PC.scenarios(), scenario_run(monkeypatch)
    n, b, h, w = s["heat"].shape
    out, spec = r["out"], r["spec"]
    PC.assert_argmax_margin(spec["us"], 2 * n * PC.TOL_MAX, "free-running")
    PC.assert_link_margins(spec["path"], spec["margin"], 2 * n * PC.TOL_MAX + PC.LINK_MARGIN, "free-running")
    assert spec["rows"][:, 0, T.RESET].tolist() == [1] + [0] * (n - 1)
    assert spec["rows"][:, 1, T.RESET].tolist() == [float(t in (0, 12)) for t in range(n)]
    for t in range(n):
        assert_step_close(out["deltas"][t, :, 0], out["rows"][t], spec["deltas"][t], spec["rows"][t], G.TRK["radius"], h, w,
                          ("free-running", t), scale=t + 1)
    exact = [T.PATH_Y, T.PATH_X, T.PATH_LINK, T.PATH_COS, T.PATH_SIN]
    assert np.array_equal(out["path"][..., exact], spec["path"][..., exact])
    assert spec["path"][:, 1, T.PATH_LINK].tolist() == [float(t in (11, 23)) for t in range(n)]
    scale = np.arange(1, n + 1)[:, None] * PC.TOL_MAX
    for c in (T.PATH_PROB, T.PATH_SCORE):
        assert np.all(np.abs(out["path"][..., c] - spec["path"][..., c]) <= (scale + 2 * PC.U24) * spec["path"][..., c] + PC.ABS), c
    err = PC.path_errors(out["path"], s["pos"])
    print("most likely path: mean error %s px, at the starts %s px, smallest link margin %s u"
          % (err.mean(0), err[[0, 0, 12], [0, 1, 1]], np.nanmin(spec["margin"], 0) / PC.U24))


@pytest.mark.parametrize("track", [0, 1], ids=["original", "moved"])
def test_the_path_beats_the_filters_arg_max(monkeypatch, track):
    """The device's mean path error — against the rounded true position: the path is a sequence of grid cells — is below the
    mean arg-max error of the histogram filter as this suite and the README state it (step_spec's PRED_Y, PRED_X against the
    true position, computed here as test_tracking_gpu.py and test_smoother.py compute it): moved scenario 0.333 px against
    1.903 px, original scenario 0.434 px against 0.482 px.

    Held to the same reference the path is never worse and, where the filter is fooled, strictly better: against the rounded
    position the filter has 1.764 px on the moved scenario (path 0.333 px).  On the original scenario no distractor falls on a
    start frame, the filter is never fooled, and path and filter visit the very same 24 pixels (0.434 px both): there the
    first inequality rests on the reference alone."""
    s, r = PC.scenarios(), scenario_run(monkeypatch)
    n = s["heat"].shape[0]
    offsets, taps = T.motion_taps_spec(s["odo"][:, track], G.TRK["sigma"], G.TRK["radius"])
    post = np.zeros((1,) + s["heat"].shape[2:], np.float32)
    fil, fil_cell = np.zeros(n), np.zeros(n)
    for t in range(n):
        post, row = T.step_spec(post, s["heat"][t, track:track + 1], s["ori"][t, track:track + 1], offsets[t:t + 1], taps[t:t + 1],
                                G.TRK["outlier"], reset=[int(s["starts"][t, track])])
        fil[t] = np.hypot(row[0, T.PRED_Y] - s["pos"][t, track, 0], row[0, T.PRED_X] - s["pos"][t, track, 1])
        fil_cell[t] = np.hypot(row[0, T.PRED_Y] - np.rint(s["pos"][t, track, 0]), row[0, T.PRED_X] - np.rint(s["pos"][t, track, 1]))
    err = PC.path_errors(r["out"]["path"], s["pos"])[:, track]
    print("track %d: mean path error %.4f px; filter %.4f px against the true position, %.4f px against its cell"
          % (track, err.mean(), fil.mean(), fil_cell.mean()))
    assert err.mean() < fil.mean()
    assert err.mean() <= fil_cell.mean() and (track == 0 or err.mean() < fil_cell.mean())
    assert np.all(err[s["starts"][:, track] != 0] == 0)


def test_one_track_takes_the_short_shapes(monkeypatch):
    """B = 1 with ori [T,2,h,w] and shift_px [T,2]: the bits of that track in the B = 2 run."""
    s, r = PC.scenarios(), scenario_run(monkeypatch)
    out = r["mlp"].run(dev(s["heat"][:, 1:2], torch.float32), dev(s["ori"][:, 1], torch.float32), dev(s["odo"][:, 1], torch.float64),
                       starts=s["starts"][:, 1])
    assert tuple(out["path"].shape) == (24, 1, 8) and tuple(out["rows"].shape) == (24, 1, 14) and tuple(out["deltas"].shape)[:3] == (24, 1, 1)
    for key in ("rows", "path"):
        assert np.array_equal(out[key].cpu().numpy()[:, 0].view(np.int64), r["out"][key][:, 1].view(np.int64)), key
    assert np.array_equal(out["deltas"].cpu().numpy()[:, 0].view(np.int32), r["out"]["deltas"][:, 1].view(np.int32))
    with pytest.raises(ValueError):
        r["mlp"].run(dev(s["heat"][:, 1:2], torch.float32), dev(s["ori"][:, 1], torch.float32), dev(s["odo"][:5, 1], torch.float64))
    with pytest.raises(ValueError):
        r["mlp"].run(dev(s["heat"][:, 1:2], torch.float32), dev(s["ori"][:3, 1], torch.float32), dev(s["odo"][:, 1], torch.float64))


def test_evaluate_sequence_with_the_path(tmp_path, monkeypatch):
    """The nine-frame synthetic Oxford tree of test_tracking_gpu.py with a stub forward: path_tracks equal backtrack_spec on
    the specification's free-running maps (margins asserted first), path_rows equal metrics_spec of one-hot maps at the
    specification's path, "raw" and "filtered" are bit-equal to a call without the keyword, still one read-back."""
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
        state = {"k": 0}

        def forward(grd, sat):
            k, b = state["k"], grd.shape[0]
            state["k"] = k + b
            return (None, heats[k:k + b].contiguous(), oris[k:k + b].contiguous())
        return forward

    seen_batches = []

    class Recording(DS.DeviceBatches):
        def __iter__(self):
            for batch in super().__iter__():
                seen_batches.append(batch)
                yield batch

    kw = dict(batch_size=4, device="cuda", workers=2, targets=True, grd_hw=(154, 231), ascending_bins=True)
    base = E.evaluate_sequence(stub_for(), DS.DeviceBatches(ds, **kw), T.HistogramFilter(1, sigma_px=2.0, outlier=0.02), shift, starts)
    assert sorted(base) == ["filtered", "filtered_rows", "indices", "raw", "raw_rows", "tracks"]
    seen = _record_backtrack(monkeypatch)
    real_cpu, reads = torch.Tensor.cpu, []

    def counting_cpu(self, *a, **k):
        if self.is_cuda and self.dtype == torch.float64 and self.dim() == 2:
            reads.append(tuple(self.shape))
        return real_cpu(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "cpu", counting_cpu)
    res = E.evaluate_sequence(stub_for(), Recording(ds, **kw), T.HistogramFilter(1, sigma_px=2.0, outlier=0.02), shift, starts, path=True)
    monkeypatch.setattr(torch.Tensor, "cpu", real_cpu)
    assert reads == [(n, 58)] and len(seen) == 1
    assert sorted(res) == sorted(list(base) + ["path", "path_rows", "path_tracks"])
    for key in ("raw_rows", "filtered_rows", "tracks"):
        assert np.array_equal(res[key].view(np.int64), base[key].view(np.int64)), key
    for key in ("raw", "filtered"):
        assert repr(res[key]) == repr(base[key]), key
    # the specification, free-running on the device's own taps
    offsets, taps = seen[0][0].cpu().numpy(), seen[0][1].cpu().numpy()
    want_o, want_k = T.motion_taps_spec(shift, 2.0, 7)
    assert np.array_equal(offsets.reshape(n, 2), want_o) and np.all(np.abs(taps.reshape(want_k.shape).astype(np.float64) - want_k) <= np.spacing(want_k))
    h_heat, h_ori = heats.cpu().numpy(), oris.cpu().numpy()
    deltas, rows, us = np.zeros((n, 1, 512, 512), np.float32), np.zeros((n, 1, 14)), np.zeros((n, 1, 512, 512))
    reset = starts.astype(np.int32).reshape(n, 1)
    for i in range(n):
        deltas[i], rows[i], us[i] = T.viterbi_step_spec(deltas[i - 1], h_heat[i], h_ori[i:i + 1], offsets[i], taps[i], 0.02, reset=reset[i],
                                                        return_u=True)
    want, margin = T.backtrack_spec(deltas, h_ori.reshape(n, 1, 2, 512, 512), offsets, taps, rows, reset, return_margin=True)
    PC.assert_argmax_margin(us, 2 * n * PC.TOL_MAX, "sequence")
    PC.assert_link_margins(want, margin, 2 * n * PC.TOL_MAX + PC.LINK_MARGIN, "sequence")
    got = res["path_tracks"]
    exact = [T.PATH_Y, T.PATH_X, T.PATH_LINK, T.PATH_COS, T.PATH_SIN]
    assert np.array_equal(got[:, exact], want[:, 0, exact])
    for c in (T.PATH_PROB, T.PATH_SCORE):
        assert np.all(np.abs(got[:, c] - want[:, 0, c]) <= (n * PC.TOL_MAX + 2 * PC.U24) * want[:, 0, c] + PC.ABS), c
    onehot = np.zeros((n, 1, 512, 512), np.float32)
    onehot[np.arange(n), 0, want[:, 0, T.PATH_Y].astype(int), want[:, 0, T.PATH_X].astype(int)] = 1.0
    gt = np.concatenate([b.gt.cpu().numpy() for b in seen_batches])
    gt_ori = np.concatenate([b.gt_ori.cpu().numpy() for b in seen_batches])
    heading = np.concatenate([b.heading_deg.cpu().numpy() for b in seen_batches])
    rows_want = E.metrics_spec(onehot, h_ori, gt, gt_ori, heading, np.full(n, E.OXFORD_METRES_PER_PIXEL))
    a, b = res["path_rows"], rows_want
    assert np.array_equal(a[:, :4], b[:, :4])
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.all(np.abs(a - b)[~np.isnan(b)] <= 1e-9 + 1e-9 * np.abs(b[~np.isnan(b)]))
    assert res["path"]["n"] == n and res["path"]["mean_pixel_error"] == float(np.mean(b[:, E.PIXEL]))
    follow = [i for i in range(n) if i % 2 == 1 and not starts[i]]
    assert follow and np.all(res["raw_rows"][follow, E.PIXEL] > 20) and np.all(a[follow, E.PIXEL] <= 2)
    with pytest.raises(ValueError):
        E.evaluate_sequence(stub_for(), DS.DeviceBatches(ds, **kw), T.HistogramFilter(1), None, starts, motion=np.zeros((n, 6)), path=True)
