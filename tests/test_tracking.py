"""CPU-side checks of the histogram filter (ccvpe_amd/tracking.py): the motion taps against their numpy twin, the properties
of the step's specification, the Oxford shifts against the loader's own ground-truth pixels, and the refusals of
ccvpe_belief_step_f32 that need no GPU."""
import numpy as np
import pytest
import torch

from ccvpe_amd import _lib, tracking as T


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32)))


@pytest.mark.parametrize("radius", [0, 1, 4, 32])
def test_motion_taps_match_the_numpy_twin(radius):
    """Half-integer, negative and large shifts; a scalar and a per-track sigma; sigma = 0: offsets equal, taps within 1 fp32
    ulp of motion_taps_spec (both normalise in float64; only exp may differ in its last float64 place), sums within 2^-22."""
    shifts = np.array([[0.0, 0.0], [0.5, -0.5], [-2.4, 3.5], [1.5, -1.5], [30.6, -40.2], [-0.49999, 0.49999], [600.25, -7.75],
                       [-3.0, 2.0]])
    for sigma in (0.0, 0.3, 1.5, 10.0, np.linspace(0.0, 4.0, len(shifts))):
        want_o, want_k = T.motion_taps_spec(shifts, sigma, radius)
        sig = torch.as_tensor(sigma, dtype=torch.float64) if isinstance(sigma, np.ndarray) else float(sigma)
        got_o, got_k = T.motion_taps(torch.from_numpy(shifts), sig, radius)
        assert got_o.dtype == torch.int32 and got_k.dtype == torch.float32
        assert tuple(got_o.shape) == (len(shifts), 2) and tuple(got_k.shape) == (len(shifts), 2, 2 * radius + 1)
        assert np.array_equal(got_o.numpy(), want_o)
        assert np.all(np.abs(got_k.numpy().astype(np.float64) - want_k.astype(np.float64)) <= _ulp32(want_k))
        # fp32 rounding of 2R+1 non-negative taps that sum to 1 in float64: each is off by <= 2^-25 of itself
        assert np.all(np.abs(got_k.numpy().astype(np.float64).sum(-1) - 1.0) <= 2.0 ** -22)
        assert np.all(got_k.numpy() >= 0)
    o, k = T.motion_taps_spec([[0.5, -0.5], [1.5, -2.5]], 1.0, 2)
    assert o.tolist() == [[1, 0], [2, -2]]                       # floor(s + 0.5): halves round up
    o, k = T.motion_taps_spec([[2.3, -7.0]], 0.0, 3)
    assert o.tolist() == [[2, -7]] and k[0, 0].tolist() == [0, 0, 0, 1, 0, 0, 0] and k[0, 1].tolist() == [0, 0, 0, 1, 0, 0, 0]
    # the fractional part moves the taps' centre of mass: a shift of +0.3 leans towards d = +1
    o, k = T.motion_taps_spec([[0.3, 0.0]], 1.0, 4)
    d = np.arange(-4, 5)
    assert abs(float((k[0, 0] * d).sum()) - 0.3) < 1e-3 and abs(float((k[0, 1] * d).sum())) < 1e-7


def _softmax_map(rng, b, h, w):
    z = rng.standard_normal((b, h, w)) * 4
    p = np.exp(z - z.max(axis=(1, 2), keepdims=True))
    return (p / p.sum(axis=(1, 2), keepdims=True)).astype(np.float32)


def _unit_ori(rng, b, h, w):
    a = rng.uniform(0, 2 * np.pi, (b, h, w))
    return np.stack([np.cos(a), np.sin(a)], 1).astype(np.float32)


def test_step_spec_translation_pins_the_sign_convention():
    h, w, y0, x0 = 23, 31, 9, 17
    prior = np.zeros((1, h, w), np.float32)
    prior[0, y0, x0] = 1.0
    heat = np.full((1, h, w), 1.0 / (h * w), np.float32)
    ori = _unit_ori(np.random.default_rng(0), 1, h, w)
    post, rows, u = T.step_spec(prior, heat, ori, [[3, -5]], np.ones((1, 2, 1), np.float32), 0.0, return_u=True)
    assert np.count_nonzero(u[0]) == 1 and u[0, y0 + 3, x0 - 5] > 0
    assert rows[0, T.PRED_Y] == y0 + 3 and rows[0, T.PRED_X] == x0 - 5 and rows[0, T.RESET] == 0
    assert abs(rows[0, T.PROB] - 1.0) < 1e-6 and rows[0, T.SURVIVED] == 1.0
    assert rows[0, T.MEAN_Y] == y0 + 3 and rows[0, T.MEAN_X] == x0 - 5 and abs(rows[0, T.VAR_YY]) < 1e-12
    assert rows[0, T.COS] == ori[0, 0, y0 + 3, x0 - 5] and rows[0, T.SIN] == ori[0, 1, y0 + 3, x0 - 5]
    # an asymmetric tap moves mass the same way: ky = [0, 0, 1] puts i = +1 on the prior's pixel -> one row further down
    ky = np.array([0, 0, 1], np.float32)
    kx = np.array([1, 0, 0], np.float32)
    post, rows = T.step_spec(prior, heat, ori, [[0, 0]], np.stack([ky, kx])[None], 0.0)
    assert rows[0, T.PRED_Y] == y0 + 1 and rows[0, T.PRED_X] == x0 - 1
    # the formula, not shift-crop-blur: a peak moved one row above the grid still blurs back into row 0 (i = +1)
    edge = np.zeros((1, h, w), np.float32)
    edge[0, 0, x0] = 1.0
    ky = np.array([0.25, 0.5, 0.25], np.float32)
    post, rows, u = T.step_spec(edge, heat, ori, [[-1, 0]], np.stack([ky, np.array([0, 1, 0], np.float32)])[None], 0.0, return_u=True)
    assert np.count_nonzero(u[0]) == 1 and rows[0, T.PRED_Y] == 0 and rows[0, T.PRED_X] == x0 and rows[0, T.SURVIVED] == 0.25


def test_step_spec_identity_motion_is_the_bayes_product():
    rng = np.random.default_rng(1)
    h, w = 19, 27
    prior, heat = _softmax_map(rng, 2, h, w), _softmax_map(rng, 2, h, w)
    ori = _unit_ori(rng, 2, h, w)
    post, rows = T.step_spec(prior, heat, ori, np.zeros((2, 2), np.int32), np.ones((2, 2, 1), np.float32), 0.0)
    for b in range(2):
        prod = prior[b].astype(np.float64) * heat[b].astype(np.float64)
        want = prod / prod.sum()
        assert np.allclose(post[b], want, rtol=2e-7, atol=0)
        assert abs(rows[b, T.EVIDENCE] - prod.sum()) <= 1e-15 * prod.sum()
        assert abs(rows[b, T.SURVIVED] - prior[b].astype(np.float64).sum()) < 1e-12
        assert (rows[b, T.PRED_Y], rows[b, T.PRED_X]) == np.unravel_index(np.argmax(prod), prod.shape)
        assert rows[b, T.RESET] == 0
        c, s = rows[b, T.COS], rows[b, T.SIN]
        assert abs(rows[b, T.ANGLE] - np.degrees(np.arctan2(s, c)) % 360) < 1e-3      # unit vectors: acos rule = atan2


def test_step_spec_mass_off_the_grid_resets_to_the_measurement():
    rng = np.random.default_rng(2)
    h, w = 17, 21
    prior, heat = _softmax_map(rng, 3, h, w), _softmax_map(rng, 3, h, w)
    ori = _unit_ori(rng, 3, h, w)
    _, taps = T.motion_taps_spec(np.zeros((3, 2)), 1.0, 2)
    offsets = np.array([[h + 2, 0], [0, -(w + 2)], [2 ** 31 - 1, -2 ** 31]])
    alpha = 0.25
    post, rows = T.step_spec(prior, heat, ori, offsets, taps, alpha)
    m = (1 - np.float64(np.float32(alpha))) * heat.astype(np.float64) + np.float64(np.float32(alpha)) / (h * w)
    for b in range(3):
        assert rows[b, T.RESET] == 2 and rows[b, T.SURVIVED] == 0.0
        assert np.allclose(post[b], m[b] / m[b].sum(), rtol=2e-7, atol=0)
        assert abs(rows[b, T.EVIDENCE] - m[b].sum()) < 1e-12
    # the reset flag gives the same posterior, says 1, and skips the predict
    post1, rows1 = T.step_spec(prior, heat, ori, np.zeros((3, 2), np.int32), taps, alpha, reset=[1, 1, 1])
    assert np.array_equal(post1, post) and np.all(rows1[:, T.RESET] == 1) and np.all(rows1[:, T.SURVIVED] == 0)
    # partial loss: SURVIVED is the mass that stayed
    post2, rows2 = T.step_spec(prior, heat, ori, [[5, 0]] * 3, np.ones((3, 2, 1), np.float32), 0.0)
    for b in range(3):
        assert abs(rows2[b, T.SURVIVED] - prior[b, :h - 5].astype(np.float64).sum()) < 1e-12 and rows2[b, T.RESET] == 0


def test_oxford_shifts_follow_the_loaders_ground_truth(tmp_path):
    """The difference between consecutive samples' ground-truth pixels (256 - center) against shift_px.  On the default
    fixture tree the two agree within 1.5 px (the loader's two int() truncations plus rounding).  The bound that holds for ANY
    pair of frames is wider and is checked on a second, longer tree: the loader rounds the patch coordinate (0.5 map px =
    0.32 px per frame) and then truncates 256 - 0.64 p TOWARDS ZERO, so a frame's pixel is off by less than 1 px upwards in one
    half of the patch and downwards in the other; two frames on opposite sides of the patch centre differ by up to
    2 * (1 + 0.32) = 2.64 px (the longer tree has such pairs: up to 2.0 px)."""
    from ccvpe_amd import datasets as DS
    from test_datasets import make_oxford_tree
    for sub, n, bound in (("a", 3, 1.5), ("b", 6, 2.64)):
        (tmp_path / sub).mkdir()
        g, sat_path = make_oxford_tree(str(tmp_path / sub), n=n)
        _check_oxford_tree(DS, g, sat_path, bound)
    te = DS.OxfordPairs(g, sat_path, split="test")
    shift, starts = T.oxford_shifts(te, indices=[1, 2, 4, 6, 7])
    assert starts.tolist() == [True, False, True, True, False]      # first index, a gap, a new traversal
    full, _ = T.oxford_shifts(te)
    assert np.array_equal(shift[[1, 4]], full[[2, 7]])
    with pytest.raises(ValueError):
        T.oxford_shifts(DS.OxfordPairs(g, sat_path, split="train"))


def _check_oxford_tree(DS, g, sat_path, bound):
    for split in ("test", "val"):
        ds = DS.OxfordPairs(g, sat_path, split=split)
        shift, starts = T.oxford_shifts(ds)
        assert shift.shape == (len(ds), 2) and shift.dtype == np.float64 and starts.dtype == bool
        firsts = np.cumsum([0] + ds.list_lengths)[:-1]
        assert np.flatnonzero(starts).tolist() == firsts.tolist()
        assert np.all(shift[starts] == 0)
        px = np.array([[256 - ds.sample(i)["center"][1], 256 - ds.sample(i)["center"][0]] for i in range(len(ds))])
        moved = 0
        for i in range(1, len(ds)):
            if starts[i]:
                continue
            assert np.all(np.abs((px[i] - px[i - 1]) - shift[i]) <= bound), (i, px[i] - px[i - 1], shift[i])
            moved += int(np.any(np.abs(shift[i]) > 2))
        assert moved > 0                                            # the fixture's vehicles do move


def test_histogram_filter_refuses_bad_settings_without_a_gpu():
    with pytest.raises(ValueError, match="radius"):
        T.HistogramFilter(1, sigma_px=11.0, device="cpu")           # ceil(33) + 1 = 34 > 32
    with pytest.raises(ValueError, match="radius"):
        T.HistogramFilter(1, sigma_px=1.0, radius=33, device="cpu")
    with pytest.raises(ValueError, match="outlier"):
        T.HistogramFilter(1, sigma_px=1.0, outlier=1.5, device="cpu")
    assert (T.PRED_Y, T.PRED_X, T.PROB, T.COS, T.SIN, T.ANGLE, T.EVIDENCE, T.RESET, T.MEAN_Y, T.MEAN_X, T.VAR_YY, T.VAR_XX,
            T.COV_YX, T.SURVIVED) == tuple(range(14))


def test_belief_step_rejects_bad_arguments_without_a_gpu():
    """ccvpe_belief_step_f32 validates before it launches (the pattern of test_abi.py: fake aligned pointers that are never
    dereferenced): CCVPE_EINVAL and a message, nothing enqueued."""
    lib = _lib.load()
    EINVAL = -1
    n = 64 * 64 * 4
    prior, heat, ori, off, taps, post, scratch, rows = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000, 0x800000

    def call(prior=prior, radius=8, outlier=0.1, post=post, scratch=scratch, rows=rows, batch=2, h=64, w=64, taps=taps):
        return lib.ccvpe_belief_step_f32(prior, heat, ori, off, taps, radius, outlier, None, post, scratch, rows, batch, h, w, None)

    assert call(radius=33) == EINVAL and b"radius" in lib.ccvpe_last_error()
    assert call(radius=-1) == EINVAL and b"radius" in lib.ccvpe_last_error()
    assert call(outlier=1.5) == EINVAL and b"outlier" in lib.ccvpe_last_error()
    assert call(outlier=float("nan")) == EINVAL and b"outlier" in lib.ccvpe_last_error()
    assert call(post=prior) == EINVAL and b"overlap" in lib.ccvpe_last_error()
    assert call(post=prior + 2 * n - 4) == EINVAL and b"overlap" in lib.ccvpe_last_error()       # the last float of B = 2 maps
    assert call(prior=post + 2 * n - 4) == EINVAL and b"overlap" in lib.ccvpe_last_error()
    # launch two reads heat (a reset) and ori (the row) after launch one wrote U into post: neither may share memory with it
    assert call(post=heat) == EINVAL and b"heat and post overlap" in lib.ccvpe_last_error()
    assert call(post=heat - 2 * n + 4) == EINVAL and b"heat and post overlap" in lib.ccvpe_last_error()
    assert call(post=ori + 4 * n - 4) == EINVAL and b"ori and post overlap" in lib.ccvpe_last_error()          # ori is [B,2,h,w]
    assert call(post=ori - 2 * n + 4) == EINVAL and b"ori and post overlap" in lib.ccvpe_last_error()
    assert call(rows=None) == EINVAL and b"null" in lib.ccvpe_last_error()
    assert call(taps=None) == EINVAL and b"null" in lib.ccvpe_last_error()
    assert call(rows=rows + 4) == EINVAL and b"8-byte" in lib.ccvpe_last_error()
    assert call(scratch=scratch + 4) == EINVAL and b"8-byte" in lib.ccvpe_last_error()
    assert call(h=0) == EINVAL and b"shape" in lib.ccvpe_last_error()
    assert call(batch=0) == EINVAL and b"shape" in lib.ccvpe_last_error()
    assert call(h=65536, w=65536) == EINVAL
    # scratch doubles per track: 18 per 16 x 64 tile, nothing launched
    assert lib.ccvpe_belief_partials(512, 512) == 32 * 8 * 18 and lib.ccvpe_belief_partials(37, 53) == 3 * 1 * 18
    assert lib.ccvpe_belief_partials(0, 5) == EINVAL and lib.ccvpe_belief_partials(65536, 65536) == EINVAL
    assert lib.ccvpe_belief_partials(1, 2 ** 31 - 1) == EINVAL            # h w rounded up to a multiple of 4 must stay an int
    assert lib.ccvpe_belief_partials(1, 2 ** 31 - 16) == ((2 ** 31 - 16 + 63) // 64) * 18
