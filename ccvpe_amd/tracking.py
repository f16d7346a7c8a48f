"""Sequence localisation: a histogram filter (recursive Bayes filter over the map grid) on the network's heat-maps.

The forward gives a normalised likelihood on the 512 x 512 grid per frame, and its heat-maps are multi-modal: a single frame
is often ambiguous and the wrong mode wins the arg-max.  On a drive (Oxford RobotCar traversals, KITTI) the belief of the
previous frame, moved by the odometry and by the motion of the aerial patch and blurred by the motion noise, is the prior of
the next one:

    predict   Q[y,x] = sum_i ky[i+R] sum_j kx[j+R] prior[y - oy - i, x - ox - j]      (prior = 0 outside the grid)
    measure   M = (1 - outlier) heat + outlier / (h w),   U = Q M,   Z = sum U
    posterior post = U / Z, the estimate is read off it (arg-max, mean, covariance)

`step_spec` states one step in numpy float64 and is the oracle of every test; `ops.belief_step` runs it on the device in two
launches (csrc/belief.hip); `HistogramFilter` owns the belief buffers of a set of tracks; `motion_taps` turns a sub-pixel shift
and a noise level into the integer offset and the blur taps; `oxford_shifts` derives the per-frame shifts of an Oxford
traversal; `evaluate.evaluate_sequence` reports the reference's protocol numbers for the raw and the filtered estimate.

Where the patch frame also turns between two frames (KITTI: every aerial patch is re-centred on the vehicle, turned to its
heading and rotated by the sample's theta) the predict is a rigid motion: the prior is resampled bilinearly through the inverse
map of `rigid_motion` and then blurred with centred taps — `step_rigid_spec` is the specification, `ops.belief_step_rigid` the
device step, `HistogramFilter.step(motion=...)` the filter's entry and `kitti_motions` the per-frame motions of a KITTI test
split.

Offline — a recorded drive, evaluated after the fact — the estimate of frame t is the SMOOTHED one, given the whole drive:
`SequenceSmoother` filters one track forward, keeps every posterior and walks back with the backward step

    G = M_t beta_t,   B' = adjoint of the predict applied to G,   smooth_s = alpha_s B' / sum,   beta_s = B' / sum

(`smooth_step_spec` / `smooth_step_rigid_spec` are the specifications, `ops.belief_smooth_step` / `ops.belief_smooth_step_rigid`
the device steps, `invert_motion` the reverse of a rigid motion row); `evaluate.evaluate_sequence(..., smooth=True)` reports it.

One trajectory — the jointly most likely sequence of grid cells, which the per-frame arg-max of the smoothed marginals is
not — is the max-product (Viterbi) solution: `MostLikelyPath` runs the forward step with the predict's sums replaced by maxima
(`viterbi_step_spec`, `ops.belief_viterbi_step`) and keeps every map, then walks back in one launch (`backtrack_spec`,
`ops.belief_backtrack`), recomputing each link's decision at the one pixel the path visits; there are no back-pointer maps.
`evaluate.evaluate_sequence(..., path=True)` reports it.

Out of scope: a change of scale between patch frames, learned motion models, bf16 beliefs; for the smoother also several
tracks per `SequenceSmoother` and fixed-lag (online) smoothing; for the path the rigid (KITTI) form — its warp is a bilinear mix,
not a maximum, so its back-pointer needs a definition of its own — stored back-pointer maps, log-domain maps, bf16 maps and
fixed-lag decoding.
"""
import functools
import math
import os

import numpy as np
import torch

# columns of a track row (ccvpe_belief_step_f32 / step_spec)
(PRED_Y, PRED_X, PROB, COS, SIN, ANGLE, EVIDENCE, RESET, MEAN_Y, MEAN_X, VAR_YY, VAR_XX, COV_YX, SURVIVED) = range(14)
# columns of a path row (ccvpe_belief_backtrack_f32 / backtrack_spec)
(PATH_Y, PATH_X, PATH_PROB, PATH_COS, PATH_SIN, PATH_ANGLE, PATH_LINK, PATH_SCORE) = range(8)
MAX_RADIUS = 32


def motion_taps_spec(shift_px, sigma_px, radius):
    """numpy twin of motion_taps: per axis o = floor(s + 0.5), f = s - o, k[d] = exp(-(d - f)^2 / (2 sigma^2)) for d = -R..R,
    normalised in float64 and cast to fp32; sigma = 0 gives the one-hot tap at d = 0.
    Returns (offsets int32 [B,2], taps float32 [B,2,2R+1])."""
    s = np.asarray(shift_px, dtype=np.float64).reshape(-1, 2)
    sig = np.broadcast_to(np.asarray(sigma_px, dtype=np.float64).reshape(-1), (s.shape[0],))
    o = np.floor(s + 0.5)
    f = s - o
    d = np.arange(-radius, radius + 1, dtype=np.float64)
    taps = np.zeros((s.shape[0], 2, 2 * radius + 1), dtype=np.float64)
    for b in range(s.shape[0]):
        for a in range(2):
            if sig[b] > 0:
                k = np.exp(-(d - f[b, a]) ** 2 / (2 * sig[b] ** 2))
                taps[b, a] = k / k.sum()
            else:
                taps[b, a, radius] = 1.0
    return np.clip(o, -2 ** 31, 2 ** 31 - 1).astype(np.int32), taps.astype(np.float32)


def motion_taps(shift_px, sigma_px, radius):
    """Integer offsets and blur taps of a sub-pixel shift (dy, dx) per track with Gaussian motion noise: (offsets int32 [B,2],
    taps fp32 [B,2,2R+1]) as ops.belief_step takes them (motion_taps_spec is the numpy twin).  Computed with torch on the device
    of `shift_px` — shifts that are already on the GPU cost no sync and, with a float sigma_px, no copy.  sigma_px: a float, or one
    value per track (a tensor, best on the same device; a host tensor or a sequence is copied there)."""
    s = torch.as_tensor(shift_px).to(torch.float64).reshape(-1, 2)
    if isinstance(sigma_px, (int, float)):                                      # a fill on the device: no host-to-device copy
        sig = torch.full((s.shape[0], 1, 1), float(sigma_px), dtype=torch.float64, device=s.device)
    else:
        sig = torch.as_tensor(sigma_px, dtype=torch.float64).to(s.device).reshape(-1, 1, 1).expand(s.shape[0], 1, 1)
    o = torch.floor(s + 0.5)
    f = (s - o).unsqueeze(-1)                                                   # [B,2,1]
    d = torch.arange(-radius, radius + 1, dtype=torch.float64, device=s.device)
    on = sig > 0
    safe = torch.where(on, sig, torch.ones_like(sig))
    k = torch.exp(-(d - f) ** 2 / (2 * safe ** 2))
    k = k / k.sum(dim=-1, keepdim=True)
    onehot = (d == 0).to(torch.float64).expand_as(k)
    taps = torch.where(on, k, onehot).to(torch.float32).contiguous()
    return o.clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32).contiguous(), taps


def _predict_spec(prior, oy, ox, ky, kx):
    return _blur_spec(_moved_spec(prior, oy, ox, (len(ky) - 1) // 2), ky, kx)


def _moved_spec(prior, oy, ox, r):
    h, w = prior.shape
    # pad[r + y, r + x] = prior[y - oy, x - ox] for y in [-r, h + r): the prior is zero outside ITS grid, the moved prior is
    # not cropped before the blur (mass is lost only where it ends up off the grid)
    pad = np.zeros((h + 2 * r, w + 2 * r), dtype=np.float64)
    ys, xs = np.arange(-r, h + r, dtype=np.int64) - int(oy), np.arange(-r, w + r, dtype=np.int64) - int(ox)
    vy, vx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
    if vy.any() and vx.any():
        pad[np.ix_(vy, vx)] = prior[np.ix_(ys[vy], xs[vx])]
    return pad


def _maxblur_spec(pad, ky, kx):
    """_blur_spec with every sum replaced by a maximum from a zero start, the same separable order; np.fmax ignores a NaN
    candidate, as fmaxf does on the device."""
    r = (len(ky) - 1) // 2
    h, w = pad.shape[0] - 2 * r, pad.shape[1] - 2 * r
    row = np.zeros((h + 2 * r, w), dtype=np.float64)
    out = np.zeros((h, w), dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for j in range(-r, r + 1):
            row = np.fmax(row, np.float64(kx[j + r]) * pad[:, r - j:r - j + w])
        for i in range(-r, r + 1):
            out = np.fmax(out, np.float64(ky[i + r]) * row[r - i:r - i + h, :])
    return out


def _blur_spec(pad, ky, kx):
    """The separable blur of a moved prior that carries its R halo: [h + 2R, w + 2R] -> [h, w], rows then columns."""
    r = (len(ky) - 1) // 2
    h, w = pad.shape[0] - 2 * r, pad.shape[1] - 2 * r
    row = np.zeros((h + 2 * r, w), dtype=np.float64)
    for j in range(-r, r + 1):
        row += np.float64(kx[j + r]) * pad[:, r - j:r - j + w]
    out = np.zeros((h, w), dtype=np.float64)
    for i in range(-r, r + 1):
        out += np.float64(ky[i + r]) * row[r - i:r - i + h, :]
    return out


def _angle_spec(c, s):
    """The angle rule of the evaluation kernels: NaN unless |cos|, |sin| <= 1 (compared in float32)."""
    if not (np.abs(np.float32(c)) <= 1 and np.abs(np.float32(s)) <= 1):
        return float("nan")
    up = math.degrees(math.acos(float(c)))
    return (-up) % 360 if s < 0 else up


def step_spec(prior, heat, ori, offsets, taps, outlier=0.0, reset=None, return_u=False):
    """The specification of ccvpe_belief_step_f32 in numpy float64, one track at a time.  prior, heat [B,h,w] or [B,1,h,w]
    float32 >= 0; ori [B,2,h,w]; offsets [B,2] (oy, ox); taps [B,2,2R+1] float32 (y then x); outlier in [0,1] (taken as the
    float32 the C ABI receives); reset [B] or None.

    Predict: Q[y,x] = sum_i ky[i+R] sum_j kx[j+R] prior[y - oy - i, x - ox - j], prior = 0 outside the grid.  Measure:
    M = (1 - outlier) heat + outlier / (h w), U = Q M, Z = sum U, S = sum Q.  Reset: 1 when reset[b] != 0 (the predict is
    skipped: S = 0), 2 when not (Z > 0 and finite); then U := M, Z := sum M.  post = U * float32(1 / Z), stored as float32.
    Row: first maximum of U (PRED_Y, PRED_X), post there (PROB), ori there (COS, SIN) and its angle (ANGLE), Z (EVIDENCE),
    RESET, the mean and covariance of U / Z over integer pixel coordinates (MEAN_Y, MEAN_X, VAR_YY, VAR_XX, COV_YX), S
    (SURVIVED).  Returns (post float32 [B,h,w], rows float64 [B,14]) and, with return_u, U float64 [B,h,w]."""
    b = np.asarray(heat).shape[0]
    offsets = np.asarray(offsets).reshape(b, 2)
    return _step_spec(prior, heat, ori, lambda t, p, ky, kx: _predict_spec(p, offsets[t, 0], offsets[t, 1], ky, kx), taps,
                      outlier, reset, return_u)


def viterbi_step_spec(prev, heat, ori, offsets, taps, outlier=0.0, reset=None, return_u=False):
    """The specification of ccvpe_belief_viterbi_step_f32: `step_spec` with the sums of the predict replaced by maxima,

        row[r,x] = max(0, max_j kx[j+R] pad[r, x - j]),   P[y,x] = max(0, max_i ky[i+R] row[y - i, x])

    with pad the previous map moved by (oy, ox), zero outside its grid — P[y,x] is the best ky[i+R] kx[j+R] prev[y - oy - i,
    x - ox - j].  Everything after the predict is step_spec's: M, U = P M, Z = sum U, the reset states, post = U * float32(1 / Z)
    and the 14 columns (SURVIVED = sum P).  The map is normalised by its SUM, not its peak: the peak of post stays at or above
    1 / (h w), so the recursion cannot underflow.  A NaN candidate is ignored and negative inputs count as zero."""
    b = np.asarray(heat).shape[0]
    offsets = np.asarray(offsets).reshape(b, 2)
    return _step_spec(prev, heat, ori,
                      lambda t, p, ky, kx: _maxblur_spec(_moved_spec(p, offsets[t, 0], offsets[t, 1], (len(ky) - 1) // 2), ky, kx),
                      taps, outlier, reset, return_u)


def backtrack_spec(deltas, ori, offsets, taps, rows, reset=None, return_margin=False):
    """The specification of ccvpe_belief_backtrack_f32 in numpy float64: the most likely path through the maps of a
    viterbi_step_spec forward pass.  deltas [T,B,h,w] float32 (the posts), ori [T,B,2,h,w], offsets [T,B,2] and taps
    [T,B,2,2R+1] (the motion INTO each frame), rows [T,B,14] (the forward rows), reset [T,B] or None (frame 0 always counts
    as set).  Returns path float64 [T,B,8], columns PATH_Y ... PATH_SCORE.

    Per track, from t = T-1 down: frame T-1 takes its row's (PRED_Y, PRED_X), LINK 1.  For t >= 1, when reset[t] != 0 or
    rows[t, RESET] != 0 frame t is a segment start and frame t-1 takes its row's arg-max, LINK 1.  Otherwise the candidates
    are the source pixels (sy, sx) = (y_t - oy - i, x_t - ox - j), |i|, |j| <= R, inside the grid, with value
    ky[i+R] * (kx[j+R] * deltas[t-1, sy, sx]); only positive finite values compete; frame t-1 takes the largest, the smallest
    flat index sy w + sx on equal values: LINK 0, SCORE the value.  With no candidate it takes its row's arg-max: LINK 2,
    SCORE 0 (as for LINK 1).  A row's pixel is clamped to the grid.  PROB, COS, SIN are read at the path pixel of frame t from
    deltas[t] and ori[t]; ANGLE follows the evaluation kernels' rule.

    return_margin: also [T,B] float64, at every LINK 0 entry the relative gap (best - second) / best of its decision, NaN
    elsewhere.  `second` is the largest competing value whose factors (ky, kx, delta) are not all equal to the winner's —
    candidates with the winner's own three factors give the winner's bits in any arithmetic and are settled by the index
    rule — or 0 when there is none."""
    deltas = np.asarray(deltas, dtype=np.float32)
    n, b, h, w = deltas.shape[0], deltas.shape[1], deltas.shape[-2], deltas.shape[-1]
    deltas = deltas.reshape(n, b, h, w)
    ori = np.asarray(ori, dtype=np.float32).reshape(n, b, 2, h, w)
    offsets = np.asarray(offsets).reshape(n, b, 2).astype(np.int64)
    taps = np.asarray(taps, dtype=np.float32).reshape(n, b, 2, -1)
    rows = np.asarray(rows, dtype=np.float64).reshape(n, b, 14)
    reset = None if reset is None else np.asarray(reset).reshape(n, b)
    r = (taps.shape[3] - 1) // 2
    path = np.full((n, b, 8), np.nan, dtype=np.float64)
    margin = np.full((n, b), np.nan, dtype=np.float64)

    def row_pixel(t, k):
        py, px = rows[t, k, PRED_Y], rows[t, k, PRED_X]
        return (int(min(py, h - 1)) if py >= 0 else 0), (int(min(px, w - 1)) if px >= 0 else 0)      # +inf clamps, NaN gives 0

    for k in range(b):
        (y, x), link, score = row_pixel(n - 1, k), 1, 0.0
        for t in range(n - 1, -1, -1):
            c, s = ori[t, k, 0, y, x], ori[t, k, 1, y, x]
            path[t, k] = (y, x, deltas[t, k, y, x], c, s, _angle_spec(c, s), link, score)
            if t == 0:
                break
            start = (reset is not None and reset[t, k] != 0) or rows[t, k, RESET] != 0
            best = None
            if not start:
                ky, kx = taps[t, k, 0].astype(np.float64), taps[t, k, 1].astype(np.float64)
                cands = []
                for i in range(-r, r + 1):
                    for j in range(-r, r + 1):
                        sy, sx = y - int(offsets[t, k, 0]) - i, x - int(offsets[t, k, 1]) - j
                        if 0 <= sy < h and 0 <= sx < w:
                            d = np.float64(deltas[t - 1, k, sy, sx])
                            with np.errstate(invalid="ignore", over="ignore"):
                                v = ky[i + r] * (kx[j + r] * d)
                            if v > 0 and np.isfinite(v):
                                cands.append((-v, sy * w + sx, (ky[i + r], kx[j + r], d)))
                if cands:
                    cands.sort(key=lambda e: (e[0], e[1]))
                    best = cands[0]
                    second = max([-e[0] for e in cands[1:] if e[2] != best[2]] + [0.0])
            if best is not None:
                (y, x), link, score = divmod(best[1], w), 0, -best[0]
                margin[t - 1, k] = (score - second) / score
            else:
                (y, x), link, score = row_pixel(t - 1, k), (1 if start else 2), 0.0
    return (path, margin) if return_margin else path


def rigid_motion(shift_px, angle_deg, hw, centre=None):
    """The inverse map of a rigid motion of the grid, [B,6] float64 rows (a00, a01, a02, a10, a11, a12): output pixel (y, x)
    takes its value from the previous belief at

        sy = (a00 y + a01 x) + a02,   sx = (a10 y + a11 x) + a12.

    The forward motion is q = c + Rot(angle)(p - c) + shift with shift = (dy, dx) and c = `centre` (y, x), by default the grid
    centre ((h-1)/2, (w-1)/2).  A positive angle turns counter-clockwise as seen in the image (x right, y down) — the sense of
    Pillow's `rotate` and of the KITTI loader's `ori`: a point 10 px right of the centre lands 10 px above it at 90 degrees.
    The angle is reduced to a quarter turn plus a remainder in [-45, 45] before sin / cos, so multiples of 90 degrees give
    exact 0 / +-1 entries.  shift_px [B,2] (or one pair), angle_deg [B] (or one value), centre [B,2] or one pair."""
    s = np.asarray(shift_px, dtype=np.float64).reshape(-1, 2)
    ang = np.asarray(angle_deg, dtype=np.float64).reshape(-1)
    n = max(s.shape[0], ang.shape[0])
    s, ang = np.broadcast_to(s, (n, 2)), np.broadcast_to(ang, (n,))
    c = np.asarray(((hw[0] - 1) / 2.0, (hw[1] - 1) / 2.0) if centre is None else centre, dtype=np.float64).reshape(-1, 2)
    c = np.broadcast_to(c, (n, 2))
    out = np.zeros((n, 6), dtype=np.float64)
    for t in range(n):
        a = math.fmod(float(ang[t]), 360.0) if math.isfinite(float(ang[t])) else float("nan")
        if a != a:
            out[t] = np.nan
            continue
        k = int(math.floor(a / 90.0 + 0.5))
        rem = math.radians(a - 90.0 * k)
        cr, sr = math.cos(rem), math.sin(rem)                                  # rem = 0 gives exactly (1, 0)
        co, si = ((cr, sr), (-sr, cr), (-cr, -sr), (sr, -cr))[k % 4]            # cos, sin of 90 k + rem
        # forward in (y, x): q - c - shift = [[co, -si], [si, co]] (p - c); the inverse is the transpose
        ty, tx = c[t, 0] + s[t, 0], c[t, 1] + s[t, 1]
        out[t] = (co, si, c[t, 0] - (co * ty + si * tx), -si, co, c[t, 1] - (-si * ty + co * tx))
    return out


def _warp_spec(prior, m, r):
    """W on the grid extended by the blur's halo, [h + 2R, w + 2R]: the bilinear sample of the prior (0 outside its grid) at
    (sy, sx) of every pixel y in [-R, h + R), x in [-R, w + R); weights cast to fp32, combines in float64."""
    h, w = prior.shape
    ys = np.arange(-r, h + r, dtype=np.float64).reshape(-1, 1)
    xs = np.arange(-r, w + r, dtype=np.float64).reshape(1, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        sy = (m[0] * ys + m[1] * xs) + m[2]
        sx = (m[3] * ys + m[4] * xs) + m[5]
        ok = np.isfinite(sy) & np.isfinite(sx) & (sy > -1) & (sy < h) & (sx > -1) & (sx < w)
    sy, sx = np.where(ok, sy, 0.0), np.where(ok, sx, 0.0)
    fy0, fx0 = np.floor(sy), np.floor(sx)
    fy, fx = sy - fy0, sx - fx0
    wy1, wy0 = fy.astype(np.float32).astype(np.float64), (1 - fy).astype(np.float32).astype(np.float64)
    wx1, wx0 = fx.astype(np.float32).astype(np.float64), (1 - fx).astype(np.float32).astype(np.float64)
    pad = np.zeros((h + 2, w + 2), dtype=np.float64)                            # index + 1: taps at -1 and at h, w are 0
    pad[1:-1, 1:-1] = prior
    iy, ix = fy0.astype(np.int64) + 1, fx0.astype(np.int64) + 1
    top = wx0 * pad[iy, ix] + wx1 * pad[iy, ix + 1]
    bot = wx0 * pad[iy + 1, ix] + wx1 * pad[iy + 1, ix + 1]
    return np.where(ok, wy0 * top + wy1 * bot, 0.0)


def step_rigid_spec(prior, heat, ori, motion, taps, outlier=0.0, reset=None, return_u=False):
    """The specification of ccvpe_belief_step_rigid_f32: `step_spec` with the predict replaced by a warp and the same blur.
    motion [B,6] float64, the inverse map as `rigid_motion` returns it (any values, NaN and inf included):

        W[y,x] = bilinear sample of the prior at (sy, sx) = ((a00 y + a01 x) + a02, (a10 y + a11 x) + a12), prior = 0 outside
                 the grid: y0 = floor(sy), fy = sy - y0, wy1 = float32(fy), wy0 = float32(1 - fy), wx1, wx0 likewise,
                 top = wx0 v00 + wx1 v01, bot = wx0 v10 + wx1 v11, W = wy0 top + wy1 bot; 0 where (sy, sx) is not finite or
                 not in (-1, h) x (-1, w)
        Q      = the separable blur of W with `taps` (W is taken on the grid plus its R halo, not cropped before the blur)

    and everything after that — measure, reset rules, the 14 columns, SURVIVED = sum Q — as step_spec.  Sub-pixel shifts live
    in the warp, so callers pass centred taps: motion_taps(zeros, sigma, R).  For angle 0 and a FRACTIONAL shift this is not
    the translate path's result: here the prior is resampled bilinearly, there the Gaussian taps themselves are shifted (for
    angle 0 and integer shifts the two are equal, value for value)."""
    b = np.asarray(heat).shape[0]
    motion = np.asarray(motion, dtype=np.float64).reshape(b, 6)
    return _step_spec(prior, heat, ori, lambda t, p, ky, kx: _blur_spec(_warp_spec(p, motion[t], (len(ky) - 1) // 2), ky, kx),
                      taps, outlier, reset, return_u)


def _step_spec(prior, heat, ori, predict, taps, outlier, reset, return_u):
    heat = np.asarray(heat, dtype=np.float32)
    b, h, w = heat.shape[0], heat.shape[-2], heat.shape[-1]
    heat = heat.reshape(b, h, w).astype(np.float64)
    prior = np.asarray(prior, dtype=np.float32).reshape(b, h, w).astype(np.float64)
    ori = np.asarray(ori, dtype=np.float32).reshape(b, 2, h, w)
    taps = np.asarray(taps, dtype=np.float32).reshape(b, 2, -1)
    alpha = np.float64(np.float32(outlier))
    post = np.zeros((b, h, w), dtype=np.float32)
    us = np.zeros((b, h, w), dtype=np.float64)
    rows = np.full((b, 14), np.nan, dtype=np.float64)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    for t in range(b):
        m = (1 - alpha) * heat[t] + alpha / (h * w)
        state, survived = 0, 0.0
        if reset is not None and int(np.asarray(reset).reshape(-1)[t]) != 0:
            state = 1
        else:
            q = predict(t, prior[t], taps[t, 0], taps[t, 1])
            u = q * m
            z, survived = float(u.sum()), float(q.sum())
            if not (z > 0 and np.isfinite(z)):
                state = 2
        if state:
            u = m
            z = float(u.sum())
        post[t], rows[t] = _normalise_spec(u, z, ori[t], state, survived, yy, xx)
        us[t] = u
    return (post, rows, us) if return_u else (post, rows)


def _normalise_spec(u, z, ori, state, survived, yy, xx):
    """The end of a step, forward or backward: (u * float32(1 / z) stored as float32, the row read off u)."""
    w = u.shape[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.float64(np.float32(np.float64(1.0) / np.float64(z)))
        post = (u * inv).astype(np.float32)
        p = u / z
        my, mx = float((p * yy).sum()), float((p * xx).sum())
        var_yy, var_xx = float((p * (yy - my) ** 2).sum()), float((p * (xx - mx) ** 2).sum())
        cov = float((p * (yy - my) * (xx - mx)).sum())
    k = int(np.argmax(u.reshape(-1)))
    py, px = divmod(k, w)
    c, s = ori[0, py, px], ori[1, py, px]
    return post, (py, px, post[py, px], c, s, _angle_spec(c, s), z, state, my, mx, var_yy, var_xx, cov, survived)


def invert_motion(motion):
    """The inverse of rigid-motion rows, [B,6] -> [B,6] float64: if a row maps (y, x) to (sy, sx), the result maps (sy, sx)
    back to (y, x).  A general 2 x 2 inverse with every product, sum and quotient rounded on its own (the device does the
    same operations in the same order): exact for the 0 / +-1 rotations `rigid_motion` produces with whole or half-pixel
    translations.  A singular or non-finite row gives a row of NaN, which samples nothing."""
    m = np.array(motion, dtype=np.float64).reshape(-1, 6)
    a00, a01, a02, a10, a11, a12 = (m[:, k] for k in range(6))
    with np.errstate(all="ignore"):
        det = a00 * a11 - a01 * a10
        b00, b01, b10, b11 = a11 / det, -a01 / det, -a10 / det, a00 / det
        out = np.stack([b00, b01, -(b00 * a02 + b01 * a12), b10, b11, -(b10 * a02 + b11 * a12)], axis=1)
    ok = np.isfinite(m).all(axis=1) & np.isfinite(det) & (det != 0)
    out[~ok] = np.nan
    return out


def smooth_step_spec(beta, heat, alpha, ori, offsets, taps, outlier=0.0, cut=None, return_v=False):
    """The specification of ccvpe_belief_smooth_step_f32 in numpy float64: one backward step of the forward-backward smoother
    for the pair of frames (s, t = s + 1), one track at a time.  beta [B,h,w] or [B,1,h,w] float32 > 0: the backward message
    of frame t at any scale; heat: the heat-map of frame t; alpha: the filter's posterior of frame s; ori [B,2,h,w] of frame
    s; offsets [B,2] and taps [B,2,2R+1]: the FORWARD step's own inputs of frame t; cut [B] or None.

    Measure: M = (1 - outlier) heat + outlier / (h w), G = M beta.  Back-predict, the exact adjoint of the forward predict:
    B'[y,x] = sum_i ky[i+R] sum_j kx[j+R] G[y + oy + i, x + ox + j], G = 0 outside the grid (the forward predict with the
    offsets negated and both tap vectors reversed).  V = alpha B', Z = sum V, S = sum B'.  State: 1 when cut[b] != 0 (frame s
    is the last of its segment; the back-predict is skipped: S = 0), 2 when not (Z > 0 and finite and S > 0 and finite); then
    V := alpha, Z := sum alpha and the message is float32(1 / (h w)) everywhere.  smooth = V * float32(1 / Z) and
    beta_out = B' * float32(1 / S), stored as float32.  Row: the forward step's columns read off V — RESET holds the state,
    SURVIVED holds S.  Returns (smooth float32 [B,h,w], beta_out float32 [B,h,w], rows float64 [B,14]) and, with return_v, V
    float64 [B,h,w]."""
    b = np.asarray(heat).shape[0]
    offsets = np.asarray(offsets).reshape(b, 2)
    return _smooth_step_spec(beta, heat, alpha, ori, lambda t, g, ky, kx: _predict_spec(g, -int(offsets[t, 0]), -int(offsets[t, 1]),
                                                                                      ky[::-1], kx[::-1]),
                             taps, outlier, cut, return_v)


def smooth_step_rigid_spec(beta, heat, alpha, ori, motion, taps, outlier=0.0, cut=None, return_v=False):
    """The specification of ccvpe_belief_smooth_step_rigid_f32: `smooth_step_spec` with the back-predict

        B' = blur(warp(G; invert_motion(motion)), taps reversed)

    where motion [B,6] is the FORWARD rigid step's own input of frame t and warp is `step_rigid_spec`'s bilinear rule.  This
    is NOT the exact adjoint of the rigid predict — the adjoint of a bilinear gather is a scatter — but the same continuous
    model discretised along the reverse motion: exact in the continuum, because the blur is isotropic and the motion has unit
    Jacobian.  For angle 0 or quarter turns with whole-pixel shifts (and centred taps) it equals smooth_step_spec value for
    value."""
    b = np.asarray(heat).shape[0]
    back = invert_motion(np.asarray(motion, dtype=np.float64).reshape(b, 6))
    return _smooth_step_spec(beta, heat, alpha, ori,
                             lambda t, g, ky, kx: _blur_spec(_warp_spec(g, back[t], (len(ky) - 1) // 2), ky[::-1], kx[::-1]),
                             taps, outlier, cut, return_v)


def _smooth_step_spec(beta, heat, alpha, ori, backpredict, taps, outlier, cut, return_v):
    heat = np.asarray(heat, dtype=np.float32)
    b, h, w = heat.shape[0], heat.shape[-2], heat.shape[-1]
    heat = heat.reshape(b, h, w).astype(np.float64)
    beta = np.asarray(beta, dtype=np.float32).reshape(b, h, w).astype(np.float64)
    alpha = np.asarray(alpha, dtype=np.float32).reshape(b, h, w).astype(np.float64)
    ori = np.asarray(ori, dtype=np.float32).reshape(b, 2, h, w)
    taps = np.asarray(taps, dtype=np.float32).reshape(b, 2, -1)
    a = np.float64(np.float32(outlier))
    smooth, message = np.zeros((b, h, w), dtype=np.float32), np.zeros((b, h, w), dtype=np.float32)
    vs = np.zeros((b, h, w), dtype=np.float64)
    rows = np.full((b, 14), np.nan, dtype=np.float64)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    for t in range(b):
        state, s = 0, 0.0
        if cut is not None and int(np.asarray(cut).reshape(-1)[t]) != 0:
            state = 1
        else:
            m = (1 - a) * heat[t] + a / (h * w)
            bp = backpredict(t, m * beta[t], taps[t, 0], taps[t, 1])
            v = alpha[t] * bp
            z, s = float(v.sum()), float(bp.sum())
            if not (z > 0 and np.isfinite(z) and s > 0 and np.isfinite(s)):
                state = 2
        if state:
            v = alpha[t]
            z = float(v.sum())
            message[t] = np.float32(np.float64(1.0) / np.float64(h * w))
        else:
            message[t] = (bp * np.float64(np.float32(np.float64(1.0) / np.float64(s)))).astype(np.float32)
        smooth[t], rows[t] = _normalise_spec(v, z, ori[t], state, s, yy, xx)
        vs[t] = v
    return (smooth, message, rows, vs) if return_v else (smooth, message, rows)


class HistogramFilter(object):
    """The beliefs of `n_tracks` independent tracks on an h x w grid, stepped on the device.

    Owns two belief buffers (ping-pong: the step reads one and writes the other), the step's scratch and a rows tensor.
    sigma_px: the motion noise in pixels (a float; `step` may override it per call, per track); radius: of the blur taps,
    None = ceil(3 sigma) + 1, at most 32 (ValueError above); outlier: the weight of the uniform floor mixed into every
    heat-map, in [0, 1] — with 0 a heat-map that is exactly zero where the prediction has its mass resets the track.
    The first step after construction or after `reset` starts from the measurement alone."""

    def __init__(self, n_tracks, hw=(512, 512), sigma_px=1.0, radius=None, outlier=0.0, device="cuda"):
        from . import ops
        self.hw, self.sigma_px, self.radius, outlier = _drive_settings(hw, sigma_px, radius, outlier)
        self.n_tracks = int(n_tracks)
        if self.n_tracks <= 0:
            raise ValueError("n_tracks must be positive")
        self.outlier, self.device = float(outlier), torch.device(device)
        h, w = self.hw
        self._buf = [torch.zeros((self.n_tracks, 1, h, w), device=self.device, dtype=torch.float32) for _ in range(2)]
        self._cur = 0
        self._scratch = torch.empty((self.n_tracks * ops.belief_partials(h, w),), device=self.device, dtype=torch.float64)
        self.rows = torch.zeros((self.n_tracks, 14), device=self.device, dtype=torch.float64)
        self._reset = torch.ones((self.n_tracks,), device=self.device, dtype=torch.int32)

    @property
    def belief(self):
        """The current posterior [B,1,h,w] (the shape ops.eval_metrics takes as a heat-map).  The tensor is reused two steps
        later: clone it to keep it."""
        return self._buf[self._cur]

    def reset(self, tracks=None):
        """The next step of `tracks` (indices or a mask; None = all) starts from the measurement."""
        if tracks is None:
            self._reset.fill_(1)
        else:
            self._reset[tracks] = 1

    def step(self, heatmap, ori, shift_px=None, sigma_px=None, rows_out=None, motion=None):
        """One filter step: heatmap [B,1,h,w], ori [B,2,h,w] from the forward, and exactly one of (ValueError otherwise)
        shift_px [B,2] = (dy, dx), the motion of the vehicle in the grid since the previous step (odometry minus the motion of
        the aerial patch), or motion [B,6] float64, the inverse map of a rigid motion of the grid (`rigid_motion`,
        `kitti_motions`): the belief is then resampled through it and blurred with centred taps (ops.belief_step_rigid).
        Both are tensors on any device or arrays.  Returns the rows [B,14] (columns PRED_Y ... SURVIVED): `rows_out` when given
        (a slice of a caller's table), else self.rows, which the next step overwrites."""
        from . import ops
        if tuple(heatmap.shape) != (self.n_tracks, 1) + self.hw:
            raise ValueError("step: heatmap must be %s, got %s" % ((self.n_tracks, 1) + self.hw, tuple(heatmap.shape)))
        move, taps = _move_taps("step", shift_px, motion, (self.n_tracks,), self.device,
                                self.sigma_px if sigma_px is None else sigma_px, self.radius)
        rows = self.rows if rows_out is None else rows_out
        step = ops.belief_step if motion is None else ops.belief_step_rigid
        step(self._buf[self._cur], heatmap, ori, move, taps, outlier=self.outlier, reset=self._reset,
             post=self._buf[1 - self._cur], scratch=self._scratch, out=rows)
        self._reset.zero_()
        self._cur = 1 - self._cur
        return rows


@functools.lru_cache(maxsize=8)
def _zero_shift(count, device):
    return torch.zeros((count, 2), device=device, dtype=torch.float64)


def _move_taps(who, shift_px, motion, shape, device, sigma_px, radius):
    """(move, taps) as the ops step functions take them, from exactly one of shift_px [*shape,2] and motion [*shape,6] (tensors
    on any device or arrays; ValueError otherwise): the offsets int32 [n,2] and their taps, or the motion rows float64 [n,6] on
    `device` with centred taps, n = prod(shape).  `who` names the caller in the messages."""
    if (shift_px is None) == (motion is None):
        raise ValueError("%s: pass exactly one of shift_px and motion" % who)
    count = int(np.prod(shape))
    if motion is None:
        name, cols, move = "shift_px", 2, torch.as_tensor(shift_px).to(device)
    else:
        move = motion if torch.is_tensor(motion) else torch.from_numpy(np.array(motion, dtype=np.float64))      # a copy
        name, cols, move = "motion", 6, move.to(device=device, dtype=torch.float64)
    if move.numel() != cols * count:
        raise ValueError("%s: %s must be [%s,%d]" % (who, name, ",".join(str(k) for k in shape), cols))
    if motion is None:
        return motion_taps(move.reshape(count, 2), sigma_px, radius)
    return move.reshape(count, 6).contiguous(), motion_taps(_zero_shift(count, torch.device(device)), sigma_px, radius)[1]


def _drive_settings(hw, sigma_px, radius, outlier):
    """The settings SequenceSmoother and MostLikelyPath share, validated: (hw, sigma_px, radius, outlier)."""
    hw = (int(hw[0]), int(hw[1]))
    if hw[0] <= 0 or hw[1] <= 0:
        raise ValueError("hw must be positive")
    sigma_px = float(sigma_px)
    if not sigma_px >= 0:
        raise ValueError("sigma_px must be >= 0")
    radius = int(math.ceil(3 * sigma_px)) + 1 if radius is None else int(radius)
    if not 0 <= radius <= MAX_RADIUS:
        raise ValueError("radius %d outside [0, %d]: use a smaller sigma_px or pass radius" % (radius, MAX_RADIUS))
    if not 0.0 <= float(outlier) <= 1.0:
        raise ValueError("outlier must be in [0, 1]")
    return hw, sigma_px, radius, float(outlier)


class SequenceSmoother(object):
    """The forward-backward smoother of ONE track over a recorded drive: the belief of frame t given the whole drive.

    `run` filters the T frames forward (ops.belief_step / ops.belief_step_rigid, as HistogramFilter steps) and keeps every
    posterior, then walks back with ops.belief_smooth_step / ops.belief_smooth_step_rigid: 2 launches per frame each way, no
    read-back.  Memory: h w 4 bytes per frame for the posteriors (1 MB at 512 x 512), beside the caller's heat and ori; as
    much again with keep_beliefs.  sigma_px, radius, outlier: as HistogramFilter (same ValueErrors).
    Out of scope: several tracks per smoother, fixed-lag (online) smoothing, bf16 maps, a change of scale between patch
    frames.  The most likely path is MostLikelyPath's."""

    def __init__(self, hw=(512, 512), sigma_px=1.0, radius=None, outlier=0.0, device="cuda"):
        self.hw, self.sigma_px, self.radius, self.outlier = _drive_settings(hw, sigma_px, radius, outlier)
        self.device = torch.device(device)

    def run(self, heat, ori, shift_px=None, motion=None, starts=None, keep_beliefs=False):
        """heat [T,1,h,w], ori [T,2,h,w] on the device, in drive order; exactly one of shift_px [T,2] = (dy, dx) and motion
        [T,6] float64 (`rigid_motion` rows), the motion INTO each frame as HistogramFilter.step takes it (tensors on any device
        or arrays; row 0 is not used); starts [T] marks frames where the filter restarts (frame 0 always does).
        Returns {"filtered": rows [T,14] of the forward pass, "smoothed": rows [T,14] of the smoothed beliefs (RESET: 0 chained,
        1 last frame of its segment, 2 the message died out; SURVIVED: the back-predicted mass), "beliefs": the smoothed
        beliefs [T,1,h,w] with keep_beliefs, else None}, all on the device."""
        if heat.dim() != 4 or tuple(heat.shape[1:]) != (1,) + self.hw or heat.shape[0] < 1:
            raise ValueError("run: heat must be [T,1,%d,%d], got %s" % (self.hw + (tuple(heat.shape),)))
        n = int(heat.shape[0])
        if tuple(ori.shape) != (n, 2) + self.hw:
            raise ValueError("run: ori must be [%d,2,%d,%d], got %s" % ((n,) + self.hw + (tuple(ori.shape),)))
        dev = self.device
        move, taps = _move_taps("run", shift_px, motion, (n,), dev, self.sigma_px, self.radius)
        reset = torch.zeros((n,), device=dev, dtype=torch.int32)
        if starts is not None:
            st = torch.as_tensor(np.asarray(starts).reshape(-1).astype(np.int32))
            if st.numel() != n:
                raise ValueError("run: starts must hold one entry per frame (%d)" % n)
            reset.copy_(st)
        reset[0] = 1
        alphas = self.forward(heat, ori, move, taps, reset)
        return self.backward(heat, ori, move, taps, reset, alphas[0], alphas[1], keep_beliefs)

    def _steps(self, rigid):
        from . import ops
        return (ops.belief_step_rigid, ops.belief_smooth_step_rigid) if rigid else (ops.belief_step, ops.belief_smooth_step)

    def forward(self, heat, ori, move, taps, reset):
        """The forward pass: every posterior written straight into a [T,1,h,w] table.  move: offsets int32 [T,2] or motion
        float64 [T,6]; reset int32 [T].  Returns (posteriors, rows [T,14])."""
        from . import ops
        step = self._steps(move.dtype == torch.float64)[0]
        n, (h, w) = int(heat.shape[0]), self.hw
        table = torch.empty((n, 1, h, w), device=self.device, dtype=torch.float32)
        rows = torch.empty((n, 14), device=self.device, dtype=torch.float64)
        scratch = torch.empty((ops.belief_partials(h, w),), device=self.device, dtype=torch.float64)
        first = table[n - 1:n] if n > 1 else torch.zeros((1, 1, h, w), device=self.device)      # frame 0 resets: not read
        for t in range(n):
            step(table[t - 1:t] if t else first, heat[t:t + 1], ori[t:t + 1], move[t:t + 1], taps[t:t + 1], outlier=self.outlier,
                 reset=reset[t:t + 1], post=table[t:t + 1], scratch=scratch, out=rows[t:t + 1])
        return table, rows

    def backward(self, heat, ori, move, taps, reset, alphas, filtered, keep_beliefs=False):
        """The backward pass over the posteriors `alphas` [T,1,h,w] and the forward rows `filtered` [T,14] of a forward pass
        with the same inputs.  The cut flags are made on the device: frame t is the last of its segment when frame t + 1 is
        a start, when the forward pass reset there (RESET != 0), or when there is no frame t + 1."""
        from . import ops
        back = self._steps(move.dtype == torch.float64)[1]
        n, (h, w) = int(heat.shape[0]), self.hw
        cut = torch.ones((n,), device=self.device, dtype=torch.int32)
        if n > 1:
            cut[:-1] = ((reset[1:] != 0) | (filtered[1:, RESET] != 0)).to(torch.int32)
        rows = torch.empty((n, 14), device=self.device, dtype=torch.float64)
        scratch = torch.empty((ops.belief_partials(h, w),), device=self.device, dtype=torch.float64)
        beta = [torch.empty((1, 1, h, w), device=self.device, dtype=torch.float32) for _ in range(2)]
        beliefs = torch.empty((n, 1, h, w), device=self.device, dtype=torch.float32) if keep_beliefs else None
        one = None if keep_beliefs else torch.empty((1, 1, h, w), device=self.device, dtype=torch.float32)
        for t in range(n - 1, -1, -1):
            nxt = min(t + 1, n - 1)                                            # the last frame is cut: frame `nxt` is not read
            back(beta[(t + 1) & 1], heat[nxt:nxt + 1], alphas[t:t + 1], ori[t:t + 1], move[nxt:nxt + 1], taps[nxt:nxt + 1],
                 outlier=self.outlier, cut=cut[t:t + 1], beta_out=beta[t & 1], smooth=beliefs[t:t + 1] if keep_beliefs else one,
                 scratch=scratch, out=rows[t:t + 1])
        return {"filtered": filtered, "smoothed": rows, "beliefs": beliefs}


class MostLikelyPath(object):
    """The jointly most likely sequence of grid cells (max-product, Viterbi) of B tracks over a recorded drive.

    `run` makes the forward pass with ops.belief_viterbi_step — two launches per frame for all B tracks, every map kept in a
    [T,B,1,h,w] table — and then ONE ops.belief_backtrack launch; no read-back.  Memory: h w 4 bytes per frame and track
    (1 MB at 512 x 512), beside the caller's heat and ori.  There are no back-pointer maps: the backtrack recomputes each link
    at the one pixel the path visits.  sigma_px, radius, outlier: as HistogramFilter (same ValueErrors).
    Out of scope: the rigid (KITTI) form — the warp is a bilinear mix, not a maximum, so its back-pointer needs a definition of
    its own — stored back-pointer maps, log-domain maps, bf16 maps, fixed-lag decoding."""

    def __init__(self, hw=(512, 512), sigma_px=1.0, radius=None, outlier=0.0, device="cuda"):
        self.hw, self.sigma_px, self.radius, self.outlier = _drive_settings(hw, sigma_px, radius, outlier)
        self.device = torch.device(device)

    def run(self, heat, ori, shift_px, starts=None):
        """heat [T,B,h,w], ori [T,B,2,h,w] (or [T,2,h,w] for B = 1) on the device, in drive order; shift_px [T,B,2] (or [T,2]
        for B = 1) = (dy, dx), the motion INTO each frame as HistogramFilter.step takes it (a tensor on any device or an array;
        row 0 is not used); starts [T] (all tracks) or [T,B] marks frames where a track restarts (frame 0 always does).
        Returns {"rows": [T,B,14] of the forward pass (tracking.PRED_Y ... SURVIVED), "path": [T,B,8] (PATH_Y ... PATH_SCORE;
        LINK: 0 chained, 1 the last frame of its segment, 2 no source pixel had mass), "deltas": the forward maps
        [T,B,1,h,w]}, all on the device."""
        from . import ops
        if heat.dim() != 4 or tuple(heat.shape[2:]) != self.hw or heat.shape[0] < 1 or heat.shape[1] < 1:
            raise ValueError("run: heat must be [T,B,%d,%d], got %s" % (self.hw + (tuple(heat.shape),)))
        n, b = int(heat.shape[0]), int(heat.shape[1])
        h, w = self.hw
        if b == 1 and tuple(ori.shape) == (n, 2, h, w):
            ori = ori.reshape(n, 1, 2, h, w)
        if tuple(ori.shape) != (n, b, 2, h, w):
            raise ValueError("run: ori must be [%d,%d,2,%d,%d], got %s" % (n, b, h, w, tuple(ori.shape)))
        dev = self.device
        offsets, taps = _move_taps("run", shift_px, None, (n, b), dev, self.sigma_px, self.radius)
        offsets, taps = offsets.reshape(n, b, 2), taps.reshape(n, b, 2, 2 * self.radius + 1)
        reset = torch.zeros((n, b), device=dev, dtype=torch.int32)
        if starts is not None:
            st = np.asarray(starts)
            if st.size not in (n, n * b):
                raise ValueError("run: starts must be [%d] or [%d,%d]" % (n, n, b))
            st = np.broadcast_to(st.reshape(n, -1), (n, b)).astype(np.int32)
            reset.copy_(torch.as_tensor(np.ascontiguousarray(st)))
        reset[0] = 1
        table = torch.empty((n, b, 1, h, w), device=dev, dtype=torch.float32)
        rows = torch.empty((n, b, 14), device=dev, dtype=torch.float64)
        scratch = torch.empty((b * ops.belief_partials(h, w),), device=dev, dtype=torch.float64)
        first = table[n - 1] if n > 1 else torch.zeros((b, 1, h, w), device=dev)                  # frame 0 resets: not read
        for t in range(n):
            ops.belief_viterbi_step(table[t - 1] if t else first, heat[t].reshape(b, 1, h, w), ori[t], offsets[t], taps[t],
                                    outlier=self.outlier, reset=reset[t], post=table[t], scratch=scratch, out=rows[t])
        path = ops.belief_backtrack(table, ori, offsets, taps, rows, reset)
        return {"rows": rows, "path": path, "deltas": table}


def oxford_shifts(pairs, indices=None):
    """Per-frame grid shifts of an Oxford RobotCar val / test split: (shift_px float64 [n,2] as (dy, dx), starts bool [n]).

        shift_t = (512 / 800) * ((pos_t - pos_{t-1}) - (origin_t - origin_{t-1}))

    pos_t is the vehicle's map position (`pairs._position`) and origin_t the origin of the grid patch that holds it
    (`pairs._grid`): the second term is the 256-pixel jump of the frame when the vehicle crosses into the next patch.
    `starts` marks the first frame of each traversal (from `pairs.list_lengths`), the first index, and any index that does not
    follow its predecessor; a start has shift 0 and is where a filter must be reset.

    The shifts are exact sub-pixel values; the loader's ground-truth PIXELS are not: it rounds the patch coordinate and then
    truncates 256 - 0.64 p towards zero, so the difference of two consecutive ground-truth pixels departs from shift_t by up to
    2.64 px when the two frames lie on opposite sides of the patch centre (under 1.64 px on the same side).

    NOTE: this uses the GROUND-TRUTH pose difference as the odometry — the data set has no independent odometry in its lists.
    It shows what the filter does with good odometry; it is not a fair comparison against single-frame results."""
    if getattr(pairs, "split", None) not in ("val", "test"):
        raise ValueError("oxford_shifts needs an OxfordPairs val or test split (training patches have random offsets)")
    idx = np.arange(len(pairs)) if indices is None else np.asarray(indices, dtype=np.int64)
    first = set(int(v) for v in np.cumsum([0] + list(pairs.list_lengths))[:-1])
    shift = np.zeros((len(idx), 2), dtype=np.float64)
    starts = np.zeros((len(idx),), dtype=bool)
    prev = None
    for n, i in enumerate(idx):
        col, row = pairs._position(int(i))
        cur = (row, col, 400.0 * pairs._grid(row)[0], 400.0 * pairs._grid(col)[0])
        if n == 0 or int(i) in first or int(i) != int(idx[n - 1]) + 1:
            starts[n] = True
        else:
            shift[n, 0] = 512.0 / 800.0 * ((cur[0] - prev[0]) - (cur[2] - prev[2]))
            shift[n, 1] = 512.0 / 800.0 * ((cur[1] - prev[1]) - (cur[3] - prev[3]))
        prev = cur
    return shift, starts


EARTH_RADIUS_M = 6378137.0                  # WGS-84 equatorial radius: the local tangent plane of kitti_motions


def _rot2(rad):
    c, s = math.cos(rad), math.sin(rad)
    return np.array([[c, -s], [s, c]], dtype=np.float64)


def _kitti_frame(pairs, i):
    """What places the patch of test sample i in the world: (name, lat, lon, heading [rad], ori [deg], shift, cam) with
    shift and cam in map pixels, x east / y UP after the heading turn (the loader's image offsets with y flipped)."""
    from . import datasets
    name = pairs.lines[i].split(" ")[0]
    with open(pairs.paths(name)[1]) as f:
        rec = f.readline().split(" ")
    sx, sy, ori = pairs.perturbation(i)
    mpp = pairs.meter_per_pixel
    shift = np.array([sx * pairs.shift_px_lon, sy * pairs.shift_px_lat])
    cam = np.array([datasets.KITTI_CAMERA_SHIFT[0] / mpp, -datasets.KITTI_CAMERA_SHIFT[1] / mpp])
    return name, float(rec[0]), float(rec[1]), float(rec[5]), float(ori), shift, cam


def _kitti_pair_motion(pairs, prev, cur, with_camera):
    """The motion from the patch of frame `prev` to the patch of frame `cur` (outputs of _kitti_frame) as a rigid_motion row.
    Patch frame t relates to the world by the loader's chain (KITTIPairs.sample: rotate(-heading), the camera offset, the
    shift, rotate(ori), centre crop), in map pixels with y up and p measured from the patch centre:

        F_t(p) = G_t + Rot(heading_t) [ Rot(-ori_t) p + shift_t + cam ]

    G_t is the map centre = the GPS antenna, from latitude and longitude on a local tangent plane.  with_camera adds the
    camera's own displacement dC = (G_t - G_{t-1}) + (Rot(heading_t) - Rot(heading_{t-1})) cam to the world point."""
    _, lat0, lon0, h0, o0, s0, cam = prev
    _, lat1, lon1, h1, o1, s1, _ = cur
    mpp = pairs.meter_per_pixel
    mid = math.radians(0.5 * (lat0 + lat1))
    dg = np.array([EARTH_RADIUS_M * math.cos(mid) * math.radians(lon1 - lon0), EARTH_RADIUS_M * math.radians(lat1 - lat0)]) / mpp
    world = -dg                                                                  # G_{t-1} - G_t
    if with_camera:
        world = world + (dg + (_rot2(h1) - _rot2(h0)) @ cam)
    r_out = _rot2(math.radians(o1))
    # the image of the patch centre, and the total turn; in the image (y down) the shift is (dy, dx) = (-T_y, T_x)
    t = r_out @ (_rot2(-h1) @ (world + _rot2(h0) @ (s0 + cam)) - s1 - cam)
    angle = (o1 - o0) + math.degrees(h0 - h1)
    from . import datasets
    return rigid_motion([-t[1], t[0]], angle, (datasets.KITTI_CROP, datasets.KITTI_CROP))[0]


def _need_kitti_test(pairs, who):
    if not getattr(pairs, "test", False) or not hasattr(pairs, "perturbation"):
        raise ValueError("%s needs a KITTIPairs(test=True) split (training perturbations are random draws)" % who)


def kitti_frame_motion(pairs, i_prev, i_cur):
    """The change of the PATCH FRAME alone between two samples of a KITTIPairs(test=True) split, as a rigid_motion row
    [6]: a world-fixed point seen at p in the patch of sample i_prev is seen at q in the patch of sample i_cur, and the row
    maps q back to p (F_cur^-1 o F_prev in the notation of kitti_motions)."""
    _need_kitti_test(pairs, "kitti_frame_motion")
    return _kitti_pair_motion(pairs, _kitti_frame(pairs, int(i_prev)), _kitti_frame(pairs, int(i_cur)), False)


def kitti_motions(pairs, indices=None):
    """Per-frame rigid motions of a KITTI test split: (motion float64 [n,6] as `rigid_motion` rows, starts bool [n]).

    Every KITTI aerial patch is re-centred on the vehicle, turned so that the heading points east, shifted and rotated by the
    sample's theta, so the belief of frame t-1 reaches the grid of frame t through a rotation plus a translation:

        motion_t = F_t^-1 o (F_{t-1} + dC),      F_t(p) = G_t + mpp Rot(heading_t) [ Rot(-ori_t) p + shift_t + cam ]

    (image y flipped; see _kitti_pair_motion) where dC is the camera's world displacement: the OXTS latitude and longitude
    (fields 0 and 1) on a local tangent plane with R = 6 378 137 m, converted to map pixels with the loader's metres per pixel,
    plus the antenna-to-camera lever arm under the heading change.  `starts` marks the first index, a change of drive
    (name[:38]) and a frame number that is not greater than its predecessor's; a start carries the identity motion and is
    where a filter must be reset.  A training split raises ValueError: its perturbations are random draws.

    NOTE: this uses the GROUND-TRUTH pose difference as the odometry — the OXTS record is what the data set's ground truth is
    made of.  It shows what the filter does with good odometry; it is not a fair comparison against single-frame results."""
    _need_kitti_test(pairs, "kitti_motions")
    idx = np.arange(len(pairs)) if indices is None else np.asarray(indices, dtype=np.int64)
    motion = np.tile(np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]), (len(idx), 1))
    starts = np.zeros((len(idx),), dtype=bool)
    prev = None
    for n, i in enumerate(idx):
        cur = _kitti_frame(pairs, int(i))
        if n == 0 or cur[0][:38] != prev[0][:38] or _kitti_frame_number(cur[0]) <= _kitti_frame_number(prev[0]):
            starts[n] = True
        else:
            motion[n] = _kitti_pair_motion(pairs, prev, cur, True)
        prev = cur
    return motion, starts


def _kitti_frame_number(name):
    return int(os.path.splitext(name[38:])[0])
