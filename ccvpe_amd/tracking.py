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

Out of scope: rotation between patch frames (the grid only translates), KITTI's randomly rotated test patches, learned
motion models, bf16 beliefs.
"""
import math

import numpy as np
import torch

# columns of a track row (ccvpe_belief_step_f32 / step_spec)
(PRED_Y, PRED_X, PROB, COS, SIN, ANGLE, EVIDENCE, RESET, MEAN_Y, MEAN_X, VAR_YY, VAR_XX, COV_YX, SURVIVED) = range(14)
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
    h, w = prior.shape
    r = (len(ky) - 1) // 2
    # pad[r + y, r + x] = prior[y - oy, x - ox] for y in [-r, h + r): the prior is zero outside ITS grid, the moved prior is
    # not cropped before the blur (mass is lost only where it ends up off the grid)
    pad = np.zeros((h + 2 * r, w + 2 * r), dtype=np.float64)
    ys, xs = np.arange(-r, h + r, dtype=np.int64) - int(oy), np.arange(-r, w + r, dtype=np.int64) - int(ox)
    vy, vx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
    if vy.any() and vx.any():
        pad[np.ix_(vy, vx)] = prior[np.ix_(ys[vy], xs[vx])]
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
    heat = np.asarray(heat, dtype=np.float32)
    b, h, w = heat.shape[0], heat.shape[-2], heat.shape[-1]
    heat = heat.reshape(b, h, w).astype(np.float64)
    prior = np.asarray(prior, dtype=np.float32).reshape(b, h, w).astype(np.float64)
    ori = np.asarray(ori, dtype=np.float32).reshape(b, 2, h, w)
    offsets = np.asarray(offsets).reshape(b, 2)
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
            q = _predict_spec(prior[t], offsets[t, 0], offsets[t, 1], taps[t, 0], taps[t, 1])
            u = q * m
            z, survived = float(u.sum()), float(q.sum())
            if not (z > 0 and np.isfinite(z)):
                state = 2
        if state:
            u = m
            z = float(u.sum())
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.float64(np.float32(np.float64(1.0) / np.float64(z)))
            post[t] = (u * inv).astype(np.float32)
            p = u / z
            my, mx = float((p * yy).sum()), float((p * xx).sum())
            var_yy, var_xx = float((p * (yy - my) ** 2).sum()), float((p * (xx - mx) ** 2).sum())
            cov = float((p * (yy - my) * (xx - mx)).sum())
        k = int(np.argmax(u.reshape(-1)))
        py, px = divmod(k, w)
        c, s = ori[t, 0, py, px], ori[t, 1, py, px]
        rows[t] = (py, px, post[t, py, px], c, s, _angle_spec(c, s), z, state, my, mx, var_yy, var_xx, cov, survived)
        us[t] = u
    return (post, rows, us) if return_u else (post, rows)


class HistogramFilter(object):
    """The beliefs of `n_tracks` independent tracks on an h x w grid, stepped on the device.

    Owns two belief buffers (ping-pong: the step reads one and writes the other), the step's scratch and a rows tensor.
    sigma_px: the motion noise in pixels (a float; `step` may override it per call, per track); radius: of the blur taps,
    None = ceil(3 sigma) + 1, at most 32 (ValueError above); outlier: the weight of the uniform floor mixed into every
    heat-map, in [0, 1] — with 0 a heat-map that is exactly zero where the prediction has its mass resets the track.
    The first step after construction or after `reset` starts from the measurement alone."""

    def __init__(self, n_tracks, hw=(512, 512), sigma_px=1.0, radius=None, outlier=0.0, device="cuda"):
        from . import ops
        self.n_tracks, self.hw = int(n_tracks), (int(hw[0]), int(hw[1]))
        self.sigma_px = float(sigma_px)
        if self.sigma_px < 0:
            raise ValueError("sigma_px must be >= 0")
        self.radius = int(math.ceil(3 * self.sigma_px)) + 1 if radius is None else int(radius)
        if not 0 <= self.radius <= MAX_RADIUS:
            raise ValueError("radius %d outside [0, %d]: use a smaller sigma_px or pass radius" % (self.radius, MAX_RADIUS))
        if not 0.0 <= float(outlier) <= 1.0:
            raise ValueError("outlier must be in [0, 1]")
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

    def step(self, heatmap, ori, shift_px, sigma_px=None, rows_out=None):
        """One filter step: heatmap [B,1,h,w], ori [B,2,h,w] from the forward; shift_px [B,2] = (dy, dx), the motion of the
        vehicle in the grid since the previous step (odometry minus the motion of the aerial patch), a tensor on any device or
        an array.  Returns the rows [B,14] (columns PRED_Y ... SURVIVED): `rows_out` when given (a slice of a caller's table),
        else self.rows, which the next step overwrites."""
        from . import ops
        if tuple(heatmap.shape) != (self.n_tracks, 1) + self.hw:
            raise ValueError("step: heatmap must be %s, got %s" % ((self.n_tracks, 1) + self.hw, tuple(heatmap.shape)))
        shift = torch.as_tensor(shift_px).to(self.device)
        if shift.numel() != 2 * self.n_tracks:
            raise ValueError("step: shift_px must be [%d,2]" % self.n_tracks)
        offsets, taps = motion_taps(shift, self.sigma_px if sigma_px is None else sigma_px, self.radius)
        rows = self.rows if rows_out is None else rows_out
        ops.belief_step(self._buf[self._cur], heatmap, ori, offsets, taps, outlier=self.outlier, reset=self._reset,
                        post=self._buf[1 - self._cur], scratch=self._scratch, out=rows)
        self._reset.zero_()
        self._cur = 1 - self._cur
        return rows


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
