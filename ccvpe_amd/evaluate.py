"""Sample-sharded evaluation loop (the caller side of the path: /root/reference/train_VIGOR.py:246-338,
train_KITTI.py:283-380), MI355X-style:

  * samples shard across ranks (harness.shard_indices) — inference has no data-path collective;
  * per batch: forward -> device-side post-processing (ccvpe_eval_postprocess_f32): 6 floats per
    sample come back instead of the reference's D2H copy of the full 512x512 heat-map and
    orientation field (3 MB per sample, train_VIGOR.py:288-289);
  * per-sample metrics exactly as the reference computes them on the host
    (train_VIGOR.py:294-324): pixel distance of the arg-max to the ground truth, metres via the
    per-sample ground resolution, orientation error min(|d|, 360-|d|);
  * one all_gather of the [n,4] result rows at the end (RCCL on GPUs, gloo in the CPU test), rank 0
    reports mean / median (train_VIGOR.py:330-336).

`forward_fn(grd, sat)` returns the 9-tuple; `postprocess_fn(heatmap, ori)` returns [B,6]
(y, x, cos, sin, angle_deg, prob) — ccvpe_amd.ops.eval_postprocess on the GPU.

The reference's full TEST PROTOCOLS (longitudinal / lateral error, recall under 1 / 3 / 5 m and degrees, probability at the
ground truth, Oxford's three traversals) are the second half of this file: `evaluate_batches` drives a
`datasets.DeviceBatches` through the forward and ccvpe_eval_metrics_f32 (twelve doubles per sample, `metrics_spec` is its
numpy specification), reads ONE table back after the loop, and `summarise` / `format_report` produce what the three test
scripts print.  `evaluate_sequence` runs the same protocol along a drive, for the raw heat-maps and for the belief of a
histogram filter (ccvpe_amd.tracking).
"""
import math

import numpy as np
import torch
import torch.distributed as dist

from . import harness


def _angle_from_cos_sin(c, s):
    """train_VIGOR.py:317-322 (ground-truth side of the orientation error)."""
    a = math.degrees(math.acos(max(-1.0, min(1.0, c))))
    return (-a) % 360 if s < 0 else a


def sample_metrics(post_row, gt_yx, gt_cos_sin, metres_per_pixel):
    """(pixel_distance, metre_distance, orientation_error or NaN, prob) for one sample."""
    y, x, c, s, ang, prob = [float(v) for v in post_row]
    pd = math.sqrt((gt_yx[0] - y) ** 2 + (gt_yx[1] - x) ** 2)                  # train_VIGOR.py:298
    md = pd * metres_per_pixel                                                  # :300-307
    oe = float("nan")
    if not math.isnan(ang):                                                     # :311 (|cos|,|sin| <= 1)
        a_gt = _angle_from_cos_sin(gt_cos_sin[0], gt_cos_sin[1])
        d = abs(a_gt - ang)
        oe = min(d, 360 - d)                                                    # :324
    return pd, md, oe, prob


def _gather_rows(local, nmax, device=None):
    """All ranks' rows ordered by their first column (the sample index, >= 0).  local: [m, C] float64 on the host, m <= nmax on
    every rank: shards are padded to nmax rows with index -1, gathered (RCCL on GPUs, gloo on the CPU) and the padding dropped."""
    distributed = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size() if distributed else 1
    if distributed and world > 1:
        buf = torch.full((nmax, local.shape[1]), -1.0, dtype=torch.float64)
        buf[:local.shape[0]] = local
        if device is not None and dist.get_backend() == "nccl":
            buf = buf.to(device)
        gathered = [torch.empty_like(buf) for _ in range(world)]
        dist.all_gather(gathered, buf)
        allrows = torch.cat([g.cpu() for g in gathered])
        allrows = allrows[allrows[:, 0] >= 0]
    else:
        allrows = local
    return allrows[allrows[:, 0].argsort()]


def evaluate(forward_fn, postprocess_fn, samples, batch_size, device=None):
    """samples: sequence of dicts with keys grd [3,h,w], sat [3,512,512], gt_yx (y,x), gt_cos_sin,
    metres_per_pixel.  Returns (on every rank) a dict of global statistics + the gathered rows
    [n_samples,4] ordered by sample index."""
    distributed = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size() if distributed else 1
    rank = dist.get_rank() if distributed else 0
    mine = harness.shard_indices(len(samples), world, rank)
    rows = []
    for i in range(0, len(mine), batch_size):
        idx = mine[i:i + batch_size]
        grd = torch.stack([samples[j]["grd"] for j in idx])
        sat = torch.stack([samples[j]["sat"] for j in idx])
        if device is not None:
            grd, sat = grd.to(device), sat.to(device)
        out = forward_fn(grd, sat)
        post = postprocess_fn(out[1], out[2]).cpu()                             # [b,6] only
        for k, j in enumerate(idx):
            s = samples[j]
            rows.append((j,) + sample_metrics(post[k], s["gt_yx"], s["gt_cos_sin"], s["metres_per_pixel"]))
    local = torch.tensor(rows, dtype=torch.float64).reshape(-1, 5)
    # shards differ by at most one sample: the common padded length
    allrows = _gather_rows(local, (len(samples) + world - 1) // world, device)
    res = allrows[:, 1:].numpy()
    oe = res[:, 2][~np.isnan(res[:, 2])]
    return {
        "n": int(res.shape[0]),
        "mean_pixel_error": float(np.mean(res[:, 0])), "median_pixel_error": float(np.median(res[:, 0])),
        "mean_metre_error": float(np.mean(res[:, 1])), "median_metre_error": float(np.median(res[:, 1])),
        "mean_orientation_error": float(np.mean(oe)) if oe.size else float("nan"),
        "median_orientation_error": float(np.median(oe)) if oe.size else float("nan"),
        "mean_probability": float(np.mean(res[:, 3])),
        "rows": res,
    }


# ---- the reference test protocols: twelve numbers per sample, the reports of the three test scripts ---------------------
# columns of a metric row (ccvpe_eval_metrics_f32 / metrics_spec)
PRED_Y, PRED_X, GT_Y, GT_X, PIXEL, METRE, LONGITUDINAL, LATERAL, ANGLE, ORIENTATION, PROB, PROB_AT_GT = range(12)
THRESHOLDS = (1, 3, 5)
# ground resolution of the 512 x 512 aerial inputs, metres per pixel (train_VIGOR.py:300-307, train_OxfordRobotCar.py:204,249)
VIGOR_METRES_PER_PIXEL = {"NewYork": 0.113248 / 512 * 640, "Seattle": 0.100817 / 512 * 640,
                          "SanFrancisco": 0.118141 / 512 * 640, "Chicago": 0.111262 / 512 * 640}
OXFORD_METRES_PER_PIXEL = 0.09240351462361521 / 512 * 800


def metrics_spec(heatmap, ori, gt, gt_ori, heading_deg, metres_per_pixel):
    """The specification of ccvpe_eval_metrics_f32: the per-sample body of the reference's test loops (train_KITTI.py:309-343,
    train_OxfordRobotCar.py:218-246, train_VIGOR.py:294-326) in numpy float64, one sample at a time.  heatmap, gt [B,1,h,w] and
    ori, gt_ori [B,2,h,w] float32 (arrays or host tensors), heading_deg and metres_per_pixel [B] -> [B,12] float64."""
    heatmap, ori, gt, gt_ori = (np.asarray(t, dtype=np.float32) for t in (heatmap, ori, gt, gt_ori))
    heading_deg = np.asarray(heading_deg, dtype=np.float64).reshape(-1)
    metres_per_pixel = np.asarray(metres_per_pixel, dtype=np.float64).reshape(-1)
    rows = np.full((heatmap.shape[0], 12), np.nan, dtype=np.float64)
    n, w = heatmap.shape[2] * heatmap.shape[3], heatmap.shape[3]
    for b in range(heatmap.shape[0]):
        kp, kg = int(np.argmax(heatmap[b].reshape(n))), int(np.argmax(gt[b].reshape(n)))      # first maxima, row-major
        (py, px), (gy, gx) = divmod(kp, w), divmod(kg, w)
        dy, dx = gy - py, gx - px
        pixel = np.sqrt(np.float64(dy * dy + dx * dx))
        bearing = np.arctan2(np.float64(abs(dx)), np.float64(abs(dy))) * 180 / math.pi        # GT -> prediction, atan2(0, 0) = 0
        turn = np.abs(heading_deg[b] - bearing) * np.pi / 180                                  # heading as given: no wrap
        r = rows[b]
        r[PRED_Y], r[PRED_X], r[GT_Y], r[GT_X] = py, px, gy, gx
        r[PIXEL], r[METRE] = pixel, pixel * metres_per_pixel[b]
        r[LONGITUDINAL] = np.abs(np.cos(turn) * pixel) * metres_per_pixel[b]
        r[LATERAL] = np.abs(np.sin(turn) * pixel) * metres_per_pixel[b]
        c, s = ori[b, 0, py, px], ori[b, 1, py, px]
        if np.abs(c) <= 1 and np.abs(s) <= 1:                        # float32 comparisons, as the reference's
            up = math.degrees(math.acos(c))
            r[ANGLE] = (-up) % 360 if s < 0 else up
            d = abs(_angle_from_cos_sin(float(gt_ori[b, 0, gy, gx]), float(gt_ori[b, 1, gy, gx])) - r[ANGLE])
            r[ORIENTATION] = min(d, 360 - d)
        r[PROB], r[PROB_AT_GT] = heatmap[b, 0, py, px], heatmap[b, 0, gy, gx]
    return rows


def _mean(x):
    return float(np.mean(x)) if len(x) else float("nan")


def _median(x):
    return float(np.median(x)) if len(x) else float("nan")


def _within(x):
    return {t: float(np.sum(x < t) / len(x)) if len(x) else float("nan") for t in THRESHOLDS}


def _summarise_one(rows):
    # the probabilities are float32 values; the reference averages its list of them in float32 and prints a float32
    p_gt, p_max = rows[:, PROB_AT_GT].astype(np.float32), rows[:, PROB].astype(np.float32)
    oe = rows[:, ORIENTATION]
    oe = oe[~np.isnan(oe)]                                           # the reference appends to this list only when |cos|,|sin| <= 1
    out = {"n": int(rows.shape[0])}
    for name, x in (("pixel_error", rows[:, PIXEL]), ("metre_error", rows[:, METRE]),
                    ("longitudinal_error", rows[:, LONGITUDINAL]), ("lateral_error", rows[:, LATERAL]),
                    ("orientation_error", oe), ("probability_at_gt", p_gt), ("probability", p_max)):
        out["mean_" + name], out["median_" + name] = _mean(x), _median(x)
    out["lateral_within"] = _within(rows[:, LATERAL])
    out["longitudinal_within"] = _within(rows[:, LONGITUDINAL])
    out["orientation_within"] = _within(oe)
    return out


def summarise(rows, sets=None):
    """The quantities the reference's test scripts print, from [n,12] metric rows: n, mean_/median_ of pixel_error, metre_error,
    longitudinal_error, lateral_error, orientation_error (non-NaN entries only), probability_at_gt and probability (at the
    arg-max; these two are taken in float32 as the reference takes them, and returned widened), and lateral_within / longitudinal_within / orientation_within = {1: , 3: , 5: } as sum(x < t) / len(x).
    sets: ordered mapping name -> row positions (index array, slice or boolean mask); the same statistics per set are under
    "sets"."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 12)
    out = _summarise_one(rows)
    if sets:
        out["sets"] = {name: _summarise_one(rows[sel]) for name, sel in sets.items()}
    return out


def _three(d):
    return " ".join(str(d[t]) for t in THRESHOLDS)


def _report_kitti(s, title):
    bar = "-" * 39
    return ([bar] + ([title] if title else []) +
            ["mean localization error (m):  %s" % s["mean_metre_error"],
             "median localization error (m):  %s" % s["median_metre_error"], bar,
             "mean orientation error (degrees):  %s" % s["mean_orientation_error"],
             "median orientation error (degrees):  %s" % s["median_orientation_error"], bar,
             "percentage of samples with lateral localization error under 1m, 3m, and 5m:  " + _three(s["lateral_within"]),
             "percentage of samples with longitudinal localization error under 1m, 3m, and 5m:  " + _three(s["longitudinal_within"]),
             "percentage of samples with orientation error under 1 degree, 3 degrees, and 5 degrees:  " + _three(s["orientation_within"])])


def _report_oxford(s, title):
    return (([title] if title else []) +
            ["mean error (m):  %s" % s["mean_metre_error"], "median error (m):  %s" % s["median_metre_error"],
             "mean longitudinal error (m):  %s" % s["mean_longitudinal_error"],
             "median longitudinal error (m):  %s" % s["median_longitudinal_error"],
             "mean lateral error (m):  %s" % s["mean_lateral_error"], "median lateral error (m):  %s" % s["median_lateral_error"],
             "mean orientation error (deg):  %s" % s["mean_orientation_error"],
             "median orientation error (deg):  %s" % s["median_orientation_error"],
             "percentage of samples with longitudinal localization error under 1m, 3m, and 5m:  " + _three(s["longitudinal_within"]),
             "percentage of samples with lateral localization error under 1m, 3m, and 5m:  " + _three(s["lateral_within"]),
             "percentage of samples with orientation error under 1 degree, 3 degrees, and 5 degrees:  " + _three(s["orientation_within"])])


def format_report(summary, kind):
    """The lines the reference's test script of `kind` prints ('vigor': train_VIGOR.py:329-338, 'kitti': train_KITTI.py:345-360,
    'oxford': train_OxfordRobotCar.py:248-268), as one string.  KITTI and Oxford report set by set when the summary has sets,
    each under its name, and the whole run otherwise.  Where this departs from the scripts: the title line of a block
    ('Test 1 set', 'test1') is the SET's name, so a summary without sets prints no title — pass sets={"Test 1 set": ...} to
    summarise / evaluate_batches for KITTI's; and Oxford's mean / median error is taken over metres per sample, where the script
    scales the mean pixel distance afterwards (the last place may differ).  The probabilities print as the float32 values they
    are, like the script's."""
    if kind == "vigor":
        bar = "-" * 39
        lines = ["mean localization error (m):  %s" % summary["mean_metre_error"],
                 "median localization error (m):  %s" % summary["median_metre_error"], bar,
                 "mean orientation error (degrees):  %s" % summary["mean_orientation_error"],
                 "median orientation error (degrees):  %s" % summary["median_orientation_error"], bar,
                 "mean probability at gt %s" % np.float32(summary["mean_probability_at_gt"]),
                 "median probability at gt %s" % np.float32(summary["median_probability_at_gt"])]
    elif kind in ("kitti", "oxford"):
        blocks = list(summary["sets"].items()) if summary.get("sets") else [(None, summary)]
        one = _report_kitti if kind == "kitti" else _report_oxford
        lines = []
        for k, (title, s) in enumerate(blocks):
            if kind == "oxford" and k:
                lines.append("-" * 70)
            lines += one(s, title)
    else:
        raise ValueError("kind must be 'vigor', 'kitti' or 'oxford'")
    return "\n".join(lines)


def default_metres_per_pixel(pairs):
    """The ground resolution the reference's test script uses for `pairs`: a float (KITTI, Oxford) or the per-city table
    (VIGOR)."""
    from . import datasets
    if isinstance(pairs, datasets.KITTIPairs):
        return float(pairs.meter_per_pixel)                                     # train_KITTI.py:317
    if isinstance(pairs, datasets.OxfordPairs):
        return OXFORD_METRES_PER_PIXEL
    if isinstance(pairs, datasets.VIGORPairs):
        return VIGOR_METRES_PER_PIXEL
    raise ValueError("no default metres_per_pixel for %s: pass a float or a {city: float} table" % type(pairs).__name__)


def default_sets(pairs):
    """name -> sample indices: test1 / test2 / test3 of an Oxford test split (its three traversals, reported one by one,
    train_OxfordRobotCar.py:209-400); None — one set — otherwise."""
    from . import datasets
    if isinstance(pairs, datasets.OxfordPairs) and pairs.split == "test":
        ends = np.cumsum(pairs.list_lengths)
        return {"test%d" % (k + 1): np.arange(e - n, e) for k, (n, e) in enumerate(zip(pairs.list_lengths, ends))}
    return None


def evaluate_batches(forward_fn, batches, metres_per_pixel=None, sets=None):
    """The reference's test protocol over a `datasets.DeviceBatches` built with targets=True: per batch the forward (no_grad) and
    ONE ccvpe_eval_metrics_f32 launch that writes the batch's rows into a device table [n,12]; nothing is copied to the host
    inside the loop — the table is read back once after it, gathered over the ranks (each rank iterates its own shard of
    `batches`) and ordered by sample index.  metres_per_pixel: a float, a {city: float} table looked up through batch.cities, or
    None = default_metres_per_pixel(batches.pairs).  sets: name -> sample indices, None = default_sets(batches.pairs).
    Returns summarise(...) + "rows" [n,12] + "indices" [n] on every rank."""
    from . import ops
    if not batches.targets:
        raise ValueError("evaluate_batches needs DeviceBatches(..., targets=True): the ground truth comes from the batch")
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    if world > 1 and batches.shard != "exact":
        raise ValueError("evaluate_batches needs DeviceBatches(..., shard='exact') on several ranks: a '%s' shard repeats or drops "
                         "samples, and the gathered statistics would count them wrongly" % batches.shard)
    mpp = default_metres_per_pixel(batches.pairs) if metres_per_pixel is None else metres_per_pixel
    if sets is None:
        sets = default_sets(batches.pairs)
    dev = batches.device
    n_local = len(batches.indices)
    table = torch.empty((n_local, 12), device=dev, dtype=torch.float64)
    if not isinstance(mpp, dict):
        mpp_const = torch.full((max(1, batches.batch_size),), float(mpp), device=dev, dtype=torch.float64)
    indices, k = [], 0
    for batch in batches:
        b = len(batch.indices)
        with torch.no_grad():
            out = forward_fn(batch.grd, batch.sat)
        m = (torch.tensor([mpp[c] for c in batch.cities], device=dev, dtype=torch.float64) if isinstance(mpp, dict)
             else mpp_const[:b])
        ops.eval_metrics(out[1], out[2], batch.gt, batch.gt_ori, batch.heading_deg, m, out=table[k:k + b])
        indices += [int(i) for i in batch.indices]
        k += b
    host = table[:k].cpu()                                                       # the one read-back (and the one sync)
    local = torch.cat([torch.tensor(indices, dtype=torch.float64).reshape(-1, 1), host], dim=1)
    nmax = local.shape[0]
    if world > 1:
        t = torch.tensor([nmax], dtype=torch.int64, device=dev if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)                                 # shards may differ in length
        nmax = int(t.item())
    allrows = _gather_rows(local, nmax, dev).numpy()
    idx, rows = allrows[:, 0].astype(np.int64), allrows[:, 1:]
    masks = {name: np.isin(idx, np.asarray(sel)) for name, sel in sets.items()} if sets else None
    res = summarise(rows, masks)
    res["rows"], res["indices"] = rows, idx
    return res


def evaluate_sequence(forward_fn, batches, filt, shift_px, starts, metres_per_pixel=None, sets=None, motion=None, smooth=False,
                      path=False):
    """The reference's test protocol along a drive, for the raw heat-maps AND for the belief of a histogram filter
    (ccvpe_amd.tracking.HistogramFilter with one track).  `batches`: a DeviceBatches in drive order — unshuffled, one rank,
    targets=True (ValueError otherwise); shift_px [n,2] and starts [n] per sample of `batches.indices`, e.g. from
    tracking.oxford_shifts(batches.pairs, batches.indices).  motion [n,6] (tracking.kitti_motions(batches.pairs,
    batches.indices): KITTI's patch frame turns between frames): every frame then steps with its motion row through the
    rigid step and shift_px may be None.  Per batch one forward and one ccvpe_eval_metrics_f32 launch for
    the raw maps; then per frame one `filt.step` (reset first where starts says so) and one ccvpe_eval_metrics_f32 launch on the
    belief, all into device tables; ONE read-back after the loop.
    Returns {"raw": summarise(...), "filtered": summarise(...), "tracks": [n,14] (tracking.PRED_Y ... SURVIVED),
    "raw_rows": [n,12], "filtered_rows": [n,12], "indices": [n]}.

    smooth=True adds the forward-backward smoothed estimate (tracking.SequenceSmoother with the filter's settings: the belief
    of every frame given the WHOLE drive).  The loop then also keeps, per frame and on the device, the heat-map, ori (2 maps),
    the ground-truth map, gt_ori (2 maps) and the filter's posterior, plus metres per pixel and the heading: 7 fp32 maps, 7 MB
    per frame at 512 x 512, and the smoothed beliefs (1 MB per frame) during the backward pass.  After the loop: the backward
    pass (two launches per frame) and one ccvpe_eval_metrics_f32 launch per smoothed belief; still ONE read-back.  The result
    gains "smoothed": summarise(...), "smoothed_rows": [n,12] and "smoothed_tracks": [n,14] (RESET holds the backward state).
    With smooth=False the returned dict and the launches are exactly those described above.

    path=True adds the most likely path (tracking.MostLikelyPath with the filter's settings: ONE trajectory, the jointly most
    likely sequence of grid cells; shift_px only — the rigid form is out of scope, ValueError with motion).  The loop keeps the
    frames as smooth=True does; after it come the max-product forward pass (two launches per frame), one backtrack launch and
    the protocol rows of a one-hot map at every path pixel (written on the device, no sync); still ONE read-back.  The result
    gains "path": summarise(...), "path_rows": [n,12] and "path_tracks": [n,8] (tracking.PATH_Y ... PATH_SCORE).  With
    path=False the returned dict and the launches are exactly those described above."""
    from . import ops
    if path and motion is not None:
        raise ValueError("evaluate_sequence: path=True takes shift_px; the most likely path under a rigid motion is out of scope")
    if not batches.targets:
        raise ValueError("evaluate_sequence needs DeviceBatches(..., targets=True): the ground truth comes from the batch")
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    idx = np.asarray(batches.indices, dtype=np.int64)
    # the loader's own settings decide, not the order that came out: a shuffle can leave indices ascending by chance, and a
    # shard of a larger world is ascending too
    if world > 1 or batches.world != 1 or batches.shuffle or len(idx) == 0 or np.any(np.diff(idx) <= 0):
        raise ValueError("evaluate_sequence needs the frames in drive order on one rank: DeviceBatches(..., shuffle=False, "
                         "world=1) with ascending indices")
    if filt.n_tracks != 1:
        raise ValueError("evaluate_sequence steps one track: HistogramFilter(1, ...)")
    starts = np.asarray(starts).reshape(-1).astype(bool)
    n = len(idx)
    if motion is not None:
        motion = np.asarray(motion, dtype=np.float64)
        if len(starts) != n or motion.shape != (n, 6):
            raise ValueError("evaluate_sequence: motion must be [%d,6] and starts hold one entry per sample of batches.indices" % n)
    elif shift_px is None:
        raise ValueError("evaluate_sequence: pass shift_px [n,2], or motion [n,6] for a patch frame that turns")
    elif len(starts) != n or len(shift_px) != n:
        raise ValueError("evaluate_sequence: shift_px and starts must hold one entry per sample of batches.indices (%d)" % n)
    mpp = default_metres_per_pixel(batches.pairs) if metres_per_pixel is None else metres_per_pixel
    if sets is None:
        sets = default_sets(batches.pairs)
    dev = batches.device
    if motion is not None:
        motions = torch.as_tensor(motion).to(dev)
    else:
        shifts = torch.as_tensor(np.asarray(shift_px, dtype=np.float64).reshape(n, 2)).to(dev)
    raw, fil, trk = (torch.empty((n, c), device=dev, dtype=torch.float64) for c in (12, 12, 14))
    if not isinstance(mpp, dict):
        mpp_const = torch.full((max(1, batches.batch_size),), float(mpp), device=dev, dtype=torch.float64)
    k = 0
    kept = None                                                                 # smooth: [n, ...] copies of heat, ori, gt, gt_ori, heading, m
    posts = torch.empty((n, 1) + tuple(filt.hw), device=dev, dtype=torch.float32) if smooth else None
    for batch in batches:
        b = len(batch.indices)
        with torch.no_grad():
            out = forward_fn(batch.grd, batch.sat)
        m = (torch.tensor([mpp[c] for c in batch.cities], device=dev, dtype=torch.float64) if isinstance(mpp, dict)
             else mpp_const[:b])
        heat, ori = out[1], out[2]
        ops.eval_metrics(heat, ori, batch.gt, batch.gt_ori, batch.heading_deg, m, out=raw[k:k + b])
        if smooth or path:                                                      # copies: a forward may reuse its output buffers
            frame = (heat, ori, batch.gt, batch.gt_ori, batch.heading_deg, m)
            if kept is None:
                kept = [torch.empty((n,) + tuple(f.shape[1:]), device=dev, dtype=f.dtype) for f in frame]
            for table, f in zip(kept, frame):
                table[k:k + b].copy_(f)
        for j in range(b):
            if starts[k + j]:
                filt.reset()
            if motion is not None:
                filt.step(heat[j:j + 1], ori[j:j + 1], motion=motions[k + j:k + j + 1], rows_out=trk[k + j:k + j + 1])
            else:
                filt.step(heat[j:j + 1], ori[j:j + 1], shifts[k + j:k + j + 1], rows_out=trk[k + j:k + j + 1])
            ops.eval_metrics(filt.belief, ori[j:j + 1], batch.gt[j:j + 1], batch.gt_ori[j:j + 1], batch.heading_deg[j:j + 1],
                             m[j:j + 1], out=fil[k + j:k + j + 1])
            if smooth:
                posts[k + j:k + j + 1].copy_(filt.belief)
        k += b
    tables = [raw, fil, trk]
    if smooth:
        tables += _smooth_sequence(filt, kept, posts, trk, motions if motion is not None else shifts, motion is not None, starts)
    if path:
        tables += _path_sequence(filt, kept, shifts, starts)
    table = torch.cat(tables, dim=1).cpu().numpy()                               # the one read-back (and the one sync)
    raw_rows, fil_rows, tracks = table[:, :12], table[:, 12:24], table[:, 24:38]
    masks = {name: np.isin(idx, np.asarray(sel)) for name, sel in sets.items()} if sets else None
    res = {"raw": summarise(raw_rows, masks), "filtered": summarise(fil_rows, masks), "tracks": tracks,
           "raw_rows": raw_rows, "filtered_rows": fil_rows, "indices": idx}
    if smooth:
        res["smoothed_rows"], res["smoothed_tracks"] = table[:, 38:50], table[:, 50:64]
        res["smoothed"] = summarise(res["smoothed_rows"], masks)
    if path:
        c = 64 if smooth else 38
        res["path_rows"], res["path_tracks"] = table[:, c:c + 12], table[:, c + 12:c + 20]
        res["path"] = summarise(res["path_rows"], masks)
    return res


def _path_sequence(filt, kept, shifts, starts, chunk=64):
    """evaluate_sequence(path=True) after its loop: tracking.MostLikelyPath over the kept frames and the protocol rows of a
    one-hot map at every path pixel, `chunk` frames per ccvpe_eval_metrics_f32 launch.  The one-hot maps are written on the
    device from the path table (no sync).  Returns device tables [n,12] and [n,8]."""
    from . import ops, tracking
    heat, ori, gt, gt_ori, heading, m = kept
    dev, n = heat.device, heat.shape[0]
    h, w = filt.hw
    out = tracking.MostLikelyPath(filt.hw, filt.sigma_px, filt.radius, filt.outlier, dev).run(heat, ori, shifts, starts)
    track = out["path"].reshape(n, 8)
    pixel = (track[:, tracking.PATH_Y] * w + track[:, tracking.PATH_X]).to(torch.int64).reshape(n, 1)
    rows = torch.empty((n, 12), device=dev, dtype=torch.float64)
    onehot = torch.empty((min(n, chunk), 1, h, w), device=dev, dtype=torch.float32)
    for k in range(0, n, chunk):
        b = min(chunk, n - k)
        onehot[:b].zero_()
        onehot[:b].reshape(b, h * w).scatter_(1, pixel[k:k + b], 1.0)
        ops.eval_metrics(onehot[:b], ori[k:k + b], gt[k:k + b], gt_ori[k:k + b], heading[k:k + b], m[k:k + b], out=rows[k:k + b])
    return [rows, track]


def _smooth_sequence(filt, kept, posts, filtered, move, rigid, starts):
    """evaluate_sequence(smooth=True) after its loop: the backward pass of tracking.SequenceSmoother over the kept frames and
    the filter's posteriors, and the protocol rows of every smoothed belief.  Returns device tables [n,12] and [n,14]."""
    from . import ops, tracking
    dev, n = posts.device, posts.shape[0]
    sm = tracking.SequenceSmoother(filt.hw, filt.sigma_px, filt.radius, filt.outlier, dev)
    heat, ori, gt, gt_ori, heading, m = kept
    if rigid:
        _, taps = tracking.motion_taps(torch.zeros((n, 2), device=dev, dtype=torch.float64), sm.sigma_px, sm.radius)
        move = move.to(torch.float64).reshape(n, 6).contiguous()
    else:
        move, taps = tracking.motion_taps(move, sm.sigma_px, sm.radius)
    reset = torch.as_tensor(starts.astype(np.int32)).to(dev)
    out = sm.backward(heat, ori, move, taps, reset, posts, filtered, keep_beliefs=True)
    rows = torch.empty((n, 12), device=dev, dtype=torch.float64)
    for t in range(n):
        ops.eval_metrics(out["beliefs"][t:t + 1], ori[t:t + 1], gt[t:t + 1], gt_ori[t:t + 1], heading[t:t + 1], m[t:t + 1],
                         out=rows[t:t + 1])
    return [rows, out["smoothed"]]
