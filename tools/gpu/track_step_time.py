"""The histogram-filter step (ccvpe_belief_step_f32, two launches) beside a torch-ops composition of the same update on the same
device, 512 x 512, R = 8, at B = 1 and B = 64: three alternating rounds, device events around N back-to-back steps, medians
(DESIGN.md section 4 quotes them; figures, not a gate):

    python tools/gpu/track_step_time.py [--out DIR]

  hip        ops.belief_step, no read-back (the row stays on the device)
  filter     tracking.HistogramFilter.step with the shifts on the device: motion_taps (a dozen small torch launches), the step and
             the clearing of the reset flags — what a caller of the filter pays per frame, no read-back
  hip_rb     the same as hip plus the read-back of the [B,14] rows, for a like-for-like with the composition
  torch      shift (slice copy into zeros), two grouped conv2d (rows, columns), product with the outlier-mixed heat-map, sum,
             divide, arg-max and its read-back; the shift is one slice copy per track
  torch_shared  the same with ONE slice copy for the whole batch (every track moved by the same offset): the cheapest
             composition, not the same result at B > 1
  floor      one pass over the step's bytes — prior and heat read, U written, U read, post written: 5 B h w 4 bytes — at the
             device-to-device copy rate measured in the same call

Writes track_step_timing.json into --out."""
import argparse

import numpy as np
import torch
import torch.nn.functional as F

from track_common import ALPHA, H, R, W, floor, scene, timed, write
from ccvpe_amd import ops, tracking  # noqa: E402  (track_common puts the repository root on sys.path)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=".")
args = ap.parse_args()


def case(B, n):
    prior, heat, _, ori, shift, _ = scene(B)
    offsets, taps = tracking.motion_taps(shift, 2.5, R)
    post = torch.empty_like(prior)
    scratch = torch.empty((B * ops.belief_partials(H, W),), device="cuda", dtype=torch.float64)
    rows = torch.empty((B, 14), device="cuda", dtype=torch.float64)
    off_host = offsets.cpu().tolist()
    ky = taps[:, 0].reshape(B, 1, 2 * R + 1, 1).flip(2).contiguous()      # conv2d correlates: flip for a convolution
    kx = taps[:, 1].reshape(B, 1, 1, 2 * R + 1).flip(3).contiguous()
    uniform = ALPHA / (H * W)

    def hip():
        ops.belief_step(prior, heat, ori, offsets, taps, outlier=ALPHA, post=post, scratch=scratch, out=rows)

    filt = tracking.HistogramFilter(B, hw=(H, W), sigma_px=2.5, radius=R, outlier=ALPHA)

    def filter_step():
        filt.step(heat, ori, shift, rows_out=rows)

    def hip_rb():
        hip()
        return rows.cpu()

    def composed(shared=False):
        # the moved prior on a canvas with an R halo — the prior is zero outside ITS grid, the moved prior is not cropped
        # before the blur — then two "valid" grouped convolutions
        moved = torch.zeros((B, 1, H + 2 * R, W + 2 * R), device="cuda")
        for b, (oy, ox) in enumerate(off_host[:1] if shared else off_host):
            ys = slice(max(0, R + oy), min(H + 2 * R, H + R + oy))
            xs = slice(max(0, R + ox), min(W + 2 * R, W + R + ox))
            yd, xd = slice(ys.start - R - oy, ys.stop - R - oy), slice(xs.start - R - ox, xs.stop - R - ox)
            if shared:                                                     # every track moved by track 0's offset: ONE copy
                moved[:, 0, ys, xs] = prior[:, 0, yd, xd]
            else:
                moved[b, 0, ys, xs] = prior[b, 0, yd, xd]
        q = F.conv2d(moved.reshape(1, B, H + 2 * R, W + 2 * R), kx, groups=B)
        q = F.conv2d(q, ky, groups=B).reshape(B, 1, H, W)
        u = q * ((1 - ALPHA) * heat + uniform)
        z = u.sum(dim=(1, 2, 3), keepdim=True, dtype=torch.float64)
        p = u * (1.0 / z).float()
        return p, p.reshape(B, -1).argmax(1).cpu()                         # the estimate reaches the host: one sync per step

    # the two compute the same thing (fp32 roundings differ: last bits)
    hip()
    p, am = composed()
    torch.cuda.synchronize()
    same_argmax = bool((am == (rows[:, 0] * W + rows[:, 1]).long().cpu()).all())
    max_rel = float(((post - p).abs().amax(dim=(1, 2, 3)) / p.amax(dim=(1, 2, 3))).max())       # per track, against its peak
    res = {"B": B, "steps_per_round": n, "same_argmax": same_argmax, "max_diff_over_peak_vs_torch": max_rel,
           "hip_us": [], "filter_us": [], "hip_rb_us": [], "torch_us": [], "torch_shared_us": [], "copy_us": []}
    src, dst = torch.empty_like(prior), torch.empty_like(prior)
    for _ in range(3):
        res["hip_us"].append(timed(hip, n, 20))
        res["torch_us"].append(timed(composed, max(10, n // 10), 5))
        res["filter_us"].append(timed(filter_step, n, 20))
        res["hip_rb_us"].append(timed(hip_rb, n, 20))
        res["torch_shared_us"].append(timed(lambda: composed(True), max(10, n // 10), 5))
        res["copy_us"].append(timed(lambda: dst.copy_(src), n, 20))
    for k in ("hip", "filter", "hip_rb", "torch", "torch_shared", "copy"):
        res[k + "_median_us"] = float(np.median(res[k + "_us"]))
    floor(res, B, 5)
    res["hip_over_floor"] = res["hip_median_us"] / res["floor_us"]
    res["torch_over_hip"] = res["torch_median_us"] / res["hip_median_us"]
    res["torch_over_hip_rb"] = res["torch_median_us"] / res["hip_rb_median_us"]
    res["torch_shared_over_hip_rb"] = res["torch_shared_median_us"] / res["hip_rb_median_us"]
    return res


out = {"shape": [H, W], "radius": R, "cases": [case(1, 2000), case(64, 200)]}
write(out, args.out, "track_step_timing.json")
