"""The rigid-motion filter step (ccvpe_belief_step_rigid_f32, two launches) beside the translate-only step of the same build and a
torch-ops composition of the same update, 512 x 512, R = 8, at B = 1 and B = 64: three alternating rounds, device events around N
back-to-back steps, medians (profiles/r26/README.md and DESIGN.md section 4 quote them; figures, not a gate):

    python tools/gpu/track_rigid_time.py [--out DIR] [--parent-lib OLD/libccvpe_hip.so [--bench]]

  rigid      ops.belief_step_rigid: every track with its own motion (turns of -15 .. 15 degrees, shifts of -6 .. 6 px), no read-back
  translate  ops.belief_step of the same build with the shifts alone: the baseline the gather-based warp is held against
  torch      affine_grid + grid_sample (bilinear, zeros outside) onto the canvas with its R halo, two grouped conv2d (rows,
             columns), product with the outlier-mixed heat-map, sum, divide, arg-max and its read-back
  rigid_rb   rigid plus the read-back of the [B,14] rows, for a like-for-like with the composition
  floor      one pass over the step's bytes — prior and heat read, U written, U read, post written: 5 B h w 4 bytes — at the
             device-to-device copy rate measured in the same call

Every GPU step is a child process under its own `timeout`; the first step that fails ends the run.  With --parent-lib, all six
belief entry points are compared bit for bit and timed against that older library (track_common.identity / versus); with --bench,
bench.py is then run against this build and against the older library.  Writes track_rigid_timing.json into --out."""
import json

from track_common import ALPHA, H, R, W, against_parent, child, floor, parser, scene, timed, write

args = parser(["case"]).parse_args()


def case(B, n):
    import numpy as np
    import torch
    import torch.nn.functional as F
    from ccvpe_amd import ops, tracking
    prior, heat, _, ori, shift, angle = scene(B)
    motion_host = tracking.rigid_motion(shift.cpu().numpy(), angle.cpu().numpy(), (H, W))
    motion = torch.from_numpy(motion_host).cuda()
    offsets, shifted_taps = tracking.motion_taps(shift, 2.5, R)
    _, taps = tracking.motion_taps(torch.zeros_like(shift), 2.5, R)
    post = torch.empty_like(prior)
    scratch = torch.empty((B * ops.belief_partials(H, W),), device="cuda", dtype=torch.float64)
    rows = torch.empty((B, 14), device="cuda", dtype=torch.float64)
    ky = taps[:, 0].reshape(B, 1, 2 * R + 1, 1).flip(2).contiguous()      # conv2d correlates: flip for a convolution
    kx = taps[:, 1].reshape(B, 1, 1, 2 * R + 1).flip(3).contiguous()
    uniform = ALPHA / (H * W)
    # affine_grid's theta: normalised canvas coordinates (align_corners) -> canvas pixel -> source pixel -> normalised source
    he, we = H + 2 * R, W + 2 * R
    s_out = np.array([[(we - 1) / 2.0, 0, (we - 1) / 2.0 - R], [0, (he - 1) / 2.0, (he - 1) / 2.0 - R], [0, 0, 1]])
    n_in = np.array([[2.0 / (W - 1), 0, -1], [0, 2.0 / (H - 1), -1], [0, 0, 1]])
    theta = np.zeros((B, 2, 3))
    for b in range(B):
        a = motion_host[b]
        m = np.array([[a[4], a[3], a[5]], [a[1], a[0], a[2]], [0, 0, 1]])   # (x, y, 1) -> (sx, sy, 1)
        theta[b] = (n_in @ m @ s_out)[:2]
    theta = torch.from_numpy(theta).float().cuda()

    def rigid():
        ops.belief_step_rigid(prior, heat, ori, motion, taps, outlier=ALPHA, post=post, scratch=scratch, out=rows)

    def translate():
        ops.belief_step(prior, heat, ori, offsets, shifted_taps, outlier=ALPHA, post=post, scratch=scratch, out=rows)

    def rigid_rb():
        rigid()
        return rows.cpu()

    def composed():
        grid = F.affine_grid(theta, (B, 1, he, we), align_corners=True)
        moved = F.grid_sample(prior, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        q = F.conv2d(moved.reshape(1, B, he, we), kx, groups=B)
        q = F.conv2d(q, ky, groups=B).reshape(B, 1, H, W)
        u = q * ((1 - ALPHA) * heat + uniform)
        z = u.sum(dim=(1, 2, 3), keepdim=True, dtype=torch.float64)
        p = u * (1.0 / z).float()
        return p, p.reshape(B, -1).argmax(1).cpu()                         # the estimate reaches the host: one sync per step

    # the two compute the same thing (torch's grid is fp32: the weights differ in their last places)
    rigid()
    p, am = composed()
    torch.cuda.synchronize()
    same_argmax = bool((am == (rows[:, 0] * W + rows[:, 1]).long().cpu()).all())
    max_rel = float(((post - p).abs().amax(dim=(1, 2, 3)) / p.amax(dim=(1, 2, 3))).max())       # per track, against its peak
    res = {"B": B, "steps_per_round": n, "same_argmax": same_argmax, "max_diff_over_peak_vs_torch": max_rel,
           "rigid_us": [], "translate_us": [], "rigid_rb_us": [], "torch_us": [], "copy_us": []}
    src, dst = torch.empty_like(prior), torch.empty_like(prior)
    for _ in range(3):
        res["rigid_us"].append(timed(rigid, n, 20))
        res["translate_us"].append(timed(translate, n, 20))
        res["torch_us"].append(timed(composed, max(10, n // 10), 5))
        res["rigid_rb_us"].append(timed(rigid_rb, n, 20))
        res["copy_us"].append(timed(lambda: dst.copy_(src), n, 20))
    for k in ("rigid", "translate", "rigid_rb", "torch", "copy"):
        res[k + "_median_us"] = float(np.median(res[k + "_us"]))
    floor(res, B, 5)
    res["rigid_over_floor"] = res["rigid_median_us"] / res["floor_us"]
    res["translate_over_floor"] = res["translate_median_us"] / res["floor_us"]
    res["rigid_over_translate"] = res["rigid_median_us"] / res["translate_median_us"]
    res["torch_over_rigid_rb"] = res["torch_median_us"] / res["rigid_rb_median_us"]
    return res


if args.leg == "case":
    print(json.dumps(case(args.batch, 2000 if args.batch == 1 else 200)))
else:
    out = {"shape": [H, W], "radius": R, "cases": [child(__file__, ["--leg", "case", "--batch", "1"], 240),
                                                   child(__file__, ["--leg", "case", "--batch", "64"], 240)]}
    if args.parent_lib:
        against_parent(out, "translate_step_vs_parent", args.parent_lib, args.bench)
    write(out, args.out, "track_rigid_timing.json")
