"""The backward step of the forward-backward smoother (ccvpe_belief_smooth_step_f32 / _rigid_f32, two launches) beside the
forward filter step of the same build and a torch-ops composition of the same backward update, 512 x 512, R = 8, at B = 1 and
B = 64: three alternating rounds, device events around N back-to-back steps, medians (profiles/r27/README.md and DESIGN.md
section 4 quote them; figures, not a gate):

    python tools/gpu/track_smooth_time.py [--out DIR] [--parent-lib OLD/libccvpe_hip.so [--bench]]

  smooth        ops.belief_smooth_step: every track with its own offset and taps, no read-back
  smooth_rigid  ops.belief_smooth_step_rigid: every track with its own motion (turns of -15 .. 15 degrees, shifts of -6 .. 6 px)
  forward       ops.belief_step of the same build with the same offsets and taps: the step the backward one is held against
  torch         the outlier-mixed heat-map times the message, zero-padded and shifted, two grouped conv2d with the taps as
                they are (conv2d correlates: that is the reversal), product with alpha, two sums, two divides, arg-max and its
                read-back
  smooth_rb     smooth plus the read-back of the [B,14] rows, for a like-for-like with the composition
  floor         one pass over the step's bytes — heat, beta and alpha read, B' and V written, both read, both written:
                9 B h w 4 bytes (the forward step: 5) — at the device-to-device copy rate measured in the same call

Every GPU step is a child process under its own `timeout`; the first step that fails ends the run.  With --parent-lib, all six
belief entry points are compared bit for bit and timed against that older library (track_common.identity / versus), and the
forward step is also timed through both libraries beside the legs above; with --bench, bench.py is then run against this build
and against the older library.  Writes track_smooth_timing.json into --out."""
import json
import os

from track_common import ALPHA, H, R, W, against_parent, child, floor, libraries, medians, parser, scene, write

args = parser(["case"]).parse_args()


def forward_call(lib, entry, prior, heat, ori, move, taps, post, scratch, rows, B):
    rc = getattr(lib, entry)(prior.data_ptr(), heat.data_ptr(), ori.data_ptr(), move.data_ptr(), taps.data_ptr(), R, ALPHA, None,
                             post.data_ptr(), scratch.data_ptr(), rows.data_ptr(), B, H, W, None)
    if rc != 0:
        raise RuntimeError("%s returned %d" % (entry, rc))


def case(B, n, parent_lib):
    import numpy as np
    import torch
    import torch.nn.functional as F
    from ccvpe_amd import ops, tracking
    beta, heat, alpha, ori, shift, angle = scene(B)
    motion = torch.from_numpy(tracking.rigid_motion(shift.cpu().numpy(), angle.cpu().numpy(), (H, W))).cuda()
    offsets, taps = tracking.motion_taps(shift, 2.5, R)
    _, centred = tracking.motion_taps(torch.zeros_like(shift), 2.5, R)
    beta_out, smooth, post = torch.empty_like(beta), torch.empty_like(beta), torch.empty_like(beta)
    scratch = torch.empty((B * ops.belief_partials(H, W),), device="cuda", dtype=torch.float64)
    rows = torch.empty((B, 14), device="cuda", dtype=torch.float64)
    ky = taps[:, 0].reshape(B, 1, 2 * R + 1, 1).contiguous()               # conv2d correlates: the taps as they are
    kx = taps[:, 1].reshape(B, 1, 1, 2 * R + 1).contiguous()
    uniform = ALPHA / (H * W)
    off = offsets.cpu().numpy()
    assert np.abs(off).max() <= 6

    def smooth_step():
        ops.belief_smooth_step(beta, heat, alpha, ori, offsets, taps, outlier=ALPHA, beta_out=beta_out, smooth=smooth, scratch=scratch,
                               out=rows)

    def smooth_rigid():
        ops.belief_smooth_step_rigid(beta, heat, alpha, ori, motion, centred, outlier=ALPHA, beta_out=beta_out, smooth=smooth,
                                     scratch=scratch, out=rows)

    def forward():
        ops.belief_step(alpha, heat, ori, offsets, taps, outlier=ALPHA, post=post, scratch=scratch, out=rows)

    def smooth_rb():
        smooth_step()
        return rows.cpu()

    def composed():
        g = ((1 - ALPHA) * heat + uniform) * beta
        pad = F.pad(g, (R + 6, R + 6, R + 6, R + 6))                        # G[y + oy + i, x + ox + j]: a window per track
        moved = torch.stack([pad[b, :, 6 + off[b, 0]:6 + off[b, 0] + H + 2 * R, 6 + off[b, 1]:6 + off[b, 1] + W + 2 * R] for b in range(B)])
        q = F.conv2d(moved.reshape(1, B, H + 2 * R, W + 2 * R), kx, groups=B)
        bp = F.conv2d(q, ky, groups=B).reshape(B, 1, H, W)
        v = alpha * bp
        z = v.sum(dim=(1, 2, 3), keepdim=True, dtype=torch.float64)
        s = bp.sum(dim=(1, 2, 3), keepdim=True, dtype=torch.float64)
        p, m = v * (1.0 / z).float(), bp * (1.0 / s).float()
        return p, m, p.reshape(B, -1).argmax(1).cpu()                      # the estimate reaches the host: one sync per step

    smooth_step()
    p, m, am = composed()
    torch.cuda.synchronize()
    same_argmax = bool((am == (rows[:, 0] * W + rows[:, 1]).long().cpu()).all())
    rel_p = float(((smooth - p).abs().amax(dim=(1, 2, 3)) / p.amax(dim=(1, 2, 3))).max())       # per track, against its peak
    rel_m = float(((beta_out - m).abs().amax(dim=(1, 2, 3)) / m.amax(dim=(1, 2, 3))).max())
    res = {"B": B, "steps_per_round": n, "same_argmax": same_argmax, "smooth_max_diff_over_peak_vs_torch": rel_p,
           "beta_out_max_diff_over_peak_vs_torch": rel_m}
    legs = {"smooth": smooth_step, "smooth_rigid": smooth_rigid, "forward": forward, "smooth_rb": smooth_rb}
    if parent_lib:
        old, new = libraries(parent_lib)
        legs["forward_parent_lib"] = lambda: forward_call(old, "ccvpe_belief_step_f32", alpha, heat, ori, offsets, taps, post, scratch, rows, B)
        legs["forward_raw_call"] = lambda: forward_call(new, "ccvpe_belief_step_f32", alpha, heat, ori, offsets, taps, post, scratch, rows, B)
    src, dst = torch.empty_like(beta), torch.empty_like(beta)
    legs["copy"] = lambda: dst.copy_(src)
    legs["torch"] = composed
    medians(res, legs, n, slow=("torch",))
    floor(res, B, 9)
    res["smooth_over_floor"] = res["smooth_median_us"] / res["floor_us"]
    res["smooth_over_forward"] = res["smooth_median_us"] / res["forward_median_us"]
    res["smooth_rigid_over_forward"] = res["smooth_rigid_median_us"] / res["forward_median_us"]
    res["torch_over_smooth_rb"] = res["torch_median_us"] / res["smooth_rb_median_us"]
    if parent_lib:
        res["forward_raw_call_over_parent_lib"] = res["forward_raw_call_median_us"] / res["forward_parent_lib_median_us"]
    return res


if args.leg == "case":
    print(json.dumps(case(args.batch, 2000 if args.batch == 1 else 200, args.parent_lib)))
else:
    extra = ["--parent-lib", os.path.abspath(args.parent_lib)] if args.parent_lib else []
    out = {"shape": [H, W], "radius": R, "cases": [child(__file__, ["--leg", "case", "--batch", "1"] + extra, 240),
                                                   child(__file__, ["--leg", "case", "--batch", "64"] + extra, 240)]}
    if args.parent_lib:
        against_parent(out, "forward_steps_vs_parent", args.parent_lib, args.bench)
    write(out, args.out, "track_smooth_timing.json")
