"""The max-product step (ccvpe_belief_viterbi_step_f32, two launches) beside the forward filter step of the same build and a
torch-ops composition of the same update, 512 x 512, R = 8, at B = 1 and B = 64, and the backtrack launch
(ccvpe_belief_backtrack_f32) over T = 64 frames at B = 1 and B = 64: three alternating rounds, device events around N
back-to-back calls, medians (profiles/r28/README.md and DESIGN.md section 4 quote them; figures, not a gate):

    python tools/gpu/track_path_time.py [--out DIR] [--parent-lib OLD/libccvpe_hip.so [--bench]]

  viterbi       ops.belief_viterbi_step: every track with its own offset and taps, no read-back
  forward       ops.belief_step of the same build with the same inputs: the step the max form is held against
  torch         the previous map zero-padded and shifted per track, 2R+1 shifted torch.maximum ops along x and 2R+1 along y with
                the taps broadcast per track, the outlier-mixed product, the sum, the divide, arg-max and its read-back
  viterbi_rb    viterbi plus the read-back of the [B,14] rows, for a like-for-like with the composition
  backtrack     ops.belief_backtrack over the [64,B] maps of a MostLikelyPath.run on random maps: ONE launch
  run           the whole MostLikelyPath.run (2 T + 1 launches), per frame

Every GPU step is a child process under its own `timeout`; the first step that fails ends the run.  With --parent-lib, all six
belief entry points are compared bit for bit and timed against that older library (track_common.identity / versus); with --bench,
bench.py is then run against this build and against the older library.  Writes track_path_timing.json into --out."""
import json

from track_common import ALPHA, FRAMES, H, R, W, against_parent, child, drive, floor, medians, parser, scene, write

args = parser(["step", "backtrack"]).parse_args()


def step_case(B, n):
    import numpy as np
    import torch
    import torch.nn.functional as F
    from ccvpe_amd import ops, tracking
    _, heat, prev, ori, shift, _ = scene(B)
    offsets, taps = tracking.motion_taps(shift, 2.5, R)
    post = torch.empty_like(prev)
    scratch = torch.empty((B * ops.belief_partials(H, W),), device="cuda", dtype=torch.float64)
    rows = torch.empty((B, 14), device="cuda", dtype=torch.float64)
    ky = taps[:, 0].reshape(B, 1, 2 * R + 1, 1, 1)
    kx = taps[:, 1].reshape(B, 1, 2 * R + 1, 1, 1)
    uniform = ALPHA / (H * W)
    off = offsets.cpu().numpy()
    assert np.abs(off).max() <= 6

    def viterbi():
        ops.belief_viterbi_step(prev, heat, ori, offsets, taps, outlier=ALPHA, post=post, scratch=scratch, out=rows)

    def forward():
        ops.belief_step(prev, heat, ori, offsets, taps, outlier=ALPHA, post=post, scratch=scratch, out=rows)

    def viterbi_rb():
        viterbi()
        return rows.cpu()

    def composed():
        pad = F.pad(prev, (R + 6, R + 6, R + 6, R + 6))                     # prev[y - oy - i, x - ox - j]: a window per track
        moved = torch.stack([pad[b, :, 6 - off[b, 0]:6 - off[b, 0] + H + 2 * R, 6 - off[b, 1]:6 - off[b, 1] + W + 2 * R] for b in range(B)])
        row = torch.zeros((B, 1, H + 2 * R, W), device="cuda")
        for j in range(-R, R + 1):
            row = torch.maximum(row, kx[:, :, j + R] * moved[:, :, :, R - j:R - j + W])
        p = torch.zeros((B, 1, H, W), device="cuda")
        for i in range(-R, R + 1):
            p = torch.maximum(p, ky[:, :, i + R] * row[:, :, R - i:R - i + H, :])
        u = p * ((1 - ALPHA) * heat + uniform)
        z = u.sum(dim=(1, 2, 3), keepdim=True, dtype=torch.float64)
        d = u * (1.0 / z).float()
        return d, d.reshape(B, -1).argmax(1).cpu()                          # the estimate reaches the host: one sync per step

    viterbi()
    d, am = composed()
    torch.cuda.synchronize()
    res = {"B": B, "calls_per_round": n,
           "same_argmax": bool((am == (rows[:, 0] * W + rows[:, 1]).long().cpu()).all()),
           "post_max_diff_over_peak_vs_torch": float(((post - d).abs().amax(dim=(1, 2, 3)) / d.amax(dim=(1, 2, 3))).max())}
    src, dst = torch.empty_like(prev), torch.empty_like(prev)
    legs = {"viterbi": viterbi, "forward": forward, "viterbi_rb": viterbi_rb, "copy": lambda: dst.copy_(src), "torch": composed}
    medians(res, legs, n, slow=("torch",))
    floor(res, B, 5)                                                         # prev and heat read, U written, read, written
    res["viterbi_over_floor"] = res["viterbi_median_us"] / res["floor_us"]
    res["viterbi_over_forward"] = res["viterbi_median_us"] / res["forward_median_us"]
    res["torch_over_viterbi_rb"] = res["torch_median_us"] / res["viterbi_rb_median_us"]
    return res


def backtrack_case(B, n):
    import torch
    from ccvpe_amd import ops, tracking
    d = drive(B, FRAMES)
    heat, ori, shift, mlp, out, offsets, taps, reset = (d[k] for k in ("heat", "ori", "shift", "mlp", "out", "offsets", "taps", "reset"))
    path = torch.empty((FRAMES, B, 8), device="cuda", dtype=torch.float64)
    ops.belief_backtrack(out["deltas"], ori, offsets, taps, out["rows"], reset, out=path)
    torch.cuda.synchronize()
    link = path[:, :, tracking.PATH_LINK]
    res = {"B": B, "frames": FRAMES, "calls_per_round": n, "same_path_as_run": bool(torch.equal(path, out["path"])),
           "chained_links": int((link == 0).sum()), "dead_links": int((link == 2).sum())}
    legs = {"backtrack": lambda: ops.belief_backtrack(out["deltas"], ori, offsets, taps, out["rows"], reset, out=path),
            "run": lambda: mlp.run(heat, ori, shift)}
    medians(res, legs, n, slow=("run",))
    res["backtrack_us_per_frame"] = res["backtrack_median_us"] / FRAMES
    res["run_us_per_frame"] = res["run_median_us"] / FRAMES
    return res


if args.leg == "step":
    print(json.dumps(step_case(args.batch, 2000 if args.batch == 1 else 200)))
elif args.leg == "backtrack":
    print(json.dumps(backtrack_case(args.batch, 200)))
else:
    out = {"shape": [H, W], "radius": R,
           "step": [child(__file__, ["--leg", "step", "--batch", "1"], 240), child(__file__, ["--leg", "step", "--batch", "64"], 240)],
           "backtrack": [child(__file__, ["--leg", "backtrack", "--batch", "1"], 240), child(__file__, ["--leg", "backtrack", "--batch", "64"], 300)]}
    if args.parent_lib:
        against_parent(out, "existing_steps_vs_parent", args.parent_lib, args.bench)
    write(out, args.out, "track_path_timing.json")
