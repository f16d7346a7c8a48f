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

Every GPU step is a child process under its own `timeout`; the first step that fails ends the run.  With --parent-lib, one
translate step at 512 x 512 is run through that older library and through this build in one process and post and rows are
compared bit for bit (the refactoring of the shared passes must not change ccvpe_belief_step_f32); with --bench, bench.py is then
run against this build and against the older library.  Writes track_rigid_timing.json into --out."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=".")
ap.add_argument("--parent-lib", default=None, help="an older libccvpe_hip.so: bit-compare ccvpe_belief_step_f32 against it")
ap.add_argument("--bench", action="store_true", help="with --parent-lib: bench.py against this build and against the older library")
ap.add_argument("--leg", choices=["case", "identity"], default=None, help="(internal) one child step")
ap.add_argument("--batch", type=int, default=1)
args = ap.parse_args()
H = W = 512
R, ALPHA = 8, 0.02


def timed(fn, n, warm):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / n          # microseconds per step


def scene(B):
    import torch
    import torch.nn.functional as F
    g = torch.Generator(device="cuda").manual_seed(B)
    prior = torch.softmax(torch.randn((B, H * W), device="cuda", generator=g) * 4, 1).reshape(B, 1, H, W)
    heat = torch.softmax(torch.randn((B, H * W), device="cuda", generator=g) * 4, 1).reshape(B, 1, H, W)
    ori = F.normalize(torch.randn((B, 2, H, W), device="cuda", generator=g), dim=1)
    shift = (torch.rand((B, 2), device="cuda", generator=g, dtype=torch.float64) - 0.5) * 12
    angle = (torch.rand((B,), device="cuda", generator=g, dtype=torch.float64) - 0.5) * 30
    return prior, heat, ori, shift, angle


def case(B, n):
    import numpy as np
    import torch
    import torch.nn.functional as F
    from ccvpe_amd import ops, tracking
    prior, heat, ori, shift, angle = scene(B)
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
    nbytes = B * H * W * 4
    res["copy_GBps"] = 2 * nbytes / res["copy_median_us"] / 1e3              # read + write
    res["step_bytes"] = 5 * nbytes
    res["floor_us"] = res["step_bytes"] / res["copy_GBps"] / 1e3
    res["rigid_over_floor"] = res["rigid_median_us"] / res["floor_us"]
    res["translate_over_floor"] = res["translate_median_us"] / res["floor_us"]
    res["rigid_over_translate"] = res["rigid_median_us"] / res["translate_median_us"]
    res["torch_over_rigid_rb"] = res["torch_median_us"] / res["rigid_rb_median_us"]
    return res


def identity(parent_lib):
    """ccvpe_belief_step_f32 of an older library and of this build on the same device buffers: equal bits."""
    import ctypes
    import torch
    from ccvpe_amd import _lib, ops, tracking
    B = 2
    prior, heat, ori, shift, _ = scene(B)
    offsets, taps = tracking.motion_taps(shift, 2.5, R)
    new = _lib.load()
    old = ctypes.CDLL(parent_lib)
    restype, argtypes = _lib.PROTOTYPES["ccvpe_belief_step_f32"]
    old.ccvpe_belief_step_f32.restype, old.ccvpe_belief_step_f32.argtypes = restype, argtypes
    out = []
    for lib in (old, new):
        post = torch.zeros_like(prior)
        scratch = torch.zeros((B * ops.belief_partials(H, W),), device="cuda", dtype=torch.float64)
        rows = torch.zeros((B, 14), device="cuda", dtype=torch.float64)
        rc = lib.ccvpe_belief_step_f32(prior.data_ptr(), heat.data_ptr(), ori.data_ptr(), offsets.data_ptr(), taps.data_ptr(), R, ALPHA,
                                       None, post.data_ptr(), scratch.data_ptr(), rows.data_ptr(), B, H, W, None)
        torch.cuda.synchronize()
        if rc != 0:
            raise RuntimeError("ccvpe_belief_step_f32 returned %d" % rc)
        out.append((post.cpu(), rows.cpu()))
    same_post = bool(torch.equal(out[0][0].view(torch.int32), out[1][0].view(torch.int32)))
    same_rows = bool(torch.equal(out[0][1].view(torch.int64), out[1][1].view(torch.int64)))
    return {"post_bit_identical": same_post, "rows_bit_identical": same_rows, "post_sum": float(out[1][0].double().sum())}


def child(step_args, seconds, env=None, script=None):
    """one GPU step as a process of its own under `timeout`; returns its last stdout line as JSON"""
    cmd = ["timeout", "-k", "10", str(seconds), sys.executable, script or os.path.abspath(__file__)] + step_args
    run = subprocess.run(cmd, stdout=subprocess.PIPE, env=env, cwd=ROOT)
    if run.returncode != 0:
        raise SystemExit("step %s ended with status %d: stopping here" % (" ".join(step_args), run.returncode))
    return json.loads(run.stdout.decode().strip().splitlines()[-1])


if args.leg == "case":
    print(json.dumps(case(args.batch, 2000 if args.batch == 1 else 200)))
elif args.leg == "identity":
    print(json.dumps(identity(args.parent_lib)))
else:
    out = {"shape": [H, W], "radius": R, "cases": [child(["--leg", "case", "--batch", "1"], 240),
                                                   child(["--leg", "case", "--batch", "64"], 240)]}
    if args.parent_lib:
        parent = os.path.abspath(args.parent_lib)
        out["translate_step_vs_parent"] = child(["--leg", "identity", "--parent-lib", parent], 120)
        if args.bench:
            bench = ["--gpus", "1", "--steps", "10", "--warmup", "3", "--no-cpu-baseline"]
            old_env = dict(os.environ, CCVPE_LIB=parent, CCVPE_LIB_ALLOW_MISSING="1")
            out["bench"] = {"this_build": child(bench, 400, script=os.path.join(ROOT, "bench.py")),
                            "parent_lib": child(bench, 400, env=old_env, script=os.path.join(ROOT, "bench.py"))}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "track_rigid_timing.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
