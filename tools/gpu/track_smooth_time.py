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

Every GPU step is a child process under its own `timeout`; the first step that fails ends the run.  With --parent-lib, one
translate and one rigid forward step at 512 x 512 are run through that older library and through this build in one process and
post and rows are compared bit for bit (sharing the staging, passes and merge with the backward kernels must not change
ccvpe_belief_step_f32 or ccvpe_belief_step_rigid_f32), and the forward step is timed through both libraries; with --bench,
bench.py is then run against this build and against the older library.  Writes track_smooth_timing.json into --out."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=".")
ap.add_argument("--parent-lib", default=None, help="an older libccvpe_hip.so: bit-compare both forward step entry points against it")
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
    maps = [torch.softmax(torch.randn((B, H * W), device="cuda", generator=g) * 4, 1).reshape(B, 1, H, W) for _ in range(3)]
    ori = F.normalize(torch.randn((B, 2, H, W), device="cuda", generator=g), dim=1)
    shift = (torch.rand((B, 2), device="cuda", generator=g, dtype=torch.float64) - 0.5) * 12
    angle = (torch.rand((B,), device="cuda", generator=g, dtype=torch.float64) - 0.5) * 30
    return maps[0], maps[1], maps[2], ori, shift, angle


def forward_call(lib, entry, prior, heat, ori, move, taps, post, scratch, rows, B):
    rc = getattr(lib, entry)(prior.data_ptr(), heat.data_ptr(), ori.data_ptr(), move.data_ptr(), taps.data_ptr(), R, ALPHA, None,
                             post.data_ptr(), scratch.data_ptr(), rows.data_ptr(), B, H, W, None)
    if rc != 0:
        raise RuntimeError("%s returned %d" % (entry, rc))


def old_library(parent_lib):
    import ctypes
    from ccvpe_amd import _lib
    old = ctypes.CDLL(parent_lib)
    for entry in ("ccvpe_belief_step_f32", "ccvpe_belief_step_rigid_f32"):
        fn = getattr(old, entry)
        fn.restype, fn.argtypes = _lib.PROTOTYPES[entry]
    return old


def case(B, n, parent_lib):
    import numpy as np
    import torch
    import torch.nn.functional as F
    from ccvpe_amd import _lib, ops, tracking
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
        old = old_library(parent_lib)
        legs["forward_parent_lib"] = lambda: forward_call(old, "ccvpe_belief_step_f32", alpha, heat, ori, offsets, taps, post, scratch, rows, B)
        new = _lib.load()
        legs["forward_raw_call"] = lambda: forward_call(new, "ccvpe_belief_step_f32", alpha, heat, ori, offsets, taps, post, scratch, rows, B)
    src, dst = torch.empty_like(beta), torch.empty_like(beta)
    legs["copy"] = lambda: dst.copy_(src)
    for k in list(legs) + ["torch"]:
        res[k + "_us"] = []
    for _ in range(3):
        for k, fn in legs.items():
            res[k + "_us"].append(timed(fn, n, 20))
        res["torch_us"].append(timed(composed, max(10, n // 10), 5))
    for k in list(legs) + ["torch"]:
        res[k + "_median_us"] = float(np.median(res[k + "_us"]))
    nbytes = B * H * W * 4
    res["copy_GBps"] = 2 * nbytes / res["copy_median_us"] / 1e3              # read + write
    res["step_bytes"] = 9 * nbytes
    res["floor_us"] = res["step_bytes"] / res["copy_GBps"] / 1e3
    res["smooth_over_floor"] = res["smooth_median_us"] / res["floor_us"]
    res["smooth_over_forward"] = res["smooth_median_us"] / res["forward_median_us"]
    res["smooth_rigid_over_forward"] = res["smooth_rigid_median_us"] / res["forward_median_us"]
    res["torch_over_smooth_rb"] = res["torch_median_us"] / res["smooth_rb_median_us"]
    if parent_lib:
        res["forward_raw_call_over_parent_lib"] = res["forward_raw_call_median_us"] / res["forward_parent_lib_median_us"]
    return res


def identity(parent_lib):
    """Both forward step entry points of an older library and of this build on the same device buffers: equal bits."""
    import torch
    from ccvpe_amd import _lib, ops, tracking
    B = 2
    _, heat, prior, ori, shift, angle = scene(B)
    offsets, taps = tracking.motion_taps(shift, 2.5, R)
    _, centred = tracking.motion_taps(torch.zeros_like(shift), 2.5, R)
    motion = torch.from_numpy(tracking.rigid_motion(shift.cpu().numpy(), angle.cpu().numpy(), (H, W))).cuda()
    out = {}
    for entry, move, k in (("ccvpe_belief_step_f32", offsets, taps), ("ccvpe_belief_step_rigid_f32", motion, centred)):
        got = []
        for lib in (old_library(parent_lib), _lib.load()):
            post = torch.zeros_like(prior)
            scratch = torch.zeros((B * ops.belief_partials(H, W),), device="cuda", dtype=torch.float64)
            rows = torch.zeros((B, 14), device="cuda", dtype=torch.float64)
            forward_call(lib, entry, prior, heat, ori, move, k, post, scratch, rows, B)
            torch.cuda.synchronize()
            got.append((post.cpu(), rows.cpu()))
        out[entry] = {"post_bit_identical": bool(torch.equal(got[0][0].view(torch.int32), got[1][0].view(torch.int32))),
                      "rows_bit_identical": bool(torch.equal(got[0][1].view(torch.int64), got[1][1].view(torch.int64))),
                      "post_sum": float(got[1][0].double().sum())}
    return out


def child(step_args, seconds, env=None, script=None):
    """one GPU step as a process of its own under `timeout`; returns its last stdout line as JSON"""
    cmd = ["timeout", "-k", "10", str(seconds), sys.executable, script or os.path.abspath(__file__)] + step_args
    run = subprocess.run(cmd, stdout=subprocess.PIPE, env=env, cwd=ROOT)
    if run.returncode != 0:
        raise SystemExit("step %s ended with status %d: stopping here" % (" ".join(step_args), run.returncode))
    return json.loads(run.stdout.decode().strip().splitlines()[-1])


if args.leg == "case":
    print(json.dumps(case(args.batch, 2000 if args.batch == 1 else 200, args.parent_lib)))
elif args.leg == "identity":
    print(json.dumps(identity(args.parent_lib)))
else:
    parent = os.path.abspath(args.parent_lib) if args.parent_lib else None
    extra = ["--parent-lib", parent] if parent else []
    out = {"shape": [H, W], "radius": R, "cases": [child(["--leg", "case", "--batch", "1"] + extra, 240),
                                                   child(["--leg", "case", "--batch", "64"] + extra, 240)]}
    if parent:
        out["forward_steps_vs_parent"] = child(["--leg", "identity", "--parent-lib", parent], 120)
        if args.bench:
            bench = ["--gpus", "1", "--steps", "10", "--warmup", "3", "--no-cpu-baseline"]
            old_env = dict(os.environ, CCVPE_LIB=parent, CCVPE_LIB_ALLOW_MISSING="1")
            out["bench"] = {"this_build": child(bench, 400, script=os.path.join(ROOT, "bench.py")),
                            "parent_lib": child(bench, 400, env=old_env, script=os.path.join(ROOT, "bench.py"))}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "track_smooth_timing.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
