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

Every GPU step is a child process under its own `timeout`; the first step that fails ends the run.  With --parent-lib, the four
existing step entry points (forward and backward, translate and rigid) at 512 x 512 are run through that older library and
through this build in one process and every output is compared bit for bit (the second template flag of the shared passes
must not change them); with --bench, bench.py is then run against this build and against the older library.  Writes
track_path_timing.json into --out."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=".")
ap.add_argument("--parent-lib", default=None, help="an older libccvpe_hip.so: bit-compare the four existing step entry points against it")
ap.add_argument("--bench", action="store_true", help="with --parent-lib: bench.py against this build and against the older library")
ap.add_argument("--leg", choices=["step", "backtrack", "identity"], default=None, help="(internal) one child step")
ap.add_argument("--batch", type=int, default=1)
args = ap.parse_args()
H = W = 512
R, ALPHA, FRAMES = 8, 0.02, 64


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
    return e0.elapsed_time(e1) * 1000.0 / n          # microseconds per call


def scene(B):
    import torch
    import torch.nn.functional as F
    g = torch.Generator(device="cuda").manual_seed(B)
    maps = [torch.softmax(torch.randn((B, H * W), device="cuda", generator=g) * 4, 1).reshape(B, 1, H, W) for _ in range(3)]
    ori = F.normalize(torch.randn((B, 2, H, W), device="cuda", generator=g), dim=1)
    shift = (torch.rand((B, 2), device="cuda", generator=g, dtype=torch.float64) - 0.5) * 12
    angle = (torch.rand((B,), device="cuda", generator=g, dtype=torch.float64) - 0.5) * 30
    return maps[0], maps[1], maps[2], ori, shift, angle


def medians(res, legs, n, slow=()):
    import numpy as np
    for k in legs:
        res[k + "_us"] = []
    for _ in range(3):
        for k, fn in legs.items():
            res[k + "_us"].append(timed(fn, max(10, n // 10) if k in slow else n, 5 if k in slow else 20))
    for k in legs:
        res[k + "_median_us"] = float(np.median(res[k + "_us"]))


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
    nbytes = B * H * W * 4
    res["copy_GBps"] = 2 * nbytes / res["copy_median_us"] / 1e3              # read + write
    res["step_bytes"] = 5 * nbytes                                           # prev and heat read, U written, read, written
    res["floor_us"] = res["step_bytes"] / res["copy_GBps"] / 1e3
    res["viterbi_over_floor"] = res["viterbi_median_us"] / res["floor_us"]
    res["viterbi_over_forward"] = res["viterbi_median_us"] / res["forward_median_us"]
    res["torch_over_viterbi_rb"] = res["torch_median_us"] / res["viterbi_rb_median_us"]
    return res


def backtrack_case(B, n):
    import torch
    import torch.nn.functional as F
    from ccvpe_amd import ops, tracking
    g = torch.Generator(device="cuda").manual_seed(100 + B)
    heat = torch.empty((FRAMES, B, H, W), device="cuda")
    ori = torch.empty((FRAMES, B, 2, H, W), device="cuda")
    for t in range(FRAMES):                                                  # frame by frame: no 2x temporaries of the whole drive
        heat[t] = torch.softmax(torch.randn((B, H * W), device="cuda", generator=g) * 4, 1).reshape(B, H, W)
        ori[t] = F.normalize(torch.randn((B, 2, H, W), device="cuda", generator=g), dim=1)
    shift = (torch.rand((FRAMES, B, 2), device="cuda", generator=g, dtype=torch.float64) - 0.5) * 12
    mlp = tracking.MostLikelyPath((H, W), sigma_px=2.5, radius=R, outlier=ALPHA)
    out = mlp.run(heat, ori, shift)
    offsets, taps = tracking.motion_taps(shift.reshape(-1, 2), 2.5, R)
    offsets, taps = offsets.reshape(FRAMES, B, 2), taps.reshape(FRAMES, B, 2, -1)
    path = torch.empty((FRAMES, B, 8), device="cuda", dtype=torch.float64)
    reset = torch.zeros((FRAMES, B), device="cuda", dtype=torch.int32)
    reset[0] = 1
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


def identity(parent_lib):
    """The four existing step entry points of an older library and of this build on the same device buffers: equal bits."""
    import ctypes
    import torch
    from ccvpe_amd import _lib, ops, tracking
    old = ctypes.CDLL(parent_lib)
    entries = ("ccvpe_belief_step_f32", "ccvpe_belief_step_rigid_f32", "ccvpe_belief_smooth_step_f32", "ccvpe_belief_smooth_step_rigid_f32")
    for entry in entries:
        fn = getattr(old, entry)
        fn.restype, fn.argtypes = _lib.PROTOTYPES[entry]
    B = 2
    beta, heat, prior, ori, shift, angle = scene(B)
    offsets, taps = tracking.motion_taps(shift, 2.5, R)
    _, centred = tracking.motion_taps(torch.zeros_like(shift), 2.5, R)
    motion = torch.from_numpy(tracking.rigid_motion(shift.cpu().numpy(), angle.cpu().numpy(), (H, W))).cuda()
    out = {}
    for entry in entries:
        move, k = (motion, centred) if "rigid" in entry else (offsets, taps)
        got = []
        for lib in (old, _lib.load()):
            maps = [torch.zeros_like(prior), torch.zeros_like(prior)]
            scratch = torch.zeros((B * ops.belief_partials(H, W),), device="cuda", dtype=torch.float64)
            rows = torch.zeros((B, 14), device="cuda", dtype=torch.float64)
            p = lambda t: t.data_ptr()
            if "smooth" in entry:
                rc = getattr(lib, entry)(p(beta), p(heat), p(prior), p(ori), p(move), p(k), R, ALPHA, None, p(maps[0]), p(maps[1]),
                                         p(scratch), p(rows), B, H, W, None)
            else:
                rc = getattr(lib, entry)(p(prior), p(heat), p(ori), p(move), p(k), R, ALPHA, None, p(maps[0]), p(scratch), p(rows), B,
                                         H, W, None)
            if rc != 0:
                raise RuntimeError("%s returned %d" % (entry, rc))
            torch.cuda.synchronize()
            got.append((maps[0].cpu(), maps[1].cpu(), rows.cpu()))
        out[entry] = {"maps_bit_identical": bool(torch.equal(got[0][0].view(torch.int32), got[1][0].view(torch.int32)) and
                                                 torch.equal(got[0][1].view(torch.int32), got[1][1].view(torch.int32))),
                      "rows_bit_identical": bool(torch.equal(got[0][2].view(torch.int64), got[1][2].view(torch.int64))),
                      "map_sum": float(got[1][0].double().sum())}
    return out


def child(step_args, seconds, env=None, script=None):
    """one GPU step as a process of its own under `timeout`; returns its last stdout line as JSON"""
    cmd = ["timeout", "-k", "10", str(seconds), sys.executable, script or os.path.abspath(__file__)] + step_args
    run = subprocess.run(cmd, stdout=subprocess.PIPE, env=env, cwd=ROOT)
    if run.returncode != 0:
        raise SystemExit("step %s ended with status %d: stopping here" % (" ".join(step_args), run.returncode))
    return json.loads(run.stdout.decode().strip().splitlines()[-1])


if args.leg == "step":
    print(json.dumps(step_case(args.batch, 2000 if args.batch == 1 else 200)))
elif args.leg == "backtrack":
    print(json.dumps(backtrack_case(args.batch, 200)))
elif args.leg == "identity":
    print(json.dumps(identity(args.parent_lib)))
else:
    parent = os.path.abspath(args.parent_lib) if args.parent_lib else None
    out = {"shape": [H, W], "radius": R,
           "step": [child(["--leg", "step", "--batch", "1"], 240), child(["--leg", "step", "--batch", "64"], 240)],
           "backtrack": [child(["--leg", "backtrack", "--batch", "1"], 240), child(["--leg", "backtrack", "--batch", "64"], 300)]}
    if parent:
        out["existing_steps_vs_parent"] = child(["--leg", "identity", "--parent-lib", parent], 120)
        if args.bench:
            bench = ["--gpus", "1", "--steps", "10", "--warmup", "3", "--no-cpu-baseline"]
            old_env = dict(os.environ, CCVPE_LIB=parent, CCVPE_LIB_ALLOW_MISSING="1")
            out["bench"] = {"this_build": child(bench, 400, script=os.path.join(ROOT, "bench.py")),
                            "parent_lib": child(bench, 400, env=old_env, script=os.path.join(ROOT, "bench.py"))}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "track_path_timing.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
