"""What the four tools/gpu/track_*_time.py share: the scene, the timing loop, the child-process runner, and the two checks of
this build against an older library (both loaded in one process through ctypes, same device buffers):

    python tools/gpu/track_common.py --leg identity --parent-lib OLD/libccvpe_hip.so
    python tools/gpu/track_common.py --leg versus --parent-lib OLD/libccvpe_hip.so --batch B

  identity   all six belief entry points, every output compared bit for bit: the five steps at 512 x 512, R = 8 and at 20 x 70,
             R = 3 (w % 4 != 0: the scalar forms), B = 2 with track 1's reset / cut flag set; the backtrack on the maps of a
             six-frame MostLikelyPath.run at both shapes, one track restarting half-way
  versus     all six entry points timed through the older library and through this build alternately, 512 x 512, R = 8 (T = 64
             for the backtrack): three rounds, medians, and the older library's own round-to-round spread (max - min) per leg
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
H = W = 512
R, ALPHA, FRAMES = 8, 0.02, 64
STEPS = ("ccvpe_belief_step_f32", "ccvpe_belief_step_rigid_f32", "ccvpe_belief_viterbi_step_f32", "ccvpe_belief_smooth_step_f32",
         "ccvpe_belief_smooth_step_rigid_f32")
BACKTRACK = "ccvpe_belief_backtrack_f32"
BENCH = ["--gpus", "1", "--steps", "10", "--warmup", "3", "--no-cpu-baseline"]


def parser(legs):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--parent-lib", default=None, help="an older libccvpe_hip.so: bit-compare and time the belief entry points against it")
    ap.add_argument("--bench", action="store_true", help="with --parent-lib: bench.py against this build and against the older library")
    ap.add_argument("--leg", choices=legs, default=None, help="(internal) one child step")
    ap.add_argument("--batch", type=int, default=1)
    return ap


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


def scene(B, h=H, w=W):
    """Three softmax maps [B,1,h,w], a unit orientation field, shifts of -6 .. 6 px and turns of -15 .. 15 degrees per track."""
    import torch
    import torch.nn.functional as F
    g = torch.Generator(device="cuda").manual_seed(B)
    maps = [torch.softmax(torch.randn((B, h * w), device="cuda", generator=g) * 4, 1).reshape(B, 1, h, w) for _ in range(3)]
    ori = F.normalize(torch.randn((B, 2, h, w), device="cuda", generator=g), dim=1)
    shift = (torch.rand((B, 2), device="cuda", generator=g, dtype=torch.float64) - 0.5) * 12
    angle = (torch.rand((B,), device="cuda", generator=g, dtype=torch.float64) - 0.5) * 30
    return maps[0], maps[1], maps[2], ori, shift, angle


def drive(B, frames, h=H, w=W, radius=R, starts=None):
    """Random maps of a drive through one MostLikelyPath.run, and the backtrack's own inputs."""
    import torch
    import torch.nn.functional as F
    from ccvpe_amd import tracking
    g = torch.Generator(device="cuda").manual_seed(100 + B)
    heat = torch.empty((frames, B, h, w), device="cuda")
    ori = torch.empty((frames, B, 2, h, w), device="cuda")
    for t in range(frames):                                                  # frame by frame: no 2x temporaries of the whole drive
        heat[t] = torch.softmax(torch.randn((B, h * w), device="cuda", generator=g) * 4, 1).reshape(B, h, w)
        ori[t] = F.normalize(torch.randn((B, 2, h, w), device="cuda", generator=g), dim=1)
    shift = (torch.rand((frames, B, 2), device="cuda", generator=g, dtype=torch.float64) - 0.5) * 12
    mlp = tracking.MostLikelyPath((h, w), sigma_px=2.5, radius=radius, outlier=ALPHA)
    out = mlp.run(heat, ori, shift, starts=starts)
    offsets, taps = tracking.motion_taps(shift.reshape(-1, 2), 2.5, radius)
    reset = torch.zeros((frames, B), device="cuda", dtype=torch.int32)
    if starts is not None:
        reset.copy_(torch.as_tensor(starts, dtype=torch.int32))
    reset[0] = 1
    return dict(heat=heat, ori=ori, shift=shift, mlp=mlp, out=out, offsets=offsets.reshape(frames, B, 2),
                taps=taps.reshape(frames, B, 2, -1), reset=reset)


def medians(res, legs, n, slow=()):
    """three rounds over `legs` in turn (so the legs alternate); per-call microseconds and their medians into `res`"""
    import numpy as np
    for k in legs:
        res[k + "_us"] = []
    for _ in range(3):
        for k, fn in legs.items():
            res[k + "_us"].append(timed(fn, max(10, n // 10) if k in slow else n, 5 if k in slow else 20))
    for k in legs:
        res[k + "_median_us"] = float(np.median(res[k + "_us"]))


def floor(res, B, passes):
    """one pass over the step's bytes (`passes` B h w 4) at the device-to-device copy rate of res["copy_median_us"]"""
    nbytes = B * H * W * 4
    res["copy_GBps"] = 2 * nbytes / res["copy_median_us"] / 1e3              # read + write
    res["step_bytes"] = passes * nbytes
    res["floor_us"] = res["step_bytes"] / res["copy_GBps"] / 1e3


def child(script, step_args, seconds, env=None):
    """one GPU step as a process of its own under `timeout`; returns its last stdout line as JSON"""
    cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(script)] + step_args
    run = subprocess.run(cmd, stdout=subprocess.PIPE, env=env, cwd=ROOT)
    if run.returncode != 0:
        raise SystemExit("step %s ended with status %d: stopping here" % (" ".join(step_args), run.returncode))
    print("[done] %s %s" % (os.path.basename(script), " ".join(step_args)), file=sys.stderr, flush=True)
    return json.loads(run.stdout.decode().strip().splitlines()[-1])


def against_parent(out, key, parent_lib, bench):
    """out[key]: identity; out["versus_parent"]: versus at B = 1 and 64; with `bench`, out["bench"]: bench.py through both
    libraries, three alternating rounds (the first round's lines, and ms_per_step of every round)."""
    parent = ["--parent-lib", os.path.abspath(parent_lib)]
    out[key] = child(__file__, ["--leg", "identity"] + parent, 240)
    out["versus_parent"] = [child(__file__, ["--leg", "versus", "--batch", b] + parent, 400) for b in ("1", "64")]
    if bench:
        script, runs = os.path.join(ROOT, "bench.py"), {"this_build": [], "parent_lib": []}
        old_env = dict(os.environ, CCVPE_LIB=parent[1], CCVPE_LIB_ALLOW_MISSING="1")
        for _ in range(3):
            runs["parent_lib"].append(child(script, BENCH, 400, env=old_env))
            runs["this_build"].append(child(script, BENCH, 400))
        out["bench"] = {k: v[0] for k, v in runs.items()}
        out["bench"]["ms_per_step"] = {k: [r["ms_per_step"] for r in v] for k, v in runs.items()}


def write(out, directory, name):
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, name), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


def libraries(parent_lib):
    """(the older library with the six prototypes set, this build's)"""
    import ctypes
    from ccvpe_amd import _lib
    old = ctypes.CDLL(parent_lib)
    for entry in STEPS + (BACKTRACK,):
        fn = getattr(old, entry)
        fn.restype, fn.argtypes = _lib.PROTOTYPES[entry]
    return old, _lib.load()


def _p(t):
    return None if t is None else t.data_ptr()


class StepCase(object):
    """The inputs of the five step entry points at one shape, and output buffers: call(lib, entry) runs one step."""

    def __init__(self, B, h, w, radius, flags=None):
        import torch
        from ccvpe_amd import ops, tracking
        self.a, self.heat, self.c, self.ori, shift, angle = scene(B, h, w)
        self.translate = tracking.motion_taps(shift, 2.5, radius)
        motion = torch.from_numpy(tracking.rigid_motion(shift.cpu().numpy(), angle.cpu().numpy(), (h, w))).cuda()
        self.rigid = (motion, tracking.motion_taps(torch.zeros_like(shift), 2.5, radius)[1])
        self.flags, self.radius, self.dims = flags, radius, (B, h, w)
        self.outs = [torch.zeros_like(self.heat), torch.zeros_like(self.heat)]
        self.scratch = torch.zeros((B * ops.belief_partials(h, w),), device="cuda", dtype=torch.float64)
        self.rows = torch.zeros((B, 14), device="cuda", dtype=torch.float64)

    def call(self, lib, entry):
        back = "smooth" in entry
        move, taps = self.rigid if "rigid" in entry else self.translate
        ins = [self.a, self.heat] + ([self.c] if back else []) + [self.ori, move, taps]
        rc = getattr(lib, entry)(*([_p(t) for t in ins] + [self.radius, ALPHA, _p(self.flags)] +
                                   [_p(t) for t in self.outs[:2 if back else 1]] + [_p(self.scratch), _p(self.rows)] +
                                   list(self.dims) + [None]))
        if rc != 0:
            raise RuntimeError("%s returned %d" % (entry, rc))


def backtrack_call(lib, d, path, radius=R):
    frames, B, _, h, w = d["out"]["deltas"].shape
    rc = getattr(lib, BACKTRACK)(_p(d["out"]["deltas"]), _p(d["ori"]), _p(d["offsets"]), _p(d["taps"]), radius, _p(d["out"]["rows"]),
                                 _p(d["reset"]), _p(path), frames, B, h, w, None)
    if rc != 0:
        raise RuntimeError("%s returned %d" % (BACKTRACK, rc))


def identity(parent_lib):
    import torch
    libs = libraries(parent_lib)
    bits = lambda t, dt: t.cpu().contiguous().view(dt)
    out = {}
    for h, w, radius in ((H, W, R), (20, 70, 3)):
        case = StepCase(2, h, w, radius, flags=torch.tensor([0, 1], dtype=torch.int32, device="cuda"))
        for entry in STEPS:
            got = []
            for lib in libs:
                for t in case.outs + [case.scratch, case.rows]:
                    t.zero_()
                case.call(lib, entry)
                torch.cuda.synchronize()
                got.append([bits(t, torch.int32) for t in case.outs] + [bits(case.rows, torch.int64)])
            out["%s %dx%d" % (entry, h, w)] = {"maps_bit_identical": torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]),
                                               "rows_bit_identical": torch.equal(got[0][2], got[1][2]),
                                               "map_sum": float(case.outs[0].double().sum())}
        d = drive(2, 6, h, w, radius, starts=[[0, 0], [0, 0], [0, 0], [0, 1], [0, 0], [0, 0]])
        paths = [torch.zeros((6, 2, 8), device="cuda", dtype=torch.float64) for _ in libs]
        for lib, path in zip(libs, paths):
            backtrack_call(lib, d, path, radius)
        torch.cuda.synchronize()
        out["%s %dx%d" % (BACKTRACK, h, w)] = {"path_bit_identical": torch.equal(bits(paths[0], torch.int64), bits(paths[1], torch.int64)),
                                               "same_path_as_run": torch.equal(paths[1], d["out"]["path"])}
    out["all_bit_identical"] = all(v for r in out.values() for k, v in r.items() if k != "map_sum")
    return out


def versus(parent_lib, B):
    import torch
    old, new = libraries(parent_lib)
    case, d = StepCase(B, H, W, R), drive(B, FRAMES)
    path = torch.empty((FRAMES, B, 8), device="cuda", dtype=torch.float64)
    legs = {}
    for entry in STEPS:
        for tag, lib in (("parent", old), ("this", new)):
            legs["%s %s" % (entry, tag)] = lambda lib=lib, entry=entry: case.call(lib, entry)
    for tag, lib in (("parent", old), ("this", new)):
        legs["%s %s" % (BACKTRACK, tag)] = lambda lib=lib: backtrack_call(lib, d, path)
    res = {"B": B, "calls_per_round": 2000 if B == 1 else 200}
    medians(res, legs, res["calls_per_round"])
    for entry in STEPS + (BACKTRACK,):
        spread = max(res[entry + " parent_us"]) - min(res[entry + " parent_us"])
        over = res[entry + " this_median_us"] - res[entry + " parent_median_us"]
        res[entry] = {"parent_spread_us": spread, "this_minus_parent_us": over, "within_parent_spread": over <= spread}
    return res


if __name__ == "__main__":
    args = parser(["identity", "versus"]).parse_args()
    print(json.dumps(identity(args.parent_lib) if args.leg == "identity" else versus(args.parent_lib, args.batch)))
