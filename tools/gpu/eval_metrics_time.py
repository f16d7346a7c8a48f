"""ccvpe_eval_metrics_f32 beside ccvpe_eval_postprocess_f32 at B = 64, 512 x 512: three alternating runs each, device events
around N back-to-back launches, median of the three per-launch times (DESIGN.md section 4 quotes them; a figure, not a gate):

    python tools/gpu/eval_metrics_time.py [--out DIR]

Writes eval_metrics_timing.json into --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
from ccvpe_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=".")
args = ap.parse_args()
B, H, W, N = 64, 512, 512, 1000
g = torch.Generator(device="cuda").manual_seed(1)
heat = torch.softmax(torch.randn((B, H * W), device="cuda", generator=g) * 3, 1).reshape(B, 1, H, W)
gt = torch.rand((B, 1, H, W), device="cuda", generator=g)
ori = torch.nn.functional.normalize(torch.randn((B, 2, H, W), device="cuda", generator=g), dim=1)
gto = torch.nn.functional.normalize(torch.randn((B, 2, H, W), device="cuda", generator=g), dim=1)
hd = torch.rand((B,), device="cuda", dtype=torch.float64) * 360
mpp = torch.full((B,), 0.1958, device="cuda", dtype=torch.float64)
rows = torch.empty((B, 12), device="cuda", dtype=torch.float64)


def run_metrics():
    ops.eval_metrics(heat, ori, gt, gto, hd, mpp, out=rows)


def run_post():
    ops.eval_postprocess(heat, ori)


def timed(fn):
    for _ in range(50):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / N          # microseconds per launch


res = {"metrics_us": [], "post_us": []}
for _ in range(3):
    res["metrics_us"].append(timed(run_metrics))
    res["post_us"].append(timed(run_post))
res["metrics_median_us"] = float(np.median(res["metrics_us"]))
res["post_median_us"] = float(np.median(res["post_us"]))
res["ratio"] = res["metrics_median_us"] / res["post_median_us"]
res["shape"] = [B, H, W]
res["launches_per_run"] = N
res["bytes_read_metrics"] = 2 * B * H * W * 4
res["bytes_read_post"] = B * H * W * 4
res["metrics_GBps"] = res["bytes_read_metrics"] / res["metrics_median_us"] / 1e3
res["post_GBps"] = res["bytes_read_post"] / res["post_median_us"] / 1e3
os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, "eval_metrics_timing.json"), "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
