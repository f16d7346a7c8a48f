"""Oxford RobotCar input side at B = 64: samples per second of DeviceBatches with the aerial patch cut on the host (Pillow crop
of the one large map, 1.92 MB upload and two resize launches per sample) against the device-resident map
(OxfordPairs(device_map=True): a [B, 2] origins table and ONE ccvpe_window_resize_norm_u8_f32 launch per batch), each without and
with the camera images in a DeviceImageCache (second epoch):

    python tools/gpu/oxford_input_rate.py [--out DIR] [--batches 3] [--rounds 3] [--workers 16] [--map 12000]

The synthetic tree: a 12000 x 12000 RGB map (432 MB, stored uncompressed) with the vehicles spread uniformly over it, so the 192
training windows of a pass (1.92 MB each, 369 MB) are not resident in the 256 MiB Infinity Cache; 1280 x 960 PNG camera images.
The four legs alternate, `rounds` times each, every pass with the same seeded draws, and must deliver the same checksum.  Next to
them: the launch alone by device events beside the time of reading each window's bytes once and writing the fp32 batch once at the
copy rate measured here (a figure, not a gate), and `_to_device` on the consumer thread for both aerial paths.
Writes oxford_input_rate.json into --out."""
import argparse
import io
import json
import os
import random
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
from ccvpe_amd import cache as C, datasets as DS, preprocess       # noqa: E402

CAMERA = (960, 1280)
GRD_HW, SAT_HW, BOX = (154, 231), (512, 512), DS.OXFORD_BOX
LEGS = ("host_crop", "device_map", "host_crop_grd_cache_epoch2", "device_map_grd_cache_epoch2")


def smooth_image(rng, h, w):
    """Low-frequency colour field + mild noise: a PNG decode cost between a flat and a noisy image's, as a photograph's is."""
    from PIL import Image
    small = (rng.rand(h // 16 + 1, w // 16 + 1, 3) * 255).astype(np.uint8)
    base = np.asarray(Image.fromarray(small, "RGB").resize((w, h), Image.BICUBIC), dtype=np.int16)
    return np.clip(base + rng.randint(-6, 7, size=base.shape), 1, 255).astype(np.uint8)


def make_tree(root, n, side, distinct=8, seed=0):
    """n training samples in the reference loader's layout.  The map: a random 1000 x 1000 tile repeated, plus a coarse ramp so
    that no two windows are equal; the vehicles: uniform over the map's interior, written as the UTM coordinates the loader's
    affine fit maps back to those pixels."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    g = os.path.join(root, "grd") + "/"
    os.makedirs(g)
    reps = (side + 999) // 1000
    sat = np.tile(rng.randint(0, 200, size=(1000, 1000, 3)).astype(np.uint8), (reps, reps, 1))[:side, :side]
    ramp = (np.arange(side) // 256).astype(np.uint8)
    sat += ramp[:, None, None]
    sat[:, :, 1] += ramp[None, :]
    sat_path = os.path.join(root, "satellite_map_new.bmp")
    Image.fromarray(sat, "RGB").save(sat_path)
    del sat
    src = np.hstack([np.asarray(DS.OXFORD_UTM), np.ones((5, 1))])
    dst = np.hstack([np.asarray(DS.OXFORD_PIX), np.ones((5, 1))])
    affine = np.linalg.lstsq(src, dst, rcond=None)[0]
    pix = rng.uniform(1000, side - 1000, size=(n, 2))                                     # (column, row)
    utm = (pix - affine[2, :2]) @ np.linalg.inv(affine[:2, :2])
    blobs = []
    for k in range(distinct):
        buf = io.BytesIO()
        Image.fromarray(smooth_image(rng, CAMERA[0], CAMERA[1]), "RGB").save(buf, format="PNG")
        blobs.append(buf.getvalue())
    rows = []
    for k in range(n):
        name = "training_%d.png" % k
        if k < distinct:
            with open(g + name, "wb") as f:
                f.write(blobs[k])
        else:
            os.link(g + "training_%d.png" % (k % distinct), g + name)
        rows.append("%s %d %.4f %.4f\n" % (name, 1000 + k, utm[k, 0], utm[k, 1]))
    with open(g + "training.txt", "w") as f:
        f.write("".join(rows))
    np.save(g + "train_yaw.npy", rng.uniform(0, 2 * np.pi, size=n))
    return g, sat_path


class Leg(object):
    """One configuration, kept alive over the rounds: the index (and its resident map), the iterator, the optional cache."""

    def __init__(self, g, sat_path, device_map, grd_cache, batch, workers):
        self.rng = random.Random(1)
        self.pairs = DS.OxfordPairs(g, sat_path, split="train", rng=self.rng, device_map=device_map)
        self.cache = C.DeviceImageCache("cuda", 1 << 30) if grd_cache else None
        self.it = DS.DeviceBatches(self.pairs, batch, device="cuda", workers=workers, grd_hw=GRD_HW, sat_hw=SAT_HW, n_bins=20,
                                   ascending_bins=True, cache=self.cache)

    def one_pass(self):
        """Samples per second of one pass with the draws of seed 1; the checksum keeps every batch alive until it is complete."""
        self.rng.seed(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n, check = 0, 0.0
        for b in self.it:
            n += len(b.indices)
            check += float(b.sat[:, :, ::64, ::64].sum()) + float(b.grd[:, :, ::16, ::16].sum())
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0), check


def event_ms(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def to_device_ms(leg, samples, reps=5):
    """Median host time of DeviceBatches._to_device on one decoded batch: until the call returns / until the device is done."""
    host, done = [], []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = leg.it._to_device(samples)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        del out
        host.append((t1 - t0) * 1e3)
        done.append((t2 - t0) * 1e3)
    return {"host_ms": statistics.median(host[1:]), "device_done_ms": statistics.median(done[1:])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--map", type=int, default=12000, help="side of the synthetic map in pixels")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    n = args.batch * args.batches
    res = {"batch": args.batch, "batches": args.batches, "rounds": args.rounds, "workers": args.workers,
           "map": [args.map, args.map], "map_bytes": args.map * args.map * 3, "window_bytes_per_pass": n * BOX * BOX * 3,
           "camera": list(CAMERA), "device": torch.cuda.get_device_name(0)}
    root = tempfile.mkdtemp(prefix="oxford_rate_")
    try:
        t0 = time.perf_counter()
        g, sat_path = make_tree(root, n, args.map)
        print("tree: %d samples, map %d x %d, %.1f s" % (n, args.map, args.map, time.perf_counter() - t0), flush=True)
        legs = {name: Leg(g, sat_path, "device_map" in name, "cache" in name, args.batch, args.workers) for name in LEGS}
        t0 = time.perf_counter()
        legs["device_map"].pairs.map_on("cuda")
        torch.cuda.synchronize()
        res["map_upload_s"] = time.perf_counter() - t0
        for name in LEGS:                                   # warm: code objects, page cache, the resident maps, the cache's epoch 1
            legs[name].one_pass()
        runs, checks = {name: [] for name in LEGS}, {}
        for r in range(args.rounds):
            for name in LEGS:
                rate, chk = legs[name].one_pass()
                runs[name].append(rate)
                assert checks.setdefault(name, chk) == chk, "%s: the checksum changed between rounds" % name
                print("round %d %-28s %.1f samples/s" % (r, name, rate), flush=True)
        assert len(set(checks.values())) == 1, "the legs delivered different batches: %r" % (checks,)
        res["cache"] = {name: {"entries": legs[name].cache.entries, "hits": legs[name].cache.hits, "misses": legs[name].cache.misses}
                        for name in LEGS[2:]}
        res["checksum"] = checks[LEGS[0]]
        res["samples_per_s"] = {m: {"runs": v, "median": statistics.median(v), "spread": max(v) - min(v)} for m, v in runs.items()}
        verdict = {}
        for host, dev in ((LEGS[0], LEGS[1]), (LEGS[2], LEGS[3])):
            margin = res["samples_per_s"][dev]["median"] - res["samples_per_s"][host]["median"]
            verdict[dev] = {"margin": margin, "host_spread": res["samples_per_s"][host]["spread"],
                            "met": bool(margin > res["samples_per_s"][host]["spread"] and margin > 0)}
        res["condition"] = verdict
        # the consumer thread's share, on one decoded batch of each aerial path
        res["to_device"] = {}
        for name in LEGS[:2]:
            leg = legs[name]
            leg.rng.seed(1)
            draws = [leg.pairs.draw(i) for i in range(args.batch)]
            samples = [leg.pairs.sample(i, SAT_HW, GRD_HW, draws=d) for i, d in enumerate(draws)]
            res["to_device"][name] = to_device_ms(leg, samples)
            if name == "device_map":
                origins = torch.tensor([s["sat_origin"] for s in samples], dtype=torch.int32, device="cuda")
        resident = legs["device_map"].pairs.map_on("cuda")
    finally:
        shutil.rmtree(root, ignore_errors=True)
    # the launch alone
    out = torch.empty((args.batch, 3) + SAT_HW, device="cuda", dtype=torch.float32)
    k_ms = event_ms(lambda: preprocess.window_resize_norm(resident, origins, (BOX, BOX), SAT_HW, dst=out))
    big = torch.empty((1 << 30,), device="cuda", dtype=torch.uint8)
    big2 = torch.empty_like(big)
    copy_ms = event_ms(lambda: big2.copy_(big))
    hbm = 2.0 * big.numel() / (copy_ms * 1e-3)                                   # a copy reads and writes every byte
    del big, big2
    moved = float(args.batch) * (BOX * BOX * 3 + 3 * SAT_HW[0] * SAT_HW[1] * 4)  # each window read once + the fp32 batch written
    res["window_launch"] = {"ms": k_ms, "bytes": moved, "copy_gb_per_s": hbm / 1e9, "bytes_once_ms": moved / hbm * 1e3,
                            "launch_over_bytes_once": k_ms / (moved / hbm * 1e3)}
    print("window launch %.3f ms; its bytes once %.4f ms at %.0f GB/s; _to_device %r" % (
        k_ms, res["window_launch"]["bytes_once_ms"], hbm / 1e9, res["to_device"]), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "oxford_input_rate.json"), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"samples_per_s": res["samples_per_s"], "condition": res["condition"]}))


if __name__ == "__main__":
    main()
