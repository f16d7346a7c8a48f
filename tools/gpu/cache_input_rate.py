"""VIGOR input side at B = 64 with and without the device image cache (ccvpe_amd/cache.py): samples per second of DeviceBatches
on a synthetic VIGOR tree (1024 x 2048 JPEG panoramas, 640 x 640 PNG tiles)

    (a) without a cache              — decode, upload and resample every sample, every epoch
    (b) with a cache, epoch 1        — the fill: decode + upload + resize into a slot + one gather launch per side
    (c) with the same cache, epoch 2 — all hits: one gather launch per side, no file is opened

and next to them the gather launch alone for both sides against the time of moving its bytes once at the copy rate measured in
the same run (a figure, not a gate), the consumer-thread time per batch of DeviceBatches._to_device without a cache, while
filling and on hits, and the peak device memory of one B = 64 CVM_VIGOR training step (what is left of the HBM is what
`capacity_bytes` can be):

    python tools/gpu/cache_input_rate.py [--out DIR] [--batches 3] [--rounds 3] [--workers 16] [--no-step]

The three runs alternate, `rounds` times each; the medians are what DESIGN.md section 1 quotes.  Writes cache_input_rate.json
into --out."""
import argparse
import io
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
from ccvpe_amd import cache as C, datasets as DS, preprocess                   # noqa: E402

CITIES = ("NewYork", "Seattle", "SanFrancisco", "Chicago")
PANO, TILE = (1024, 2048), 640
GRD_HW, SAT_HW = (320, 640), (512, 512)


def encoded(arr, fmt):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr, "RGB").save(buf, format=fmt, **({"quality": 90} if fmt == "JPEG" else {}))
    return buf.getvalue()


def smooth_image(rng, h, w):
    """Low-frequency colour field + mild noise: decode cost between a flat and a noise image, as a photograph's is."""
    from PIL import Image
    small = (rng.rand(h // 16 + 1, w // 16 + 1, 3) * 255).astype(np.uint8)
    base = np.asarray(Image.fromarray(small, "RGB").resize((w, h), Image.BICUBIC), dtype=np.int16)
    return np.clip(base + rng.randint(-6, 7, size=base.shape), 1, 255).astype(np.uint8)


def make_tree(root, n, distinct=8, seed=0):
    """n samples in the VIGOR layout over the four same-area cities; `distinct` different panoramas / tiles, the rest hard
    links to them under their own names (the cache keys on the path: every sample is its own entry)."""
    rng = np.random.RandomState(seed)
    panos = [encoded(smooth_image(rng, PANO[0], PANO[1]), "JPEG") for _ in range(distinct)]
    tiles = [encoded(smooth_image(rng, TILE, TILE), "PNG") for _ in range(distinct)]
    first = {}
    for ci, city in enumerate(CITIES):
        for d in ("splits_new/" + city, city + "/satellite", city + "/panorama"):
            os.makedirs(os.path.join(root, d))
        ks = list(range(ci, n, len(CITIES)))
        names = []
        for k in ks:
            for kind, blobs, name in (("panorama", panos, "p%06d.jpg" % k), ("satellite", tiles, "s%06d.png" % k)):
                path = os.path.join(root, city, kind, name)
                src = first.setdefault((kind, k % distinct), path)
                if src == path:
                    with open(path, "wb") as f:
                        f.write(blobs[k % distinct])
                else:
                    os.link(src, path)
            names.append(("p%06d.jpg" % k, "s%06d.png" % k))
        with open(os.path.join(root, "splits_new", city, "satellite_list.txt"), "w") as f:
            f.write("".join(s + "\n" for _, s in names))
        rows = ["%s %s\n" % (p, " ".join("%s %f %f" % (names[(j + q) % len(names)][1], 17.0 + q, -9.0 - q) for q in range(4)))
                for j, (p, _) in enumerate(names)]
        for fn in ("same_area_balanced_train.txt", "same_area_balanced_test.txt", "pano_label_balanced.txt"):
            with open(os.path.join(root, "splits_new", city, fn), "w") as f:
                f.write("".join(rows))


def loader_rate(it):
    """Samples per second of one pass; the checksum keeps every batch's tensors alive until they are complete."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n, check = 0, 0.0
    for b in it:
        n += len(b.indices)
        check += float(b.sat[:, :, ::64, ::64].sum()) + float(b.grd[:, :, ::64, ::64].sum())
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


def consumer_ms(fn, reps=3):
    """(host ms until the call returns, ms until the device is done) of fn, medians."""
    host, total = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        host.append((t1 - t0) * 1e3)
        total.append((time.perf_counter() - t0) * 1e3)
    return {"host_ms": statistics.median(host), "with_device_ms": statistics.median(total)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--no-step", action="store_true", help="skip the B = 64 CVM_VIGOR training step")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    B = args.batch
    res = {"batch": B, "batches": args.batches, "rounds": args.rounds, "workers": args.workers, "panorama": PANO, "tile": TILE,
           "device": torch.cuda.get_device_name(0)}
    root = tempfile.mkdtemp(prefix="vigor_rate_")
    try:
        make_tree(root, B * args.batches)
        pairs = lambda: DS.VIGORPairs(root, split="samearea", train=True, seed=1)            # noqa: E731
        kw = dict(device="cuda", workers=args.workers)
        loader_rate(DS.DeviceBatches(pairs(), B, **kw))                                      # warm: code objects, page cache
        runs = {"no_cache": [], "cache_fill": [], "cache_hits": []}
        checks = {}
        cache = C.DeviceImageCache("cuda", 4 << 30)
        for r in range(args.rounds):
            rate, checks["no_cache"] = loader_rate(DS.DeviceBatches(pairs(), B, **kw))
            runs["no_cache"].append(rate)
            cache.clear()
            ds = pairs()
            it = DS.DeviceBatches(ds, B, cache=cache, **kw)
            rate, checks["cache_fill"] = loader_rate(it)
            runs["cache_fill"].append(rate)
            ds._rng = np.random.default_rng(1)                                               # epoch 2 with epoch 1's draws: same checksum
            rate, checks["cache_hits"] = loader_rate(it)
            runs["cache_hits"].append(rate)
            print("round %d: no cache %.1f, fill %.1f, hits %.1f samples/s" % (
                r, runs["no_cache"][-1], runs["cache_fill"][-1], runs["cache_hits"][-1]), flush=True)
        assert checks["no_cache"] == checks["cache_fill"] == checks["cache_hits"], "the paths delivered different batches: %r" % (checks,)
        res["samples_per_s"] = {m: {"runs": v, "median": statistics.median(v), "spread": max(v) - min(v)} for m, v in runs.items()}
        res["cache"] = {"entries": cache.entries, "bytes_used": cache.bytes_used, "bytes_allocated": cache.bytes_allocated,
                        "hits": cache.hits, "misses": cache.misses}
        # the consumer thread's share: _to_device on one decoded batch
        it0 = DS.DeviceBatches(pairs(), B, **kw)
        plain = [it0.pairs.sample(i, SAT_HW, GRD_HW, draws=it0.pairs.draw(i)) for i in range(B)]
        it0._to_device(plain)
        res["to_device"] = {"no_cache": consumer_ms(lambda: it0._to_device(plain))}
        from concurrent.futures import ThreadPoolExecutor
        itc = DS.DeviceBatches(pairs(), B, cache=cache, **kw)
        with ThreadPoolExecutor(max_workers=args.workers) as pool:
            host, total = [], []
            for _ in range(3):                                   # the decode is outside the timed part
                cache.clear()
                miss = itc._decode_batch_cached(pool, np.arange(B), [itc.pairs.draw(i) for i in range(B)])
                m = consumer_ms(lambda: itc._to_device(miss), reps=1)
                host.append(m["host_ms"])
                total.append(m["with_device_ms"])
            res["to_device"]["cache_fill"] = {"host_ms": statistics.median(host), "with_device_ms": statistics.median(total)}
            hit = itc._decode_batch_cached(pool, np.arange(B), [itc.pairs.draw(i) for i in range(B)])
        assert all(s["grd_u8"] is None and s["sat_u8"] is None for s in hit)
        res["to_device"]["cache_hits"] = consumer_ms(lambda: itc._to_device(hit))
        print("_to_device per batch: %s" % json.dumps(res["to_device"]), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    cache.clear()
    # the gather launch alone, both sides, next to one pass over its bytes at the measured copy rate
    big = torch.empty((1 << 30,), device="cuda", dtype=torch.uint8)
    big2 = torch.empty_like(big)
    copy_ms = event_ms(lambda: big2.copy_(big))
    hbm = 2.0 * big.numel() / (copy_ms * 1e-3)                                   # a copy reads and writes every byte
    del big, big2
    res["copy_gb_per_s"] = hbm / 1e9
    res["gather_launch"] = {}
    for side, (h, w) in (("grd", GRD_HW), ("sat", SAT_HW)):
        slots = torch.randint(0, 256, (B, h, w, 3), device="cuda", dtype=torch.uint8)
        table = torch.tensor([slots.data_ptr() + i * h * w * 3 for i in range(B)], dtype=torch.int64, device="cuda")
        rolls = torch.randint(0, w, (B,), device="cuda", dtype=torch.int32) if side == "grd" else torch.zeros((B,), device="cuda", dtype=torch.int32)
        dst = torch.empty((B, 3, h, w), device="cuda")
        ms = event_ms(lambda: preprocess.gather_norm(table, rolls, (h, w), dst=dst))
        nbytes = 15.0 * B * h * w                                                # 3 B read + 12 B written per pixel
        res["gather_launch"][side] = {"ms": ms, "bytes": nbytes, "floor_ms": nbytes / hbm * 1e3, "launch_over_floor": ms / (nbytes / hbm * 1e3),
                                      "gb_per_s": nbytes / (ms * 1e-3) / 1e9}
        print("gather %s: %.3f ms for %.0f MB (%.0f GB/s); once at the copy rate (%.0f GB/s): %.3f ms" % (
            side, ms, nbytes / 1e6, nbytes / (ms * 1e-3) / 1e9, hbm / 1e9, nbytes / hbm * 1e3), flush=True)
        del slots, dst
    if not args.no_step:
        import bench
        from ccvpe_amd import models, synth
        dev = torch.device("cuda:0")
        torch.cuda.empty_cache()
        net = models.CVM_VIGOR(dev, True)
        net.load_state_dict(synth.synthetic_state_dict("vigor", 0), strict=True)
        net = net.to(dev).train()
        grd, sat = synth.synthetic_pair(B, "vigor", 1234, device=dev)
        steps = 4
        m = bench.train_measure(net, grd, sat, dev, B, steps, 2, 0, 20)
        ms = m["elapsed"] / steps * 1e3
        total = torch.cuda.get_device_properties(0).total_memory
        res["train_step"] = {"ms": ms, "pairs_per_s": B / ms * 1e3, "max_memory_allocated_bytes": int(m["peak_gib"] * 2 ** 30),
                             "max_memory_allocated_gib": m["peak_gib"], "device_total_gib": total / 2 ** 30}
        print("CVM_VIGOR B = %d fp32 training step %.1f ms (%.0f pairs/s), peak %.1f GiB of %.0f GiB" % (
            B, ms, B / ms * 1e3, m["peak_gib"], total / 2 ** 30), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "cache_input_rate.json"), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res["samples_per_s"]))


if __name__ == "__main__":
    main()
