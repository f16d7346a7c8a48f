"""KITTI input side at B = 64 with device-resident aerial maps: samples per second of DeviceBatches on the synthetic KITTI tree of
tools/gpu/kitti_input_rate.py (1280 x 1280 maps, every sample under its own path) in three legs,

    (a) KITTIPairs(device_align=True)                             the path without the map cache
    (b) KITTIPairs(device_align=True, cache_maps=True) + cache    epoch 1: every map decoded, uploaded and retained
    (c) the same iterator again                                   epoch 2: no map or camera image is opened

alternating, `rounds` times each (a fresh cache per round), and next to them the new launch alone (ccvpe_kitti_align_norm_u8_f32
over a table of cache slots) against the two launches it replaces (ccvpe_kitti_align_u8 on a packed upload +
ccvpe_gather_norm_u8_f32 over the crops), the cache's memory per map, and the B = 64 CVM_KITTI training step of the same box:

    python tools/gpu/kitti_map_cache_rate.py [--out DIR] [--batches 3] [--rounds 3] [--workers 16] [--no-step]

Writes kitti_map_cache_rate.json into --out.  Figures, not gates."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from ccvpe_amd import align, cache as C, datasets as DS, preprocess          # noqa: E402
from kitti_input_rate import event_ms, make_tree                             # noqa: E402


def one_pass(it):
    """Samples per second of one pass; the checksum keeps every batch's tensors alive until they are complete."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n, check = 0, 0.0
    for b in it:
        n += len(b.indices)
        check += float(b.sat[:, :, ::64, ::64].sum())
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0), check


def iterator(root, train_file, batch, workers, cache):
    pairs = DS.KITTIPairs(root, train_file, 20, 20, 10, rng=np.random.default_rng(1), device_align=True, cache_maps=cache is not None)
    return DS.DeviceBatches(pairs, batch, device="cuda", workers=workers, grd_hw=(256, 1024), n_bins=16, cache=cache)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--train-lines", type=int, default=20000, help="lines of the training split file, for the extrapolated size")
    ap.add_argument("--no-step", action="store_true", help="skip the B = 64 CVM_KITTI training step")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    res = {"batch": args.batch, "batches": args.batches, "rounds": args.rounds, "workers": args.workers,
           "device": torch.cuda.get_device_name(0)}
    root = tempfile.mkdtemp(prefix="kitti_maps_")
    try:
        n = args.batch * args.batches
        train_file = make_tree(root, n)
        new_cache = lambda: C.DeviceImageCache("cuda", 4 << 30)
        one_pass(iterator(root, train_file, args.batch, args.workers, None))     # warm: code objects, pinned buffer, page cache
        warm = iterator(root, train_file, args.batch, args.workers, new_cache())
        one_pass(warm), one_pass(warm)
        del warm
        runs = {"device_align": [], "cache_maps_epoch1": [], "cache_maps_epoch2": []}
        checks = {k: [] for k in runs}
        for r in range(args.rounds):
            rate, chk = one_pass(iterator(root, train_file, args.batch, args.workers, None))
            runs["device_align"].append(rate), checks["device_align"].append(chk)
            cache = new_cache()
            it = iterator(root, train_file, args.batch, args.workers, cache)
            for leg in ("cache_maps_epoch1", "cache_maps_epoch2"):
                rate, chk = one_pass(it)
                runs[leg].append(rate), checks[leg].append(chk)
            assert cache.misses == 2 * n and cache.hits == 2 * n and cache.entries == 2 * n and not cache.full
            print("round %d  device_align %.1f  fill %.1f  hits %.1f samples/s" % (
                r, runs["device_align"][-1], runs["cache_maps_epoch1"][-1], runs["cache_maps_epoch2"][-1]), flush=True)
        # every first epoch starts from the same seed: the fill leg delivers the parent leg's batches
        assert checks["device_align"] == checks["cache_maps_epoch1"], "the two paths delivered different batches: %r" % (checks,)
        res["samples_per_s"] = {m: {"runs": v, "median": statistics.median(v), "spread": max(v) - min(v)} for m, v in runs.items()}
        map_bytes = cache.bytes_used - n * 256 * 1024 * 3
        res["memory"] = {"maps": n, "map_bytes_used": map_bytes, "bytes_per_map": map_bytes // n, "bytes_allocated": cache.bytes_allocated,
                         "train_lines": args.train_lines, "train_split_gb": map_bytes // n * args.train_lines / 1e9}
        # the launches alone, on one batch of resident maps
        pairs = DS.KITTIPairs(root, train_file, 20, 20, 10, rng=np.random.default_rng(1), device_align=True)
        samples = [pairs.sample(i) for i in range(args.batch)]
    finally:
        shutil.rmtree(root, ignore_errors=True)
    del it, cache
    crop = (DS.KITTI_CROP, DS.KITTI_CROP)
    rows = torch.from_numpy(np.stack([s["align"] for s in samples])).cuda()
    maps = [torch.from_numpy(s["sat_src_u8"]).cuda() for s in samples]           # one allocation per map, as slots of many chunks
    table = torch.tensor([m.data_ptr() for m in maps], dtype=torch.int64, device="cuda")
    dst = torch.empty((args.batch, 3) + crop, device="cuda")
    new_ms = event_ms(lambda: align.kitti_align_norm(table, rows, crop, dst=dst))
    packed = torch.cat([m.reshape(-1) for m in maps])
    sizes = [m.numel() for m in maps]
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)).cuda()
    crops = torch.empty((args.batch,) + crop + (3,), device="cuda", dtype=torch.uint8)
    align_ms = event_ms(lambda: align.kitti_align(packed, offs, rows, crop, out=crops))
    ctable = torch.tensor([crops[i].data_ptr() for i in range(args.batch)], dtype=torch.int64, device="cuda")
    rolls = torch.zeros((args.batch,), dtype=torch.int32, device="cuda")
    dst2 = torch.empty_like(dst)
    gather_ms = event_ms(lambda: preprocess.gather_norm(ctable, rolls, crop, dst=dst2))
    both_ms = event_ms(lambda: (align.kitti_align(packed, offs, rows, crop, out=crops), preprocess.gather_norm(ctable, rolls, crop, dst=dst2)))
    assert torch.equal(dst, dst2), "one launch and two launches disagree"
    res["launch"] = {"align_norm_ms": new_ms, "align_u8_ms": align_ms, "gather_norm_ms": gather_ms, "align_u8_then_gather_ms": both_ms}
    print("align_norm %.3f ms; align_u8 %.3f ms + gather %.3f ms (back to back %.3f ms)" % (new_ms, align_ms, gather_ms, both_ms), flush=True)
    del maps, packed, crops, dst, dst2
    if not args.no_step:
        import bench
        from ccvpe_amd import models, synth
        dev = torch.device("cuda:0")
        net = models.CVM_KITTI("cuda")
        net.load_state_dict(synth.synthetic_state_dict("kitti", 0), strict=True)
        net = net.to(dev).train()
        grd, sat = synth.synthetic_pair(args.batch, "kitti", 1234, device=dev)
        steps = 6
        m = bench.train_measure(net, grd, sat, dev, args.batch, steps, 3, 0, 16)
        ms = m["elapsed"] / steps * 1e3
        res["train_step"] = {"ms": ms, "pairs_per_s": args.batch / ms * 1e3}
        res["epoch2_over_train_step"] = res["samples_per_s"]["cache_maps_epoch2"]["median"] / res["train_step"]["pairs_per_s"]
        print("CVM_KITTI B = %d fp32 training step %.1f ms (%.0f pairs/s)" % (args.batch, ms, args.batch / ms * 1e3), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "kitti_map_cache_rate.json"), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res["samples_per_s"]))


if __name__ == "__main__":
    main()
