"""KITTI input side at B = 64: samples per second of DeviceBatches with the aerial alignment on the host (four Pillow passes per
sample on the decode pool) against the alignment on the device (KITTIPairs(device_align=True): one packed upload + one
ccvpe_kitti_align_u8 launch per batch), on a synthetic KITTI tree with 1280 x 1280 maps, and next to them the align launch
alone, the upload alone, the decode pool alone (the device path's ceiling) and the B = 64 CVM_KITTI training step of the same box:

    python tools/gpu/kitti_input_rate.py [--out DIR] [--batches 3] [--rounds 3] [--workers 16] [--no-step]

Host and device runs alternate, `rounds` times each; the medians are what DESIGN.md section 1 quotes.  The kernel's time is put
next to the time of reading each sample's 512 x 512 source window and writing the crop ONCE at the copy rate measured here (a
figure, not a gate).  Writes kitti_input_rate.json into --out."""
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
from ccvpe_amd import align, datasets as DS                   # noqa: E402

DRIVE = "2011_09_26/2011_09_26_drive_0001_sync/"
MAP, CAMERA = 1280, (375, 1242)


def png_bytes(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr, "RGB").save(buf, format="PNG")
    return buf.getvalue()


def smooth_image(rng, h, w):
    """Low-frequency colour field + mild noise: between the issue's 'smooth' and 'noise' PNG decode costs, as a real map is."""
    from PIL import Image
    small = (rng.rand(h // 16 + 1, w // 16 + 1, 3) * 255).astype(np.uint8)
    base = np.asarray(Image.fromarray(small, "RGB").resize((w, h), Image.BICUBIC), dtype=np.int16)
    return np.clip(base + rng.randint(-6, 7, size=base.shape), 1, 255).astype(np.uint8)


def make_tree(root, n, distinct=8, seed=0):
    """n samples in the reference loader's layout; `distinct` different map / camera images, the rest hard links to them."""
    rng = np.random.RandomState(seed)
    for d in ("satmap/" + DRIVE, "raw_data/" + DRIVE + "oxts/data", "raw_data/" + DRIVE + "image_02/data"):
        os.makedirs(os.path.join(root, d))
    names = []
    for k in range(n):
        frame = "%010d.png" % k
        sat = os.path.join(root, "satmap", DRIVE, frame)
        grd = os.path.join(root, "raw_data", DRIVE, "image_02/data", frame)
        if k < distinct:
            with open(sat, "wb") as f:
                f.write(png_bytes(smooth_image(rng, MAP, MAP)))
            with open(grd, "wb") as f:
                f.write(png_bytes(smooth_image(rng, CAMERA[0], CAMERA[1])))
        else:
            os.link(os.path.join(root, "satmap", DRIVE, "%010d.png" % (k % distinct)), sat)
            os.link(os.path.join(root, "raw_data", DRIVE, "image_02/data", "%010d.png" % (k % distinct)), grd)
        with open(os.path.join(root, "raw_data", DRIVE, "oxts/data", frame.replace(".png", ".txt")), "w") as f:
            f.write("49.01 8.43 112.0 0.02 0.01 %.6f 1.0 2.0\n" % rng.uniform(-3.1, 3.1))
        names.append(DRIVE + frame)
    train_file = os.path.join(root, "train_files.txt")
    with open(train_file, "w") as f:
        f.write("".join(nm + "\n" for nm in names))
    return train_file


def loader_rate(root, train_file, device_align, batch, workers):
    """Samples per second of one pass over the tree; the checksum keeps every batch's tensors alive until they are complete."""
    pairs = DS.KITTIPairs(root, train_file, 20, 20, 10, rng=np.random.default_rng(1), device_align=device_align)
    it = DS.DeviceBatches(pairs, batch, device="cuda", workers=workers, grd_hw=(256, 1024), n_bins=16)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n, check = 0, 0.0
    for b in it:
        n += len(b.indices)
        check += float(b.sat[:, :, ::64, ::64].sum())
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0), check


def decode_rate(root, train_file, workers):
    """Samples per second of the decode pool alone (device_align: two PNG decodes + the parameter row, nothing on the device):
    the ceiling of the device path."""
    from concurrent.futures import ThreadPoolExecutor
    pairs = DS.KITTIPairs(root, train_file, 20, 20, 10, rng=np.random.default_rng(1), device_align=True)
    draws = [pairs.draw(i) for i in range(len(pairs))]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=workers) as pool:
        n = sum(1 for _ in pool.map(lambda a: pairs.sample(a[0], draws=a[1]), enumerate(draws)))
    return n / (time.perf_counter() - t0)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--no-step", action="store_true", help="skip the B = 64 CVM_KITTI training step")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    res = {"batch": args.batch, "batches": args.batches, "rounds": args.rounds, "workers": args.workers, "map": MAP,
           "device": torch.cuda.get_device_name(0)}
    root = tempfile.mkdtemp(prefix="kitti_rate_")
    try:
        train_file = make_tree(root, args.batch * args.batches)
        loader_rate(root, train_file, True, args.batch, args.workers)            # warm both paths: code objects, pinned buffer, page cache
        loader_rate(root, train_file, False, args.batch, args.workers)
        runs = {"host": [], "device": [], "decode_only": []}
        checks = {}
        for r in range(args.rounds):
            for mode in ("host", "device"):
                rate, chk = loader_rate(root, train_file, mode == "device", args.batch, args.workers)
                runs[mode].append(rate)
                checks.setdefault(mode, chk)
                print("round %d %-6s %.1f samples/s" % (r, mode, rate), flush=True)
            runs["decode_only"].append(decode_rate(root, train_file, args.workers))
            print("round %d decode pool alone %.1f samples/s" % (r, runs["decode_only"][-1]), flush=True)
        assert checks["host"] == checks["device"], "the two paths delivered different batches: %r" % (checks,)
        res["samples_per_s"] = {m: {"runs": v, "median": statistics.median(v)} for m, v in runs.items()}
        # the parts alone, on one decoded batch
        pairs = DS.KITTIPairs(root, train_file, 20, 20, 10, rng=np.random.default_rng(1), device_align=True)
        samples = [pairs.sample(i) for i in range(args.batch)]
    finally:
        shutil.rmtree(root, ignore_errors=True)
    sizes = [s["sat_src_u8"].size for s in samples]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    stage = torch.empty((int(offsets[-1]),), dtype=torch.uint8).pin_memory()
    for s, o, n in zip(samples, offsets, sizes):
        stage.numpy()[o:o + n] = s["sat_src_u8"].reshape(-1)
    src = torch.empty_like(stage, device="cuda")
    up_ms = event_ms(lambda: src.copy_(stage, non_blocking=True))
    rows = torch.from_numpy(np.stack([s["align"] for s in samples])).cuda()
    offs = torch.from_numpy(offsets[:-1].copy()).cuda()
    out = torch.empty((args.batch, DS.KITTI_CROP, DS.KITTI_CROP, 3), device="cuda", dtype=torch.uint8)
    k_ms = event_ms(lambda: align.kitti_align(src, offs, rows, (DS.KITTI_CROP, DS.KITTI_CROP), out=out))
    big = torch.empty((1 << 30,), device="cuda", dtype=torch.uint8)
    big2 = torch.empty_like(big)
    copy_ms = event_ms(lambda: big2.copy_(big))
    hbm = 2.0 * big.numel() / (copy_ms * 1e-3)                                   # a copy reads and writes every byte
    del big, big2
    window = 2.0 * args.batch * DS.KITTI_CROP * DS.KITTI_CROP * 3                # the source window read once + the crop written
    res["upload"] = {"bytes": int(offsets[-1]), "ms": up_ms, "gb_per_s": offsets[-1] / (up_ms * 1e-3) / 1e9}
    res["align_launch"] = {"ms": k_ms, "window_bytes": window, "copy_gb_per_s": hbm / 1e9, "window_floor_ms": window / hbm * 1e3,
                           "launch_over_floor": k_ms / (window / hbm * 1e3)}
    print("upload %.1f MB: %.2f ms (%.1f GB/s); align launch %.3f ms, window floor %.4f ms at %.0f GB/s" % (
        offsets[-1] / 1e6, up_ms, res["upload"]["gb_per_s"], k_ms, res["align_launch"]["window_floor_ms"], hbm / 1e9), flush=True)
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
        print("CVM_KITTI B = %d fp32 training step %.1f ms (%.0f pairs/s)" % (args.batch, ms, args.batch / ms * 1e3), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "kitti_input_rate.json"), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res["samples_per_s"]))


if __name__ == "__main__":
    main()
