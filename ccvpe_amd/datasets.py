"""VIGOR and KITTI input side of the path: dataset indexing, image decoding, iteration — feeding the
device pipeline (ccvpe_amd/preprocess.py: PIL-exact resize + normalise + panorama roll + FoV crop; ccvpe_amd/targets.py:
ground truth from three scalars per sample).

What the reference does per sample on the host (/root/reference/datasets.py:18-177, train_VIGOR.py:57-93): read the VIGOR
split files, PIL-decode the panorama and the aerial tile, torchvision Resize / ToTensor / Normalize, roll the panorama by the
sample's orientation (random, or the fixed per-sample angles of `samearea_orientation_test.npy` /
`crossarea_orientation_test.npy` for the test sets), build a 1 + 20 + 2 channel 512 x 512 ground truth in numpy (24 MB per
sample) and hand everything to a DataLoader.  Here the host keeps only what has to be on the host — the directory index and
the JPEG decode (PIL, like the reference; on a thread pool, PIL releases the GIL while decoding) — and ships the DECODED
uint8 images (3-6 MB per pair) plus three scalars per sample to the device, where the rest runs as kernels.

    pairs = VIGORPairs(root, split="samearea", train=False, ori_noise=180, random_orientation="samearea_orientation_test.npy")
    for batch in DeviceBatches(pairs, batch_size=64, device="cuda", rank=rank, world=world, shard="exact"):   # evaluation
        out = net(batch.grd, batch.sat)                     # batch.gt, batch.gt_flat, batch.gt_ori, batch.labels for training

KITTI (datasets.py:354-640, train_KITTI.py:46-100): `KITTIPairs(root, file, ...)` reads the split file, the OXTS heading and
the two images of a sample and performs the aerial image's geometric alignment — rotate to the vehicle heading, shift to the
camera, the random (training) or listed (test files) shift and rotation, centre crop — with the same PIL calls as the reference
(the result is the 512 x 512 uint8 crop), or, with `device_align=True`, leaves the alignment to ONE ccvpe_kitti_align_u8 launch per
batch that DeviceBatches makes on the decoded maps (ccvpe_amd/align.py, csrc/align.hip: bit-identical to the PIL calls); with
`cache_maps=True` and a device image cache the decoded maps stay in HBM and ONE ccvpe_kitti_align_norm_u8_f32 launch per batch aligns
and normalises them from a table of addresses, so an epoch after the first opens no image.  Resize + normalise of both images
and the 1 + 16 + 2 channel ground truth then run on the device exactly as for VIGOR:

    pairs = KITTIPairs(root, "train_files.txt", shift_range_lat=20, shift_range_lon=20, rotation_range=10)
    for batch in DeviceBatches(pairs, 64, grd_hw=(256, 1024), n_bins=16, rank=rank, world=world): ...

Oxford RobotCar (datasets.py:183-353): `OxfordPairs(grd_image_root, sat_path, split)` — list files + yaw fixtures, the UTM ->
map-pixel fit, an 800 x 800 patch of the one large aerial map per sample; `DeviceBatches(pairs, B, grd_hw=(154, 231),
ascending_bins=True)`.  With `device_map=True` the map lives in HBM and the patches of a batch are cut, resized and normalised by
ONE ccvpe_window_resize_norm_u8_f32 launch from a table of patch origins (bit-identical to the Pillow crop + resize).

Sharding: DeviceBatches gives rank r a contiguous shard of the index list (after the optional seeded shuffle, identical on
every rank).  Evaluation (`shard="exact"`): harness.shard_indices — no sample is seen twice, no collective is needed, ranks
may differ by one batch.  Training (`shard="pad"`, the default for a training split and world > 1): every rank iterates the SAME
number of batches (short shards wrap around, as torch's DistributedSampler pads), because each step all-reduces gradients.
A sample's random choices (`pairs.draw(i)`) are drawn in index order on the producer thread, decoding runs on the pool.
"""
import os
import queue
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

CITIES = {("samearea", True): ("NewYork", "Seattle", "SanFrancisco", "Chicago"),
          ("samearea", False): ("NewYork", "Seattle", "SanFrancisco", "Chicago"),
          ("crossarea", True): ("NewYork", "Seattle"),                    # datasets.py:32-38
          ("crossarea", False): ("SanFrancisco", "Chicago")}


def _label_file(split, train):
    if split == "samearea":
        return "same_area_balanced_train.txt" if train else "same_area_balanced_test.txt"    # datasets.py:66-70
    return "pano_label_balanced.txt"                                                          # datasets.py:71-72


class VIGORPairs(object):
    """Host-side index of a VIGOR split + per-sample decode.  `sample(i)` returns the DECODED images and the scalars the
    device pipeline needs; nothing here touches the GPU."""

    def __init__(self, root, label_root="splits_new", split="samearea", train=True, pos_only=True, ori_noise=180.0,
                 random_orientation=None, seed=0, strict_orientation=True):
        if split not in ("samearea", "crossarea"):
            raise ValueError("split must be 'samearea' or 'crossarea'")
        self.root, self.split, self.train, self.pos_only = root, split, bool(train), bool(pos_only)
        self.ori_noise = float(ori_noise)
        self.cities = CITIES[(split, self.train)]
        if isinstance(random_orientation, str):                   # the reference's .npy fixtures (train_VIGOR.py:73-79)
            random_orientation = np.load(random_orientation)
        self.random_orientation = None if random_orientation is None else np.asarray(random_orientation, dtype=np.float64)
        self._rng = np.random.default_rng(seed)
        self._rng_lock = threading.Lock()

        # aerial tiles: one global index over the cities of the split, in file order (datasets.py:41-55)
        sat_paths, sat_index = [], {}
        for city in self.cities:
            with open(os.path.join(root, label_root, city, "satellite_list.txt")) as f:
                for line in f:
                    name = line.rstrip("\n")
                    sat_index[name] = len(sat_paths)
                    sat_paths.append(os.path.join(root, city, "satellite", name))
        self.sat_paths = sat_paths
        # panoramas: "<pano> <sat0> <drow0> <dcol0> <sat1> ... <sat3> <drow3> <dcol3>" (positive first, then 3 semi-positives)
        grd_paths, labels, deltas, city_of = [], [], [], []
        for city in self.cities:
            path = os.path.join(root, label_root, city, _label_file(split, self.train))
            with open(path) as f:
                for lineno, line in enumerate(f, 1):
                    tok = line.split(" ")
                    if len(tok) < 13:           # the reference indexes tok[1..12] and raises here; a skipped line would shift
                        raise ValueError("%s:%d: expected 13 fields, got %d" % (path, lineno, len(tok)))   # every later fixture entry
                    grd_paths.append(os.path.join(root, city, "panorama", tok[0]))
                    labels.append([sat_index[tok[i]] for i in (1, 4, 7, 10)])
                    deltas.append([[float(tok[i]), float(tok[i + 1])] for i in (2, 5, 8, 11)])
                    city_of.append(city)
        self.grd_paths, self.city_of = grd_paths, city_of
        self.labels = np.asarray(labels, dtype=np.int64).reshape(-1, 4)
        self.deltas = np.asarray(deltas, dtype=np.float64).reshape(-1, 4, 2)       # (row, col) offsets in raw aerial pixels
        # the fixture is indexed by sample position: it must describe exactly this index (strict_orientation=False accepts a
        # longer array, as the reference silently does — used by the tests that pair the fixture's head with a small tree)
        n_ori = None if self.random_orientation is None else len(self.random_orientation)
        if n_ori is not None and (n_ori < len(grd_paths) or (strict_orientation and n_ori != len(grd_paths))):
            raise ValueError("random_orientation has %d entries for %d samples" % (n_ori, len(grd_paths)))

    def __len__(self):
        return len(self.grd_paths)

    # ---- the sample's three random choices (datasets.py:107-116,124-135) ------------------------------------------------
    def rotation_fraction(self, idx):
        """Panorama roll as a fraction of its width; orientation angle = 360 * fraction (north = 0, counter-clockwise)."""
        if self.random_orientation is not None:
            return float(self.random_orientation[idx]) / 360.0
        with self._rng_lock:
            if self.ori_noise >= 180:
                return float(self._rng.uniform(0.0, 1.0))
            r = self.ori_noise / 360.0
            return float(self._rng.uniform(-r, r))

    def positive(self, idx):
        """(aerial tile index among the sample's four, row offset, column offset) in raw aerial pixels: the positive, or —
        pos_only=False — a random one of the four whose ground-truth location lies inside the tile."""
        if self.pos_only:
            return 0, self.deltas[idx, 0, 0], self.deltas[idx, 0, 1]
        ok = [k for k in range(4) if abs(self.deltas[idx, k, 0]) < 320 and abs(self.deltas[idx, k, 1]) < 320]
        if not ok:
            raise ValueError("sample %d has no tile with the ground truth inside it" % idx)
        with self._rng_lock:
            k = int(ok[self._rng.integers(len(ok))])
        return k, self.deltas[idx, k, 0], self.deltas[idx, k, 1]

    def draw(self, idx):
        """The sample's random choices, in the order sample() makes them.  DeviceBatches calls this on ONE thread in index order
        and hands the result to sample(draws=...), so a seeded iteration is reproducible whatever the decode threads do."""
        return self.rotation_fraction(idx), self.positive(idx)

    def keys(self, idx, draws):
        """Source files of sample idx under `draws` (a draw() result), for a device image cache: the panorama's path and the
        path of the aerial tile the draw selected."""
        return {"grd": self.grd_paths[idx], "sat": self.sat_paths[self.labels[idx, draws[1][0]]]}

    def sample(self, idx, sat_hw=(512, 512), grd_hw=(320, 640), draws=None, cached=None):
        """Decode sample idx.  Returns a dict: grd_u8 / sat_u8 (HWC uint8 numpy, as PIL decodes them), roll (pixels of the
        RESIZED panorama, datasets.py:121), angle_deg, center (cx, cy) of the Gaussian on the resized aerial grid
        (cx = column offset, cy = -row offset, both rescaled and rounded as datasets.py:141-142 does), city.
        cached: {side: raw (h, w)} of the sides a device image cache already holds — such a side is not opened or decoded and
        its *_u8 entry is None (`center` takes the raw tile size from the mapping); every other key is as without it.  With
        a mapping (even an empty one) an unreadable panorama's blank image is marked `nocache=("grd",)`."""
        from PIL import Image
        mark = {}
        if cached is not None and "grd" in cached:
            grd = None
        else:
            try:
                with Image.open(self.grd_paths[idx]) as im:
                    grd = np.array(im.convert("RGB"))             # owning, writable: torch.from_numpy needs that
            except (OSError, ValueError):                                  # unreadable panorama -> blank image (datasets.py:103-105)
                grd = np.zeros((grd_hw[0], grd_hw[1], 3), dtype=np.uint8)
                if cached is not None:
                    mark = {"nocache": ("grd",)}
        rot, (k, drow, dcol) = self.draw(idx) if draws is None else draws
        if cached is not None and "sat" in cached:
            sat = None
            h_raw, w_raw = cached["sat"]
        else:
            with Image.open(self.sat_paths[self.labels[idx, k]]) as im:
                sat = np.array(im.convert("RGB"))
            h_raw, w_raw = sat.shape[0], sat.shape[1]
        row = np.round(drow / h_raw * sat_hw[0])
        col = np.round(dcol / w_raw * sat_hw[1])
        # torch.round (half to even) of rotation * width, like datasets.py:121
        roll = int(torch.round(torch.as_tensor(rot) * grd_hw[1]).int().item())
        return dict(grd_u8=grd, sat_u8=sat, roll=roll, angle_deg=rot * 360.0,
                    center=(float(col), float(-row)), city=self.city_of[idx], index=int(idx), **mark)


# ---- KITTI (datasets.py:354-372: constants of the reference's loader) ---------------------------------------------------
KITTI_LAT, KITTI_ZOOM = 49.015, 18
KITTI_CAMERA_SHIFT = (1.08, 0.26)          # metres: GPS antenna -> left colour camera (datasets.py:366)
KITTI_CROP = 512


def kitti_meter_per_pixel(lat=KITTI_LAT, zoom=KITTI_ZOOM, scale=1.0):
    """Ground resolution of the aerial maps (datasets.py:368-372: web-mercator resolution at `lat`, maps fetched at scale 2)."""
    return 156543.03392 * np.cos(lat * np.pi / 180.0) / (2 ** zoom) / 2.0 / scale


class KITTIPairs(object):
    """Host-side index of a KITTI split file + per-sample decode and aerial alignment (datasets.py:374-503 `SatGrdDataset`,
    :506-640 `SatGrdDatasetTest`).  A line of a TRAINING file is `<day>/<drive>/<frame>.png`; a line of a TEST file carries the
    sample's fixed perturbation: `<name> <shift_x> <shift_y> <theta>` (test=True).  Training perturbations are three uniform
    draws in [-1, 1) per sample — from numpy's global generator when rng is None (so `np.random.seed(s)` reproduces the
    reference's sequence sample by sample when samples are drawn in order: sample() called sequentially, or DeviceBatches, which
    calls draw() in index order on one thread), else from `rng` (a numpy Generator / RandomState; draws are serialised by a lock).

    device_align=True leaves the alignment to the device: sample() returns the map AS DECODED (`sat_src_u8`) and the parameter row
    of ccvpe_amd/align.py (`align`) instead of `sat_u8`; DeviceBatches then aligns the whole batch with one launch of
    ccvpe_kitti_align_u8, bit-identical to the Pillow calls.  Every other key, and every draw, is the same.

    cache_maps=True (with device_align=True; opt-in): the decoded map of a sample never changes between epochs, only its draw
    does, so `keys` also names the map file ("sat_src") and DeviceBatches with a cache keeps the decoded map on the device;
    sample(cached={"sat_src": (h, w)}) then does not open the map and builds the same `align` row from the cached size."""

    def __init__(self, root, file, shift_range_lat=20.0, shift_range_lon=20.0, rotation_range=10.0, test=False, rng=None,
                 device_align=False, cache_maps=False):
        self.root, self.test, self.device_align = root, bool(test), bool(device_align)
        self.cache_maps = bool(cache_maps)
        if self.cache_maps and not self.device_align:
            raise ValueError("cache_maps=True needs device_align=True: the cached maps are aligned on the device")
        self.meter_per_pixel = kitti_meter_per_pixel()
        self.shift_px_lat = shift_range_lat / self.meter_per_pixel
        self.shift_px_lon = shift_range_lon / self.meter_per_pixel
        self.rotation_range = float(rotation_range)
        with open(file) as f:
            self.lines = [ln[:-1] for ln in f.readlines()]                    # datasets.py:399 (drops the line's last character)
        self._rng, self._rng_lock = rng, threading.Lock()

    def __len__(self):
        return len(self.lines)

    def paths(self, name):
        """(aerial map, OXTS record, left colour image) of `<day>/<drive>/<frame>.png` (datasets.py:410-435)."""
        drive, frame = name[:38], name[38:]
        base = os.path.join(self.root, "raw_data", drive)
        return (os.path.join(self.root, "satmap", name),
                os.path.join(base, "oxts/data", frame.lower().replace(".png", ".txt")),
                os.path.join(base, "image_02/data", frame.lower()))

    def perturbation(self, idx):
        """(shift_x, shift_y) in units of the shift range (right / up positive, along / across the heading) and the rotation in
        degrees (counter-clockwise; 0 = the vehicle heads east in the aerial image)."""
        if self.test:
            _, sx, sy, th = self.lines[idx].split(" ")
            return -float(sx), -float(sy), float(th) * self.rotation_range          # datasets.py:585-595
        with self._rng_lock:
            u = np.random.uniform if self._rng is None else self._rng.uniform
            sx, sy, r = u(-1, 1), u(-1, 1), u(-1, 1)                                # datasets.py:452-453,463 (this order)
        return float(sx), float(sy), float(r) * self.rotation_range

    def draw(self, idx):
        """The sample's random choices (see VIGORPairs.draw)."""
        return self.perturbation(idx)

    def keys(self, idx, draws):
        """Source files of sample idx for a device image cache: the camera image; the aerial side is None — the aligned crop
        depends on the sample's draw (both device_align modes keep their path).  cache_maps: "sat_src" names the map file,
        whose DECODED image does not depend on the draw."""
        name = self.lines[idx].split(" ")[0] if self.test else self.lines[idx]
        sat_path, _, grd_path = self.paths(name)
        if self.cache_maps:
            return {"grd": grd_path, "sat": None, "sat_src": sat_path}
        return {"grd": grd_path, "sat": None}

    def sample(self, idx, sat_hw=(512, 512), grd_hw=(256, 1024), draws=None, cached=None):
        """Decode + align sample idx.  Returns the dict DeviceBatches consumes: grd_u8 (the left camera image as decoded),
        sat_u8 (the aligned, perturbed 512 x 512 aerial crop; device_align: sat_src_u8 and align in its place), roll = 0, angle_deg
        (orientation ground truth in [0, 360]),
        center = (x_offset, y_offset) of the Gaussian (datasets.py:475-476), city = the drive, index.
        cached: {"grd": raw (h, w)} when a device image cache holds the camera image — it is then not opened, grd_u8 is None;
        {"sat_src": (h, w)} (cache_maps) when it holds the decoded map — the map is not opened, sat_src_u8 is None and the
        `align` row is built from that size."""
        from PIL import Image
        name = self.lines[idx].split(" ")[0] if self.test else self.lines[idx]
        sat_path, oxts_path, grd_path = self.paths(name)
        if self.cache_maps and cached is not None and "sat_src" in cached:
            sat = None
            h, w = (int(v) for v in cached["sat_src"])
        else:
            with Image.open(sat_path, "r") as im:
                sat = im.convert("RGB")
            w, h = sat.size
        with open(oxts_path) as f:
            heading = float(f.readline().split(" ")[5])
        if cached is not None and "grd" in cached:
            grd = None
        else:
            with Image.open(grd_path, "r") as im:
                grd = np.array(im.convert("RGB"))
        sx, sy, ori = self.perturbation(idx) if draws is None else draws
        mpp = self.meter_per_pixel
        if w < KITTI_CROP or h < KITTI_CROP:
            raise ValueError("%s: aerial map %dx%d is smaller than the %d crop" % (sat_path, w, h, KITTI_CROP))
        cam_px = (KITTI_CAMERA_SHIFT[0] / mpp, KITTI_CAMERA_SHIFT[1] / mpp)
        shift_px = (sx * self.shift_px_lon, -sy * self.shift_px_lat)
        if self.device_align:
            from . import align
            aerial = dict(sat_src_u8=None if sat is None else np.array(sat),
                          align=align.kitti_align_params(heading, cam_px, shift_px, ori, w, h, KITTI_CROP))
        else:
            sat = sat.rotate(-heading / np.pi * 180)                                # east = the vehicle heading
            sat = sat.transform(sat.size, Image.AFFINE, (1, 0, cam_px[0], 0, 1, cam_px[1]), resample=Image.BILINEAR)
            sat = sat.transform(sat.size, Image.AFFINE, (1, 0, shift_px[0], 0, 1, shift_px[1]), resample=Image.BILINEAR)
            sat = sat.rotate(ori)
            left, top = int(round((w - KITTI_CROP) / 2.0)), int(round((h - KITTI_CROP) / 2.0))     # torchvision center_crop
            aerial = dict(sat_u8=np.array(sat.crop((left, top, left + KITTI_CROP, top + KITTI_CROP))))
        c, s_ = np.cos(ori / 180 * np.pi), np.sin(ori / 180 * np.pi)
        x_off = int(sx * self.shift_px_lon * c - sy * self.shift_px_lat * s_)       # int(): truncation, as the reference
        y_off = int(-sy * self.shift_px_lat * c - sx * self.shift_px_lon * s_)
        angle = 90 - ori
        if angle < 0:
            angle += 360
        elif angle > 360:
            angle -= 360
        return dict(grd_u8=grd, **aerial, roll=0, angle_deg=float(angle), center=(float(x_off), float(y_off)),
                    city=name[:38], index=int(idx))


# ---- Oxford RobotCar (datasets.py:183-353, train_OxfordRobotCar.py:49-72) ---------------------------------------------
# Ground control points of the reference's aerial map: UTM (easting, northing) -> (column, row) of `satellite_map_new.png`
# (datasets.py:252-263: four corners + centre; the affine map is their least-squares fit).
OXFORD_UTM = ((619400., 5736195.), (619400., 5734600.), (620795., 5736195.), (620795., 5734600.), (620100., 5735400.))
OXFORD_PIX = ((900., 900.), (492., 18168.), (15966., 1260.), (15553., 18528.), (8255., 9688.))
OXFORD_LISTS = {"train": (("training.txt",), "train_yaw.npy"), "val": (("validation.txt",), "val_yaw.npy"),
                "test": (("test1_j.txt", "test2_j.txt", "test3_j.txt"), "test_yaw.npy")}
OXFORD_BOX = 800                            # side of the aerial patch in map pixels (datasets.py:300,317)
OXFORD_MAP_MODES = ("RGB", "RGBA", "L")     # modes whose out-of-image crop fill converts to RGB (0, 0, 0)


class OxfordPairs(object):
    """Host-side index of an Oxford RobotCar split + per-sample decode: `<image> <...> <easting> <northing>` lines, the yaw
    fixtures (`*_yaw.npy`, radians, 0 = west, clockwise), ONE large aerial map from which an 800 x 800 patch is cut per sample —
    around the vehicle plus a random offset of up to 200 * sqrt(2) map pixels (train: two draws from Python's `random` module,
    or from `rng`, a `random.Random`), or the half-overlapping grid patch that holds the vehicle at least 200 pixels from its
    border (val / test).  The Gaussian's centre is the vehicle's position in the 512 x 512 resized patch; the orientation bins of
    this loader count UP (DeviceBatches(..., ascending_bins=True)).

    device_map=True (opt-in) leaves the aerial side to the device: sample() cuts no patch (`sat_u8` is None) and returns the
    patch's `sat_origin` = (x0, y0) on the map instead, keys() offers no aerial key in any split, and DeviceBatches serves the
    whole aerial batch with ONE ccvpe_window_resize_norm_u8_f32 launch on the map resident in HBM (`map_on`), bit-identical
    to the Pillow crop + resize.  Every draw and every other key is the same.  The map must be RGB, RGBA or L — the modes in
    which the zero fill of a crop beyond the image converts to RGB (0, 0, 0), so converting the map once equals converting
    each patch; any other mode (a palette's index 0 is a colour) raises ValueError.  The map is converted to RGB and uploaded
    once per device, on the first batch for that device, and this index object owns the device copies.  The host keeps the
    decoded Pillow image (`self.map`): the RGB array made for an upload is released right after it, and a second device
    gets its own upload from the same host image (about 1 GB of HBM each for the real map)."""

    def __init__(self, grd_image_root, sat_path, split="train", rng=None, device_map=False):
        from PIL import Image
        if split not in OXFORD_LISTS:
            raise ValueError("split must be 'train', 'val' or 'test'")
        self.root, self.split, self.sat_path = grd_image_root, split, sat_path
        Image.MAX_IMAGE_PIXELS = None                                  # the real map is 16 k x 19 k pixels
        self.map = Image.open(sat_path)
        self.map.load()
        self.device_map = bool(device_map)
        if self.device_map and self.map.mode not in OXFORD_MAP_MODES:
            raise ValueError("device_map needs an aerial map of mode %s, %s is %r" % ("/".join(OXFORD_MAP_MODES), sat_path,
                                                                                     self.map.mode))
        self._map_dev, self._map_lock = {}, threading.Lock()
        files, yaw = OXFORD_LISTS[split]
        self.rows, self.list_lengths = [], []
        for fn in files:
            with open(os.path.join(grd_image_root, fn)) as f:
                rows = [ln[:-1].split(" ") for ln in f.readlines()]
            self.list_lengths.append(len(rows))
            self.rows += rows
        self.yaw = np.load(os.path.join(grd_image_root, yaw))
        if len(self.yaw) < len(self.rows):
            raise ValueError("%s has %d entries for %d samples" % (yaw, len(self.yaw), len(self.rows)))
        utm = np.asarray([r[2:] for r in self.rows], dtype=np.float64)            # [n, 2]: easting, northing
        src = np.hstack([np.asarray(OXFORD_UTM), np.ones((5, 1))])
        dst = np.hstack([np.asarray(OXFORD_PIX), np.ones((5, 1))])
        self.utm = utm
        self.affine = np.linalg.lstsq(src, dst, rcond=None)[0]                   # 3 x 3; its last column maps the padding 1 to 1
        self._rng, self._rng_lock = rng, threading.Lock()

    def __len__(self):
        return len(self.rows)

    def offset(self):
        """Training: the (row, column) offset of the patch centre from the vehicle, in map pixels (datasets.py:296-300)."""
        import math
        import random
        with self._rng_lock:
            u = random.random if self._rng is None else self._rng.random
            alpha, r = 2 * math.pi * u(), 200 * np.sqrt(2) * u()
        return int(r * math.cos(alpha)), int(r * math.sin(alpha))

    def draw(self, idx):
        """The sample's random choice (see VIGORPairs.draw): the patch offset in training, nothing otherwise."""
        return self.offset() if self.split == "train" else None

    def _position(self, idx):
        """(column, row) of the vehicle on the map — one sample at a time, as the reference evaluates it (a batched product may
        round differently in the last place)."""
        return tuple(float(v) for v in np.dot(np.hstack([self.utm[idx:idx + 1], np.ones((1, 1))]), self.affine)[0, :2])

    @staticmethod
    def _grid(v):
        """(k, p): patch origin 400 * k such that the vehicle sits at p in [200, 600) of the patch (val / test)."""
        k = int(v // 400)
        if np.round(v - 400 * k) < 200:
            k -= 1
        return k, int(np.round(v - 400 * k))

    def map_rgb(self):
        """The map as the [H, W, 3] uint8 RGB array that device_map uploads (a fresh host array on every call)."""
        return np.array(self.map.convert("RGB"))

    def map_on(self, device):
        """The RGB map as a [H, W, 3] uint8 tensor on `device`: uploaded on the first call for that device, then shared."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        with self._map_lock:
            if device not in self._map_dev:
                self._map_dev[device] = torch.from_numpy(self.map_rgb()).to(device)
            return self._map_dev[device]

    def keys(self, idx, draws):
        """Sources of sample idx for a device image cache: the camera image's path and — val / test — "<map path>@<kc>,<kr>",
        the grid patch; a training patch has a random offset: None.  device_map: the map serves the aerial side, None always."""
        sat = None
        if self.split != "train" and not self.device_map:
            col, row = self._position(idx)
            sat = "%s@%d,%d" % (self.sat_path, self._grid(col)[0], self._grid(row)[0])
        return {"grd": os.path.join(self.root, self.rows[idx][0]), "sat": sat}

    def sample(self, idx, sat_hw=(512, 512), grd_hw=(154, 231), draws=None, cached=None):
        """cached: {side: raw (h, w)} of the sides a device image cache holds: not opened / cropped, their *_u8 entry is None.
        device_map: no patch is cut, sat_u8 is None and `sat_origin` = (x0, y0) of the patch on the map is added."""
        from PIL import Image
        if cached is not None and "grd" in cached:
            grd = None
        else:
            with Image.open(os.path.join(self.root, self.rows[idx][0])) as im:
                grd = np.array(im.convert("RGB"))
        col, row = self._position(idx)
        if self.split == "train":
            drow, dcol = self.offset() if draws is None else draws
            r0, c0 = int(row + drow), int(col + dcol)
            box = (c0 - 400, r0 - 400, c0 + 400, r0 + 400)
            cy = int(np.round((400 + drow) / 800 * 512 - 256))
            cx = int(np.round((400 + dcol) / 800 * 512 - 256))
        else:
            kc, pc = self._grid(col)
            kr, pr = self._grid(row)
            box = (kc * 400, kr * 400, kc * 400 + 800, kr * 400 + 800)
            cy = int(-(pr / 800 * 512 - 256))
            cx = int(-(pc / 800 * 512 - 256))
        aerial = {}
        if self.device_map:
            sat, aerial = None, {"sat_origin": (int(box[0]), int(box[1]))}
        else:
            sat = None if cached is not None and "sat" in cached else np.array(self.map.crop(box).convert("RGB"))
        angle = float(self.yaw[idx]) / np.pi * 180 - 90                          # 0 = north, clockwise (datasets.py:334-337)
        if angle < 0:
            angle += 360
        return dict(grd_u8=grd, sat_u8=sat, roll=0, angle_deg=float(angle), center=(float(cx), float(cy)), city="oxford",
                    index=int(idx), **aerial)


def shard_positions(n, world, rank, mode="exact"):
    """Positions of range(n) that rank `rank` of `world` iterates (see DeviceBatches: "exact" / "pad" / "truncate")."""
    from . import harness
    if mode == "exact":
        return np.asarray(harness.shard_indices(n, world, rank), dtype=np.int64)
    if mode == "truncate":
        per = n // world
        return np.arange(rank * per, (rank + 1) * per, dtype=np.int64)
    if mode == "pad":
        per = (n + world - 1) // world
        if n == 0:
            return np.zeros((0,), dtype=np.int64)
        return np.arange(rank * per, (rank + 1) * per, dtype=np.int64) % n
    raise ValueError("shard must be 'exact', 'pad' or 'truncate'")


def pairs_is_training(pairs):
    """True / False when the index object says which split it holds (VIGORPairs.train, KITTIPairs.test, OxfordPairs.split),
    None otherwise.  DeviceBatches keys its default shard mode on it: an EVALUATION set must never be padded (wrapped-around
    samples would be counted twice in the gathered metrics), whatever `targets` is."""
    if isinstance(getattr(pairs, "train", None), bool):
        return pairs.train
    if isinstance(getattr(pairs, "test", None), bool):
        return not pairs.test
    if isinstance(getattr(pairs, "split", None), str):
        return pairs.split == "train"
    return None


class Batch(object):
    """One device batch: grd [B,3,h,w_fov], sat [B,3,H,W] (normalised fp32), angle_deg [B], center [B,2], cities, indices and —
    with targets — gt [B,1,H,W], gt_flat [B,H*W], gt_ori [B,2,H,W], labels (six max-pooled orientation-binned maps).
    heading_deg [B] is the samples' angle_deg again as FLOAT64, unwrapped: the loaders' `orientation_angle`, a Python float
    that the reference's test loops use at full precision (ccvpe_amd.evaluate.evaluate_batches)."""
    __slots__ = ("grd", "sat", "angle_deg", "heading_deg", "center", "cities", "indices", "gt", "gt_flat", "gt_ori", "labels")


class DeviceBatches(object):
    """Iterates a VIGORPairs / KITTIPairs / OxfordPairs index in device batches (KITTI: grd_hw=(256, 1024), n_bins=16; Oxford:
    grd_hw=(154, 231), ascending_bins=True).  Decoding runs `workers` samples ahead on a thread pool; resize,
    normalisation, roll, FoV crop and the ground truth are kernels on `device` (no CPU fallback: preprocess raises without
    the HIP library).  fov < 360 keeps the first fov/360 of the rolled panorama's columns (train_VIGOR.py:177-178).

    Rank shards (`shard`): "exact" = the balanced contiguous shards of harness.shard_indices — every sample exactly once over the
    ranks, shard sizes differ by at most one, so ranks may run a DIFFERENT number of batches: evaluation only (no collective).
    "pad" = every rank gets ceil(n / world) samples, the short shards wrap around to the start of the index list
    (torch's DistributedSampler rule); "truncate" = every rank gets floor(n / world).  With "pad" / "truncate" len(self) is
    the same on every rank BY CONSTRUCTION — required for training, where each step all-reduces gradients inside the
    backward and a rank with one batch more would wait for its peers until the RCCL timeout.  Default: "pad" for a TRAINING
    split (`pairs_is_training`; an index object that does not say: when targets are produced) and world > 1, else "exact" —
    a test split is never padded by default, with or without targets.

    cache (ccvpe_amd.cache.DeviceImageCache, opt-in): the resized uint8 image of every source file stays on the device.  The
    producer thread asks the index for the sample's `keys`, looks them up and decodes only what is missing; the consumer
    inserts the misses (a key once per batch) and assembles each side of the batch with ONE ccvpe_gather_norm_u8_f32 launch
    over a table of slot addresses.  Sides without a key (KITTI's aligned crop, Oxford's training patch), blank panoramas and
    the misses of a full cache go through the cache's scratch slots and the same launch.  Draws are made in the same order and
    the batches are bit-identical to those without a cache.

    KITTIPairs(device_align=True, cache_maps=True) with a cache: the DECODED aerial maps stay on the device too (raw slots).  The
    producer looks the map keys up and decodes only the misses; the consumer stages and uploads only those (one pinned buffer),
    retains each new file once, reads what a full cache cannot retain from the staged upload itself, and makes ONE
    ccvpe_kitti_align_norm_u8_f32 launch over the address table straight into batch.sat (sat_hw must be (512, 512)); the ground
    side goes through the gather as before.  Bit-identical to device_align=True without the flag, draws in the same order.

    OxfordPairs(device_map=True): the aerial side of every batch, with or without a cache, is ONE
    ccvpe_window_resize_norm_u8_f32 launch on the index's device-resident map over a [B, 2] table of patch origins, written
    straight into batch.sat (tables from `sat_hw`); it never touches the cache.  Bit-identical to device_map=False."""

    def __init__(self, pairs, batch_size, device="cuda", indices=None, shuffle=False, seed=0, rank=0, world=1, workers=8,
                 prefetch=2, grd_hw=(320, 640), sat_hw=(512, 512), fov=360, targets=True, n_bins=20, drop_last=False,
                 ascending_bins=False, shard=None, cache=None):
        self.pairs, self.batch_size, self.device = pairs, int(batch_size), torch.device(device)
        self.cache = cache                                   # ccvpe_amd.cache.DeviceImageCache, or None: the path without one
        idx = np.arange(len(pairs)) if indices is None else np.asarray(indices)
        if shuffle:
            idx = idx[np.random.default_rng(seed).permutation(len(idx))]      # same permutation on every rank
        if shard is None:
            training = pairs_is_training(pairs)
            if training is None:                      # an index object that does not say: ground truth requested = training
                training = bool(targets)
            shard = "pad" if (training and world > 1) else "exact"
        self.shard = shard
        self.shuffle, self.rank, self.world = bool(shuffle), int(rank), int(world)      # how the order was made (evaluate_sequence)
        self.indices = idx[shard_positions(len(idx), world, rank, shard)]
        self.workers, self.prefetch = int(workers), int(prefetch)
        self.grd_hw, self.sat_hw, self.fov = tuple(grd_hw), tuple(sat_hw), fov
        self.keep_w = int(grd_hw[1] * fov / 360)                              # train_VIGOR.py:177: int(w * FoV / 360)
        self.targets, self.n_bins, self.drop_last, self.ascending_bins = targets, n_bins, drop_last, bool(ascending_bins)
        self._stage, self._stage_free = None, None          # device alignment: the pinned staging buffer and its upload's event
        # KITTIPairs(cache_maps=True) with a cache: decoded maps stay on the device, the align launch writes batch.sat itself
        self._maps = cache is not None and bool(getattr(pairs, "cache_maps", False))
        if self._maps and self.sat_hw != (KITTI_CROP, KITTI_CROP):
            raise ValueError("cache_maps: the align launch writes the model's input, sat_hw must be (%d, %d)" % (KITTI_CROP, KITTI_CROP))

    def __len__(self):
        n = len(self.indices)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def _decode_batch(self, pool, chunk):
        # the random choices of the chunk are drawn HERE, on the producer thread, in index order; the pool only decodes
        draws = [self.pairs.draw(int(i)) for i in chunk]
        if self.cache is not None:
            return self._decode_batch_cached(pool, chunk, draws)
        return list(pool.map(lambda a: self.pairs.sample(int(a[0]), self.sat_hw, self.grd_hw, draws=a[1]), zip(chunk, draws)))

    def _cache_key(self, side, key):
        """The cache holds RESIZED images: the key carries the side's size, so iterators of different geometry can share one."""
        hw = self.grd_hw if side == "grd" else self.sat_hw
        return "%s|%dx%d" % (key, hw[0], hw[1])

    def _decode_batch_cached(self, pool, chunk, draws):
        """Producer thread, with a cache: keys -> lookup -> decode only the sides that are missing.  Each sample carries its
        cache keys (`_keys`) and the slot addresses found (`_addr`) to the consumer."""
        keys, found = [], []
        for i, d in zip(chunk, draws):
            named = self.pairs.keys(int(i), d)
            k = {side: None if named[side] is None else self._cache_key(side, named[side]) for side in ("grd", "sat")}
            if self._maps:                                   # the decoded map, unresized: a key of its own kind
                k["sat_src"] = self.cache.raw_key(named["sat_src"])
            keys.append(k)
            hits = {side: self.cache.lookup(key) for side, key in k.items() if key is not None}
            found.append({side: hit for side, hit in hits.items() if hit is not None})

        def one(a):
            i, d, k, f = a
            s = self.pairs.sample(int(i), self.sat_hw, self.grd_hw, draws=d, cached={side: hit[1] for side, hit in f.items()})
            s["_keys"], s["_addr"] = k, {side: hit[0] for side, hit in f.items()}
            return s

        return list(pool.map(one, zip(chunk, draws, keys, found)))

    def _gather_side(self, samples, side, hw, keep_w, dst, crops=None):
        """One side of a batch through the cache: insert the misses (a key once), resize what cannot be retained into scratch
        slots, then ONE gather launch over the address table."""
        from . import preprocess
        cache, dev = self.cache, self.device
        scratch, used = None, 0
        addrs, done = [], {}
        for i, s in enumerate(samples):
            key = s["_keys"][side]
            if side in s.get("nocache", ()):
                key = None
            addr = s["_addr"].get(side)
            if addr is None and key is not None:             # inserted by an earlier sample of this batch, or by a batch that
                addr = done.get(key) or cache.address(key)   # was still in flight when the producer looked the key up
            if addr is None:
                if crops is not None:
                    img = crops[i]
                    if tuple(img.shape[:2]) == tuple(hw):    # the align kernel's crop already has the model's size: no resize
                        addr = img.data_ptr()
                else:
                    img = torch.from_numpy(s[side + "_u8"]).to(dev, non_blocking=True)
                if addr is None and key is not None:
                    addr = cache.insert(key, img, hw)
                    if addr is not None:
                        done[key] = addr
                if addr is None:
                    if scratch is None:
                        scratch = cache.scratch(len(samples), hw)
                    slot = scratch[used]
                    used += 1
                    preprocess.resize_u8(img, hw, dst=slot)
                    addr = slot.data_ptr()
            addrs.append(addr)
        table = torch.tensor(addrs, dtype=torch.int64, device=dev)
        rolls = torch.tensor([int(s["roll"]) if side == "grd" else 0 for s in samples], dtype=torch.int32, device=dev)
        preprocess.gather_norm(table, rolls, hw, keep_w=keep_w, dst=dst)

    def _align_on_device(self, samples):
        """KITTIPairs(device_align=True): the batch's decoded maps packed into ONE pinned staging buffer (reused across batches),
        one upload, the parameter rows, one ccvpe_kitti_align_u8 launch -> [B, 512, 512, 3] uint8 crops on the device."""
        from . import align
        src, offsets = self._upload_packed([s["sat_src_u8"] for s in samples])
        rows = torch.from_numpy(np.stack([s["align"] for s in samples])).to(self.device)
        return align.kitti_align(src, torch.from_numpy(offsets[:-1].copy()).to(self.device), rows, (KITTI_CROP, KITTI_CROP))

    def _upload_packed(self, maps):
        """The decoded maps back to back in the pinned staging buffer (reused across batches), ONE upload.  Returns the device
        buffer and the int64 offsets [len(maps) + 1] of the maps in it."""
        sizes = [m.size for m in maps]
        offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        total = int(offsets[-1])
        if self._stage is None or self._stage.numel() < total:
            self._stage = torch.empty((total,), dtype=torch.uint8).pin_memory()
        elif self._stage_free is not None:
            self._stage_free.synchronize()                   # the previous batch's upload has read the buffer
        stage = self._stage.numpy()
        for m, o, n in zip(maps, offsets, sizes):
            stage[o:o + n] = m.reshape(-1)
        src = self._stage[:total].to(self.device, non_blocking=True)
        self._stage_free = torch.cuda.Event()
        self._stage_free.record()
        return src, offsets

    def _align_cached_maps(self, samples, dst):
        """KITTIPairs(device_align=True, cache_maps=True) with a cache: the aerial side of a batch from device-resident maps.
        Only the maps the producer had to decode are staged and uploaded (each file once); each new key is retained in a raw
        slot of the cache, a map that cannot be retained (cache full) is read from the staged upload itself; then the address
        table and ONE ccvpe_kitti_align_norm_u8_f32 launch straight into dst = batch.sat."""
        from . import align
        cache = self.cache
        addrs, pending, first = [], [], {}
        for s in samples:
            key = s["_keys"]["sat_src"]
            addr = s["_addr"].get("sat_src")
            if addr is None:                                 # inserted by a batch that was still in flight when the producer
                addr = cache.address(key)                    # looked the key up
            if addr is None and key not in first:            # an earlier sample of this batch stages the same file
                first[key] = len(pending)
                pending.append(s["sat_src_u8"])
            addrs.append(addr)
        if pending:
            src, offsets = self._upload_packed(pending)
            staged = {}
            for key, j in first.items():
                h, w = pending[j].shape[:2]
                view = src[int(offsets[j]):int(offsets[j + 1])].view(h, w, 3)
                addr = cache.insert_raw(key, view)
                staged[key] = view.data_ptr() if addr is None else addr
            addrs = [staged[s["_keys"]["sat_src"]] if a is None else a for a, s in zip(addrs, samples)]
        table = torch.tensor(addrs, dtype=torch.int64, device=self.device)
        rows = torch.from_numpy(np.stack([s["align"] for s in samples])).to(self.device)
        align.kitti_align_norm(table, rows, (KITTI_CROP, KITTI_CROP), dst=dst)   # `src` lives until here: stream-ordered free

    def _window_side(self, samples, dst):
        """OxfordPairs(device_map=True): the aerial side of a batch = the origins table + ONE launch on the resident map."""
        from . import preprocess
        origins = torch.tensor([s["sat_origin"] for s in samples], dtype=torch.int32, device=self.device)
        preprocess.window_resize_norm(self.pairs.map_on(self.device), origins, (OXFORD_BOX, OXFORD_BOX), self.sat_hw, dst=dst)

    def _to_device(self, samples):
        from . import preprocess, targets
        dev = self.device
        b = len(samples)
        out = Batch()
        out.grd = torch.empty((b, 3, self.grd_hw[0], self.keep_w), device=dev, dtype=torch.float32)
        out.sat = torch.empty((b, 3) + self.sat_hw, device=dev, dtype=torch.float32)
        maps = bool(b) and self._maps                         # the aerial side is aligned from device-resident maps
        crops = self._align_on_device(samples) if b and "align" in samples[0] and not maps else None
        window = bool(b) and "sat_origin" in samples[0]       # the aerial side comes from a device-resident map
        if self.cache is not None:
            self._gather_side(samples, "grd", self.grd_hw, self.keep_w, out.grd)
            if maps:
                self._align_cached_maps(samples, out.sat)
            elif not window:
                self._gather_side(samples, "sat", self.sat_hw, self.sat_hw[1], out.sat, crops=crops)
        else:
            for i, s in enumerate(samples):
                g = torch.from_numpy(s["grd_u8"]).to(dev, non_blocking=True)
                if not window:
                    a = torch.from_numpy(s["sat_u8"]).to(dev, non_blocking=True) if crops is None else crops[i]
                preprocess.preprocess(g, self.grd_hw, dst=out.grd[i], roll=s["roll"], keep_w=self.keep_w)
                if not window:
                    preprocess.preprocess(a, self.sat_hw, dst=out.sat[i])
        if window:
            self._window_side(samples, out.sat)
        out.angle_deg = torch.tensor([s["angle_deg"] for s in samples], device=dev, dtype=torch.float32)
        out.heading_deg = torch.tensor([s["angle_deg"] for s in samples], device=dev, dtype=torch.float64)
        out.center = torch.tensor([s["center"] for s in samples], device=dev, dtype=torch.float32)
        out.cities = [s["city"] for s in samples]
        out.indices = [s["index"] for s in samples]
        out.gt = out.gt_flat = out.gt_ori = out.labels = None
        if self.targets:
            out.gt, out.gt_flat, out.gt_ori, out.labels = targets.train_targets(out.center, out.angle_deg % 360.0, self.n_bins,
                                                                               self.sat_hw[0], self.sat_hw[1],
                                                                               ascending=self.ascending_bins)
        return out

    def __iter__(self):
        chunks = [self.indices[i:i + self.batch_size] for i in range(0, len(self.indices), self.batch_size)]
        if self.drop_last and chunks and len(chunks[-1]) < self.batch_size:
            chunks.pop()
        q = queue.Queue(maxsize=max(1, self.prefetch))
        stop = threading.Event()

        def producer():
            try:
                with ThreadPoolExecutor(max_workers=max(1, self.workers)) as pool:
                    for chunk in chunks:
                        if stop.is_set():
                            return
                        q.put(("ok", self._decode_batch(pool, chunk)))
                q.put(("end", None))
            except BaseException as ex:                 # noqa: BLE001 — hand the failure to the consumer
                q.put(("err", ex))

        t = threading.Thread(target=producer, daemon=True)
        t.start()
        try:
            while True:
                kind, payload = q.get()
                if kind == "end":
                    return
                if kind == "err":
                    raise payload
                yield self._to_device(payload)
        finally:
            stop.set()
            while not q.empty():                       # unblock a producer waiting on a full queue
                try:
                    q.get_nowait()
                except queue.Empty:
                    break
