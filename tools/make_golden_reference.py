"""Generate the fixtures of the oracle-vs-reference tests from the REFERENCE (imported through tools/ref_import.py).

Runs only where the reference is present.  The tests (tests/test_oracle_vs_reference.py, the *_live tests of
tests/test_datasets.py) rebuild the same tiny dataset directories and the same synthetic weights / pair, and compare
what the oracle and ccvpe_amd.datasets produce with what the reference produced here:
    tests/golden/ref_vigor_prior36.npz   CVM_VIGOR_ori_prior(ori_noise=36) forward: output shapes, the logits' arg-max,
                                         the logits and the six score volumes (sampled, test_oracle_vs_reference.PRIOR36_STRIDES)
    tests/golden/reference_live.json     state_dict layouts, and the reference datasets' samples (exactly compared
                                         images / ground-truth maps as golden_util.digest values)
Usage:
    python tools/make_golden_reference.py
"""
import json
import os
import random
import shutil
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from ref_import import import_reference, import_reference_datasets   # noqa: E402
from ccvpe_amd import synth                                          # noqa: E402
from oracle import ccvpe_oracle as O                                 # noqa: E402
import golden_util as G                                              # noqa: E402
import test_datasets as TD                                           # noqa: E402
import test_oracle_vs_reference as TR                                # noqa: E402

POOLS = (64, 32, 16, 8, 4, 2)


def pooled(gt_with_ori):
    return [G.digest(F.max_pool2d(gt_with_ori[None], k, stride=k)[0]) for k in POOLS]


def forward_case(ref_models):
    c = TR.PRIOR36_CASE
    sd = synth.synthetic_state_dict("vigor", c["wseed"])
    net = ref_models.CVM_VIGOR_ori_prior("cpu", c["ori_noise"], True)
    net.load_state_dict(sd, strict=True)
    net.eval()
    grd, sat = synth.synthetic_pair(1, "vigor", c["pseed"])
    with torch.no_grad():
        out = net(grd, sat)
    d = {"shapes": np.array([list(t.shape) + [0] * (4 - t.dim()) for t in out], dtype=np.int64),
         "ndims": np.array([t.dim() for t in out], dtype=np.int64), "argmax0": out[0].argmax(1).numpy()}
    for i, stride in TR.PRIOR36_STRIDES.items():
        flat = out[i].reshape(-1).numpy()
        d["out%d" % i] = flat[G.spread_index(flat.size, stride)]
    return d


def state_dict_layouts(ref_models):
    return {kind: [[k, list(v.shape)] for k, v in net.state_dict().items()]
            for kind, net in (("vigor", ref_models.CVM_VIGOR("cpu", True)), ("kitti", ref_models.CVM_KITTI("cpu")),
                              ("oxford", ref_models.CVM_OxfordRobotCar("cpu")))}


def vigor_single(D, root):
    """test_oracle_vs_reference.test_dataset_ground_truth_and_input_transform_live"""
    TR.make_single_pano_tree(root)

    def tf(hw):
        return lambda im: O.preprocess_reference(np.asarray(im.convert("RGB")), hw)
    ds = D.VIGORDataset(root, split="samearea", train=True, transform=(tf((320, 640)), tf((512, 512))),
                        pos_only=True, ori_noise=180, random_orientation=TR.SINGLE_ORIENT)
    samples = []
    for i in range(len(ds)):
        grd, sat, gt, gt_with_ori, orientation, _, angle = ds[i]
        samples.append({"angle": float(angle), "grd": G.digest(grd), "gt": G.digest(gt), "orientation": G.digest(orientation),
                        "gt_with_ori_pooled": pooled(gt_with_ori)})
    return {"len": len(ds), "samples": samples}


def vigor_splits(D, root):
    """test_datasets.test_sample_matches_the_reference_dataset_live"""
    TD.make_vigor_tree(root, jpeg=True)

    def tf(hw):
        return lambda im: O.preprocess_reference(np.asarray(im.convert("RGB")), hw)
    orient = np.load(os.path.join(TD.GOLDEN, "crossarea_orientation_test_head256.npy"))
    res = {}
    for split, train in TD.VIGOR_LIVE_SPLITS:
        ref = D.VIGORDataset(root, split=split, train=train, transform=(tf((320, 640)), tf((512, 512))), pos_only=True,
                             ori_noise=180, random_orientation=orient)
        e = {"len": len(ref), "grd_list": [os.path.relpath(p, root) for p in ref.grd_list],
             "sat_list": [os.path.relpath(p, root) for p in ref.sat_list],
             "label": np.asarray(ref.label).tolist(), "delta": G.digest(np.asarray(ref.delta)), "samples": {}}
        for i in range(0, len(ref), 2):
            grd, sat, gt, gt_with_ori, orientation, city, angle = ref[i]
            s = {"city": city, "angle": float(angle), "grd": G.digest(grd), "sat": G.digest(sat), "gt": G.digest(gt),
                 "orientation": G.digest(orientation)}
            if train:
                s["gt_with_ori_pooled"] = pooled(gt_with_ori)
            e["samples"][str(i)] = s
        res["%s_%s" % (split, "train" if train else "test")] = e
    return res


def kitti(D, root):
    """test_datasets.test_kitti_sample_matches_the_reference_datasets_live"""
    train_file, test_file, _ = TD.make_kitti_tree(root)
    D.TF.center_crop = TD.kitti_center_crop

    def to_u8(im):
        return torch.from_numpy(np.array(im)).permute(2, 0, 1)
    res = {}
    for test in (False, True):
        cls = D.SatGrdDatasetTest if test else D.SatGrdDataset
        ref = cls(root, test_file if test else train_file, transform=(to_u8, to_u8), shift_range_lat=20, shift_range_lon=20,
                  rotation_range=(10 if test else 180))
        samples = []
        for i in range(len(ref)):
            np.random.seed(100 + i)
            sat, grd, gt, gt_with_ori, orientation, angle = ref[i]
            samples.append({"angle": float(angle), "sat": G.digest(sat.permute(1, 2, 0)),
                            "grd": G.digest(grd.permute(1, 2, 0).numpy().astype(np.float32)), "gt": G.digest(gt),
                            "orientation": G.digest(orientation), "gt_with_ori_pooled": pooled(gt_with_ori)})
        res["test" if test else "train"] = {"len": len(ref), "samples": samples}
    return res


def oxford(D, root):
    """test_datasets.test_oxford_sample_matches_the_reference_dataset_live"""
    g, sat_path = TD.make_oxford_tree(root)

    def to_u8(im):
        return torch.from_numpy(np.array(im.convert("RGB"))).permute(2, 0, 1)

    def to_512(im):
        return torch.from_numpy(np.array(im.convert("RGB").resize((512, 512)))).permute(2, 0, 1)
    res = {}
    for split in ("train", "val", "test"):
        ref = D.OxfordRobotCarDataset(g, sat_path, split=split, transform=(to_u8, to_512))
        samples = []
        for i in range(len(ref)):
            random.seed(50 + i)
            grd, sat, gt, gt_with_ori, orientation, angle = ref[i]
            samples.append({"angle": float(angle), "grd": G.digest(grd.permute(1, 2, 0)), "sat": G.digest(sat.permute(1, 2, 0)),
                            "gt": G.digest(gt), "orientation": G.digest(orientation), "gt_with_ori_pooled": pooled(gt_with_ori)})
        res[split] = {"len": len(ref), "samples": samples}
    return res


def main():
    torch.set_num_threads(8)
    ref_models, _ = import_reference()
    D = import_reference_datasets()
    d = forward_case(ref_models)
    path = os.path.join(G.GOLDEN_DIR, "ref_vigor_prior36.npz")
    np.savez_compressed(path, **d)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))
    live = {"state_dict_layout": state_dict_layouts(ref_models)}
    for key, fn in (("vigor_single", vigor_single), ("vigor_splits", vigor_splits), ("kitti", kitti), ("oxford", oxford)):
        tmp = tempfile.mkdtemp()
        try:
            live[key] = fn(D, tmp)
        finally:
            shutil.rmtree(tmp)
    path = os.path.join(G.GOLDEN_DIR, "reference_live.json")
    with open(path, "w") as f:
        json.dump(live, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
