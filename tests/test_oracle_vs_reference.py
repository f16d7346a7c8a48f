"""The oracle against the reference itself, through the reference's outputs stored in tests/golden/ (ref_vigor_prior36.npz,
reference_live.json; written by tools/make_golden_reference.py where the reference is present).  The inputs — synthetic
weights and pair, the tiny dataset directory — are rebuilt here bit-exactly.  The dataset and layout comparisons are the
same as against a live reference; the forward's large outputs are compared on stored samples (PRIOR36_STRIDES)."""
import os

import numpy as np
import torch

import golden_util as G
from ccvpe_amd import synth
from oracle import ccvpe_oracle as O

PRIOR36_CASE = dict(ori_noise=36, wseed=0, pseed=4321)
# output -> sampling stride of the stored reference values (golden_util.spread_index): the logits and the two finest score
# volumes are sampled (every element of them would take 1.4 MB at the tolerances below), the coarser volumes are whole
PRIOR36_STRIDES = {0: 8, 3: 1, 4: 1, 5: 1, 6: 2, 7: 8, 8: 16}
SINGLE_CITIES = ["NewYork", "Seattle", "SanFrancisco", "Chicago"]
SINGLE_ORIENT = np.array([0.0, 17.5, 200.25, 359.0])


def make_single_pano_tree(root):
    """A VIGOR directory with one panorama and one aerial tile per city (PNG); returns {city: (row, col) offset}."""
    from PIL import Image
    root = str(root)
    rng = np.random.RandomState(3)
    deltas = {}
    for ci, city in enumerate(SINGLE_CITIES):
        os.makedirs(os.path.join(root, "splits_new", city))
        os.makedirs(os.path.join(root, city, "satellite"))
        os.makedirs(os.path.join(root, city, "panorama"))
        sat = (rng.rand(64, 64, 3) * 255).astype(np.uint8)
        Image.fromarray(sat, "RGB").save(os.path.join(root, city, "satellite", "s.png"))
        pano = (rng.rand(96, 192, 3) * 255).astype(np.uint8)
        Image.fromarray(pano, "RGB").save(os.path.join(root, city, "panorama", "p.png"))
        with open(os.path.join(root, "splits_new", city, "satellite_list.txt"), "w") as f:
            f.write("s.png\n")
        d = (7.0 * ci - 5.0, -3.0 * ci + 11.0)                  # (row, col) offsets in raw satellite pixels
        deltas[city] = d
        line = "p.png " + " ".join("s.png %f %f" % d for _ in range(4)) + "\n"
        with open(os.path.join(root, "splits_new", city, "same_area_balanced_train.txt"), "w") as f:
            f.write(line)
    return deltas


def test_vigor_ori_prior_live(synth_sd):
    """CVM_VIGOR_ori_prior(ori_noise=36) against the reference's forward of the same weights and pair: every output shape
    and the logits' arg-max exactly; the logits within 2e-5 and the six score volumes within 2e-6 on the stored samples."""
    want = G.load("ref_vigor_prior36")
    c = PRIOR36_CASE
    sd = synth_sd("vigor", c["wseed"])
    grd, sat = synth.synthetic_pair(1, "vigor", c["pseed"])
    with torch.no_grad():
        got = O.forward(sd, grd, sat, "vigor", True, ori_noise=c["ori_noise"])
    want_shapes = [tuple(int(v) for v in s[:n]) for s, n in zip(want["shapes"], want["ndims"])]
    assert [tuple(t.shape) for t in got] == want_shapes
    assert got[0].argmax(1).tolist() == want["argmax0"].tolist()
    for i, stride in PRIOR36_STRIDES.items():
        flat = got[i].reshape(-1)
        idx = G.spread_index(flat.numel(), stride)
        w = torch.from_numpy(want["out%d" % i])
        assert w.numel() == len(idx)
        assert (flat[torch.from_numpy(idx)] - w).abs().max() < (2e-5 if i == 0 else 2e-6), "output %d" % i


def test_state_dict_layout_matches_reference():
    layouts = G.load_json("reference_live")["state_dict_layout"]
    for kind in ("vigor", "kitti", "oxford"):
        ref = layouts[kind]
        spec = synth.state_dict_spec(kind)
        assert [k for k, _, _ in spec] == [k for k, _ in ref]
        for (k, shape, _), (_, ref_shape) in zip(spec, ref):
            assert tuple(ref_shape) == tuple(shape), k


def test_dataset_ground_truth_and_input_transform_live(tmp_path):
    """the reference's own VIGORDataset.__getitem__ (datasets.py:98-177) on a tiny synthetic dataset
    directory (stored samples) against the oracle: its ground truth (gt, gt_with_ori, orientation) against
    oracle.train_targets, and its ground image (Resize -> ToTensor -> Normalize given as the transform, then the dataset's
    torch.roll) against oracle.preprocess_reference.  torchvision is absent where the fixture is made, so the transform
    passed in is the PIL + torch arithmetic torchvision performs (PIL is the real dependency)."""
    from PIL import Image
    ref = G.load_json("reference_live")["vigor_single"]
    deltas = make_single_pano_tree(tmp_path)
    orient = SINGLE_ORIENT
    assert ref["len"] == 4
    for i, city in enumerate(SINGLE_CITIES):
        r = ref["samples"][i]
        assert abs(r["angle"] - orient[i]) < 1e-9
        # ---- ground truth: cx = col_offset, cy = -row_offset (offsets rescaled to the 512 grid as the dataset does)
        row = np.round(deltas[city][0] / 64 * 512)
        col = np.round(deltas[city][1] / 64 * 512)
        g, flat, ori, labs = O.train_targets([[col, -row]], [orient[i]], 20)
        assert G.digest(g[0]) == r["gt"] and G.digest(ori[0]) == r["orientation"]
        for lab, want in zip(labs, r["gt_with_ori_pooled"]):
            assert G.digest(lab[0]) == want
        assert abs(float(flat.sum()) - 1.0) < 1e-5
        # ---- input transform + panorama roll (datasets.py:121)
        pano = np.asarray(Image.open(os.path.join(str(tmp_path), city, "panorama", "p.png")).convert("RGB"))
        roll = int(torch.round(torch.as_tensor(orient[i] / 360) * 640).int())
        assert G.digest(O.preprocess_reference(pano, (320, 640), roll=roll)) == r["grd"]
