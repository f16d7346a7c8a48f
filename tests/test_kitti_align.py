"""ccvpe_amd/align.py — the numpy restatement of Pillow's geometry that specifies ccvpe_kitti_align_u8 — against LIVE Pillow:
each pass alone, the whole lazy chain, and KITTIPairs(device_align=True).  Equal bytes everywhere, no tolerance."""
import numpy as np
import pytest

import kitti_align_cases as K
from ccvpe_amd import align
from ccvpe_amd import datasets as DS
from test_datasets import make_kitti_tree

PASS_SOURCES = ("s97x131", "s96x80", "s81")
ANGLES = (0.0, 90.0, 180.0, 270.0, 360.0, -90.0, 33.3, 123.4, 211.1, 359.9, -7.25, 1e-14, 180.0 - 1e-13, 540.0, -0.0,
          -3.14159 / np.pi * 180, 3.1415926 / np.pi * 180)
SHIFTS = ((0.0, 0.0), (3.0, -2.0), (0.5, 0.25), (-0.25, 0.5), (5.515152, 1.3276), (-17.77, 9.13), (60.2, -0.6), (-0.3, 200.0),
          (1e-9, -1e-9), (130.5, 0.0))


def test_align_module_does_not_import_pillow():
    src = open(align.__file__).read()
    assert "import PIL" not in src and "from PIL" not in src


@pytest.mark.parametrize("name", PASS_SOURCES)
def test_nearest_pass_alone_equals_pillow_rotate(name):
    from PIL import Image
    src = K.source(name)
    h, w = src.shape[:2]
    im = Image.fromarray(src, "RGB")
    for angle in ANGLES:
        want = np.array(im.rotate(angle))
        got = align.affine_nearest(src, align.rotate_fixed(angle, w, h))
        assert np.array_equal(got, want), "%s rotate(%r): %d bytes differ" % (name, angle, int((got != want).sum()))
        if angle % 360.0 in (0.0, 180.0) or (angle % 360.0 in (90.0, 270.0) and w == h):
            # Pillow's transpose shortcuts also equal the generic fixed-point walk of the rounded matrix
            walk = align.affine_nearest(src, align.fix_matrix(align.rotate_matrix(angle, w, h)))
            assert np.array_equal(walk, want), "%s rotate(%r) by matrix" % (name, angle)


@pytest.mark.parametrize("name", PASS_SOURCES)
def test_bilinear_pass_alone_equals_pillow_transform(name):
    from PIL import Image
    src = K.source(name)
    im = Image.fromarray(src, "RGB")
    for tx, ty in SHIFTS:
        want = np.array(im.transform(im.size, Image.AFFINE, (1, 0, tx, 0, 1, ty), resample=Image.BILINEAR))
        got = align.translate_bilinear(src, tx, ty)
        assert np.array_equal(got, want), "%s translate(%r, %r): %d bytes differ" % (name, tx, ty, int((got != want).sum()))


def test_case_table_is_visible():
    frac = K.check_inputs_are_visible(K.CASES)
    assert {c.src for c in K.CASES} == {"s97x131", "s96x80", "s81", "s640"}
    assert sum(c.empty for c in K.CASES) >= 1 and any(0.4 < frac[c.name] < 0.9 for c in K.CASES)     # wholly / partly outside


@pytest.mark.parametrize("case", K.CASES, ids=[c.name for c in K.CASES])
def test_lazy_chain_equals_pillow(case):
    want = K.expected(case)
    got = align.align_reference(K.source(case.src), K.params(case), case.crop)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), "%s: %d of %d bytes differ" % (case.name, int((got != want).sum()), want.size)


def test_parameter_row_layout():
    row = align.kitti_align_params(0.3, (5.5, 1.25), (-2.0, 3.0), 7.0, 131, 97, 64)
    assert row.dtype == np.int64 and row.shape == (align.ROW_LEN,)
    assert tuple(row[0:6]) == align.rotate_fixed(-0.3 / np.pi * 180, 131, 97) and tuple(row[6:12]) == align.rotate_fixed(7.0, 131, 97)
    assert tuple(row[12:16].view(np.float64)) == (5.5, 1.25, -2.0, 3.0)
    assert tuple(row[16:20]) == (131, 97, int(round((131 - 64) / 2.0)), int(round((97 - 64) / 2.0)))
    assert align.fix(0.5) == 32768 and align.fix(-0.5) == -32768 and align.fix(-1.0 / 131072) == 0      # floor(v * 65536 + 0.5)
    assert align.rotate_fixed(0.0, 131, 97) == align.rotate_fixed(360.0, 131, 97) == (65536, 0, 32768, 0, 65536, 32768)


def _same_but_aerial(a, b):
    assert [k for k in a if k not in ("sat_src_u8", "align")] == [k for k in b if k != "sat_u8"]
    for k in b:
        if k == "sat_u8":
            continue
        if isinstance(b[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k] and type(a[k]) is type(b[k]), k


@pytest.fixture(scope="module")
def kitti_tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kitti_align"))
    train_file, test_file, names = make_kitti_tree(root)
    return root, train_file, test_file, names


def test_device_align_sample_equals_host_sample_on_the_test_file(kitti_tree):
    root, _, test_file, names = kitti_tree
    host = DS.KITTIPairs(root, test_file, 20, 20, 10, test=True)
    dev = DS.KITTIPairs(root, test_file, 20, 20, 10, test=True, device_align=True)
    for i in range(len(names)):
        a, b = dev.sample(i), host.sample(i)
        assert "sat_u8" not in a and a["sat_src_u8"].shape == (640, 640, 3) and a["sat_src_u8"].dtype == np.uint8
        assert list(b) == ["grd_u8", "sat_u8", "roll", "angle_deg", "center", "city", "index"]         # the host path's dict is unchanged
        assert np.array_equal(align.align_reference(a["sat_src_u8"], a["align"]), b["sat_u8"]), i
        assert np.count_nonzero(b["sat_u8"]) > 0.4 * b["sat_u8"].size
        _same_but_aerial(a, b)


def test_device_align_sample_equals_host_sample_on_seeded_training_draws(kitti_tree):
    root, train_file, _, names = kitti_tree
    host = DS.KITTIPairs(root, train_file, 20, 20, 10, rng=np.random.default_rng(11))
    dev = DS.KITTIPairs(root, train_file, 20, 20, 10, rng=np.random.default_rng(11), device_align=True)
    for i in list(range(len(names))) + [1, 0]:                        # the generators advance in step: the same draws
        a, b = dev.sample(i), host.sample(i)
        assert np.array_equal(align.align_reference(a["sat_src_u8"], a["align"]), b["sat_u8"]), i
        _same_but_aerial(a, b)
    # draws handed in (as DeviceBatches does, from the producer thread) are used as they are
    d = (0.31, -0.77, 9.5)
    a, b = dev.sample(2, draws=d), host.sample(2, draws=d)
    assert np.array_equal(align.align_reference(a["sat_src_u8"], a["align"]), b["sat_u8"])
    _same_but_aerial(a, b)
    # a rotation range of 180 degrees (all quadrants) and numpy's global generator
    np.random.seed(5)
    b = [DS.KITTIPairs(root, train_file, 20, 20, 180).sample(i) for i in range(2)]
    np.random.seed(5)
    a = [DS.KITTIPairs(root, train_file, 20, 20, 180, device_align=True).sample(i) for i in range(2)]
    for x, y in zip(a, b):
        assert np.array_equal(align.align_reference(x["sat_src_u8"], x["align"]), y["sat_u8"])
        _same_but_aerial(x, y)


def test_c_entry_validates_before_launching():
    """Host-only: bad shapes and null pointers come back as CCVPE_EINVAL with a message, nothing is enqueued."""
    from ccvpe_amd import _lib
    lib = _lib.load()
    assert lib.ccvpe_kitti_align_u8(None, 100, 256, 256, 1, 256, 8, 8, None) == -1 and b"null pointer" in lib.ccvpe_last_error()
    for batch, ch, cw, nbytes in ((0, 8, 8, 100), (70000, 8, 8, 100), (1, 0, 8, 100), (1, 8, 40000, 100), (1, 8, 8, 0)):
        assert lib.ccvpe_kitti_align_u8(256, nbytes, 256, 256, batch, 256, ch, cw, None) == -1
        assert b"bad shape" in lib.ccvpe_last_error()
