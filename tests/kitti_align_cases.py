"""The case table of tests/test_kitti_align.py (numpy restatement vs Pillow, CPU) and tests/test_kitti_align_gpu.py
(ccvpe_kitti_align_u8 vs Pillow): sources, headings, translations and rotations of the KITTI aerial alignment, and the
Pillow chain itself — the four calls of ccvpe_amd/datasets.py KITTIPairs.sample, which are the reference's."""
import collections

import numpy as np

Case = collections.namedtuple("Case", "name src crop heading cam shift ori empty")
# sources: name -> (h, w, seed)
SOURCES = {"s97x131": (97, 131, 1), "s96x80": (96, 80, 2), "s81": (81, 81, 3), "s640": (640, 640, 4), "s1280": (1280, 1280, 5)}
CAM = (1.08 / 0.19582850865, 0.26 / 0.19582850865)          # the camera offset in pixels of the real maps: (5.515.., 1.327..)
PI = float(np.pi)

CASES = [
    # all four quadrants of both rotations, generic fractions
    Case("q1", "s97x131", 64, 0.3, CAM, (3.7, -2.2), 7.3, False),
    Case("q2", "s97x131", 64, 2.0, CAM, (-4.4, 1.9), -8.1, False),
    Case("q3", "s97x131", 64, -2.5, CAM, (2.25, 0.5), 100.0, False),
    Case("q4", "s97x131", 64, -0.9, CAM, (0.0, 0.0), 200.5, False),
    # headings next to +-pi (rotation by almost 180 degrees) and exactly +-pi (the ROTATE_180 shortcut)
    Case("pi-", "s97x131", 64, 3.14159, CAM, (1.5, -0.75), 3.0, False),
    Case("-pi+", "s97x131", 64, -3.1415926, CAM, (-2.0, 2.0), -9.9, False),
    Case("pi", "s97x131", 64, PI, CAM, (1.0, 1.0), 0.0, False),
    # 0 / 90 / 180 / 270 on a NON-square source: 0 and 180 are shortcuts, 90 and 270 take the matrix
    Case("n0", "s97x131", 64, 0.0, (0.0, 0.0), (0.0, 0.0), 0.0, False),
    Case("n90", "s97x131", 64, 0.0, CAM, (0.5, 0.25), 90.0, False),
    Case("n180", "s97x131", 64, 0.0, CAM, (-3.0, 2.0), 180.0, False),
    Case("n270", "s97x131", 64, -PI / 2, CAM, (0.3, 0.6), 270.0, False),
    # integer / half / quarter shifts (dx exactly zero or representable), windows partly and wholly outside
    Case("int", "s96x80", 48, 1.1, (3.0, -2.0), (-5.0, 4.0), 4.0, False),
    Case("half", "s96x80", 48, -1.7, (0.5, 0.25), (-0.25, 0.5), -6.0, False),
    Case("partx", "s96x80", 48, 0.2, CAM, (30.0, 0.0), 2.0, False),
    Case("party", "s96x80", 48, 0.2, CAM, (-2.5, -33.3), 358.0, False),
    Case("out", "s96x80", 48, 0.7, CAM, (500.0, 0.0), 5.0, True),
    Case("outy", "s96x80", 48, 0.7, CAM, (0.0, -96.0), 5.0, True),
    # the whole image as the window (odd size), 0 / 90 / 180 / 270 on a SQUARE source: every one a shortcut
    Case("w0", "s81", 81, 0.0, (0.0, 0.0), (0.0, 0.0), 0.0, False),
    Case("w90", "s81", 81, -PI / 2, (0.0, 0.0), (0.0, 0.0), 90.0, False),
    Case("w180", "s81", 81, PI, (1.0, 0.0), (0.0, -1.0), 180.0, False),
    Case("w270", "s81", 81, PI / 2, (0.5, 0.5), (0.25, 0.0), 270.0, False),
    Case("wgen", "s81", 81, 0.61, CAM, (-1.3, 0.9), -4.2, False),
    # the real crop, training- and test-sized perturbations (20 m = 102 pixels)
    Case("k1", "s640", 512, 1.234567, CAM, (37.91, -61.27), 8.77, False),
    Case("k2", "s640", 512, -2.87, CAM, (-102.1, 99.3), -9.6, False),
]
CASE_1280 = Case("k1280", "s1280", 512, 0.345678, CAM, (-88.25, 41.5), -7.31, False)

_sources = {}


def source(name):
    """The case's source image [h, w, 3] uint8 (uniform noise: 255 of 256 bytes are non-zero, so an image region cannot be
    mistaken for fill)."""
    if name not in _sources:
        h, w, seed = SOURCES[name]
        img = np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        img.setflags(write=False)
        _sources[name] = img
    return _sources[name]


def pillow_chain(src_u8, heading, cam, shift, ori, crop):
    """KITTIPairs.sample's alignment, with Pillow: [crop, crop, 3] uint8."""
    from PIL import Image
    sat = Image.fromarray(src_u8, "RGB")
    sat = sat.rotate(-heading / np.pi * 180)
    sat = sat.transform(sat.size, Image.AFFINE, (1, 0, cam[0], 0, 1, cam[1]), resample=Image.BILINEAR)
    sat = sat.transform(sat.size, Image.AFFINE, (1, 0, shift[0], 0, 1, shift[1]), resample=Image.BILINEAR)
    sat = sat.rotate(ori)
    w, h = sat.size
    left, top = int(round((w - crop) / 2.0)), int(round((h - crop) / 2.0))
    return np.array(sat.crop((left, top, left + crop, top + crop)))


_expected = {}


def expected(case):
    """Pillow's result for a case, computed once and shared (read-only)."""
    if case.name not in _expected:
        out = pillow_chain(source(case.src), case.heading, case.cam, case.shift, case.ori, case.crop)
        out.setflags(write=False)
        _expected[case.name] = out
    return _expected[case.name]


def params(case):
    from ccvpe_amd import align
    h, w, _ = SOURCES[case.src]
    return align.kitti_align_params(case.heading, case.cam, case.shift, case.ori, w, h, case.crop)


def check_inputs_are_visible(cases):
    """The condition on the inputs that keeps an all-zero output from passing: every case not built to be empty has more than
    40 % non-zero bytes in Pillow's own result, at least three have more than 90 %, the empty ones are empty."""
    frac = {c.name: float(np.count_nonzero(expected(c))) / expected(c).size for c in cases}
    for c in cases:
        if c.empty:
            assert frac[c.name] == 0.0, (c.name, frac[c.name])
        else:
            assert frac[c.name] > 0.40, (c.name, frac[c.name])
    assert sum(v > 0.90 for v in frac.values()) >= 3, frac
    return frac
