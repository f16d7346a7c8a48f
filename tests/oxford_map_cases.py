"""Shared case table of the device-resident aerial map tests (test_oxford_map.py on the host, test_oxford_map_gpu.py on the
device): (map h x w, box h x w, out h x w, origins (x0, y0)) on small seeded random maps.  The kernel tiles the output
16 rows x 128 columns, takes a 16-byte-store form when out_w % 4 == 0 and a scalar form otherwise; the table crosses each of
those boundaries and every border relation between a window and the map."""
import collections

import numpy as np

Case = collections.namedtuple("Case", "name map_hw box_hw out_hw origins")

CASES = (
    # the workload geometry: 800 x 800 -> 512 x 512 (ksize 5), one window inside, one across the top-left corner
    Case("workload", (1000, 900), (800, 800), (512, 512), ((60, 120), (-37, -5))),
    # ragged, non-square, both output sizes odd (scalar store form): ksize 5 rows, ksize 5 columns
    Case("ragged_29x37", (90, 110), (45, 70), (29, 37), ((11, 7), (-3, 60), (50, -9))),
    # one axis reduces (45 -> 29 rows) while the other enlarges (30 -> 37 columns)
    Case("reduce_rows_enlarge_cols", (90, 110), (45, 30), (29, 37), ((11, 7), (95, 60))),
    Case("enlarge_20_32", (50, 60), (20, 20), (32, 32), ((5, 9), (-4, 41))),
    Case("equal_24", (50, 60), (24, 24), (24, 24), ((0, 0), (36, 26), (47, -11))),
    Case("reduce4_128_32", (200, 180), (128, 128), (32, 32), ((20, 30), (-60, 100))),                    # ksize 9
    # borders: negative origin; past the right and bottom edges; wholly outside (four sides); x0 + box_w == map_w exactly
    Case("borders", (70, 80), (32, 40), (24, 28), ((-13, -7), (55, 50), (-40, 10), (80, 10), (10, -32), (10, 70), (500, -900),
                                                    (40, 19), (40, 38), (0, 0))),
    Case("single", (64, 64), (33, 31), (17, 20), ((9, 14),)),                                            # B = 1
    Case("duplicates", (64, 64), (33, 31), (17, 20), ((9, 14), (40, 40), (9, 14), (-5, 3), (40, 40))),   # B = 5
    # more than one 128-column tile with a scalar-form width, and a vector-form width whose last tile is 4 columns wide
    Case("wide_scalar_150", (60, 300), (30, 200), (20, 150), ((50, 10), (-20, 45))),
    Case("wide_vector_132", (60, 300), (40, 100), (35, 132), ((150, 5), (230, -8))),
)


def case_map(case):
    """The case's map: seeded by its shape, uniform random bytes with a few saturated blocks (clip8 at both ends)."""
    h, w = case.map_hw
    m = np.random.RandomState(h * 100003 + w).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    m[: h // 5, : w // 4] = 255
    m[h // 2: h // 2 + 3, :] = 0
    return m


def pillow_windows(map_u8, case):
    """Live Pillow: the zero-filled crops [B, box_h, box_w, 3] and their BILINEAR resizes [B, out_h, out_w, 3], uint8."""
    from PIL import Image
    im = Image.fromarray(map_u8, "RGB")
    (bh, bw), (h, w) = case.box_hw, case.out_hw
    crops = [im.crop((x0, y0, x0 + bw, y0 + bh)) for x0, y0 in case.origins]
    return (np.stack([np.array(c) for c in crops]),
            np.stack([np.array(c.resize((w, h), Image.BILINEAR)) for c in crops]))


def normalise(res_u8, mean, std):
    """ToTensor + Normalize of [B, h, w, 3] uint8 in fp32, operation for operation: [B, 3, h, w]."""
    m = np.asarray(mean, dtype=np.float32).reshape(1, 1, 1, 3)
    s = np.asarray(std, dtype=np.float32).reshape(1, 1, 1, 3)
    v = res_u8.astype(np.float32) / np.float32(255.0)
    return np.ascontiguousarray(((v - m) / s).transpose(0, 3, 1, 2))
