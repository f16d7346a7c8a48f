"""The LDS bank model (tools/lds_layout.py) on the stage-1 fragment reads of the three-plane tail (csrc/tail512.hip, SPLIT == 3):
a staged pixel row is [hi 0..15 | mid 0..15 | lo 0..15] bf16 = all 96 bytes of the wide slot, and per (tile, tap) a wave reads
three B fragments — [x_hi | x_hi], [x_mid | x_mid], [x_lo | x_hi] — at per-lane addresses.  The geometry is the two-plane one,
read from the source; every one of the three reads must cost the conflict-free 4 LDS cycles, for every full tile and tap."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lds_layout as L      # noqa: E402


def test_three_plane_fragment_reads_are_conflict_free_in_the_wide_slot():
    src = open(os.path.join(ROOT, "ccvpe_amd", "csrc", "tail512.hip")).read()
    m = re.search(r"static constexpr int LD = WIDE_SLOT \? (\d+) : (\d+);", src)
    n = re.search(r"static constexpr int HCP = WIDE_SLOT \? (\d+) : HC;", src)
    assert m and n, "TailGeom's slot geometry moved: update this test"
    ld, hcp = int(m.group(1)), int(n.group(1))
    assert ld * 4 == 96, "three bf16 planes of 16 channels fill a 96-byte slot"
    # the kernel's address rule, restated: fbase = slot * LD + (q & 1) * 4; fragment h at + 8 h floats, except that lane groups
    # 2, 3 of the third fragment read the hi plane (f3off = q < 2 ? 16 : 0)
    assert "fbase[i] = (iy * HCP + ix) * LD + (SPLIT == 3 ? qv & 1 : qv) * 4;" in src
    assert "const int f3off = qv < 2 ? 16 : 0;" in src and "(h == 1 ? 8 : 0)" in src and "h == 2 ? f3off : 0" in src
    ty, tx = 8, 16
    pw, npos = tx + 1, (ty + 1) * (tx + 1)

    def frag(tile, tap, h):
        def addr(lane):
            pc = min(tile * 16 + lane % 16, npos - 1)
            iy, ix = pc // pw, pc % pw
            q = lane // 16
            plane = (8 if h == 1 else 0) + ((16 if q < 2 else 0) if h == 2 else 0)
            return ((iy + (tap >> 1)) * hcp + ix + (tap & 1)) * ld + 4 * (q & 1) + plane
        return addr

    nfull = npos // 16                                     # the last tile of a parity is ragged (clamped lanes): not asserted
    cyc = [L.cycles("read_b128", frag(t, tap, h))[0] for t in range(nfull) for tap in range(4) for h in range(3)]
    assert len(cyc) == nfull * 12 and max(cyc) == 4, cyc   # 4 LDS cycles per ds_read_b128: conflict-free
    # the 80-byte slot could not hold three planes; the 96-byte slot in rows of TX + 2 (no row padding) would conflict
    plain = [L.cycles("read_b128", (lambda lane, t=t, tap=tap: ((min(t * 16 + lane % 16, npos - 1) // pw + (tap >> 1)) * (tx + 2) +
                                                               min(t * 16 + lane % 16, npos - 1) % pw + (tap & 1)) * ld + 4 * ((lane // 16) & 1)))[0]
             for t in range(nfull) for tap in range(4)]
    assert max(plain) > 4
    assert (ty + 2) * hcp * ld * 4 * 2 <= 48 * 1024         # two chunk buffers: no LDS growth over the two-plane tile
