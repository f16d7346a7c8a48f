"""Quad form of the three-plane bf16 upconv kernel (csrc/upconv_s3q.hip), on the CPU: every fragment read of its phase-A halo
and of its four skip parity planes is conflict-free in the bank model of tools/lds_layout.py, for every window base the kernel
can produce; the parity planes hold exactly the high-res pixels the nine taps of the four parities read; the LDS bytes of each
instantiated tile stay inside the two-workgroups-per-CU bound.  The geometry is read from the kernel source."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "ccvpe_amd", "csrc", "upconv_s3q.hip")).read()


def _const(name):
    m = re.search(r"static constexpr int[^;]*?\b%s = ([^,;]+)[,;]" % name, SRC)
    assert m, name
    return m.group(1).strip()


def _geom(nt):
    """UpS3qGeom<NT>, evaluated from the source's own expressions"""
    env = {"NT": nt}
    for name in ("TH", "HR", "HC", "PR", "PC", "ROW", "NP", "HALO_DW", "PLANES_DW", "WA_INSTR", "WA_DW", "WB_INSTR", "WB_DW"):
        env[name] = eval(_const(name).replace("/", "//"), {}, env)
    g = re.fullmatch(r"NT == 2 \? (\d+) : \(NT == 3 \? (\d+) : (\d+)\)", _const("G"))
    env["G"] = int(g.group(1)) if nt == 2 else int(g.group(2)) if nt == 3 else int(g.group(3))
    env["A_DW"] = eval(_const("A_DW"), {}, env)
    env["B_DW"] = eval(_const("B_DW"), {}, env)
    assert _const("LDS_BYTES") == "(A_DW > B_DW ? A_DW : B_DW) * 4"
    env["LDS_BYTES"] = max(env["A_DW"], env["B_DW"]) * 4
    return env


def _slots():
    exprs = dict(re.findall(r"const int ([aw]\doff) = ([^;]+);", SRC))
    assert sorted(exprs) == ["a1off", "a2off", "w1off", "w2off", "w3off"], exprs

    def slot(expr):                                               # C "c ? a : b" -> a Python function of the lane group g4
        m = re.fullmatch(r"(.+?) \? (.+?) : (.+)", expr)
        py = "(%s) if (%s) else (%s)" % (m.group(2), m.group(1), m.group(3)) if m else expr
        return lambda g4: eval(py, {"g4": g4})
    return {k: slot(v) for k, v in exprs.items()}


def test_instantiated_tiles_fit_two_workgroups_per_cu():
    # the one list the quad form's N range and its launch are generated from
    nts = sorted(int(v) for v in re.findall(r"X\((\d)\)", re.search(r"#define CCVPE_S3Q_NTS\(X\)(.*)", SRC).group(1)))
    assert nts == [2, 3, 4, 5]
    assert "if (nt == NT_) return launch_s3q<NT_>(p, stream);" in SRC and SRC.count("CCVPE_S3Q_NTS(CCVPE_CASE)") == 2
    assert "static_assert(G::LDS_BYTES <= 80 * 1024" in SRC
    for nt in nts:
        g = _geom(nt)
        assert (g["TH"], g["HR"], g["HC"], g["PR"], g["PC"], g["ROW"]) == (8, 10, 18, 9, 17, 24)
        assert g["NP"] == 16 * nt
        # a phase-A panel is the four taps of one (parity, chunk): 4 NP rows of 96 bytes, whole 1 KB pieces
        assert g["WA_INSTR"] * 1024 == 4 * g["NP"] * 96
        # a phase-B panel is one tap: NP rows, rounded up to whole pieces
        assert (g["WB_INSTR"] - 1) * 1024 < g["NP"] * 96 <= g["WB_INSTR"] * 1024
        assert g["HALO_DW"] * 4 == 10 * 18 * 96 and g["PLANES_DW"] * 4 == 18 * 34 * 96
        assert 36 % g["G"] == 0 and (36 // g["G"]) % 2 == 0          # whole stages per block; the two buffers alternate evenly
        assert g["LDS_BYTES"] <= 80 * 1024, (nt, g["LDS_BYTES"])
        # the largest G that fits: one more tap per stage would not
        bigger = [x for x in (2, 3, 4, 6) if x > g["G"]]
        assert all((g["PLANES_DW"] + 2 * x * g["WB_DW"]) * 4 > 80 * 1024 for x in bigger[:1]), nt


def test_parity_planes_hold_what_the_taps_read():
    """Output parity (py, px), tap (ky, kx), low-res pixel (ly, lx) of the tile reads high-res halo pixel (2 ly + py + ky,
    2 lx + px + kx); the kernel finds it in plane ((r & 1), (c & 1)) at (ly + (r >> 1), lx + (c >> 1)), r = py + ky, c = px + kx,
    and the staging puts halo pixel (hy, hx) into plane (hy & 1, hx & 1) at (hy >> 1, hx >> 1)."""
    assert "(((hy & 1) * 2 + (hx & 1)) * PR + (hy >> 1)) * PC + (hx >> 1)" in SRC
    assert "((((r & 1) * 2 + (c & 1)) * PR + (r >> 1)) * PC + (c >> 1)) * ROW" in SRC
    assert "const int r = (par >> 1) + tap / 3, c = (par & 1) + tap % 3;" in SRC
    g = _geom(3)
    stage = lambda hy, hx: (((hy & 1) * 2 + (hx & 1)) * g["PR"] + (hy >> 1)) * g["PC"] + (hx >> 1)
    cells = {stage(hy, hx) for hy in range(2 * g["TH"] + 2) for hx in range(34)}
    assert len(cells) == 18 * 34 == 4 * g["PR"] * g["PC"] and max(cells) == 4 * g["PR"] * g["PC"] - 1     # a bijection onto the planes
    for par in range(4):
        for tap in range(9):
            r, c = (par >> 1) + tap // 3, (par & 1) + tap % 3
            for ly in range(g["TH"]):
                for lx in range(16):
                    read = (((r & 1) * 2 + (c & 1)) * g["PR"] + (r >> 1) + ly) * g["PC"] + (c >> 1) + lx
                    assert read == stage(2 * ly + (par >> 1) + tap // 3, 2 * lx + (par & 1) + tap % 3)


def test_fragment_reads_are_conflict_free_for_every_window_base():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import lds_layout as L
    slots = _slots()
    g = _geom(3)
    row = g["ROW"]
    # the planes each fragment must deliver: 16-byte slots 0-1 = hi, 2-3 = mid, 4-5 = lo (as the per-parity kernel)
    want = {"a1off": [0, 1, 2, 3], "a2off": [4, 5, 0, 1], "w1off": [0, 1, 0, 1], "w2off": [2, 3, 2, 3], "w3off": [0, 1, 4, 5]}
    for name, f in slots.items():
        assert [f(q) // 4 for q in range(4)] == want[name] and all(f(q) % 4 == 0 for q in range(4)), name
    bases = set()
    for wave in range(4):
        for i in range(2):
            for par in range(4):
                py, px = par >> 1, par & 1
                for tap in range(4):                          # phase A: halo pixel (2 wave + i + du + py, dv + px) on
                    bases.add(((wave * 2 + i + (tap >> 1) + py) * g["HC"] + (tap & 1) + px))
                for tap in range(9):                          # phase B: plane pixel
                    r, c = py + tap // 3, px + tap % 3
                    bases.add((((r & 1) * 2 + (c & 1)) * g["PR"] + wave * 2 + i + (r >> 1)) * g["PC"] + (c >> 1))
    assert {v % 8 for v in bases} == set(range(8))            # 24 dwords a pixel: the bank pattern repeats every 8 pixels
    for base in sorted(bases):
        for name in ("a1off", "a2off"):
            addr = lambda lane: (base + lane % 16) * row + slots[name](lane // 16)
            assert L.cycles("read_b128", addr) == (4, 4), (name, base)
    # W rows: panel bases are multiples of 256 dwords (1 KB pieces), column tile j starts 16 rows further
    for nt in (2, 3, 4, 5):
        gg = _geom(nt)
        for base in {gg["HALO_DW"] % 64, gg["PLANES_DW"] % 64, (gg["HALO_DW"] + gg["NP"] * row) % 64}:
            for j in range(nt):
                for name in ("w1off", "w2off", "w3off"):
                    addr = lambda lane: base + (j * 16 + lane % 16) * row + slots[name](lane // 16)
                    assert L.cycles("read_b128", addr) == (4, 4), (name, nt, j)
