"""The folded deconv + 3x3 launchers' answers over a sweep of descriptors, against the table recorded beside this file
(tests/upconv_route_table.json, written by tools/make_upconv_route_table.py from the library built from the commit BEFORE the
launchers were split into up_fill / up_pick / upconv_run and s3_pick, loaded through CCVPE_LIB): ccvpe_upconv3x3_route for fp32
and bf16, ccvpe_upconv3x3_s3_ok and ccvpe_upconv3x3_s3_form_ok for forms 0..3, every N = 8, 16, .. 1344, at all switch
positions.  Host code only: no GPU, fake aligned pointers.  The table is the reference: a change that moves a route, a tile, a
form or an error code on purpose re-records it and says so."""
import ctypes
import json
import os
import sys

import pytest
import torch

from ccvpe_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_upconv_route_table as T      # noqa: E402

GATHER, HALO, DMA, DMA_PAIR, UP2 = range(5)                # CCVPE_UPROUTE_*
TILES = {(4, 5, 2), (4, 4, 2), (4, 3, 2), (4, 2, 2), (4, 1, 2), (4, 5, 1), (4, 3, 1), (4, 1, 1), (2, 7, 1)}     # CCVPE_TILES


def _expand(profile):
    out = []
    for count, value in zip(profile[::2], profile[1::2]):
        out += [value] * count
    return out


def _switch_states(lib):
    states = []
    for sw in T.AXES["switches"][1:]:
        prev = getattr(lib, sw)(1)
        getattr(lib, sw)(prev)
        states.append(prev)
    return states


def _skip_unless_256_cus():
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the table is recorded for 256 CUs")     # (never on the MI355X or on a box without a GPU)


def _table():
    table = json.load(open(os.path.join(ROOT, "tests", "upconv_route_table.json")))
    assert table["axes"] == T.AXES, "the sweep of tools/make_upconv_route_table.py changed: record the table again"
    return table


def test_launcher_answers_match_the_recorded_table():
    _skip_unless_256_cus()
    table = _table()
    lib = _lib.load()
    before = _switch_states(lib)
    got = T.sweep(lib, _lib.UpconvDesc)
    assert _switch_states(lib) == before, "sweep() left a switch changed"
    ns = list(T.n_values())
    assert sorted(got) == sorted(table["entries"]) and len(ns) == 168
    bad = []
    for sw, rows in got.items():
        want = table["entries"][sw]
        assert len(rows) == len(want) == 188
        for (name, profs), idx in zip(rows, want):
            for q, prof, i in zip(T.QUERIES, profs, idx):
                if prof != table["profiles"][i]:
                    a, b = _expand(prof), _expand(table["profiles"][i])
                    n = next(n for n, x, y in zip(ns, a, b) if x != y)
                    bad.append("[%s] %s N = %d: %s = %d, recorded %d" % (sw, name, n, q, a[ns.index(n)], b[ns.index(n)]))
    assert not bad, "%d differences, the first:\n%s" % (len(bad), "\n".join(bad[:20]))


def test_the_table_reaches_every_answer():
    """The sweep is worth its name only while it reaches every kind, tile, form and refusal the launchers can answer."""
    table = _table()
    ns = list(T.n_values())
    metas = [meta for _, meta, _, _ in T.cases()]
    prof = lambda sw, case, q: _expand(table["profiles"][table["entries"][sw][case][q]])
    tile = lambda r: ((r >> 8) & 0xf, (r >> 12) & 0xf, (r >> 16) & 0xf)
    seen = {0: {}, 1: {}}                                  # is_bf16 -> kind -> tiles
    codes, combos, up2_at = set(), set(), {}
    for sw in table["entries"]:
        for case, meta in enumerate(metas):
            for is_bf16 in (0, 1):
                for n, r in zip(ns, prof(sw, case, is_bf16)):
                    if r < 0:
                        codes.add(r)
                        continue
                    seen[is_bf16].setdefault(r & 0xff, set()).add(tile(r))
                    if r & 0xff == UP2:
                        assert sw != "ccvpe_set_narrow_kernels" and is_bf16 and meta["act"] in (0, 1) and meta["ldd_off"] % 8 == 0
                        assert meta["shape"] == (2, 128, 256)                        # 512 tiles; 256, h1 % 8 and w1 % 16 are not served
                        up2_at.setdefault((meta["c0"], meta["c1"], (n + 15) // 16 * 16), set()).add(n)
            cols = [prof(sw, case, q) for q in range(2, 7)]
            combos.update((sw == "ccvpe_set_s3_quad",) + c for c in zip(*cols))
            if meta["defect"] in ("c0 % 8", "ldd % 4") or (meta["defect"] == "short kpad" and meta["kpad"] != "s3"):
                assert set(prof(sw, case, 0)) == set(prof(sw, case, 1)) == {-1}, (sw, meta)
            if meta["defect"] in ("misaligned src0", "null shift9", "null src1") and meta["kpad"] != "s3":
                assert set(prof(sw, case, meta["kpad"] == "bf16")) == {-1}, (sw, meta)
            if meta["defect"] or meta["kpad"] != "s3" or meta["c1"] == 0 or (meta["shape"][2] < 16 and meta["shape"][1:] != (8, 8)):
                if meta["defect"] not in ("misaligned src0", "null shift9", "null src1"):      # (the s3 queries read no pointer)
                    assert set(cols[0]) == {0}, (sw, meta)
    assert set(seen[0]) == {GATHER, HALO, DMA_PAIR} and set(seen[1]) == {GATHER, HALO, DMA, DMA_PAIR, UP2}
    for is_bf16 in (0, 1):
        assert seen[is_bf16][GATHER] == TILES and seen[is_bf16][HALO] == TILES
        assert seen[is_bf16][DMA_PAIR] == {(4, 5, 2)}
    assert seen[1][DMA] == TILES - {(4, 3, 1)}             # the 256 x 48 tile measured slower with the DMA kernel
    assert seen[1][UP2] == {(0, 0, 0)}
    # the three up2 layers by their (c0, c1, npad) triples; [96, 16] is 8 channels off the first and is never served
    assert up2_at == {(88, 16, 48): {40, 48}, (64, 16, 32): {24, 32}, (136, 16, 32): {24, 32}}
    assert codes == {-1}                                   # CCVPE_EINVAL: the only code a query answers
    # (switch off, _ok, _form_ok 0..3): not served; served below / from 4096 pixels, outside / inside the quad form's range
    assert combos == {(False, 0, 0, 0, 0, 0), (True, 0, 0, 0, 0, 0),
                      (False, 1, 1, 1, 0, 0), (False, 1, 1, 1, 2, 0), (False, 2, 1, 1, 0, 0), (False, 2, 2, 1, 2, 0),
                      (True, 1, 1, 1, 0, 0), (True, 1, 1, 1, 2, 0), (True, 2, 1, 1, 0, 0), (True, 2, 1, 1, 2, 0)}
    # the 4096-pixel rule lies between 15 and 16 images of 16 x 16; an 8 x 8 layer is served only with the 160-column tile
    for case, meta in enumerate(metas):
        if meta["kpad"] == "s3" and (meta["c0"], meta["c1"]) == (64, 16) and not meta["defect"] and meta["act"] == 0:
            ok, quad = prof("all_on", case, 2), prof("all_on", case, 5)
            if meta["shape"] in ((15, 16, 16), (16, 16, 16)):
                assert set(ok) == {0, 2 if meta["shape"][0] == 16 else 1}
                assert [n for n, q in zip(ns, quad) if q == 2] == list(range(24, 81, 8))      # npad 32 .. 80
            if meta["shape"][1:] == (8, 8):
                assert all((o > 0) == (tile(r) == (4, 5, 2)) for o, r in zip(ok, prof("all_on", case, 0))) and 0 < sum(ok) < len(ok)


# (c0, c1, n, h1) of the ten B = 64 decoder layers (DECODER_B64 of tests/test_upconv_s3_quad_gpu.py) and the launch recorder's name
# for form 0 (auto) and form 1, computed with the rules ops.upconv3x3_s3 had before ccvpe_upconv3x3_s3_route: the tile of a Python
# mirror of pick_cfg(), ",pair" for 8 x 8 images, the quad kernel where ccvpe_upconv3x3_s3_form_ok answers 2.  bench.py and
# profiles/pmc_traffic.json key on these names
RECORDER_NAMES_B64 = [
    ((1304, 320, 640, 8), "upconv_s3_kernel<4,5,2,pair>", "upconv_s3_kernel<4,5,2,pair>"),
    ((648, 112, 320, 16), "upconv_s3_kernel<4,5,2>", "upconv_s3_kernel<4,5,2>"),
    ((328, 40, 160, 32), "upconv_s3_kernel<4,5,2>", "upconv_s3_kernel<4,5,2>"),
    ((168, 24, 80, 64), "upconv_s3q_kernel<2,5>", "upconv_s3_kernel<4,5,1>"),
    ((88, 16, 40, 128), "upconv_s3q_kernel<2,3>", "upconv_s3_kernel<4,3,1>"),
    ((1304, 320, 640, 8), "upconv_s3_kernel<4,5,2,pair>", "upconv_s3_kernel<4,5,2,pair>"),
    ((640, 112, 256, 16), "upconv_s3_kernel<4,4,2>", "upconv_s3_kernel<4,4,2>"),
    ((256, 40, 128, 32), "upconv_s3_kernel<4,4,2>", "upconv_s3_kernel<4,4,2>"),
    ((128, 24, 64, 64), "upconv_s3q_kernel<2,4>", "upconv_s3_kernel<4,2,2>"),
    ((64, 16, 32, 128), "upconv_s3q_kernel<2,2>", "upconv_s3_kernel<4,1,2>"),
]


def test_recorder_names_of_the_b64_decoder_layers():
    from ccvpe_amd import ops
    _lib.load()
    for (c0, c1, n, h1), auto, per_parity in RECORDER_NAMES_B64:
        d = _lib.UpconvDesc(src0=T.PTR, src1=T.PTR, w=T.PTR, shift9=T.PTR, dst=T.PTR, c0=c0, ld0=c0, c1=c1, ld1=c1, batch=64, h1=h1,
                            w1=h1, n=n, kpad=T.kpad_of("s3", c0, c1), ldd=n, act=1)
        assert (ops.upconv_s3_route_name(d, 0), ops.upconv_s3_route_name(d, 1)) == (auto, per_parity), (c0, c1, n, h1)
        quad = auto.startswith("upconv_s3q")
        assert (ops.upconv_s3_route_name(d, 2) == auto) if quad else _raises(ops.upconv_s3_route_name, d, 2)


def _raises(fn, *args):
    with pytest.raises(_lib.CcvpeError):
        fn(*args)
    return True


def test_s3_route_agrees_with_the_other_queries():
    """ccvpe_upconv3x3_s3_route over the same sweep: its form field is ccvpe_upconv3x3_s3_form_ok's answer for forms 0..2, and it is
    0 exactly where ccvpe_upconv3x3_s3_ok is 0 (no answer of the three-plane family depends on the CU count)."""
    lib = _lib.load()
    route, ok, form_ok = lib.ccvpe_upconv3x3_s3_route, lib.ccvpe_upconv3x3_s3_ok, lib.ccvpe_upconv3x3_s3_form_ok
    before = _switch_states(lib)
    served = 0
    for sw, name, d, ldd_off in T.visit(lib, _lib.UpconvDesc):
        ref = ctypes.byref(d)
        for n in T.n_values():
            d.n, d.ldd = n, n + ldd_off
            o = ok(ref)
            for form in range(3):
                r, f = route(ref, form), form_ok(ref, form)
                assert (r & 0xf) == f and (r == 0) == (f == 0), (sw, name, n, form, r, f)
                assert form == 2 or (r == 0) == (o == 0), (sw, name, n, form, r, o)      # (forms 0 and 1 compute every served desc)
            assert route(ref, 3) == 0
            served += o > 0
    assert _switch_states(lib) == before and served > 1000
