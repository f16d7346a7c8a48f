"""The matching table against the launcher's own decision, without a GPU.

ccvpe_match_route answers — from the host function the launch itself calls — which kernel form and instantiation serves a matching
call.  Every row of tests/matching_kernel_shapes.py, and both sides of every gate pair, must get exactly the answer the row claims
at all three positions of ccvpe_set_match_mfma; the plain-Python restatements of the tile geometry agree with it; and the rows
together claim every instantiation of the three kernels, so a routing change shows up here as a stale row and not as a kernel that
quietly stopped being tested.
"""
import ctypes
import os

import pytest

from ccvpe_amd import _lib

import matching_kernel_shapes as S

ROWS = S.rows()
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _at_every_switch(lib, fn):
    assert lib.ccvpe_set_match_mfma(2) == 2, "another test left the matching switch changed"
    try:
        for pos in (0, 1, 2):
            lib.ccvpe_set_match_mfma(pos)
            fn(pos)
    finally:
        lib.ccvpe_set_match_mfma(2)
    assert lib.ccvpe_set_match_mfma(2) == 2


def test_every_row_routes_as_it_claims_at_every_switch_position(lib):
    assert len({r.name for r in ROWS}) == len(ROWS)

    def check(pos):
        for r in ROWS:
            S.assert_route(lib, r, r.claims[pos], " at switch %d" % pos)
    _at_every_switch(lib, check)
    for r in ROWS:
        assert all(p in (0, 1, 2) for p in r.switches) and len(set(r.switches)) == len(r.switches), r.name
        assert r.b * r.h * r.w <= 65536 * 1.01, "%s: larger than the streaming gate's floor needs" % r.name


def test_gate_pairs_flip_the_route(lib):
    pairs = S.gate_pairs()
    assert len(pairs) == 6
    launched = {r.name for r in ROWS}

    def check(pos):
        for near, far in pairs:
            S.assert_route(lib, near, near.claims[pos], " at switch %d" % pos)
            S.assert_route(lib, far, far.claims[pos], " at switch %d" % pos)
    _at_every_switch(lib, check)
    for near, far in pairs:
        assert near.name in launched and 2 in near.switches and near.claims[2].form == S.STREAM, near.name
        assert far.claims[2].form != S.STREAM and far.bf16 == near.bf16, far.name
        changed = [f for f in S.Row._fields[1:14] if getattr(near, f) != getattr(far, f)]
        assert changed, far.name
        print("%s: %s -> form %d" % (far.name, changed, far.claims[2].form))
    by = {far.name: (near, far) for near, far in pairs}
    near, far = by["gate ldo - C 64 | 68"]
    assert (near.ldo - near.c, far.ldo - far.c) == (64, 68)
    near, far = by["gate B hw 65536 | 65520"]
    assert (near.b * near.h * near.w, far.b * far.h * far.w) == (65536, 65520) and (far.h * far.w) % 16 == 0
    assert (len(by["gate n_shifts 9 | 8"][0].shifts), len(by["gate n_shifts 9 | 8"][1].shifts)) == (9, 8)
    assert (len(by["gate n_shifts 32 | 33"][0].shifts), len(by["gate n_shifts 32 | 33"][1].shifts)) == (32, 33)
    assert (by["gate n_tail 0 | 1"][0].n_tail, by["gate n_tail 0 | 1"][1].n_tail) == (0, 1)
    assert (by["gate C 80 | 88"][0].c, by["gate C 80 | 88"][1].c) == (80, 88)


def test_restated_tile_geometry_is_the_table(lib):
    for c, (lpp, tp, npt, ks, slices) in S.TILE.items():
        assert S.match_lpp(c) == lpp and 256 // lpp == tp, c
        assert S.npt_ks(tp) == (npt, ks), c
        assert S.k_slices(c, ks) == slices, c
        assert slices[0][0] == 0 and slices[-1][1] == (c + 15) // 16 and all(a[1] == b[0] for a, b in zip(slices, slices[1:])), c
        s = S.match_pitch(c, lpp)
        assert s >= c + 4 and s % 4 == 0 and (lpp >= 16 or ((s // 4) % lpp == 0 and (s // 4 // lpp) % 2 == 1)), c
    # the tile classes the table is there for
    t = S.TILE
    assert [b - a for a, b in t[104][4]] == [3, 4] and [b - a for a, b in t[200][4]] == [3, 3, 3, 4] and [b - a for a, b in t[392][4]] == [6, 6, 6, 7]
    assert all(c % 16 == 8 for c in (24, 40, 104, 200, 392))
    assert (t[24][2], t[40][2], t[80][2], t[104][3], t[160][3], t[200][3], t[320][3], t[392][1]) == (16, 8, 4, 2, 2, 4, 4, 8)
    # rows whose claims carry offsets the restatement derives
    for r in ROWS:
        offs = S.offsets(r.shifts, r.stride, r.woff, r.c)
        for p in set(r.switches) | {0}:
            cl = r.claims[p]
            if cl.form != S.STREAM:
                assert S.vec_of(offs) == cl.vec, r.name
            assert cl.partial == (r.l < r.c), r.name


def test_streaming_rows_hold_their_run_geometry_at_256_cus():
    rows = S.stream_rows()
    assert len(rows) == 32
    geos = set()
    for r in rows:
        hw = r.h * r.w
        assert hw % 16 == 0 and 65536 <= r.b * hw <= 65536 * 1.01 and r.n_tail == 0 and r.ldo - r.c <= 64, r.name
        g = S.stream_geometry(r.b, hw)
        geos.add((r.b, r.h, r.w))
        if (r.b, r.h, r.w) == S.GEOS["5x16x821"]:
            assert (g.tiles, g.tpw, g.run, g.wgs, g.last_tiles) == (4105, 3, 12, 343, 1), r.name
            assert g.straddled == (821, 1642, 2463, 3284), "%s: every sample boundary must fall inside a run" % r.name
        else:
            assert (g.tiles, g.tpw, g.run, g.wgs, g.last_tiles) == (4096, 2, 8, 512, 8), r.name
    assert geos == set(S.GEOS.values())
    for bf16 in (False, True):
        mine = [r for r in rows if r.bf16 == bf16]
        assert {(r.b, r.h, r.w) for r in mine} == set(S.GEOS.values())
    assert {r.c for r in rows} == {24, 32, 40, 48, 56, 64, 72, 80}
    assert any(r.n_max < len(r.shifts) for r in rows) and any(r.stride == 3 for r in rows)
    assert any(r.ldo - r.c == 64 for r in rows) and any(r.ldx > r.c for r in rows)
    for nb in (2, 3, 4, 5):                                             # both members of every NB class, in both storage types
        for bf16 in (False, True):
            cs = {r.c for r in rows if r.claims[2].nb == nb and r.bf16 == bf16}
            assert cs == {16 * nb - 8, 16 * nb}, (nb, bf16, cs)


def _launched(form):
    return {S.inst_key(r, r.claims[p]) for r in ROWS for p in r.switches if r.claims[p].form == form}


def test_rows_claim_every_instantiation():
    types, flags = (False, True), (False, True)
    stream = {(S.STREAM, t, 16 * m, p, nb) for t in types for m in (1, 2) for p in flags for nb in (2, 3, 4, 5)}
    assert len(stream) == 32 and _launched(S.STREAM) == stream, sorted(stream - _launched(S.STREAM))
    tiled = {(S.TILED, t, n, p, v) for t in types for n in (16, 32) for p in flags for v in (4, 2)}
    assert len(tiled) == 16 and _launched(S.TILED) == tiled, sorted(tiled - _launched(S.TILED))
    # the vector-ALU form at DEFAULT routing: 9..32 hypotheses reach it only with an odd table offset (VEC 1)
    default = {(S.VALU, t, n, p, v) for t in types for n in (1, 8, 48) for p in flags for v in (4, 2, 1)}
    default |= {(S.VALU, t, n, p, 1) for t in types for n in (16, 24) for p in flags}
    assert len(default) == 44
    at_default = {S.inst_key(r, r.claims[2]) for r in ROWS if 2 in r.switches and r.claims[2].form == S.VALU}
    assert at_default == default, sorted(default ^ at_default)
    # ... and with the switch at 0 the remaining NPAD 16 / 24 x VEC 4 / 2 forms: all 60
    every = {(S.VALU, t, n, p, v) for t in types for n in (1, 8, 16, 24, 48) for p in flags for v in (4, 2, 1)}
    assert _launched(S.VALU) == every, sorted(every - _launched(S.VALU))
    # every tile class of the matrix-core form with one and with two 16-row hypothesis tiles
    classes = {}
    for r in ROWS:
        for p in r.switches:
            cl = r.claims[p]
            if cl.form == S.TILED:
                classes.setdefault((cl.tp, cl.npt, cl.ks), set()).add(cl.npad)
    assert classes == {k: {16, 32} for k in ((256, 16, 1), (128, 8, 1), (64, 4, 1), (32, 2, 2), (16, 1, 4), (8, 1, 4))}, classes
    tiled_rows = [r for r in ROWS if r.claims[2].form == S.TILED]
    assert {r.c for r in tiled_rows} == {24, 40, 80, 104, 160, 200, 320, 392, 1280, 2048}
    assert all(0 in r.switches for r in tiled_rows) and {p for r in tiled_rows for p in r.switches} == {0, 1, 2}
    assert any(r.ldx > r.c for r in tiled_rows) and any(r.n_max < len(r.shifts) and r.n_tail for r in tiled_rows)
    assert {len(r.shifts) for r in tiled_rows} >= {9, 16, 17, 32} and any(r.h * r.w < r.claims[2].tp for r in tiled_rows)
    for form in (S.VALU, S.TILED):                                      # both bf16 output store widths of the tiled kernel
        eo = {r.ldo % 8 == 0 for r in ROWS if r.bf16 and r.claims[2].form == form}
        assert eo == {False, True}, form
    valu_rows = [r for r in ROWS if r.claims[2].form == S.VALU]
    assert any(r.ldx > r.c for r in valu_rows) and {len(r.shifts) for r in valu_rows} >= {8, 9, 16, 17, 32, 33, 41}


def _route(lib, elem, l, shifts, n_max, n_tail, stride, woff, ldx, ldo, b, hw, c):
    sh = (ctypes.c_int * max(len(shifts), 1))(*shifts)
    return lib.ccvpe_match_route(elem, l, sh, len(shifts), n_max, n_tail, stride, woff, ldx, ldo, b, hw, c, None)


def test_invalid_arguments_give_the_launch_error_codes(lib):
    """(element size, L, shifts, n_max, n_tail, stride, window_offset, ldx, ldo, B, hw, C), each invalid in one way; the launch
    entry points validate before they touch the device, so they can be asked on a machine without a GPU too"""
    two = [0, 1]
    bad = [
        ("no hypotheses", (4, 40, [], 1, 0, 2, 0, 40, 48, 1, 64, 40), b"n_shifts"),
        ("49 hypotheses", (4, 40, list(range(49)), 1, 0, 2, 0, 40, 48, 1, 64, 40), b"n_shifts"),
        ("n_max 0", (4, 40, two, 0, 0, 2, 0, 40, 48, 1, 64, 40), b"n_max"),
        ("n_max > n_shifts", (4, 40, two, 3, 0, 2, 0, 40, 48, 1, 64, 40), b"n_max"),
        ("n_tail > n_shifts", (4, 40, two, 2, 3, 2, 0, 40, 48, 1, 64, 40), b"n_max/n_tail"),
        ("C % 8", (4, 36, two, 2, 0, 2, 0, 36, 40, 1, 64, 36), b"C%8"),
        ("ldx % 4", (4, 40, two, 2, 0, 2, 0, 42, 48, 1, 64, 40), b"ldx%4"),
        ("ldo % 4", (4, 40, two, 2, 0, 2, 0, 40, 46, 1, 64, 40), b"ldo%4"),
        ("ldo < C + 1 + n_tail", (4, 40, two, 2, 2, 2, 0, 40, 40, 1, 64, 40), b"ldo>=C+1+n_tail"),
        ("bf16 ldx % 8", (2, 40, two, 2, 0, 2, 0, 44, 48, 1, 64, 40), b"bf16 rows"),
        ("L > C", (4, 48, two, 2, 0, 2, 0, 40, 48, 1, 64, 40), b"bad L"),
        ("L < 1", (4, 0, two, 2, 0, 2, 0, 40, 48, 1, 64, 40), b"bad L"),
        ("batch > 65535", (4, 40, two, 2, 0, 2, 0, 40, 48, 65536, 16, 40), b"batch"),
        ("LDS above 160 KB", (4, 4096, list(range(48)), 48, 0, 2, 0, 4096, 4100, 1, 64, 4096), b"of LDS"),
    ]
    for name, args, msg in bad:
        assert _route(lib, *args) == EINVAL, name
        assert msg in lib.ccvpe_last_error(), (name, lib.ccvpe_last_error())
        elem, l, shifts, n_max, n_tail, stride, woff, ldx, ldo, b, hw, c = args
        sh = (ctypes.c_int * max(len(shifts), 1))(*shifts)
        fn = lib.ccvpe_match_level_bf16 if elem == 2 else lib.ccvpe_match_level_f32
        rc = fn(256, ldx, 256, max(l, 1), l, sh, len(shifts), n_max, n_tail, stride, woff, 256, 256, ldo, b, hw, c, None)   # fake aligned pointers: never dereferenced
        assert rc == EINVAL and msg in lib.ccvpe_last_error(), (name, rc, lib.ccvpe_last_error())
    assert _route(lib, 3, 40, two, 2, 0, 2, 0, 40, 48, 1, 64, 40) == EINVAL and b"element size" in lib.ccvpe_last_error()
    assert lib.ccvpe_match_route(4, 40, None, 2, 2, 0, 2, 0, 40, 48, 1, 64, 40, None) == EINVAL
    assert _route(lib, 4, 40, two, 2, 0, 2, 0, 40, 48, 1, 64, 40) == S.VALU          # the same call, valid; `out` may be NULL
