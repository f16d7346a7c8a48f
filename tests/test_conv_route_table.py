"""The conv dispatcher's answers over a sweep of descriptors, against the table recorded beside this file
(tests/conv_route_table.json, written by tools/make_conv_route_table.py from the library BEFORE the dispatcher was split into
fill_params / pick_route / splitk_want): route, conv3x3 form, split-K scratch and fused-matching query for fp32, bf16 and bf16
with an fp32 output, every N = 8, 16, .. 1344, four layer kinds, gate / residual / activation, eight shapes, and again with the
narrow, ring and narrow-projection kernels switched off.  Host code only: no GPU, fake aligned pointers.  A change that moves a
route, a form, a split decision or an error code on purpose re-records the table and says so."""
import json
import os
import sys

import pytest
import torch

from ccvpe_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_conv_route_table as T      # noqa: E402

QUERIES = ("ccvpe_conv_igemm_route", "ccvpe_conv3x3_variant", "ccvpe_conv_igemm_splitk_floats", "ccvpe_conv3x3_match1_ok")


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


def test_dispatcher_answers_match_the_recorded_table():
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the table is recorded for 256 CUs")     # (never on the MI355X or on a box without a GPU)
    table = json.load(open(os.path.join(ROOT, "tests", "conv_route_table.json")))
    assert table["axes"] == T.AXES, "the sweep of tools/make_conv_route_table.py changed: record the table again"
    lib = _lib.load()
    before = _switch_states(lib)
    got = T.sweep(lib, _lib.ConvDesc)
    assert _switch_states(lib) == before, "sweep() left a switch changed"
    ns = list(T.n_values())
    assert sorted(got) == sorted(table["entries"]) and len(ns) == 168
    families, bad = set(), []
    for sw, rows in got.items():
        want = table["entries"][sw]
        assert len(rows) == len(want) == 1920
        for (name, profs), idx in zip(rows, want):
            for q, prof, i in zip(QUERIES, profs, idx):
                if prof != table["profiles"][i]:
                    a, b = _expand(prof), _expand(table["profiles"][i])
                    n = next(n for n, x, y in zip(ns, a, b) if x != y)
                    bad.append("[%s] %s N = %d: %s = %d, recorded %d" % (sw, name, n, q, a[ns.index(n)], b[ns.index(n)]))
            families.update(r & 0xff for r in profs[0][1::2] if r >= 0)
    assert not bad, "%d differences, the first:\n%s" % (len(bad), "\n".join(bad[:20]))
    # the sweep is worth its name only while it reaches every family, refusals, split and un-split layers and the fused matching
    assert families == {0, 1, 2, 3, 4, 5}, families
    flat = [table["profiles"][i][1::2] for rows in table["entries"].values() for idx in rows for i in idx[2:]]
    assert any(v < 0 for p in flat for v in p) and any(v > 0 for p in flat for v in p)
    assert any(1 in table["profiles"][idx[3]][1::2] for idx in table["entries"]["all_on"])
    assert any(table["profiles"][idx[1]][1::2] != [0] and min(table["profiles"][idx[1]][1::2]) > 0 for idx in table["entries"]["all_on"])
