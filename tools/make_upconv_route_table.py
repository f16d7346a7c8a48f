"""Records what the folded deconv + 3x3 launchers (csrc/upconv_impl.h, upconv_s3.hip, upconv_s3q.hip, narrow_bf16.hip) answer over
a sweep of descriptors: ccvpe_upconv3x3_route for fp32 and bf16, ccvpe_upconv3x3_s3_ok and ccvpe_upconv3x3_s3_form_ok for forms
0..3, negative codes included.  Host code only, fake aligned pointers, no GPU.  tests/test_upconv_route_table.py replays the
sweep against the table committed beside it, so a change of a launcher that moves any route, tile, form or refusal fails on the
CPU.

    python tools/make_upconv_route_table.py [-o tests/upconv_route_table.json]      # CCVPE_LIB=... records another build

The table is recorded with 256 CUs (num_cus() without a device, and an MI355X's count).

File: {"axes": the sweep, "profiles": [...], "entries": {switch: [[seven profile indices] per case]}}; a profile is one query's
answers along N = 8, 16, .. 1344, run-length encoded as [count, value, count, value, ...]; the seven numbers of a case (QUERIES)
index `profiles`; cases come in the order of cases().
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

QUERIES = ("route_f32", "route_bf16", "s3_ok", "s3_form_ok(0)", "s3_form_ok(1)", "s3_form_ok(2)", "s3_form_ok(3)")

AXES = {
    "n": [8, 1344, 8],                                     # first, last, step: every multiple of 8
    # kpad of the pack: fp32 (K rounded to 16), bf16 (to 32), three-plane (48 per 16-channel stage)
    "kpads": ["f32", "bf16", "s3"],
    # the main cross, (c0, c1) x (B, H1, W1).  Channels: a skip of one block and of two, no skip with the DMA's W-row
    # precondition 3 c0 + ceil32(c0) <= Kpad failing (48) and holding (64) in bf16, failing in fp32 (40).  Shapes: narrower than
    # 16 pixels and not 8 x 8, 8 x 8 with an odd and an even batch, 8 x 16, ragged on both edges, 15 and 16 images of 16 x 16
    # (the three-plane size rule: 4096 low-res pixels)
    "channels": [[64, 16], [48, 0], [64, 0], [40, 0], [168, 24]],
    "shapes": [[2, 4, 12], [3, 8, 8], [2, 8, 8], [2, 8, 16], [2, 9, 17], [15, 16, 16], [16, 16, 16]],
    "acts": [0, 1, 2, 3],                                  # crossed with [64, 16] at 2 x 9 x 17 only
    # the up2 layers (csrc/narrow_bf16.hip) and one 8 channels off; 512 tiles of 8 x 16 are served, 256 are not; h1 % 8, w1 % 16;
    # ldd = n against n + 4; every activation on the served shape
    "up2_channels": [[88, 16], [64, 16], [136, 16], [96, 16]],
    "up2_shapes": [[2, 128, 256], [1, 128, 256], [3, 124, 256], [3, 128, 248]],
    "up2_ldd_offsets": [0, 4],
    # level 6 of the decoders: at B = 64 the 8 x 8 images reach the 4096-pixel rule
    "level6": [[[1304, 320], [64, 8, 8]], [[1304, 320], [3, 8, 8]], [[64, 16], [64, 8, 8]]],
    # one defect each on [64, 16] at 2 x 9 x 17
    "defects": ["c0 % 8", "short kpad", "ldd % 4", "misaligned src0", "null shift9", "null src1"],
    # 4 M < 2^31 but more than 2^31 workgroups where N takes nine or more column tiles (ragged 1 x 17 images: two pixel tiles each)
    "huge": [[64, 16], [30000000, 1, 17]],
    "switches": ["all_on", "ccvpe_set_narrow_kernels", "ccvpe_set_s3_quad"],
}
PTR = 256                                                  # a fake 16-byte aligned pointer: the queries never dereference it


def n_values():
    lo, hi, step = AXES["n"]
    return range(lo, hi + 1, step)


def kpad_of(kind, c0, c1):
    if kind == "s3":
        return 48 * (4 * ((c0 + 15) // 16) + 9 * ((c1 + 15) // 16))
    sk = 16 if kind == "f32" else 32
    return (4 * c0 + 9 * c1 + sk - 1) // sk * sk


def _case(kind, c0, c1, shape, act=0, ldd_off=0, defect=None):
    b, h1, w1 = shape
    f = dict(src0=PTR, src1=PTR if c1 else None, w=PTR, shift9=PTR, dst=PTR, c0=c0, ld0=c0, c1=c1, ld1=c1, batch=b, h1=h1, w1=w1,
             kpad=kpad_of(kind, c0, c1), act=act)
    if defect == "c0 % 8":
        f.update(c0=c0 - 4, ld0=c0 - 4)
    elif defect == "short kpad":
        f["kpad"] -= {"f32": 16, "bf16": 32, "s3": 48}[kind]
    elif defect == "ldd % 4":
        ldd_off = 2
    elif defect == "misaligned src0":
        f["src0"] = PTR + 4
    elif defect == "null shift9":
        f["shift9"] = None
    elif defect == "null src1":
        f["src1"] = None
    name = "%s c0=%d c1=%d %dx%dx%d act=%d ldd=n+%d%s" % (kind, c0, c1, b, h1, w1, act, ldd_off, " [%s]" % defect if defect else "")
    meta = dict(kpad=kind, c0=c0, c1=c1, shape=tuple(shape), act=act, ldd_off=ldd_off, defect=defect)
    return name, meta, f, ldd_off


def cases():
    """(name, meta, fields of the descriptor other than n / ldd, ldd - n) in the table's order."""
    for kind in AXES["kpads"]:
        for c0, c1 in AXES["channels"]:
            for shape in AXES["shapes"]:
                yield _case(kind, c0, c1, shape)
        for act in AXES["acts"][1:]:
            yield _case(kind, 64, 16, (2, 9, 17), act=act)
        for (c0, c1), shape in AXES["level6"]:
            yield _case(kind, c0, c1, shape)
        for defect in AXES["defects"]:
            yield _case(kind, 64, 16, (2, 9, 17), defect=defect)
        yield _case(kind, AXES["huge"][0][0], AXES["huge"][0][1], AXES["huge"][1])
    for c0, c1 in AXES["up2_channels"]:
        for shape in AXES["up2_shapes"]:
            for off in AXES["up2_ldd_offsets"]:
                yield _case("bf16", c0, c1, shape, ldd_off=off)
        for act in AXES["acts"][1:]:
            yield _case("bf16", c0, c1, AXES["up2_shapes"][0], act=act)


def rle(values):
    out = []
    for v in values:
        if out and out[-1] == v:
            out[-2] += 1
        else:
            out += [1, v]
    return out


def visit(lib, UpconvDesc):
    """(switch, name, desc, ldd - n) per switch position and case; a switch is off while its cases are visited and restored after."""
    for sw in AXES["switches"]:
        prev = getattr(lib, sw)(0) if sw != "all_on" else None
        try:
            for name, _, fields, ldd_off in cases():
                yield sw, name, UpconvDesc(**fields), ldd_off
        finally:
            if prev is not None:
                getattr(lib, sw)(prev)


def sweep(lib, UpconvDesc):
    """{switch: [(name, [one run-length encoded profile per entry of QUERIES]) per case]}."""
    route, ok, form_ok = lib.ccvpe_upconv3x3_route, lib.ccvpe_upconv3x3_s3_ok, lib.ccvpe_upconv3x3_s3_form_ok
    ns = list(n_values())
    out = {}
    for sw, name, d, ldd_off in visit(lib, UpconvDesc):
        ref = ctypes.byref(d)
        cols = [[] for _ in QUERIES]
        for n in ns:
            d.n, d.ldd = n, n + ldd_off
            cols[0].append(route(ref, 0))
            cols[1].append(route(ref, 1))
            cols[2].append(ok(ref))
            for form in range(4):
                cols[3 + form].append(form_ok(ref, form))
        out.setdefault(sw, []).append((name, [rle(c) for c in cols]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "tests", "upconv_route_table.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from ccvpe_amd import _lib
    table = sweep(_lib.load(), _lib.UpconvDesc)
    index, entries = {}, {}
    for sw, rows in table.items():
        entries[sw] = [[index.setdefault(json.dumps(p), len(index)) for p in profs] for _, profs in rows]
    profiles = [json.loads(k) for k in index]              # (dicts keep insertion order: position = index)
    with open(args.out, "w") as f:
        f.write('{"axes": %s,\n"profiles": [\n%s],\n"entries": {\n%s}}\n' % (
            json.dumps(AXES), ",\n".join(json.dumps(p, separators=(",", ":")) for p in profiles),
            ",\n".join('"%s": %s' % (sw, json.dumps(e, separators=(",", ":"))) for sw, e in entries.items())))
    print("%s: %d cases x %d switch settings, %d profiles, %d bytes (library: %s)" % (
        args.out, len(entries["all_on"]), len(entries), len(profiles), os.path.getsize(args.out), _lib.LIB_PATH))


if __name__ == "__main__":
    main()
