"""Records what the conv dispatcher (csrc/conv_igemm.hip) answers over a sweep of descriptors: ccvpe_conv_igemm_route,
ccvpe_conv3x3_variant, ccvpe_conv_igemm_splitk_floats and ccvpe_conv3x3_match1_ok (L = 16), negative codes included.  Host
code only, fake aligned pointers, no GPU.  tests/test_conv_route_table.py replays the sweep against the table committed
beside it, so a change of the dispatcher that moves any route, form or split decision fails on the CPU.

    python tools/make_conv_route_table.py [-o tests/conv_route_table.json]      # CCVPE_LIB=... records another build

The table is recorded with 256 CUs (num_cus() without a device, and an MI355X's count).

File: {"axes": the sweep, "profiles": [...], "entries": {switch: [[route, variant, splitk, match1] per case]}}; a profile is
one query's answers along N = 8, 16, .. 1344, run-length encoded as [count, value, count, value, ...]; the four numbers of a
case index `profiles`; cases come in the order of cases().
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

AXES = {
    "n": [8, 1344, 8],                                     # first, last, step: every multiple of 8
    "types": ["f32", "bf16", "bf16_out_f32"],
    "kinds": {"1x1s1": [1, 1, 0], "3x3s1": [3, 1, 1], "3x3s2": [3, 2, 1], "1x1s2": [1, 2, 0]},      # kernel, stride, pad
    # (c0, (B, H, W)): the cross of c0 = 16, 64, 144, 256, 672, 1344 with the eight shapes, thinned so that the replay takes
    # seconds (N is never thinned).  Every c0 and every shape appears, paired where a rule has a threshold: split-K at B = 1
    # with a long K against its B = 64 un-split twin, M no multiple of a tile, a gated tile that would span two samples
    # (64 x 20 x 40), the narrow projection kernel on planes of >= 64 K pixels with K = 16 (both types) and K = 256 (bf16 only),
    # the narrow 3x3 kernel at 64 channels and — c0 = 32 is added for it — with the fused matching, which 64 channels rule out
    "c0_shapes": [[1344, [1, 16, 16]], [64, [2, 11, 20]], [144, [3, 19, 23]], [672, [8, 32, 32]], [1344, [64, 16, 16]],
                  [672, [64, 20, 40]], [64, [64, 64, 64]], [32, [64, 64, 64]], [16, [2, 256, 256]], [256, [2, 256, 256]]],
    "acts": [0, 1, 2, 3],
    "switches": ["all_on", "ccvpe_set_narrow_kernels", "ccvpe_set_pw_ring_kernels", "ccvpe_set_pwn_kernels"],
    "match1_L": 16,
}
PTR = 256                                                  # a fake 16-byte aligned pointer: the queries never dereference it


def n_values():
    lo, hi, step = AXES["n"]
    return range(lo, hi + 1, step)


def cases():
    """(name, type, fields of the descriptor other than n / ldd / ldres) in the table's order.  1x1 layers carry BN scale + shift,
    3x3 layers a shift only (the folded form the decoders use, as in tests/test_abi.py)."""
    for typ in AXES["types"]:
        sk = 16 if typ == "f32" else 32
        for kind, (k, stride, pad) in AXES["kinds"].items():
            for c0, (b, h, w) in AXES["c0_shapes"]:
                for c1 in ((0, c0) if k == 3 else (0,)):
                    for gate in ((0, 1) if k == 1 else (0,)):          # the descriptor allows a gate on 1x1 single-source layers only
                        for res in (0, 1):
                            for act in AXES["acts"]:
                                f = dict(src0=PTR, src1=PTR if c1 else None, gate=PTR if gate else None, w=PTR, scale=PTR if k == 1 else None, shift=PTR,
                                         residual=PTR if res else None, dst=PTR, c0=c0, ld0=c0, c1=c1, ld1=c1, batch=b, in_h=h, in_w=w,
                                         kh=k, kw=k, stride=stride, pad=pad, kpad=(k * k * (c0 + c1) + sk - 1) // sk * sk, act=act,
                                         out_mode=0)
                                yield ("%s %s c0=%d c1=%d gate=%d res=%d act=%d %dx%dx%d" % (typ, kind, c0, c1, gate, res, act, b, h, w),
                                       typ, f, res)


def rle(values):
    out = []
    for v in values:
        if out and out[-1] == v:
            out[-2] += 1
        else:
            out += [1, v]
    return out


def sweep(lib, ConvDesc):
    """{switch: [(name, [route profile, variant profile, splitk profile, match1 profile]) per case]}, profiles run-length encoded."""
    route, variant = lib.ccvpe_conv_igemm_route, lib.ccvpe_conv3x3_variant
    splitk, match1 = lib.ccvpe_conv_igemm_splitk_floats, lib.ccvpe_conv3x3_match1_ok
    L, ns = AXES["match1_L"], list(n_values())
    out = {}
    for sw in AXES["switches"]:
        prev = getattr(lib, sw)(0) if sw != "all_on" else None
        try:
            rows = []
            for name, typ, fields, res in cases():
                d = ConvDesc(**fields)
                ref = ctypes.byref(d)
                bf16, of32 = int(typ != "f32"), int(typ == "bf16_out_f32")
                r, v, s, m = [], [], [], []
                for n in ns:
                    d.n = d.ldd = n
                    d.ldres = n if res else 0
                    r.append(route(ref, bf16, of32))
                    v.append(variant(ref, bf16))
                    s.append(splitk(ref, bf16))
                    d.ldd = n + 8                          # the fused matching writes its scores behind the N channels of a row
                    m.append(match1(ref, of32, L))
                rows.append((name, [rle(r), rle(v), rle(s), rle(m)]))
            out[sw] = rows
        finally:
            if prev is not None:
                getattr(lib, sw)(prev)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "tests", "conv_route_table.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from ccvpe_amd import _lib
    table = sweep(_lib.load(), _lib.ConvDesc)
    index, profiles, entries = {}, [], {}
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
