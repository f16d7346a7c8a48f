"""CPU-side checks of the three-plane pack of csrc/pw_s3.hip (models._pack_pw_s3) and of the host-only queries ccvpe_pw_s3_ok /
ccvpe_pw_s3_route.  The kernel's LDS rows and fragment offsets are upconv_s3.hip's (csrc/split3_impl.h), whose bank model
tests/test_upconv_s3.py checks."""
import ctypes

import torch

from ccvpe_amd import _lib, models, synth


def _w(n, k, seed=0):
    return models._pad2(synth.normal((n, k), 900 + seed, k ** -0.5))


def test_planes_sum_exactly_to_the_weights():
    for n, k in ((80, 240), (126, 1280), (320, 1152), (1280, 4 * 64)):
        wp = _w(n, k, n)
        w3 = models._pack_pw_s3(wp)
        npad = (n + 15) // 16 * 16
        assert w3.dtype == torch.bfloat16 and tuple(w3.shape) == (k // 16, npad, 48) and w3.is_contiguous()
        hi, mid, lo = models._unpack_pw_s3(w3)
        assert torch.equal((hi.double() + mid.double() + lo.double()).float(), wp)        # exact: 8 + 8 + 8 significant bits
        assert torch.equal(hi, wp.to(torch.bfloat16).float())                             # hi is the round-to-nearest bf16 of w
        assert torch.all(hi[n:] == 0) and torch.all(lo[n:] == 0)                           # the zero rows of the N padding stay zero


def test_layout_round_trips():
    """Element (stage s, row n, plane q, channel c) of the pack is plane q of w[n, 16 s + c]: the kernel's stage order, a stage's
    panel being `npad` contiguous 96-byte rows."""
    n, k = 112, 672
    wp = torch.arange(n * k, dtype=torch.float32).reshape(n, k) % 251.0                    # small integers: hi holds them exactly
    w3 = models._pack_pw_s3(wp)
    for s, r, c in ((0, 0, 0), (3, 17, 5), (41, 111, 15), (20, 64, 8)):
        assert w3[s, r, c].item() == wp[r, 16 * s + c].item()
        assert w3[s, r, 16 + c].item() == 0 and w3[s, r, 32 + c].item() == 0
    flat = w3.reshape(-1)
    assert flat[(3 * n + 17) * 48 + 5].item() == wp[17, 53].item()
    hi, mid, lo = models._unpack_pw_s3(w3)
    assert torch.equal(hi, wp) and not mid.any() and not lo.any()
    assert torch.equal(models._pack_pw_s3(hi + mid + lo), w3)


def test_pack_is_refused_for_other_inputs():
    assert models._pack_pw_s3(None) is None
    assert models._pack_pw_s3(_w(80, 240).to(torch.bfloat16)) is None
    assert models._pack_pw_s3(torch.zeros((80, 248))) is None                              # K % 16
    assert models._pack_pw_s3(torch.zeros((4, 80, 240))) is None


def test_eval_pack_carries_the_three_plane_packs_and_no_other_pack_does():
    sd = synth.synthetic_state_dict("vigor", 0)
    pk = models._pack_model(sd, "vigor", 20, torch.float32, fold=True)
    for e in (pk.grd, pk.sat):
        have = [i for i, b in enumerate(e.blocks) if b.w_proj3 is not None]
        assert have == list(range(4, 16))                                                  # mid >= 240
        assert e.w_head3 is not None and tuple(e.w_head3.shape) == (20, 1280, 48)
    assert tuple(pk.gd_w3.shape) == (80, 128, 48) and tuple(pk.sd_w3.shape) == (320, 1280, 48)
    for other in (models._pack_model(sd, "vigor", 20, torch.float32, fold=False),
                  models._pack_model(sd, "vigor", 20, torch.bfloat16, fold=True)):
        assert other.gd_w3 is None and other.sd_w3 is None and other.grd.w_head3 is None
        assert all(b.w_proj3 is None for b in other.sat.blocks)


def _desc(k, n, b, h, w, two=False, kpad=None):
    d = _lib.ConvDesc()
    d.src0 = d.w = d.dst = d.gate = d.scale = d.shift = 256                                # fake aligned pointers: never dereferenced
    d.c0, d.ld0, d.batch, d.in_h, d.in_w = k, k, b, h, w
    d.kh, d.kw, d.stride, d.pad = (2, 2, 2, 0) if two else (1, 1, 1, 0)
    d.n, d.ldd = n, (n + 3) // 4 * 4
    d.kpad = kpad if kpad is not None else 3 * (4 if two else 1) * k
    if two:
        d.gate = None
    return d


def test_ok_and_route_queries_without_a_gpu():
    lib = _lib.load()
    ok = lambda d: lib.ccvpe_pw_s3_ok(ctypes.byref(d))
    tile = lambda d: (lambda r: ((r >> 8) & 0xf, (r >> 12) & 0xf, (r >> 16) & 0xf, (r >> 20) & 0xf))(lib.ccvpe_pw_s3_route(ctypes.byref(d)))
    assert lib.ccvpe_pw_s3_ok(None) == 0 and lib.ccvpe_pw_s3_route(None) == 0 and lib.ccvpe_pw_s3_f32(None, None) == -1
    # all of N in one workgroup up to 320 columns; wider layers tile N with the 320-column tile
    for n, want in ((80, (2, 5, 1, 4)), (64, (2, 5, 1, 4)), (112, (2, 7, 1, 4)), (126, (2, 2, 4, 8)), (192, (2, 3, 4, 8)), (320, (2, 5, 4, 8)), (1280, (2, 5, 4, 8))):
        d = _desc(672, n, 64, 16, 16)
        assert ok(d) >= 1 and tile(d) == want, (n, tile(d))
    assert ok(_desc(1280, 1280, 64, 16, 16, two=True)) >= 1
    assert ok(_desc(240, 40, 64, 32, 32)) == 0                                             # N <= 48
    assert ok(_desc(248, 80, 64, 32, 32)) == 0                                             # K % 16
    assert ok(_desc(672, 112, 64, 32, 32, kpad=672)) == 0                                  # the fp32 pack's kpad
    d = _desc(672, 112, 64, 32, 32)
    d.src0 = 260
    assert ok(d) == 0                                                                      # misaligned
    d = _desc(672, 112, 64, 32, 32)
    d.kh = d.kw = 3
    d.pad = 1
    assert ok(d) == 0
    d = _desc(672, 112, 64, 32, 32)
    d.act = 1
    assert ok(d) == 0                                                                      # ReLU epilogue: not instantiated
    d = _desc(672, 112, 64, 32, 32)
    d.c1, d.src1 = 8, 256
    assert ok(d) == 0
    d = _desc(672, 112, 64, 32, 32)
    d.kpad = 672
    assert lib.ccvpe_pw_s3_f32(ctypes.byref(d), None) == -1 and b"three-plane pack" in lib.ccvpe_last_error()


def test_fragment_offsets_are_those_of_upconv_s3():
    """csrc/split3_impl.h's S3Frag (what pw_s3.hip reads its fragments with) holds, expression for expression, the five per-lane
    slot offsets spelled out in csrc/upconv_s3.hip — the ones tests/test_upconv_s3.py runs through the bank model of
    tools/lds_layout.py — and the same 24-dword row."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ccvpe_amd", "csrc")
    up = open(os.path.join(csrc, "upconv_s3.hip")).read()
    hdr = open(os.path.join(csrc, "split3_impl.h")).read()
    want = dict(re.findall(r"const int ([aw]\d)off = ([^;]+);", up))
    assert sorted(want) == ["a1", "a2", "w1", "w2", "w3"]
    init = re.search(r"explicit S3Frag\(int g4\)\s*:\s*(.+?)\s*\{\}", hdr, re.S).group(1)
    got = dict(re.findall(r"([aw]\d)\((.+?)\)(?:, (?=[aw]\d\()|$)", init))
    assert got == want, (got, want)
    assert int(re.search(r"constexpr int S3_ROW = (\d+);", hdr).group(1)) == int(re.search(r"constexpr int ROW = (\d+);", up).group(1))
    pw = open(os.path.join(csrc, "pw_s3.hip")).read()
    assert "ROW = S3_ROW" in pw and "S3Frag fr(lane >> 4)" in pw
