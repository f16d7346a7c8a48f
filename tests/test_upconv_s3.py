"""Three-plane bf16 route of the fp32 folded deconv + 3x3 layers (csrc/upconv_s3.hip), on the CPU: the split is exact, the
packed planes sum bit-exactly to the fp32 pack with zero padding, the layout (stage order, taps, parity, padding) reproduces
the layer when it is walked the way the kernel walks it, and the kernel's LDS rows are conflict-free in the bank model."""
import os
import sys

import torch
import torch.nn.functional as F

from ccvpe_amd import synth
from ccvpe_amd.models import _pack_upconv, _pack_upconv_s3, _split3_bf16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layer(cref, cp, cd, c1, co, seed):
    wd = synth.normal((cref, cd, 2, 2), seed, (1.0 / cref) ** 0.5)
    bd = synth.normal((cd,), seed + 1, 0.3)
    w3 = synth.normal((co, cd + c1, 3, 3), seed + 2, (1.0 / (9 * (cd + c1))) ** 0.5)
    b3 = synth.normal((co,), seed + 3, 0.1)
    fw, shift9 = _pack_upconv(wd, bd, [(0, 0, cref)], cp, w3, b3, torch.float32)
    return wd, bd, w3, b3, fw, shift9


def test_split_is_exact_and_planes_shrink_by_2_pow_8():
    g = torch.Generator().manual_seed(5)
    mant = torch.randn((4096,), generator=g)
    expo = torch.randint(-60, 61, (4096,), generator=g).float()
    v = torch.cat([mant * torch.exp2(expo), torch.randn((4096,), generator=g), -torch.rand((1024,), generator=g),
                   torch.tensor([0.0, 1.0, -1.0, 2.0 ** -60, -2.0 ** 60, 1.0 + 2.0 ** -23, 255.0 / 256.0])])
    assert (v < 0).any() and v.abs().max() > 2.0 ** 50 and v[v != 0].abs().min() < 2.0 ** -50
    hi, mid, lo = _split3_bf16(v)
    assert hi.dtype == mid.dtype == lo.dtype == torch.bfloat16
    assert torch.equal(hi.double() + mid.double() + lo.double(), v.double())
    assert bool((mid.double().abs() <= 2.0 ** -8 * v.double().abs()).all())
    assert bool((lo.double().abs() <= 2.0 ** -16 * v.double().abs()).all())


def test_packed_planes_sum_bit_exactly_to_the_fp32_pack_and_pads_are_zero():
    cref, cp, cd, c1, co = 81, 88, 40, 24, 40                       # c0 = 8 mod 16, c1 = 24 (half-empty block), N = 40 (Npad 48)
    _, _, _, _, fw, _ = _layer(cref, cp, cd, c1, co, 700)
    w3p = _pack_upconv_s3(fw, cp, c1)
    nb0, nb1, npad = 6, 2, 48
    assert w3p.dtype == torch.bfloat16 and tuple(w3p.shape) == (4, 4 * nb0 + 9 * nb1, npad, 48) and w3p.is_contiguous()
    total = w3p[..., :16].double() + w3p[..., 16:32].double() + w3p[..., 32:].double()          # [4][stage][npad][16]
    a = total[:, :4 * nb0].reshape(4, nb0, 4, npad, 16).permute(0, 3, 2, 1, 4).reshape(4, npad, 4, nb0 * 16)
    s = total[:, 4 * nb0:].reshape(4, 9, nb1, npad, 16).permute(0, 3, 1, 2, 4).reshape(4, npad, 9, nb1 * 16)
    assert torch.equal(a[..., :cp].reshape(4, npad, 4 * cp), fw[:, :, :4 * cp].double())
    assert torch.equal(s[..., :c1].reshape(4, npad, 9 * c1), fw[:, :, 4 * cp:4 * cp + 9 * c1].double())
    assert float(a[..., cp:].abs().max()) == 0.0 and float(s[..., c1:].abs().max()) == 0.0        # pad columns
    assert float(w3p[:, :, co:].float().abs().max()) == 0.0                                       # pad rows
    assert float(a[..., cref:cp].abs().max()) == 0.0                                              # (padding channels of the concat buffer)
    # not built for bf16 packs or a layer without a skip
    assert _pack_upconv_s3(fw, cp, c1, torch.bfloat16) is None and _pack_upconv_s3(fw.to(torch.bfloat16), cp, c1) is None
    assert _pack_upconv_s3(fw, cp, 0) is None


def test_six_product_walk_of_the_packed_planes_reproduces_the_layer():
    """The kernel's stage walk in plain torch: per stage one (tap, 16-channel block) of split activations against the packed
    [hi|mid|lo] rows, six products; against the fp64 composition conv2d(cat[conv_transpose2d(x), skip])."""
    cref, cp, cd, c1, co, b, h, w = 17, 24, 12, 24, 10, 2, 4, 5
    wd, bd, w3, b3, fw, shift9 = _layer(cref, cp, cd, c1, co, 720)
    x = F.relu(synth.normal((b, cref, h, w), 730))
    skip = F.relu(synth.normal((b, c1, 2 * h, 2 * w), 731))
    want = F.conv2d(torch.cat([F.conv_transpose2d(x.double(), wd.double(), bd.double(), stride=2), skip.double()], 1),
                    w3.double(), b3.double(), padding=1)
    w3p = _pack_upconv_s3(fw, cp, c1)
    nb0, nb1 = 2, 2
    xs = torch.zeros((b, h + 2, w + 2, nb0 * 16))
    xs[:, 1:-1, 1:-1, :cref] = x.permute(0, 2, 3, 1)
    ss = torch.zeros((b, 2 * h + 2, 2 * w + 2, nb1 * 16))
    ss[:, 1:-1, 1:-1, :c1] = skip.permute(0, 2, 3, 1)

    def six(act, wrow):                                           # act [B,h,w,16] fp32, wrow [co,48] bf16 planes
        xh, xm, xl = (t.double() for t in _split3_bf16(act))
        wh, wm, wl = wrow[:, :16].double(), wrow[:, 16:32].double(), wrow[:, 32:].double()
        mm = lambda p, q: torch.einsum("bhwc,nc->bhwn", p, q)
        return mm(xh, wh) + mm(xm, wh) + mm(xh, wm) + mm(xm, wm) + mm(xl, wh) + mm(xh, wl)

    got = torch.zeros((b, 2 * h, 2 * w, co), dtype=torch.float64)
    for py in range(2):
        for px in range(2):
            par = py * 2 + px
            acc = torch.zeros((b, h, w, co), dtype=torch.float64)
            for blk in range(nb0):
                for tap in range(4):
                    du, dv = tap >> 1, tap & 1
                    act = xs[:, du + py:du + py + h, dv + px:dv + px + w, 16 * blk:16 * blk + 16]
                    acc += six(act, w3p[par, blk * 4 + tap, :co])
            for tap in range(9):
                ky, kx = tap // 3, tap % 3
                for blk in range(nb1):
                    act = ss[:, py + ky:py + ky + 2 * h:2, px + kx:px + kx + 2 * w:2, 16 * blk:16 * blk + 16]
                    acc += six(act, w3p[par, 4 * nb0 + tap * nb1 + blk, :co])
            got[:, py::2, px::2] = acc
    rows = torch.tensor([0] + [1] * (2 * h - 2) + [2])
    cols = torch.tensor([0] + [1] * (2 * w - 2) + [2])
    got += shift9.double()[rows[:, None] * 3 + cols[None, :]]
    err = (got.permute(0, 3, 1, 2) - want).abs().max().item()
    assert err <= 1e-6 * want.abs().max().item(), err


def test_lds_rows_of_24_dwords_are_conflict_free_for_every_fragment_and_window_base():
    """csrc/upconv_s3.hip keeps W rows and activation pixels as unswizzled 96-byte [hi|mid|lo] rows; every fragment is one
    ds_read_b128 with the 16-byte slot picked per lane group.  The row pitch, the PAIR gap and the five per-lane slot expressions
    are read from the kernel source and run through the bank model of tools/lds_layout.py."""
    import re
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import lds_layout as L
    src = open(os.path.join(ROOT, "ccvpe_amd", "csrc", "upconv_s3.hip")).read()
    row = int(re.search(r"constexpr int ROW = (\d+);", src).group(1))
    gap = int(re.search(r"frow \+ \(PAIR \? (\d+) \* \(frow >> 3\) : 0\)", src).group(1))
    exprs = dict(re.findall(r"const int ([aw]\doff) = ([^;]+);", src))
    assert sorted(exprs) == ["a1off", "a2off", "w1off", "w2off", "w3off"], exprs

    def slot(expr):                                               # C "c ? a : b" -> a Python function of the lane group g4
        m = re.fullmatch(r"(.+?) \? (.+?) : (.+)", expr)
        py = "(%s) if (%s) else (%s)" % (m.group(2), m.group(1), m.group(3)) if m else expr
        return lambda g4: eval(py, {"g4": g4})
    # the planes each fragment must deliver: 16-byte slots 0-1 = hi, 2-3 = mid, 4-5 = lo
    want = {"a1off": [0, 1, 2, 3], "a2off": [4, 5, 0, 1], "w1off": [0, 1, 0, 1], "w2off": [2, 3, 2, 3], "w3off": [0, 1, 4, 5]}
    for name, expr in exprs.items():
        f = slot(expr)
        assert [f(g) // 4 for g in range(4)] == want[name] and all(f(g) % 4 == 0 for g in range(4)), (name, expr)
        for base in range(32):
            for pair in (False, True):
                addr = lambda lane: (base + lane % 16 + (gap * ((lane % 16) >> 3) if pair else 0)) * row + f(lane // 16)
                assert L.cycles("read_b128", addr) == (4, 4), (name, base, pair)
