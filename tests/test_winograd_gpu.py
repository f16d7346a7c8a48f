"""Winograd F(2x2,3x3) kernel of the fp32 convK.2 layers (csrc/conv3x3_wino.hip) on the MI355X: every decoder conv.1 shape
against an fp64 convolution, with an error budget of 4x the direct kernel's on the same inputs; borders, row pitches != the
channel count, N = 40, partial workgroup tiles; which shapes take the route; a whole forward against the direct path."""
import pytest
import torch

from ccvpe_amd import models, synth

pytestmark = pytest.mark.gpu

# (C = N, H = W) of the conv.1 layers: localisation levels 6..2, orientation levels 6..2 (B = 64 in the headline)
SHAPES = [(640, 16), (320, 32), (160, 64), (80, 128), (40, 256), (256, 32), (128, 64), (64, 128), (32, 256)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from ccvpe_amd import ops as _ops, _lib
    _lib.load()
    return _ops


def _conv64(x, w, bias):
    """x [B,H,W,C] fp32, w [N,C,3,3] -> fp64 [B,H,W,N] (unfold + matmul in fp64 on the device)."""
    b, h, wd, c = x.shape
    xp = torch.nn.functional.pad(x.double().permute(0, 3, 1, 2), (1, 1, 1, 1))
    cols = torch.nn.functional.unfold(xp, 3)                                    # [B, C*9, H*W]
    out = torch.einsum("bkp,nk->bpn", cols, w.double().reshape(w.shape[0], -1))
    return (out + bias.double()).reshape(b, h, wd, -1)


def _batch_for(ops, c, n, h, w, u):
    b = max(1, -(-16384 // (h * w)))
    probe = torch.empty((1, 1, 1, c), device="cuda")
    while not ops.conv3x3_wino_ok(probe, c, u, n, batch=b, in_h=h, in_w=w):
        b *= 2
        assert b <= 256, "no batch takes the Winograd route at %s" % ((c, n, h, w),)
    return b


def _case(ops, c, n, h, w, pad_in=0, pad_out=0, seed=0):
    wt = synth.normal((n, c, 3, 3), 10 + seed, (1.0 / (9 * c)) ** 0.5).cuda()
    bias = synth.normal((n,), 20 + seed, 0.1).cuda()
    u = models._pack_wino(wt)
    b = _batch_for(ops, c, n, h, w, u)
    xin = synth.normal((b, h, w, c + pad_in), 30 + seed).cuda()
    x = xin[..., :c]
    ref = _conv64(x, wt, bias)
    dst = torch.full((b, h, w, n + pad_out), 7.0, device="cuda")
    got = ops.conv3x3_wino(xin, c, u, n, batch=b, in_h=h, in_w=w, shift=bias, dst=dst, ld0=c + pad_in)
    direct = ops.conv_igemm(xin, c, models._pack_conv(wt), n, batch=b, in_h=h, in_w=w, kh=3, kw=3, pad=1, shift=bias,
                            ld0=c + pad_in)
    torch.cuda.synchronize()
    assert torch.all(dst[..., n:] == 7.0), "wrote past n inside the row pitch"
    scale = ref.abs().max().item()
    e_w = (got[..., :n].double() - ref).abs().max().item() / scale
    e_d = (direct.double() - ref).abs().max().item() / scale
    print("wino err c=%d n=%d %dx%d b=%d: winograd %.2e direct %.2e" % (c, n, h, w, b, e_w, e_d))
    return e_w, e_d


@pytest.mark.parametrize("c,hw", SHAPES)
def test_conv1_shapes_against_fp64(ops, c, hw):
    e_w, e_d = _case(ops, c, c, hw, hw, pad_in=8 if c % 64 else 0, pad_out=8 if c == 40 else 0)
    assert e_w <= 4 * max(e_d, 1e-7), "Winograd error %.3e vs direct %.3e" % (e_w, e_d)
    assert e_w < 1e-5


@pytest.mark.parametrize("c,n,h,w", [(48, 40, 20, 36), (56, 72, 34, 18), (96, 8, 30, 30)])
def test_partial_tiles_pitches_and_narrow_n(ops, c, n, h, w):
    """H / W not multiples of the 16 x 16 workgroup block, c0 not a multiple of 16, N below / not a multiple of 32."""
    e_w, e_d = _case(ops, c, n, h, w, pad_in=4, pad_out=4, seed=1)
    assert e_w <= 4 * max(e_d, 1e-7), "Winograd error %.3e vs direct %.3e" % (e_w, e_d)
    assert e_w < 1e-5


def test_route_gate(ops):
    probe = torch.empty((1, 1, 1, 640), device="cuda")
    u = lambda c, n: torch.empty((-(-n // 32) * 32, 16 * (-(-c // 16) * 16)), device="cuda")
    ok = lambda c, n, hw, b, **k: ops.conv3x3_wino_ok(probe[..., :c] if c <= 640 else probe, c, u(c, n), n, batch=b,
                                                      in_h=hw, in_w=hw, **k)
    for c, hw in SHAPES:                                   # the B = 64 decoder shapes take it
        assert ok(c, c, hw, 64), (c, hw)
    assert not ok(640, 640, 16, 1)                         # below 16384 output pixels
    assert not ok(640, 640, 16, 8)                         # small batch: the direct path splits K there
    assert not ok(16, 16, 256, 64)                         # c0 < 32
    assert not ok(64, 64, 8, 64)                           # 8 x 8 at B = 64: 4096 pixels
    assert not ops.conv3x3_wino_ok(probe.to(torch.bfloat16), 640, u(640, 640), 640, batch=64, in_h=16, in_w=16)
    from ccvpe_amd import _lib
    from ccvpe_amd._lib import ConvDesc
    d = ops._wino_desc(probe, 64, u(64, 64), 64, 64, 17, 18, None, None, 64, 640)       # odd H
    assert _lib.load().ccvpe_conv3x3_wino_ok(d) == 0
    assert isinstance(d, ConvDesc)


def test_forward_matches_direct_path(monkeypatch):
    """A B = 4 fp32 forward reaches the Winograd kernel on three decoder layers: logits within the forward tests' tolerance of
    the direct path, same arg-max."""
    from ccvpe_amd import ops
    sd = synth.synthetic_state_dict("vigor", 0)
    net = models.CVM_VIGOR_ori_prior("cuda", 0, True)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    grd, sat = synth.synthetic_pair(4, "vigor", 5)
    grd, sat = grd.cuda(), sat.cuda()
    calls = []
    real = ops.conv3x3_wino

    def spy(*a, **k):
        calls.append(a[3])
        return real(*a, **k)
    monkeypatch.setattr(ops, "conv3x3_wino", spy)
    with torch.no_grad():
        out_w = [t.clone() for t in net(grd, sat)[:2]]
        monkeypatch.setattr(models, "WINO", False)
        out_d = [t.clone() for t in net(grd, sat)[:2]]
    assert len(calls) >= 3, calls
    lw, ld = out_w[0], out_d[0]
    assert (lw - ld).abs().max().item() <= 1e-5 * ld.abs().max().item()
    assert torch.equal(lw.argmax(1), ld.argmax(1))
