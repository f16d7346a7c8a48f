"""Three-plane bf16 kernel of the fp32 folded deconv + 3x3 layers (csrc/upconv_s3.hip) on the MI355X: every tile family,
ragged tiles, all nine border classes and the level-6 PAIR form against the fp64 composition, with an error budget of 4x
today's fp32 kernel's on the same inputs; row pitches wider than the channel counts; the gate; a whole forward against the
fp32 route."""
import pytest
import torch
import torch.nn.functional as F

from ccvpe_amd import models, synth

pytestmark = pytest.mark.gpu

# (cp, cref, cd, c1, co, h1, w1, batch)
ROWS = [(88, 81, 40, 16, 40, 18, 16, 2), (168, 161, 80, 24, 80, 9, 20, 2), (328, 321, 160, 40, 160, 7, 17, 2),
        (648, 641, 320, 112, 320, 5, 16, 2), (64, 64, 32, 16, 32, 19, 35, 2), (128, 128, 64, 24, 64, 8, 32, 2),
        (256, 256, 128, 40, 128, 6, 16, 2),
        (1304, 1281, 1024, 320, 640, 8, 8, 3)]            # level 6, PAIR form: the odd batch leaves the last tile half empty
# (c0, c1, n, h1) of the ten B = 64 decoder layers: localisation levels 6..2, orientation levels 6..2
DECODER_B64 = [(1304, 320, 640, 8), (648, 112, 320, 16), (328, 40, 160, 32), (168, 24, 80, 64), (88, 16, 40, 128),
               (1304, 320, 640, 8), (640, 112, 256, 16), (256, 40, 128, 32), (128, 24, 64, 64), (64, 16, 32, 128)]
# what ccvpe_upconv3x3_s3_ok's measured size rule returns for them (csrc/upconv_s3.hip)
DECODER_B64_OK = [2] * 10


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from ccvpe_amd import ops as _ops, _lib
    _lib.load()
    return _ops


def _ref64(x, skip, wd, bd, w3, b3):
    """relu(conv3x3(cat[deconv2x2s2(x) + bd, skip]) + b3) in fp64 on the device; x [B,h,w,cref], skip [B,2h,2w,c1] NHWC fp32
    -> [B,2h,2w,co].  The deconv is a per-pixel matmul + pixel shuffle, the conv unfold + matmul."""
    b, h, w, _ = x.shape
    cd = wd.shape[1]
    d = torch.einsum("bhwc,cdij->bdhiwj", x.double(), wd.double()).reshape(b, cd, 2 * h, 2 * w) + bd.double()[None, :, None, None]
    cat = torch.cat([d, skip.double().permute(0, 3, 1, 2)], 1)
    cols = F.unfold(F.pad(cat, (1, 1, 1, 1)), 3)                                  # [B, C*9, 4hw]
    out = torch.einsum("bkp,nk->bpn", cols, w3.double().reshape(w3.shape[0], -1)) + b3.double()
    return F.relu(out).reshape(b, 2 * h, 2 * w, -1)


def _case(ops, cp, cref, cd, c1, co, h1, w1, b, pad=0):
    x = torch.zeros((b, h1, w1, cp + pad))
    x[..., :cref] = synth.normal((b, h1, w1, cref), 600 + cp)                    # channels cref..cp: padding of the concat buffer
    x[..., cp:] = 3.0                                                             # beyond the channel count: never read into the result
    skipw = synth.normal((b, 2 * h1, 2 * w1, c1 + pad), 601)
    wd = synth.normal((cref, cd, 2, 2), 602, (1.0 / cref) ** 0.5).cuda()
    bd = synth.normal((cd,), 603, 0.3).cuda()
    w3 = synth.normal((co, cd + c1, 3, 3), 604, (1.0 / (9 * (cd + c1))) ** 0.5).cuda()
    b3 = synth.normal((co,), 605, 0.1).cuda()
    x, skipw = x.cuda(), skipw.cuda()
    ref = _ref64(x[..., :cref], skipw[..., :c1], wd, bd, w3, b3)
    fw, fshift = models._pack_upconv(wd, bd, [(0, 0, cref)], cp, w3, b3, torch.float32)
    fw3 = models._pack_upconv_s3(fw, cp, c1)
    kw = dict(batch=b, h1=h1, w1=w1, c1=c1)
    assert ops.upconv3x3_s3_ok(x, cp, fw3, co, src1=skipw, ld0=cp + pad, ld1=c1 + pad, ldd=co + pad, **kw) >= 1
    dst = torch.full((b, 2 * h1, 2 * w1, co + pad), 7.0, device="cuda")
    got = ops.upconv3x3_s3(x, cp, fw3, fshift, co, src1=skipw, act=ops.ACT_RELU, dst=dst, ld0=cp + pad, ld1=c1 + pad, **kw)
    f32 = ops.upconv3x3(x[..., :cp].contiguous(), cp, fw, fshift, co, src1=skipw[..., :c1].contiguous(), act=ops.ACT_RELU, **kw)
    torch.cuda.synchronize()
    assert got.data_ptr() == dst.data_ptr()
    assert torch.all(dst[..., co:] == 7.0), "wrote past n inside the row pitch"
    scale = ref.abs().max().item()
    e_s3 = (got[..., :co].double() - ref).abs().max().item() / scale
    e_f32 = (f32.double() - ref).abs().max().item() / scale
    print("upconv_s3 err cp=%d c1=%d n=%d %dx%d b=%d pad=%d: s3 %.2e fp32 %.2e" % (cp, c1, co, h1, w1, b, pad, e_s3, e_f32))
    return e_s3, e_f32


@pytest.mark.parametrize("cp,cref,cd,c1,co,h1,w1,b", ROWS)
def test_every_tile_family_against_fp64(ops, cp, cref, cd, c1, co, h1, w1, b):
    e_s3, e_f32 = _case(ops, cp, cref, cd, c1, co, h1, w1, b)
    assert e_s3 <= 4 * max(e_f32, 1e-7), "three-plane error %.3e vs fp32 kernel %.3e" % (e_s3, e_f32)
    assert e_s3 < 1e-5


def test_row_pitches_wider_than_the_channel_counts(ops):
    """Sources with 8 extra (non-zero) columns per pixel and a destination with 8 sentinel columns: nothing is read into the
    result from, or written, past the channel counts."""
    e_s3, e_f32 = _case(ops, 168, 161, 80, 24, 80, 9, 20, 2, pad=8)
    assert e_s3 <= 4 * max(e_f32, 1e-7), "three-plane error %.3e vs fp32 kernel %.3e" % (e_s3, e_f32)
    assert e_s3 < 1e-5


def test_gate(ops):
    from ccvpe_amd import _lib
    probe = torch.empty((1, 1, 1, 2048), device="cuda")
    w3 = lambda c0, c1, n: torch.empty((4, 4 * (-(-c0 // 16)) + 9 * (-(-c1 // 16)), -(-n // 16) * 16, 48), device="cuda",
                                       dtype=torch.bfloat16)
    ok = lambda c0, c1, n, h1, b, **k: ops.upconv3x3_s3_ok(probe, c0, w3(c0, c1, n), n, batch=b, h1=h1, w1=h1, src1=probe, c1=c1,
                                                           ld0=c0, ld1=c1, **k)
    assert [ok(c0, c1, n, h1, 64) for c0, c1, n, h1 in DECODER_B64] == DECODER_B64_OK
    assert ok(648, 112, 320, 16, 1) == 1 and ok(648, 112, 320, 16, 15) == 1     # computed, but fewer than 4096 low-res pixels
    assert ok(648, 112, 320, 16, 16) == 2
    # bf16 storage, a layer without a skip, 8-pixel images that are not the level-6 form, an n without a tile, the fp32 pack's kpad
    assert ops.upconv3x3_s3_ok(probe.to(torch.bfloat16), 648, w3(648, 112, 320), 320, batch=64, h1=16, w1=16,
                               src1=probe.to(torch.bfloat16), c1=112, ld0=648, ld1=112) == 0
    assert ops.upconv3x3_s3_ok(probe, 48, w3(48, 0, 16), 16, batch=64, h1=256, w1=256, ld0=48) == 0
    assert ok(168, 24, 80, 8, 64) == 0 and ok(168, 24, 96, 32, 64) == 0
    x = torch.zeros((1, 12, 12, 168), device="cuda")
    sk = torch.zeros((1, 24, 24, 24), device="cuda")
    bad = w3(168, 24, 80)
    assert ops.upconv3x3_s3_ok(x, 168, bad, 80, batch=1, h1=12, w1=12, src1=sk, c1=24) == 0
    with pytest.raises(_lib.CcvpeError, match="narrower than 16"):     # refused with an error code, nothing is launched
        ops.upconv3x3_s3(x, 168, bad, torch.zeros((9, 80), device="cuda"), 80, batch=1, h1=12, w1=12, src1=sk, c1=24)
    d = ops._s3_desc(probe, 648, w3(648, 112, 320), None, 320, 64, 16, 16, probe, 112, 0, None, 320, 648, 112)
    d.kpad = 3600                                                      # the fp32 pack's
    assert _lib.load().ccvpe_upconv3x3_s3_ok(d) == 0


def test_forward_matches_fp32_route(monkeypatch):
    """A B = 2 fp32 forward with the size rule (and the fold's own pixel threshold) opened reaches the three-plane kernel on all
    ten folded decoder layers: logits and the raw orientation field within 1e-5 of scale of the fp32 route, same arg-max."""
    from ccvpe_amd import ops
    sd = synth.synthetic_state_dict("vigor", 0)
    net = models.CVM_VIGOR_ori_prior("cuda", 0, True)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    grd, sat = synth.synthetic_pair(2, "vigor", 5)
    grd, sat = grd.cuda(), sat.cuda()
    calls = []
    real = ops.upconv3x3_s3

    def spy(*a, **k):
        calls.append(a[4])
        return real(*a, **k)
    monkeypatch.setattr(ops, "upconv3x3_s3", spy)
    monkeypatch.setattr(models, "SPLIT3", True)
    monkeypatch.setattr(models, "SPLIT3_MIN_OK", 1)
    monkeypatch.setattr(models, "FOLD_MIN_PIXELS", 1)
    net.ori_raw_output = True            # conv1_ori's output before F.normalize: a linear chain like the logits, comparable by scale
    with torch.no_grad():
        out_s = [t.clone() for t in net(grd, sat)[:3]]
        n_calls = len(calls)
        monkeypatch.setattr(models, "SPLIT3", False)
        out_f = [t.clone() for t in net(grd, sat)[:3]]
    assert n_calls >= 8 and len(calls) == n_calls, calls
    ls, lf = out_s[0], out_f[0]
    e_log = (ls - lf).abs().max().item() / lf.abs().max().item()
    # the five orientation layers: the un-normalised (cos, sin) field goes through the same kernels at the same depth as the logits
    e_ori = (out_s[2] - out_f[2]).abs().max().item() / out_f[2].abs().max().item()
    # heat map = softmax(logits): logits within d = 1e-5 max |logit| move every probability by a factor inside exp(+-2 d)
    d = 1e-5 * lf.abs().max().item()
    e_heat = (out_s[1] - out_f[1]).abs().max().item() / out_f[1].abs().max().item()
    print("forward s3 vs fp32 route: logits %.2e  raw orientation %.2e  heat map %.2e (bound %.2e)" % (e_log, e_ori, e_heat, 2.5 * d))
    assert e_log <= 1e-5
    assert torch.equal(ls.argmax(1), lf.argmax(1))
    assert e_ori <= 1e-5
    assert e_heat <= 2.5 * d
