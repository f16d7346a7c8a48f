"""Quad form of the three-plane bf16 upconv kernel (csrc/upconv_s3q.hip: all four output parities per workgroup) on the MI355X:
forced per-parity (form 1), forced quad (form 2) and the fp32 kernel against the fp64 composition, the quad form on the budget
of 4x the fp32 kernel's error on the same inputs; bit-identity of the two forms where the layer has one skip block; row pitches
wider than the channel counts; the form gate and what auto picks for the ten B = 64 decoder layers; a whole forward with and
without the quad form."""
import pytest
import torch
import torch.nn.functional as F

from ccvpe_amd import models, synth

pytestmark = pytest.mark.gpu

# (cp, cref, cd, c1, co, h1, w1, batch)
CASES = [(88, 81, 40, 16, 40, 18, 16, 2), (64, 64, 32, 16, 32, 19, 35, 2), (168, 161, 80, 24, 80, 9, 20, 2),
         (128, 128, 64, 24, 64, 8, 32, 2),
         (88, 81, 40, 16, 40, 3, 16, 1),                   # image shorter than one tile
         (64, 64, 32, 16, 32, 9, 17, 3)]                   # one column spills into a second column tile; odd batch
# (c0, c1, n, h1) of the ten B = 64 decoder layers: localisation levels 6..2, orientation levels 6..2
DECODER_B64 = [(1304, 320, 640, 8), (648, 112, 320, 16), (328, 40, 160, 32), (168, 24, 80, 64), (88, 16, 40, 128),
               (1304, 320, 640, 8), (640, 112, 256, 16), (256, 40, 128, 32), (128, 24, 64, 64), (64, 16, 32, 128)]
# ccvpe_upconv3x3_s3_form_ok(desc, 2) for them: the quad form serves 16 < n <= 80
DECODER_B64_QUAD_OK = [0, 0, 0, 2, 2, 0, 0, 0, 2, 2]
# what auto picks (ccvpe_upconv3x3_s3_form_ok(desc, 0)): the measured rule of csrc/upconv_s3.hip (profiles/r11/up_probe.txt):
# the quad form wherever it serves, from 4096 low-res pixels on
DECODER_B64_AUTO = [1, 1, 1, 2, 2, 1, 1, 1, 2, 2]


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
    """-> (quad or None, per_parity, errors of quad / per-parity / fp32 kernel vs fp64, relative to the reference's scale)"""
    from ccvpe_amd import _lib
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
    pitch = dict(src1=skipw, ld0=cp + pad, ld1=c1 + pad)
    assert ops.upconv3x3_s3_form_ok(x, cp, fw3, co, 1, ldd=co + pad, **pitch, **kw) == 1
    scale = ref.abs().max().item()
    out, err = {}, {}
    for form in (1, 2):
        dst = torch.full((b, 2 * h1, 2 * w1, co + pad), 7.0, device="cuda")
        if ops.upconv3x3_s3_form_ok(x, cp, fw3, co, form, ldd=co + pad, **pitch, **kw) == 0:
            assert form == 2
            with pytest.raises(_lib.CcvpeError):                                  # refused with an error code, nothing is launched
                ops.upconv3x3_s3(x, cp, fw3, fshift, co, act=ops.ACT_RELU, dst=dst, form=2, **pitch, **kw)
            torch.cuda.synchronize()
            assert torch.all(dst == 7.0)
            out[form] = None
            continue
        got = ops.upconv3x3_s3(x, cp, fw3, fshift, co, act=ops.ACT_RELU, dst=dst, form=form, **pitch, **kw)
        torch.cuda.synchronize()
        assert got.data_ptr() == dst.data_ptr()
        assert torch.all(dst[..., co:] == 7.0), "form %d wrote past n inside the row pitch" % form
        out[form] = got[..., :co]
        err[form] = (out[form].double() - ref).abs().max().item() / scale
    f32 = ops.upconv3x3(x[..., :cp].contiguous(), cp, fw, fshift, co, src1=skipw[..., :c1].contiguous(), act=ops.ACT_RELU, **kw)
    torch.cuda.synchronize()
    e_f32 = (f32.double() - ref).abs().max().item() / scale
    print("upconv_s3 forms cp=%d c1=%d n=%d %dx%d b=%d pad=%d: quad %s per-parity %.2e fp32 %.2e" % (
        cp, c1, co, h1, w1, b, pad, "%.2e" % err[2] if 2 in err else "not served", err[1], e_f32))
    return out[2], out[1], err.get(2), err[1], e_f32


def _check(quad, per, e_q, e_p, e_f32, c1):
    assert e_p <= 4 * max(e_f32, 1e-7) and e_p < 1e-5, "per-parity error %.3e vs fp32 kernel %.3e" % (e_p, e_f32)
    if quad is None:                                          # an n the quad form was dropped for: refused in _case
        return
    assert e_q <= 4 * max(e_f32, 1e-7), "quad error %.3e vs fp32 kernel %.3e" % (e_q, e_f32)
    assert e_q < 1e-5
    if c1 <= 16:
        assert torch.equal(quad, per), "one skip block: the two forms add the same products in the same order"
    else:
        print("  two skip blocks: max |quad - per-parity| = %.3e" % (quad - per).abs().max().item())


@pytest.mark.parametrize("cp,cref,cd,c1,co,h1,w1,b", CASES)
def test_quad_and_per_parity_against_fp64(ops, cp, cref, cd, c1, co, h1, w1, b):
    _check(*_case(ops, cp, cref, cd, c1, co, h1, w1, b), c1)


def test_row_pitches_wider_than_the_channel_counts(ops):
    """The N = 40 case with 8 extra (non-zero) columns per source pixel and 8 sentinel columns per destination pixel: nothing is
    read into the result from, or written, past the channel counts."""
    _check(*_case(ops, 88, 81, 40, 16, 40, 18, 16, 2, pad=8), 16)


def test_form_gate_and_what_auto_picks(ops):
    from ccvpe_amd import _lib
    lib = _lib.load()
    probe = torch.empty((1, 1, 1, 2048), device="cuda")
    w3 = lambda c0, c1, n: torch.empty((4, 4 * (-(-c0 // 16)) + 9 * (-(-c1 // 16)), -(-n // 16) * 16, 48), device="cuda",
                                       dtype=torch.bfloat16)
    ok = lambda c0, c1, n, h1, b, form: ops.upconv3x3_s3_form_ok(probe, c0, w3(c0, c1, n), n, form, batch=b, h1=h1, w1=h1,
                                                                 src1=probe, c1=c1, ld0=c0, ld1=c1)
    assert [ok(c0, c1, n, h1, 64, 1) for c0, c1, n, h1 in DECODER_B64] == [1] * 10
    assert [ok(c0, c1, n, h1, 64, 2) for c0, c1, n, h1 in DECODER_B64] == DECODER_B64_QUAD_OK
    assert [ok(c0, c1, n, h1, 64, 0) for c0, c1, n, h1 in DECODER_B64] == DECODER_B64_AUTO
    assert ok(88, 16, 40, 16, 15, 0) == 1 and ok(88, 16, 40, 16, 16, 0) == 2     # fewer than 4096 low-res pixels: not measured
    assert ok(88, 16, 40, 16, 15, 2) == 2                                        # ... but computed when forced
    assert ok(88, 16, 40, 128, 64, 3) == 0 and ok(168, 24, 80, 8, 64, 1) == 0    # no such form; a desc _ok refuses
    prev = lib.ccvpe_set_s3_quad(0)
    try:
        assert prev == 1
        assert [ok(c0, c1, n, h1, 64, 0) for c0, c1, n, h1 in DECODER_B64] == [1] * 10
        assert [ok(c0, c1, n, h1, 64, 2) for c0, c1, n, h1 in DECODER_B64] == DECODER_B64_QUAD_OK    # forcing ignores the switch
    finally:
        lib.ccvpe_set_s3_quad(prev)
    x = torch.zeros((1, 16, 16, 648), device="cuda")
    sk = torch.zeros((1, 32, 32, 112), device="cuda")
    with pytest.raises(_lib.CcvpeError, match="quad form"):                      # n = 320: refused with an error code, nothing is launched
        ops.upconv3x3_s3(x, 648, w3(648, 112, 320), torch.zeros((9, 320), device="cuda"), 320, batch=1, h1=16, w1=16, src1=sk, c1=112,
                         form=2)


def test_forward_with_and_without_the_quad_form(monkeypatch):
    """A B = 2 fp32 forward with the three-plane route opened on all ten folded layers, the form left to the library, against
    the same forward with the quad form switched off: logits and the raw orientation field within 1e-5 of scale, same arg-max;
    the quad kernel ran on at least the two level-2 layers (2 x 128 x 128 low-res pixels each)."""
    from ccvpe_amd import ops, _lib
    lib = _lib.load()
    sd = synth.synthetic_state_dict("vigor", 0)
    net = models.CVM_VIGOR_ori_prior("cuda", 0, True)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    grd, sat = synth.synthetic_pair(2, "vigor", 5)
    grd, sat = grd.cuda(), sat.cuda()
    calls = []
    real = ops.upconv3x3_s3

    def spy(*a, **k):
        form = ops.upconv3x3_s3_form_ok(a[0], a[1], a[2], a[4], 0, batch=k["batch"], h1=k["h1"], w1=k["w1"], src1=k["src1"], c1=k["c1"])
        calls.append((a[4], form))                     # what auto is about to run
        return real(*a, **k)
    monkeypatch.setattr(ops, "upconv3x3_s3", spy)
    monkeypatch.setattr(models, "SPLIT3", True)
    monkeypatch.setattr(models, "SPLIT3_MIN_OK", 1)
    monkeypatch.setattr(models, "FOLD_MIN_PIXELS", 1)
    net.ori_raw_output = True            # conv1_ori's output before F.normalize: a linear chain like the logits, comparable by scale
    with torch.no_grad():
        out_q = [t.clone() for t in net(grd, sat)[:3]]
        with_quad = list(calls)
        del calls[:]
        prev = lib.ccvpe_set_s3_quad(0)
        try:
            out_p = [t.clone() for t in net(grd, sat)[:3]]
        finally:
            lib.ccvpe_set_s3_quad(prev)
    assert len(with_quad) >= 8 and [n for n, _ in calls] == [n for n, _ in with_quad]
    assert sorted(n for n, f in with_quad if f == 2)[:2] == [32, 40] and all(f == 1 for _, f in calls), (with_quad, calls)
    lq, lp = out_q[0], out_p[0]
    e_log = (lq - lp).abs().max().item() / lp.abs().max().item()
    e_ori = (out_q[2] - out_p[2]).abs().max().item() / out_p[2].abs().max().item()
    print("forward quad vs per-parity: logits %.2e  raw orientation %.2e  quad layers n = %s" % (
        e_log, e_ori, [n for n, f in with_quad if f == 2]))
    assert e_log <= 1e-5
    assert torch.equal(lq.argmax(1), lp.argmax(1))
    assert e_ori <= 1e-5
