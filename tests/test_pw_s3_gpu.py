"""Three-plane bf16 kernel of the fp32 1x1 GEMMs behind the encoders' depthwise stage and of the descriptor heads
(csrc/pw_s3.hip) on the MI355X: every tile, ragged tiles that straddle samples with a gate per sample, row pitches wider than the
channel counts, the residual, the swish epilogue with N tiled, the 2x2 stride-2 form — against the fp64 composition of the same
fp32 inputs, with an error budget of 4x today's fp32 kernel's and an elementwise worst-case bound; the _ok answers; a whole
forward against the conv_igemm route."""
import pytest
import torch

from ccvpe_amd import models, synth

pytestmark = pytest.mark.gpu

# (K, N, ground M, aerial M) of the B = 64 layers of DESIGN section 4's table: the projections of blocks 5, 6-7, 8, 9-10, 11, 12-14,
# 15 and _conv_head; then the two descriptor heads (ground 1x1, aerial 2x2 stride 2 with K = 4 * 1280)
ENCODER_B64 = [(240, 80, 51200, 65536), (480, 80, 51200, 65536), (480, 112, 51200, 65536), (672, 112, 51200, 65536),
               (672, 192, 12800, 16384), (1152, 192, 12800, 16384), (1152, 320, 12800, 16384), (320, 1280, 12800, 16384)]
# what ccvpe_pw_s3_ok's measured size rule returns for them (csrc/pw_s3.hip): (ground, aerial) per row
ENCODER_B64_OK = [(2, 2)] * 8
HEADS_B64_OK = (2, 2)          # ground descriptors (1280 -> 126, M = 12 800), aerial descriptor (5120 -> 1280, M = 4 096)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from ccvpe_amd import ops as _ops, _lib
    _lib.load()
    return _ops


def _case(ops, k, n, b, h, w, *, gate=True, scale=True, shift=True, resid=False, act=0, pad=0, dpad=None, two=False, seed=0):
    """One layer through pw_s3 and conv_igemm against fp64; returns (e_s3, e_f32, got).  pad: extra (non-zero) columns per source
    / residual row and (dpad, default pad) sentinel columns per destination row."""
    dpad = pad if dpad is None else dpad
    taps = 4 if two else 1
    kk = taps * k
    ho, wo = (h // 2, w // 2) if two else (h, w)
    x = torch.full((b, h, w, k + pad), 3.0)
    x[..., :k] = synth.normal((b, h, w, k), 700 + seed)
    wt = synth.normal((n, kk), 701 + seed, kk ** -0.5).cuda()
    g = synth.uniform((b, k), 702 + seed, 0.05, 1.0).cuda() if gate else None
    sc = synth.uniform((n,), 703 + seed, 0.5, 1.5).cuda() if scale else None
    sh = synth.normal((n,), 704 + seed, 0.3).cuda() if shift else None
    r = None
    if resid:
        r = torch.full((b, ho, wo, n + pad), 5.0)
        r[..., :n] = synth.normal((b, ho, wo, n), 705 + seed)
        r = r.cuda()
    x = x.cuda()
    # fp64 composition of the same fp32 inputs
    a = x[..., :k].double()
    if gate:
        a = a * g.double()[:, None, None, :]
    if two:      # k = (ky * 2 + kx) * c0 + ch
        a = a[:, :2 * ho, :2 * wo].reshape(b, ho, 2, wo, 2, k).permute(0, 1, 3, 2, 4, 5).reshape(b, ho, wo, kk)
    pre = a @ wt.double().t()
    mag = a.abs() @ wt.double().abs().t()                       # sum_k |a g w|
    s64 = sc.double() if scale else torch.ones((n,), dtype=torch.float64, device="cuda")
    t = pre * s64 + (sh.double() if shift else 0.0)
    if act == ops.ACT_SWISH:
        t = t * torch.sigmoid(t)
    ref = t + (r[..., :n].double() if resid else 0.0)
    wp = models._pad2(wt)
    w3 = models._pack_pw_s3(wp)
    kw = dict(batch=b, in_h=h, in_w=w, gate=g, residual=r, act=act)
    assert ops.pw_s3_ok(x, k, w3, n, two=two, ldd=n + dpad, **kw) >= 1
    dst = torch.full((b, ho, wo, n + dpad), 7.0, device="cuda")
    got = ops.pw_s3(x, k, w3, n, two=two, scale=sc, shift=sh, dst=dst, **kw)
    cv = dict(kh=2, kw=2, stride=2) if two else {}
    f32 = ops.conv_igemm(x, k, wp, n, scale=sc, shift=sh, ldd=n + dpad, **kw, **cv)
    torch.cuda.synchronize()
    assert got.data_ptr() == dst.data_ptr()
    if dpad:
        assert torch.all(dst[..., n:] == 7.0), "wrote past n inside the row pitch"
    ref_max = ref.abs().max().item()
    err = (got[..., :n].double() - ref).abs()
    e_s3 = err.max().item() / ref_max
    e_f32 = (f32[..., :n].double() - ref).abs().max().item() / ref_max
    print("pw_s3 err K=%d N=%d M=%d two=%d pad=%d: s3 %.2e fp32 %.2e" % (kk, n, b * ho * wo, two, pad, e_s3, e_f32))
    # worst-case fp32 accumulation + three dropped products of at most 2^-24 |x||w| each: catches a misplaced element
    bound = (kk + 8) * 2.0 ** -24 * s64.abs() * mag + 2.0 ** -23 * ref.abs()
    worst = (err - bound).max().item()
    assert worst <= 0, "an element is %.3e outside its worst-case bound" % worst
    assert e_s3 <= 4 * max(e_f32, 1e-7), "three-plane error %.3e vs fp32 kernel %.3e" % (e_s3, e_f32)
    assert e_s3 < 1e-5
    return e_s3, e_f32, got


def test_k240_odd_stage_count_n80(ops):
    _case(ops, 240, 80, 2, 9, 11)                                # 15 stages; M = 198: two 128-row tiles, the second ragged


def test_k672_n112_seven_column_tiles(ops):
    _case(ops, 672, 112, 2, 10, 13, resid=True, seed=10)        # M = 260: three tiles


def test_k1152_n192_ragged_tiles_straddle_samples(ops):
    """M = 3 x 5 x 7 = 105 rows in 64-row tiles: 35 rows per sample, so both tiles mix samples and every row takes its own
    sample's gate; run twice: bit-identical."""
    _, _, a = _case(ops, 1152, 192, 3, 5, 7, resid=True, seed=20)
    a = a.clone()
    _, _, b = _case(ops, 1152, 192, 3, 5, 7, resid=True, seed=20)
    assert torch.equal(a, b), "two runs differ"


def test_n320_residual_and_row_pitches_wider_than_the_channel_counts(ops):
    """ld0 = K + 8, ldres = ldd = n + 8: nothing is read into the result from, or written, past the channel counts."""
    _case(ops, 672, 320, 2, 7, 9, resid=True, pad=8, seed=30)


def test_swish_head_n1280_tiles_n(ops):
    _case(ops, 320, 1280, 2, 4, 4, gate=False, act=2, seed=40)


def test_2x2_stride2_descriptor_form(ops):
    _case(ops, 64, 126, 3, 6, 6, gate=False, scale=False, two=True, dpad=2, seed=50)      # ldd = 128 like the ground head's; the 128-column tile


def test_no_gate_no_scale(ops):
    _case(ops, 128, 80, 2, 8, 9, gate=False, scale=False, shift=False, seed=60)


def test_ok_answers(ops):
    from ccvpe_amd import _lib
    probe = torch.empty((1, 1, 1, 8192), device="cuda")
    w3 = lambda kk, n: torch.empty((kk // 16, -(-n // 16) * 16, 48), device="cuda", dtype=torch.bfloat16)
    gate = torch.empty((64 * 2048,), device="cuda")

    def ok(k, n, b, h, w, two=False, **kw):
        return ops.pw_s3_ok(probe, k, w3((4 if two else 1) * k, n), n, batch=b, in_h=h, in_w=w, two=two, ld0=k, **kw)
    # the measured size rule at B = 64 (ground 20 x 40 / 10 x 20, aerial 32 x 32 / 16 x 16), pinned
    got = [(ok(k, n, 64, *((20, 40) if mg == 51200 else (10, 20)), gate=gate), ok(k, n, 64, *((32, 32) if ma == 65536 else (16, 16)), gate=gate))
           for k, n, mg, ma in ENCODER_B64]
    assert got == ENCODER_B64_OK, got
    assert (ok(1280, 126, 64, 10, 20, ldd=128), ok(1280, 1280, 64, 16, 16, two=True)) == HEADS_B64_OK
    assert ok(240, 40, 64, 32, 32) == 0                                      # N <= 48: block 4 stays with the narrow projection kernel
    assert ok(1152, 192, 1, 4, 4) == 1                                        # computed, but below every measured size
    # dtype, K % 16, a bad pack size, misalignment
    assert ops.pw_s3_ok(probe.to(torch.bfloat16), 672, w3(672, 112), 112, batch=64, in_h=32, in_w=32, ld0=672) == 0
    assert ops.pw_s3_ok(probe, 672, w3(672, 112).float(), 112, batch=64, in_h=32, in_w=32, ld0=672) == 0
    assert ops.pw_s3_ok(probe, 248, torch.empty((15, 80, 48), device="cuda", dtype=torch.bfloat16), 80, batch=64, in_h=32, in_w=32, ld0=248) == 0
    assert ops.pw_s3_ok(probe, 672, w3(656, 112), 112, batch=64, in_h=32, in_w=32, ld0=672) == 0          # a stage short
    assert ops.pw_s3_ok(probe, 672, w3(672, 128), 112, batch=64, in_h=32, in_w=32, ld0=672) == 0          # rows of another n
    assert ops.pw_s3_ok(probe[..., 1:], 672, w3(672, 112), 112, batch=64, in_h=32, in_w=32, ld0=672) == 0  # src0 4 bytes off 16
    assert ok(672, 112, 64, 32, 32, act=ops.ACT_RELU) == 0
    x = torch.zeros((1, 4, 4, 672), device="cuda")
    with pytest.raises(_lib.CcvpeError, match="three-plane pack"):          # refused with an error code, nothing is launched
        d = ops._pw_s3_desc(x, 672, w3(672, 112), 112, 1, 4, 4, False, None, None, None, None, 0, x, 112, 672)
        d.kpad = 672                                                         # the fp32 pack's
        assert _lib.load().ccvpe_pw_s3_ok(d) == 0
        _lib.check(_lib.load().ccvpe_pw_s3_f32(d, None), "ccvpe_pw_s3_f32")


def test_forward_matches_conv_igemm_route(monkeypatch):
    """A B = 2 fp32 forward with the size rule opened reaches the three-plane kernel on every layer it serves (11 projections + the
    head per encoder, the two descriptor heads): logits, raw orientation and heat map within 1e-5 of scale of the
    CCVPE_SPLIT3_PW=0 route, same arg-max."""
    from ccvpe_amd import ops
    sd = synth.synthetic_state_dict("vigor", 0)
    net = models.CVM_VIGOR_ori_prior("cuda", 0, True)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    grd, sat = synth.synthetic_pair(2, "vigor", 5)
    grd, sat = grd.cuda(), sat.cuda()
    monkeypatch.setattr(models, "SPLIT3", True)
    monkeypatch.setattr(models, "SPLIT3_PW", True)
    monkeypatch.setattr(models, "SPLIT3_PW_MIN_OK", 1)
    net.ori_raw_output = True            # conv1_ori's output before F.normalize: a linear chain like the logits, comparable by scale
    rec = ops.LaunchRecorder()
    ops.set_recorder(rec)
    try:
        with torch.no_grad():
            out_s = [t.clone() for t in net(grd, sat)[:3]]
    finally:
        ops.set_recorder(None)
    names = [it[0] for it in rec.items if it[0].startswith("pw_s3_kernel<")]
    tags = [it[1] for it in rec.items if it[0].startswith("pw_s3_kernel<")]
    assert len(names) == 2 * 12 + 2, (len(names), tags)
    assert sum(t.startswith("2x2 s2") for t in tags) == 1
    assert set(names) == {"pw_s3_kernel<2,5,1,4>", "pw_s3_kernel<2,7,1,4>", "pw_s3_kernel<2,2,4,8>", "pw_s3_kernel<2,3,4,8>", "pw_s3_kernel<2,5,4,8>"}
    monkeypatch.setattr(models, "SPLIT3_PW", False)
    rec = ops.LaunchRecorder()
    ops.set_recorder(rec)
    try:
        with torch.no_grad():
            out_f = [t.clone() for t in net(grd, sat)[:3]]
    finally:
        ops.set_recorder(None)
    assert not [it[0] for it in rec.items if it[0].startswith("pw_s3_kernel<")]
    ls, lf = out_s[0], out_f[0]
    e_log = (ls - lf).abs().max().item() / lf.abs().max().item()
    e_ori = (out_s[2] - out_f[2]).abs().max().item() / out_f[2].abs().max().item()
    e_heat = (out_s[1] - out_f[1]).abs().max().item() / out_f[1].abs().max().item()
    print("forward pw_s3 vs conv_igemm route: logits %.2e  raw orientation %.2e  heat map %.2e" % (e_log, e_ori, e_heat))
    assert e_log <= 1e-5
    assert torch.equal(ls.argmax(1), lf.argmax(1))
    assert torch.equal(out_s[1].reshape(2, -1).argmax(1), out_f[1].reshape(2, -1).argmax(1))
    assert e_ori <= 1e-5
    assert e_heat <= 1e-5
