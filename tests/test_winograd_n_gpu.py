"""conv3x3_wino_n_kernel (csrc/conv3x3_wino_n.hip) on the MI355X: the fp32 Winograd conv.1 with all N <= 80 columns in one
workgroup is bit-identical to conv3x3_wino_kernel; its fused one-hypothesis matching against the float64 composition
(convolution, then ccvpe_match_level's definition), within 2x the error of the two-launch path (conv3x3_wino + match_level) on
the same inputs; a B = 2 forward through the new route against the old one."""
import pytest
import torch

from ccvpe_amd import models, synth

pytestmark = pytest.mark.gpu

B = 2
SHAPES = [(40, 40), (80, 80), (32, 32), (64, 64), (48, 40)]        # (c0, N); c0 = 40: a last chunk of 8 valid channels
SIZES = [(16, 16), (18, 34)]                                       # one full tile; edge tiles in both directions, even sizes
REAL_STRIDE = {80: 4, 40: 2, 64: 4, 32: 2}                         # MATCH_STRIDES["vigor"] of the level the layer feeds
# (shift, stride or None = the level's real one, window_offset, L as a fraction of N, zero neighbourhood + zero bias)
MATCH_CFGS = {"full": (0, 1, 0, 1.0, False), "rolled": (3, None, 0, 0.5, False), "offset": (-2, 1, 5, 0.8, True)}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from ccvpe_amd import ops as _ops, _lib
    _lib.load()
    return _ops


@pytest.fixture(scope="module")
def layers():
    """(c0, n, h, w) -> inputs and the float64 convolution, computed once per shape and left unchanged."""
    cache = {}

    def get(c, n, h, w):
        key = (c, n, h, w)
        if key not in cache:
            wt = synth.normal((n, c, 3, 3), 11, (1.0 / (9 * c)) ** 0.5).cuda()
            bias = synth.normal((n,), 21, 0.1).cuda()
            xin = synth.normal((B, h, w, c + 4), 31).cuda()                    # ld0 > c0
            xz = xin.clone()
            xz[0, 4:7, 4:7, :] = 0.0                                           # the 3 x 3 neighbourhood of pixel (0, 5, 5)
            cache[key] = dict(wt=wt, u=models._pack_wino(wt), bias=bias, zbias=torch.zeros_like(bias), xin=xin, xz=xz)
        return cache[key]
    return get


def _conv64(x, w, bias):
    """x [B,H,W,C] fp32, w [N,C,3,3] -> fp64 [B,H,W,N]"""
    b, h, wd, c = x.shape
    xp = torch.nn.functional.pad(x.double().permute(0, 3, 1, 2), (1, 1, 1, 1))
    cols = torch.nn.functional.unfold(xp, 3)
    out = torch.einsum("bkp,nk->bpn", cols, w.double().reshape(w.shape[0], -1))
    return (out + bias.double()).reshape(b, h, wd, -1)


def _match64(x, g, L, shift, stride, window_offset, ldo):
    """ccvpe_match_level's definition for one rotation hypothesis, in float64: channel c of x meets g[(c + off) mod N] where that
    index is below L, off = (-shift * stride - window_offset) mod N; cosine without eps; rows [x / max(|x|, 1e-12) | score | 0]."""
    b, h, w, n = x.shape
    off = (-(shift * stride + window_offset)) % n
    k = (torch.arange(n, device=x.device) + off) % n
    inw = k < L
    gg = torch.zeros((b, n), dtype=torch.float64, device=x.device)
    gg[:, inw] = g.double()[:, k[inw]]
    dt = torch.einsum("bhwc,bc->bhw", x, gg)
    wn = (x[..., inw] ** 2).sum(-1).sqrt()
    gnorm = g.double()[:, :L].norm(dim=1)
    score = dt / (wn * gnorm[:, None, None])
    cat = torch.zeros((b, h, w, ldo), dtype=torch.float64, device=x.device)
    cat[..., :n] = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    cat[..., n] = score
    return score[:, None], cat


def _rel_err(got, ref):
    """max |got - ref| / max |ref| over the finite reference values; where the reference is NaN (0 / 0) `got` must be too"""
    nan = ref.isnan()
    assert torch.equal(got.isnan(), nan), "NaN pattern differs from the float64 reference"
    d = (got.double() - ref)[~nan].abs().max().item()
    return d / ref[~nan].abs().max().item()


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("c,n", SHAPES)
def test_bit_identical_to_conv3x3_wino(ops, layers, c, n, h, w):
    lay = layers(c, n, h, w)
    kw = dict(batch=B, in_h=h, in_w=w, ld0=c + 4)
    assert ops.conv3x3_wino_n_ok(lay["xin"], c, lay["u"], n, ldd=n + 4, **kw) >= 1
    d_ref = torch.full((B, h, w, n + 4), 7.0, device="cuda")                  # ldd > n
    d_new = torch.full((B, h, w, n + 4), 7.0, device="cuda")
    ops.conv3x3_wino(lay["xin"], c, lay["u"], n, shift=lay["bias"], dst=d_ref, **kw)
    ops.conv3x3_wino_n(lay["xin"], c, lay["u"], n, shift=lay["bias"], dst=d_new, **kw)
    torch.cuda.synchronize()
    assert torch.all(d_new[..., n:] == 7.0), "wrote past n inside the row pitch"
    assert torch.equal(d_new, d_ref)
    ref = _conv64(lay["xin"][..., :c], lay["wt"], lay["bias"])                # (and both are the convolution)
    assert (d_new[..., :n].double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


@pytest.mark.parametrize("cfg", sorted(MATCH_CFGS))
@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("c,n", SHAPES)
def test_fused_matching_against_float64(ops, layers, c, n, h, w, cfg):
    """scores and cat of ccvpe_conv3x3_wino_match1_f32 against float64, elementwise relative to max |ref|; the bound is 2x the
    two-launch path's error on the same inputs (only the order of two short per-pixel sums differs)."""
    shift, stride, wo, lfrac, zero = MATCH_CFGS[cfg]
    stride = REAL_STRIDE[n] if stride is None else stride
    L = max(1, int(n * lfrac))
    lay = layers(c, n, h, w)
    xin, bias = (lay["xz"], lay["zbias"]) if zero else (lay["xin"], lay["bias"])
    g = synth.normal((B, L + 8), 41).cuda()
    ldo = (n + 1 + 7) // 8 * 8
    kw = dict(batch=B, in_h=h, in_w=w)
    x64 = _conv64(xin[..., :c], lay["wt"], bias)
    if zero:
        assert float(x64[0, 5, 5].abs().max()) == 0.0                         # the 1e-12 clamp is reached
    sc_ref, cat_ref = _match64(x64, g[:, :L], L, shift, stride, wo, ldo)

    assert ops.conv3x3_match1(xin, c, lay["u"], n, None, L, shift, stride, ldo, bias=bias, query_only=True, **kw) >= 1
    sc, cat = ops.conv3x3_match1(xin, c, lay["u"], n, g[:, :L], L, shift, stride, ldo, bias=bias, window_offset=wo, **kw)
    y = ops.conv3x3_wino(xin, c, lay["u"], n, shift=bias, ld0=c + 4, **kw)
    sc2, cat2 = ops.match_level(y, g[:, :L], L, [shift], 1, 0, stride, ldo, channels=n, window_offset=wo)
    torch.cuda.synchronize()
    assert tuple(sc.shape) == (B, 1, h, w) and tuple(cat.shape) == (B, h, w, ldo) and cat.dtype == torch.float32
    assert float(cat[..., n + 1:].abs().max()) == 0.0, "pad columns must be written as zero"
    if zero:
        assert float(cat[0, 5, 5, :n].abs().max()) == 0.0
    e_sc, e_sc2 = _rel_err(sc, sc_ref), _rel_err(sc2, sc_ref)
    e_cat, e_cat2 = _rel_err(cat, cat_ref), _rel_err(cat2, cat_ref)
    print("wino_match err c0=%d n=%d %dx%d %-6s L=%d shift=%d stride=%d wo=%d: scores fused %.3e two-launch %.3e | cat fused %.3e "
          "two-launch %.3e" % (c, n, h, w, cfg, L, shift, stride, wo, e_sc, e_sc2, e_cat, e_cat2))
    assert e_sc2 < 1e-4 and e_cat2 < 1e-4, "the float64 reference and match_level disagree"
    assert e_sc <= 2 * e_sc2, "scores: fused %.3e vs two-launch %.3e" % (e_sc, e_sc2)
    assert e_cat <= 2 * e_cat2, "cat: fused %.3e vs two-launch %.3e" % (e_cat, e_cat2)


def test_forward_through_the_new_route(monkeypatch):
    """A B = 2 CVM_VIGOR_ori_prior(0) forward with the size rule opened reaches both forms of the kernel; against the route
    switched off: same arg-max for logits and heat map, logits within 1e-5 of their scale."""
    from ccvpe_amd import ops, _lib
    lib = _lib.load()
    sd = synth.synthetic_state_dict("vigor", 0)
    net = models.CVM_VIGOR_ori_prior("cuda", 0, True)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    grd, sat = synth.synthetic_pair(2, "vigor", 5)
    grd, sat = grd.cuda(), sat.cuda()
    calls = []
    real_n, real_m = ops.conv3x3_wino_n, ops._conv3x3_match1_f32

    def spy_n(*a, **k):
        calls.append(("conv", a[3]))
        return real_n(*a, **k)

    def spy_m(*a, **k):
        if not a[-1]:                          # (not query_only)
            calls.append(("match", a[3]))
        return real_m(*a, **k)
    monkeypatch.setattr(ops, "conv3x3_wino_n", spy_n)
    monkeypatch.setattr(ops, "_conv3x3_match1_f32", spy_m)
    prev = lib.ccvpe_set_wino_n(0)
    try:
        with torch.no_grad():
            out_off = [t.clone() for t in net(grd, sat)[:2]]
        assert not calls, calls
        lib.ccvpe_set_wino_n(1)
        monkeypatch.setattr(models, "WINO_N_MIN_OK", 1)
        with torch.no_grad():
            out_on = [t.clone() for t in net(grd, sat)[:2]]
    finally:
        lib.ccvpe_set_wino_n(prev)
    assert ("match", 80) in calls and ("match", 40) in calls, calls
    assert ("conv", 64) in calls and ("conv", 32) in calls, calls
    l_on, l_off = out_on[0], out_off[0]
    assert (l_on - l_off).abs().max().item() <= 1e-5 * l_off.abs().max().item()
    assert torch.equal(l_on.argmax(1), l_off.argmax(1))
    assert torch.equal(out_on[1].reshape(2, -1).argmax(1), out_off[1].reshape(2, -1).argmax(1))
