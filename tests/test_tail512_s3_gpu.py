"""Three-plane bf16 stage 1 of the fused 512 x 512 decoder tail (csrc/tail512.hip, ccvpe_tail_desc.split == 2) on the MI355X:
against the float64 composition on the budget of 4x the exact fp32 kernel's error on the same inputs; the heat-map softmax from
the partials of the same launch; the persistent tile walk at more than 4096 tiles; determinism and refusals; a whole fp32
forward with and without the route."""
import pytest
import torch
import torch.nn.functional as F

from ccvpe_amd import models, synth

pytestmark = pytest.mark.gpu

# (cp, cref, cout, h1, w1, b)
CASES = [(48, 41, 1, 32, 48, 3),
         (40, 33, 1, 32, 16, 3),        # the third chunk is half empty
         (32, 32, 2, 16, 32, 3),
         (48, 41, 1, 16, 16, 1)]        # one tile column


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from ccvpe_amd import ops as _ops, _lib
    _lib.load()
    return _ops


def _weights(cp, cref, cout):
    """-> host fp32 (wd, bd, w3, b3, w2, b2) and the device operands (fw, fshift, w2p, b2) of ops.tail512"""
    wd = synth.normal((cref, 16, 2, 2), 902, (1.0 / cref) ** 0.5)
    bd = synth.normal((16,), 903, 0.3)
    w3 = synth.normal((16, 16, 3, 3), 904, (1.0 / (9 * 16)) ** 0.5)
    b3 = synth.normal((16,), 905, 0.1)
    w2 = synth.normal((cout, 16, 3, 3), 906, (1.0 / (9 * 16)) ** 0.5)
    b2 = synth.normal((cout,), 907, 0.1)
    fw, fshift = models._pack_upconv(wd.cuda(), bd.cuda(), [(0, 0, cref)], cp, w3.cuda(), b3.cuda(), torch.float32)
    return (wd, bd, w3, b3, w2, b2), (fw, fshift, w2.permute(0, 2, 3, 1).contiguous().cuda(), b2.cuda())


def _ref64(x_nchw, cref, host):
    """deconv (k2 s2) -> conv3x3 + ReLU -> conv3x3 (16 -> cout), un-normalised, in float64 on the host"""
    wd, bd, w3, b3, w2, b2 = [t.double() for t in host]
    mid = F.relu(F.conv2d(F.conv_transpose2d(x_nchw[:, :cref].double().cpu(), wd, bd, stride=2), w3, b3, padding=1))
    return F.conv2d(mid, w2, b2, padding=1)


def _budget(err3, err0, what):
    """The project's budget for an exact-product split (Winograd, upconv_s3): <= 4 x max(exact fp32 kernel's error, 1e-7), < 1e-5"""
    print("%s: three-plane %.3e  exact fp32 %.3e  (of max |ref|)" % (what, err3, err0))
    assert err3 <= 4 * max(err0, 1e-7), "%s: three-plane %.3e vs exact fp32 %.3e" % (what, err3, err0)
    assert err3 < 1e-5, "%s: three-plane %.3e" % (what, err3)


_CACHE = {}


def _case(ops, cp, cref, cout, h1, w1, b):
    """One shape, computed once for the tests that share it: (x, device operands, ref64, split=2 raw output, exact raw output)"""
    key = (cp, cref, cout, h1, w1, b)
    if key not in _CACHE:
        x = synth.normal((b, cp, h1, w1), 900 + cp)
        x[:, cref:] = 0
        host, dev = _weights(cp, cref, cout)
        xd = x.permute(0, 2, 3, 1).contiguous().cuda()
        want = _ref64(x, cref, host)
        got3 = ops.tail512(xd, cp, *dev, cout, False, batch=b, h1=h1, w1=w1, split=2)
        got0 = ops.tail512(xd, cp, *dev, cout, False, batch=b, h1=h1, w1=w1, split=0)
        _CACHE[key] = (xd, dev, want, got3, got0)
    return _CACHE[key]


@pytest.mark.parametrize("cp,cref,cout,h1,w1,b", CASES)
def test_three_plane_tail_against_float64(ops, cp, cref, cout, h1, w1, b):
    """split = 2 and the exact kernel (split = 0), both un-normalised, against the float64 composition: image borders, tile
    aprons, the ragged last MFMA tile, a half-empty chunk; cout = 2 additionally normalised, masked where the raw norm is small."""
    xd, dev, want, got3, got0 = _case(ops, cp, cref, cout, h1, w1, b)
    assert tuple(got3.shape) == (b, cout, 2 * h1, 2 * w1) and got3.dtype == torch.float32
    scale = want.abs().max().item()
    err3 = (got3.cpu().double() - want).abs().max().item() / scale
    err0 = (got0.cpu().double() - want).abs().max().item() / scale
    _budget(err3, err0, "tail512 cp=%d cout=%d %dx%d" % (cp, cout, h1, w1))
    if cout == 2:
        got_n = ops.tail512(xd, cp, *dev, 2, True, batch=b, h1=h1, w1=w1, split=2)
        want_n = F.normalize(want, p=2, dim=1)
        ok = (want.pow(2).sum(1, keepdim=True).sqrt() > 1e-2).expand_as(want_n)
        err = ((got_n.cpu().double() - want_n).abs() * ok).max().item()
        assert err <= 1e-4, "tail512 ori, normalised: %.3e" % err
        assert float((got_n.pow(2).sum(1).sqrt() - 1).abs().max()) < 1e-5


@pytest.mark.parametrize("cp,cref,cout,h1,w1,b", [c for c in CASES if c[2] == 1][:2])
def test_heat_map_softmax_from_the_partials(ops, cp, cref, cout, h1, w1, b):
    """The (max, sum exp) partials of a split = 2 launch give the heat-map softmax of its logits; asking for them does not
    change the logits."""
    xd, dev, _, got3, _ = _case(ops, cp, cref, cout, h1, w1, b)
    lg, smx = ops.tail512(xd, cp, *dev, 1, False, batch=b, h1=h1, w1=w1, split=2, want_softmax=True)
    assert torch.equal(lg, got3)
    heat = ops.softmax_apply(lg.reshape(b, -1), smx)
    want_h = torch.softmax(lg.reshape(b, -1).double().cpu(), dim=1)
    assert float((heat.cpu().double() - want_h).abs().max() / want_h.max()) < 1e-5
    assert float((heat.sum(1) - 1).abs().max()) < 1e-5


def test_persistent_walk_over_more_than_4096_tiles(ops):
    """cout 1, 48 channels, 128 x 128 low-res, B = 65: 8320 tiles of 8 x 16, three per workgroup at the 4096-workgroup cap, the
    last workgroup ragged.  Samples 0, B / 2 and B - 1 on the float64 budget, the whole output against the exact kernel."""
    cp, cref, h1, w1, b = 48, 41, 128, 128, 65
    assert (h1 // 8) * (w1 // 16) * b > 2 * 4096
    xd = synth.normal((b, h1, w1, cp), 950, device="cuda")
    xd[..., cref:] = 0
    host, dev = _weights(cp, cref, 1)
    got3 = ops.tail512(xd, cp, *dev, 1, False, batch=b, h1=h1, w1=w1, split=2)
    got0 = ops.tail512(xd, cp, *dev, 1, False, batch=b, h1=h1, w1=w1, split=0)
    pick = [0, b // 2, b - 1]
    want = _ref64(xd[pick].permute(0, 3, 1, 2), cref, host)
    scale = want.abs().max().item()
    err3 = (got3[pick].cpu().double() - want).abs().max().item() / scale
    err0 = (got0[pick].cpu().double() - want).abs().max().item() / scale
    _budget(err3, err0, "persistent walk, samples %s" % pick)
    whole = (got3 - got0).abs().max().item() / got0.abs().max().item()
    print("persistent walk, all %d samples vs the exact kernel: %.3e" % (b, whole))
    assert whole <= 1e-5


def test_determinism_and_refusals(ops):
    from ccvpe_amd import _lib
    cp, cref, cout, h1, w1, b = CASES[0]
    xd, dev, _, got3, _ = _case(ops, cp, cref, cout, h1, w1, b)
    again = ops.tail512(xd, cp, *dev, 1, False, batch=b, h1=h1, w1=w1, split=2)
    assert torch.equal(again, got3)
    # what the library does not serve is refused before anything is launched: the output buffer keeps its sentinel
    real_empty = ops._empty
    made = []

    def sentinel_empty(*a, **k):
        t = real_empty(*a, **k)
        t.fill_(-7.0)
        made.append(t)
        return t
    host2, dev2 = _weights(48, 41, 2)
    bad = [dict(x=xd, c0=cp, dev=dev2, cout=2, split=2),                                         # cout 2 with 48 channels
           dict(x=xd.to(torch.bfloat16), c0=cp, dev=(dev[0].to(torch.bfloat16),) + dev[1:], cout=1, split=2),   # bf16 operands
           dict(x=xd, c0=cp, dev=dev, cout=1, split=3)]                                          # no such mode
    ops._empty = sentinel_empty
    try:
        for k in bad:
            del made[:]
            with pytest.raises(_lib.CcvpeError):
                ops.tail512(k["x"], k["c0"], *k["dev"], k["cout"], False, batch=b, h1=h1, w1=w1, split=k["split"])
            torch.cuda.synchronize()
            assert made and all(bool((t == -7.0).all()) for t in made)
    finally:
        ops._empty = real_empty


def test_forward_with_and_without_the_three_plane_tails(monkeypatch):
    """A B = 2 fp32 forward with both tails on three planes against the same forward with exact fp32 tails: logits and the raw
    orientation field within 1e-5 of scale, same arg-max; ops.tail512 saw split == 2 (0) on both tails."""
    from ccvpe_amd import ops
    sd = synth.synthetic_state_dict("vigor", 0)
    net = models.CVM_VIGOR_ori_prior("cuda", 0, True)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    grd, sat = synth.synthetic_pair(2, "vigor", 5)
    grd, sat = grd.cuda(), sat.cuda()
    calls = []
    real = ops.tail512

    def spy(*a, **k):
        calls.append((a[6], k.get("split", False)))      # (cout, split)
        return real(*a, **k)
    monkeypatch.setattr(ops, "tail512", spy)
    monkeypatch.setattr(models, "SPLIT3", True)
    net.ori_raw_output = True            # conv1_ori's output before F.normalize: a linear chain like the logits, comparable by scale
    with torch.no_grad():
        monkeypatch.setattr(models, "SPLIT3_TAIL", True)
        out_s = [t.clone() for t in net(grd, sat)[:3]]
        on = list(calls)
        del calls[:]
        monkeypatch.setattr(models, "SPLIT3_TAIL", False)
        out_e = [t.clone() for t in net(grd, sat)[:3]]
    assert sorted(on) == [(1, 2), (2, 2)] and sorted(calls) == [(1, 0), (2, 0)], (on, calls)
    assert all(type(s) is int for _, s in on + calls)
    ls, le = out_s[0], out_e[0]
    e_log = (ls - le).abs().max().item() / le.abs().max().item()
    e_ori = (out_s[2] - out_e[2]).abs().max().item() / out_e[2].abs().max().item()
    print("forward, three-plane tails vs exact fp32 tails: logits %.2e  raw orientation %.2e" % (e_log, e_ori))
    assert e_log <= 1e-5
    assert torch.equal(ls.argmax(1), le.argmax(1))
    assert e_ori <= 1e-5


def test_planned_forward_runs_the_three_plane_tails(monkeypatch):
    """The tail descriptor is recorded whole (ccvpe_amd/plan.py): a planned B = 2 fp32 forward gives the bits of the eager forward
    with the route on — and those are not the bits of the exact fp32 tails, so the plan replays the three-plane instantiation."""
    from ccvpe_amd import plan
    net = models.CVM_VIGOR_ori_prior("cuda", 0, True)
    net.load_state_dict(synth.synthetic_state_dict("vigor", 0), strict=True)
    net = net.cuda().eval()
    grd, sat = synth.synthetic_pair(2, "vigor", 31)
    grd, sat = grd.cuda(), sat.cuda()
    monkeypatch.setattr(models, "SPLIT3", True)
    monkeypatch.setattr(models, "SPLIT3_TAIL", True)
    with torch.no_grad():
        eager = [t.clone() for t in net(grd, sat)]
        pf = plan.PlannedForward(net, grd, sat)
        got = [t.clone() for t in pf(grd, sat)]
        torch.cuda.synchronize()
        monkeypatch.setattr(models, "SPLIT3_TAIL", False)
        exact = [t.clone() for t in net(grd, sat)]
    assert all(torch.equal(a, b) for a, b in zip(got, eager))
    assert not torch.equal(eager[0], exact[0])
