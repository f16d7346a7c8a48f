"""Three-plane bf16 form of the fp32 fused MBConv front kernel (csrc/mbconv_front.hip: mbconv_front_s3_kernel) on the MI355X: each of
its five instantiations alone at small planes with ragged tiles in both directions, circular padding on and off, a launch whose
workgroups loop over several chunks with a ragged last chunk group and one with a single chunk group per tile — against the fp64
composition of the same fp32 inputs (expand, BN0, swish, pad or wrap, depthwise, BN1, swish), with an error budget of 4x the fp32
kernel's; the squeeze partials, sentinels, run-to-run bits, the _ok answers; a whole forward against the fp32-kernel route."""
import os

import pytest
import torch

from ccvpe_amd import models, synth

pytestmark = pytest.mark.gpu

# (k, stride, cin) of mbconv_front_s3_kernel<3,2,1,8> <3,1,2,8> <5,2,2,4> <5,1,3,8> <3,2,3,4>: EfficientNet-B0's blocks 1-5
FORMS = [(3, 2, 16), (3, 1, 24), (5, 2, 24), (5, 1, 40), (3, 2, 40)]
ERROR_TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r23", "error_table.txt")
_rows = []


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from ccvpe_amd import ops as _ops, _lib
    _lib.load()
    yield _ops
    if _rows:                                 # the error table of this run (profiles/r23/error_table.txt)
        try:
            with open(ERROR_TABLE, "w") as f:
                f.write("max|err| / max|ref| against the fp64 composition of the same fp32 inputs (tests/test_mbconv_front_s3_gpu.py)\n")
                f.write("%-44s %10s %10s %10s %10s\n" % ("case", "y s3", "y fp32", "part s3", "part fp32"))
                f.writelines(_rows)
        except OSError:
            pass


def _toh(k, s, cin):                          # output rows per tile (csrc/mbconv_front.hip: mbf_toh); 16 columns
    n = (cin + 15) // 16
    if s == 2:
        return 8 if n == 1 else 4
    return 16 if (n == 1 and k == 3) else 8


def _grouping(k, s, cin, mid, b, ho, wo):
    """(chunks per workgroup, chunk groups per tile) of the launch: the launcher cuts the mid / 16 chunk loop of a tile into groups
    while there are fewer than 2048 tiles."""
    tiles = b * -(-ho // _toh(k, s, cin)) * -(-wo // 16)
    nch = mid // 16
    ng = max(1, min(nch, -(-2048 // tiles)))
    cpg = -(-nch // ng)
    return cpg, -(-nch // cpg)


def _ref64(x, w, s0, b0, wd, s1, b1, k, s, circ):
    """fp64 on the device: expand, BN0, swish, zero pad (circ: wrap the columns), depthwise, BN1, swish; NHWC."""
    b, h, wdt, _ = x.shape
    t = x.double() @ w.double().t()
    t = t * s0.double() + b0.double()
    t = t * torch.sigmoid(t)
    tot = (k - 1) if s == 1 else (k - 2)
    pb = (k - 1) // 2 if s == 1 else (k - 2) // 2
    pa = tot - pb
    ho, wo = (h + tot - k) // s + 1, (wdt + tot - k) // s + 1
    if circ:
        t = torch.cat([t[:, :, wdt - pb:] if pb else t[:, :, :0], t, t[:, :, :pa]], 2)
    else:
        t = torch.nn.functional.pad(t, (0, 0, pb, pa))
    t = torch.nn.functional.pad(t, (0, 0, 0, 0, pb, pa))
    acc = torch.zeros((b, ho, wo, t.shape[3]), dtype=torch.float64, device=x.device)
    for ky in range(k):
        for kx in range(k):
            acc += t[:, ky:ky + (ho - 1) * s + 1:s, kx:kx + (wo - 1) * s + 1:s] * wd[ky, kx].double()
    u = acc * s1.double() + b1.double()
    return u * torch.sigmoid(u)


def _case(ops, k, s, cin, b, h, w, circ, mid=None, seed=0, name=None, device_x=False):
    """One layer through mbconv_front_s3 and mbconv_front against fp64; returns (y, part, again) of the three-plane kernel, again()
    launching it once more on the same inputs.  device_x: a large x is drawn on the device."""
    mid = 6 * cin if mid is None else mid
    if device_x:
        x = torch.randn((b, h, w, cin), device="cuda", generator=torch.Generator("cuda").manual_seed(800 + seed))
    else:
        x = synth.normal((b, h, w, cin), 800 + seed).cuda()
    wt = synth.normal((mid, cin), 801 + seed, (2.0 / cin) ** 0.5).cuda()
    s0, b0 = synth.uniform((mid,), 802 + seed, 0.5, 1.5).cuda(), synth.normal((mid,), 803 + seed, 0.2).cuda()
    wd = synth.normal((k, k, mid), 804 + seed, 1.0 / k).cuda()
    s1, b1 = synth.uniform((mid,), 805 + seed, 0.5, 1.5).cuda(), synth.normal((mid,), 806 + seed, 0.2).cuda()
    ref = _ref64(x, wt, s0, b0, wd, s1, b1, k, s, circ)
    we = models._pad2(wt)
    w3 = models._pack_pw_s3(we)
    assert ops.mbconv_front_s3_ok(x, w3, mid, k, s) >= 1
    nblk = ops.mbconv_front_supported(h, w, cin, mid, k, s)
    ho, wo = ref.shape[1], ref.shape[2]
    assert nblk == -(-ho // _toh(k, s, cin)) * -(-wo // 16)
    # sentinels behind both outputs: the allocator hands the kernel a view of a larger buffer
    ny, npart = b * ho * wo * mid, b * nblk * mid
    real_empty = ops._empty
    bufs = []

    def guarded(shape, device=None, dtype=torch.float32):
        n = 1
        for d in shape:
            n *= d
        buf = torch.full((n + 256,), 7.0, device=device, dtype=dtype)
        bufs.append((buf, n))
        return buf[:n].view(shape)
    ops._empty = guarded
    try:
        got, part = ops.mbconv_front_s3(x, w3, s0, b0, wd, s1, b1, mid, k, s, circ)
    finally:
        ops._empty = real_empty
    f32, part32 = ops.mbconv_front(x, we, s0, b0, wd, s1, b1, mid, k, s, circ)
    torch.cuda.synchronize()
    assert sorted(n for _, n in bufs) == sorted((ny, npart))
    for buf, n in bufs:
        assert torch.all(buf[n:] == 7.0), "wrote beyond the output"
    assert tuple(got.shape) == (b, ho, wo, mid) and tuple(part.shape) == (b, nblk, mid) == tuple(part32.shape)
    ref_max = ref.abs().max().item()
    e_s3 = (got.double() - ref).abs().max().item() / ref_max
    e_f32 = (f32.double() - ref).abs().max().item() / ref_max
    # squeeze partials: per (tile, channel) sums of the outputs of the tile; compared as sums over the sample's tiles
    # against the fp64 sums, and row by row against the fp64 sum of each tile
    toh = _toh(k, s, cin)
    pref = torch.zeros((b, nblk, mid), dtype=torch.float64, device="cuda")
    tx = -(-wo // 16)
    for ty in range(-(-ho // toh)):
        for txi in range(tx):
            pref[:, ty * tx + txi] = ref[:, ty * toh:(ty + 1) * toh, txi * 16:(txi + 1) * 16].sum(dim=(1, 2))
    p_max = pref.abs().max().item()
    p_s3 = (part.double() - pref).abs().max().item() / p_max
    p_f32 = (part32.double() - pref).abs().max().item() / p_max
    label = name or "k%d s%d cin %d mid %d B%d %dx%d %s" % (k, s, cin, mid, b, h, w, "wrap" if circ else "zero")
    print("mbconv_front_s3 err %s: y s3 %.2e fp32 %.2e | partials s3 %.2e fp32 %.2e" % (label, e_s3, e_f32, p_s3, p_f32))
    _rows.append("%-44s %10.2e %10.2e %10.2e %10.2e\n" % (label, e_s3, e_f32, p_s3, p_f32))
    assert e_s3 <= 4 * max(e_f32, 1e-7), "three-plane error %.3e vs fp32 kernel %.3e" % (e_s3, e_f32)
    assert e_s3 < 1e-5
    assert p_s3 <= 4 * max(p_f32, 1e-7), "three-plane squeeze-partial error %.3e vs fp32 kernel %.3e" % (p_s3, p_f32)
    assert p_s3 < 1e-5
    return got, part, lambda: ops.mbconv_front_s3(x, w3, s0, b0, wd, s1, b1, mid, k, s, circ)


@pytest.mark.parametrize("circ", [False, True])
@pytest.mark.parametrize("k,s,cin", FORMS)
def test_each_form_alone_with_ragged_tiles(ops, k, s, cin, circ):
    """B = 2; 20 x 36 (stride 1) / 22 x 38 -> 11 x 19 (stride 2): the last tile row and the last tile column are ragged, the halo
    crosses every image border.  So few tiles that every workgroup owns one chunk."""
    h, w = (20, 36) if s == 1 else (22, 38)
    tot = (k - 1) if s == 1 else (k - 2)
    ho, wo = (h + tot - k) // s + 1, (w + tot - k) // s + 1
    assert ho % _toh(k, s, cin) and wo % 16
    assert _grouping(k, s, cin, 6 * cin, 2, ho, wo)[0] == 1
    _case(ops, k, s, cin, 2, h, w, circ, seed=10 * cin + k + s)


def test_workgroups_loop_over_two_chunks_with_a_ragged_last_group(ops):
    """Block 5's form at 2 x 124 x 250: 16 x 8 tiles per sample (both ragged) = 256 tiles, so the 15 chunks are cut into 8 groups of
    2, the last with one chunk: the W double buffer in LDS is re-filled inside the loop and the loop ends early in the last group."""
    k, s, cin = 3, 2, 40
    assert _grouping(k, s, cin, 240, 2, 62, 125) == (2, 8) and 15 % 2
    _case(ops, k, s, cin, 2, 124, 250, True, seed=77)


def test_single_chunk_group_per_tile_and_two_runs_bit_identical(ops):
    """Block 1's form with mid = 48 at 8 x 250 x 500: 16 x 16 tiles per sample = 2048 tiles, one workgroup per tile walks all three
    chunks (odd: both LDS buffers of W are re-used).  Run twice: identical bits."""
    k, s, cin, mid = 3, 2, 16, 48
    assert _grouping(k, s, cin, mid, 8, 125, 250) == (3, 1)
    y0, p0, again = _case(ops, k, s, cin, 8, 250, 500, False, mid=mid, seed=91, device_x=True)
    y1, p1 = again()
    assert y1.data_ptr() != y0.data_ptr()
    assert torch.equal(y0, y1) and torch.equal(p0, p1), "two runs differ"


def test_ok_answers(ops):
    from ccvpe_amd import _lib
    lib = _lib.load()
    w3 = lambda cin, mid: torch.empty(((cin + 15) // 16, mid, 48), device="cuda", dtype=torch.bfloat16)
    x = lambda b, h, w, cin: torch.empty((b, h, w, cin), device="cuda")
    for k, s, cin in FORMS:
        assert ops.mbconv_front_s3_ok(x(2, 20, 36, cin), w3(cin, 6 * cin), 6 * cin, k, s) >= 1
        assert ops.mbconv_front_s3_ok(x(2, 20, 36, cin).to(torch.bfloat16), w3(cin, 6 * cin), 6 * cin, k, s) == 0      # bf16 storage
        assert ops.mbconv_front_s3_ok(x(2, 20, 36, cin), w3(cin, 6 * cin).float(), 6 * cin, k, s) == 0                  # not a bf16 pack
        assert ops.mbconv_front_s3_ok(x(2, 20, 36, cin), w3(cin + 16, 6 * cin), 6 * cin, k, s) == 0                     # a block too many
        assert ops.mbconv_front_s3_ok(x(2, 20, 36, cin), None, 6 * cin, k, s) == 0
    for cin in (80, 112, 192):                                                   # late blocks: mbconv_plane_kernel's
        for k, s in ((3, 1), (5, 1), (5, 2)):
            assert lib.ccvpe_mbconv_front_s3_ok(32, 32, cin, 6 * cin, k, s, 64) == 0
    assert lib.ccvpe_mbconv_front_s3_ok(64, 64, 40, 240, 5, 2, 64) == 0           # k = 5, s = 2, Cin > 32
    assert lib.ccvpe_mbconv_front_s3_ok(64, 64, 48, 288, 5, 2, 64) == 0
    # the measured size rule at B = 64 (ground, aerial planes of blocks 1-5), pinned: profiles/r23/mbf_s3_probe.txt
    planes = [((160, 320), (256, 256)), ((80, 160), (128, 128)), ((80, 160), (128, 128)), ((40, 80), (64, 64)), ((40, 80), (64, 64))]
    got = [tuple(lib.ccvpe_mbconv_front_s3_ok(h, w, cin, 6 * cin, k, s, 64) for h, w in pl) for (k, s, cin), pl in zip(FORMS, planes)]
    assert got == B64_OK, got
    with pytest.raises(_lib.CcvpeError, match="three-plane pack"):              # the fp32 pack's kpad: refused, nothing is launched
        xx = torch.zeros((1, 20, 36, 24), device="cuda")
        v = torch.zeros((144,), device="cuda")
        y, part = torch.zeros((1, 20, 36, 144), device="cuda"), torch.zeros((1, 9, 144), device="cuda")
        _lib.check(lib.ccvpe_mbconv_front_s3_f32(xx.data_ptr(), w3(24, 144).data_ptr(), 32, v.data_ptr(), v.data_ptr(),
                                                 torch.zeros((3, 3, 144), device="cuda").data_ptr(), v.data_ptr(), v.data_ptr(),
                                                 y.data_ptr(), part.data_ptr(), 1, 20, 36, 24, 144, 3, 1, 0, None), "ccvpe_mbconv_front_s3_f32")


# ccvpe_mbconv_front_s3_ok at B = 64 per block 1-5: (ground, aerial)
B64_OK = [(1, 1), (2, 2), (2, 2), (2, 2), (2, 2)]


def test_forward_matches_the_fp32_kernel_route(monkeypatch):
    """A B = 2 fp32 forward with the size rule opened runs blocks 1-5 of both encoders through the three-plane kernel: logits, raw
    orientation and heat map within 1e-5 of scale of the CCVPE_SPLIT3_MB=0 route (r21 saw order 1e-6 for the projections), same
    arg-max."""
    from ccvpe_amd import ops
    sd = synth.synthetic_state_dict("vigor", 0)
    net = models.CVM_VIGOR_ori_prior("cuda", 0, True)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    grd, sat = synth.synthetic_pair(2, "vigor", 5)
    grd, sat = grd.cuda(), sat.cuda()
    monkeypatch.setattr(models, "SPLIT3", True)
    monkeypatch.setattr(models, "SPLIT3_MB", True)
    monkeypatch.setattr(models, "SPLIT3_MB_MIN_OK", 1)
    net.ori_raw_output = True            # conv1_ori's output before F.normalize: a linear chain like the logits, comparable by scale

    def run():
        rec = ops.LaunchRecorder()
        ops.set_recorder(rec)
        try:
            with torch.no_grad():
                out = [t.clone() for t in net(grd, sat)[:3]]
        finally:
            ops.set_recorder(None)
        return out, [it[0] for it in rec.items if it[0].startswith("mbconv_front")]
    out_s, names = run()
    assert sorted(n for n in names if n.startswith("mbconv_front_s3_kernel<")) == sorted(
        2 * ["mbconv_front_s3_kernel<%d,%d>" % (k, s) for k, s, _ in FORMS]), names
    assert not [n for n in names if n.startswith("mbconv_front_kernel<")]
    monkeypatch.setattr(models, "SPLIT3_MB", False)
    out_f, names = run()
    assert not [n for n in names if n.startswith("mbconv_front_s3_kernel<")] and len([n for n in names if n.startswith("mbconv_front_kernel<")]) == 10
    ls, lf = out_s[0], out_f[0]
    e_log = (ls - lf).abs().max().item() / lf.abs().max().item()
    e_ori = (out_s[2] - out_f[2]).abs().max().item() / out_f[2].abs().max().item()
    e_heat = (out_s[1] - out_f[1]).abs().max().item() / out_f[1].abs().max().item()
    print("forward mbconv_front_s3 vs fp32 front kernel route: logits %.2e  raw orientation %.2e  heat map %.2e" % (e_log, e_ori, e_heat))
    assert e_log <= 1e-5
    assert torch.equal(ls.argmax(1), lf.argmax(1))
    assert torch.equal(out_s[1].reshape(2, -1).argmax(1), out_f[1].reshape(2, -1).argmax(1))
    assert e_ori <= 1e-5
    assert e_heat <= 1e-5
