"""Python-side operator layer: torch tensors in, C-ABI calls out (include/ccvpe_hip.h).

Each function enqueues exactly one library call on torch's current HIP stream.  torch is used
for device memory and streams only; every arithmetic step runs in libccvpe_hip.so.  No
function here has a CPU or eager fallback.
"""
import ctypes

import torch

from . import _lib
from ._lib import ConvDesc, check

ACT_NONE, ACT_RELU, ACT_SWISH, ACT_RELU_MASK = 0, 1, 2, 3
SPLIT_K_CALLS = 0        # number of conv_igemm calls that took the split-K path (tests / diagnostics)
SPLIT_K = __import__("os").environ.get("CCVPE_SPLIT_K", "1") == "1"      # split-K for small-batch GEMMs (0 disables)
OUT_NHWC, OUT_DECONV2X = 0, 1

# Optional launch recorder (bench.py): when set, every library call is bracketed by HIP events on
# the launching stream and reported as (kernel family, tag, algorithmic flops, algorithmic bytes).
_recorder = None


def set_recorder(rec):
    global _recorder
    _recorder = rec


class LaunchRecorder(object):
    """Collects (name, tag, flops, bytes, start_event, end_event) per library call."""

    def __init__(self):
        self.items = []

    def begin(self):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(torch.cuda.current_stream())
        return ev

    def end(self, name, tag, flops, nbytes, ev0):
        ev1 = torch.cuda.Event(enable_timing=True)
        ev1.record(torch.cuda.current_stream())
        self.items.append((name, tag, flops, nbytes, ev0, ev1))

    def summary(self):
        """name -> dict(calls, ms, flops, bytes); call after torch.cuda.synchronize()."""
        out = {}
        for name, tag, flops, nbytes, e0, e1 in self.items:
            d = out.setdefault(name, dict(calls=0, ms=0.0, flops=0.0, bytes=0.0))
            d["calls"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += flops
            d["bytes"] += nbytes
        return out


def igemm_tile(n, is3x3=False):
    """Mirror of pick_cfg() in csrc/conv_igemm.hip: (BM, BN) chosen for a GEMM N (reporting only: the split-K launch's name)."""
    npad = (n + 15) // 16 * 16
    cfgs = [(4, 5, 2), (4, 4, 2), (4, 3, 2), (4, 2, 2), (4, 1, 2), (4, 5, 1), (4, 3, 1), (4, 1, 1), (2, 7, 1)]
    best, best_cost = None, None
    for mt, nt, wn in cfgs:
        bn = 16 * nt * wn
        tiles = (npad + bn - 1) // bn
        cost = tiles * bn * 1000 + (1000 - bn)
        if best_cost is None or cost < best_cost:
            best, best_cost = (mt, nt, wn), cost
    mt, nt, wn = best
    return "%s<%d,%d,%d>" % ("conv3x3_f32_kernel" if is3x3 else "igemm_f32_kernel", mt, nt, wn)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


ROUTE_FAMILIES = {0: "igemm", 1: "pw_gemm", 2: "conv3x3", 3: "c3n", 4: "pw_ring", 5: "pwn"}


def conv_route(desc, is_bf16, out_f32=False):
    """(family, MT, NT, WN) of the kernel ccvpe_conv_igemm_f32 / _bf16 runs for `desc` (ccvpe_conv_igemm_route: the
    library's own dispatch, nothing is launched)."""
    r = _lib.load().ccvpe_conv_igemm_route(ctypes.byref(desc), int(bool(is_bf16)), int(bool(out_f32)))
    if r < 0:
        check(int(r), "ccvpe_conv_igemm_route")
    return ROUTE_FAMILIES[r & 0xff], (r >> 8) & 0xf, (r >> 12) & 0xf, (r >> 16) & 0xf


def conv3x3_variant(desc, is_bf16):
    """(NW, DMA, TPS) — waves per workgroup, W tile by LDS-DMA, taps per K stage — of the conv3x3_kernel instantiation that serves
    `desc` (ccvpe_conv3x3_variant: the launcher's own decision), or None when the call does not route to conv3x3_kernel."""
    r = _lib.load().ccvpe_conv3x3_variant(ctypes.byref(desc), int(bool(is_bf16)))
    if r < 0:
        check(int(r), "ccvpe_conv3x3_variant")
    return (r & 0xf, bool((r >> 4) & 1), (r >> 8) & 0xf) if r else None


UPROUTE_KERNELS = {0: "upconv_kernel", 1: "upconv_halo_kernel", 2: "upconv_dma_kernel", 3: "upconv_dma_kernel", 4: "up2_kernel"}


def upconv_route(desc, is_bf16):
    """(kernel, MT, NT, WN, pair) ccvpe_upconv3x3_f32 / _bf16 runs for `desc` (nothing is launched)."""
    r = _lib.load().ccvpe_upconv3x3_route(ctypes.byref(desc), int(bool(is_bf16)))
    if r < 0:
        check(int(r), "ccvpe_upconv3x3_route")
    return UPROUTE_KERNELS[r & 0xff], (r >> 8) & 0xf, (r >> 12) & 0xf, (r >> 16) & 0xf, (r & 0xff) == 3


def upconv_route_name(desc, is_bf16):
    """Kernel name as rocprofv3 prints it (minus namespace): the key of profiles/pmc_traffic.json."""
    k, mt, nt, wn, pair = upconv_route(desc, is_bf16)
    ty = "bf16" if is_bf16 else "f32"
    if k == "up2_kernel":
        return "up2_kernel<bf16,%d,%d>" % (desc.c0, desc.n)
    return "%s<%s,%d,%d,%d%s>" % (k, ty, mt, nt, wn, ",pair" if pair else "")


def upconv_s3_route_name(desc, form=0):
    """The same for ccvpe_upconv3x3_s3_form_f32(desc, form): ccvpe_upconv3x3_s3_route, the library's own decision, no launch."""
    r = _lib.load().ccvpe_upconv3x3_s3_route(ctypes.byref(desc), form)
    if r <= 0:
        raise _lib.CcvpeError("ccvpe_upconv3x3_s3_route: form %d does not compute this layer" % form)
    mt, nt, wn = (r >> 8) & 0xf, (r >> 12) & 0xf, (r >> 16) & 0xf
    return "upconv_s3q_kernel<%d,%d>" % (mt, nt) if r & 0xf == 2 else "upconv_s3_kernel<%d,%d,%d%s>" % (mt, nt, wn, ",pair" if r & 16 else "")


def conv_route_name(desc, is_bf16, out_f32=False):
    """Kernel family name of the launch the library would make for this descriptor, as the launch recorder and
    profiles/pmc_traffic.json spell it: `<family>_f32_kernel<MT,NT,WN>` in fp32, `<family>_kernel<bf16,MT,NT,WN>` in bf16
    (the narrow 3x3 kernel c3n exists in bf16 only and is named by its column count)."""
    fam, mt, nt, wn = conv_route(desc, is_bf16, out_f32)
    if fam == "c3n":
        return "c3n_kernel<bf16,%d>" % desc.n
    if is_bf16:
        return "%s_kernel<bf16,%d,%d,%d>" % (fam, mt, nt, wn)
    return "%s_f32_kernel<%d,%d,%d>" % (fam, mt, nt, wn)


# Plan recording (ccvpe_amd/plan.py): while a forward is being recorded every tensor this layer allocates comes from the
# recorder's workspace and every tensor whose pointer goes to the library is remembered (weights are collected from those).
_record = None


def _empty(shape, device=None, dtype=torch.float32):
    if _record is not None:
        return _record.empty(shape, dtype, device)
    return torch.empty(shape, device=device, dtype=dtype)


def _ptr(t):
    if t is None:
        return None
    if _record is not None:
        _record.note(t)
    return ctypes.c_void_p(t.data_ptr())


def _chk(t, name, dtype=torch.float32):
    if t is None:
        return
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise ValueError("%s must be a contiguous %s device tensor (got %s %s contiguous=%s)" % (
            name, dtype, t.device, t.dtype, t.is_contiguous()))


def _act_dtype(t):
    """Activation storage type of a call: fp32 or bf16 (selects the _f32 / _bf16 entry point)."""
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("activations must be fp32 or bf16, got %s" % t.dtype)
    return t.dtype


def conv_igemm(src0, c0, w_packed, n, *, batch, in_h, in_w, kh=1, kw=1, stride=1, pad=0,
               src1=None, c1=0, gate=None, scale=None, shift=None, residual=None, act=ACT_NONE,
               out_mode=OUT_NHWC, dst=None, ldd=None, ld0=None, ld1=None, algo_k=None, out_f32=False, route_only=False,
               variant_only=False):
    """Implicit-GEMM conv / deconv / linear (ccvpe_conv_igemm_f32 / _bf16 by src0.dtype).
    src tensors are NHWC.  out_f32 (bf16 only): write an fp32 result."""
    lib = _lib.load()
    dt = _act_dtype(src0)
    odt = torch.float32 if (out_f32 or dt == torch.float32) else dt
    for t, nm in ((src0, "src0"), (src1, "src1"), (w_packed, "w"), (residual, "residual")):
        _chk(t, nm, dt)
    for t, nm in ((gate, "gate"), (scale, "scale"), (shift, "shift")):
        _chk(t, nm)
    _chk(dst, "dst", odt)
    ld0 = ld0 if ld0 is not None else src0.shape[-1]
    ld1 = ld1 if ld1 is not None else (src1.shape[-1] if src1 is not None else 0)
    ho = (in_h + 2 * pad - kh) // stride + 1
    wo = (in_w + 2 * pad - kw) // stride + 1
    if out_mode == OUT_DECONV2X:
        cout = n // 4
        oshape = (batch, 2 * ho, 2 * wo)
    else:
        cout = n
        oshape = (batch, ho, wo)
    if dst is None:
        ldd = ldd if ldd is not None else cout
        dst = _empty(oshape + (ldd,), device=src0.device, dtype=odt)
    elif ldd is None:
        ldd = dst.shape[-1]
    d = ConvDesc()
    d.src0, d.src1, d.gate, d.w = _ptr(src0), _ptr(src1), _ptr(gate), _ptr(w_packed)
    d.scale, d.shift, d.residual, d.dst = _ptr(scale), _ptr(shift), _ptr(residual), _ptr(dst)
    d.c0, d.ld0, d.c1, d.ld1 = c0, ld0, c1, ld1
    d.batch, d.in_h, d.in_w = batch, in_h, in_w
    d.kh, d.kw, d.stride, d.pad = kh, kw, stride, pad
    d.n, d.kpad = n, w_packed.shape[1]
    d.ldd = ldd
    d.ldres = residual.shape[-1] if residual is not None else 0
    d.act, d.out_mode = act, out_mode
    if route_only:        # (family, MT, NT, WN) the one-pass entry point would run for this call; nothing is launched
        return conv_route(d, dt != torch.float32, bool(out_f32))
    if variant_only:      # (NW, DMA, TPS) of conv3x3_kernel for this call, None when another kernel serves it; nothing is launched
        return conv3x3_variant(d, dt != torch.float32)
    rec = _recorder
    ev0 = rec.begin() if rec is not None else None
    want = lib.ccvpe_conv_igemm_splitk_floats(ctypes.byref(d), int(dt != torch.float32)) if SPLIT_K else 0
    if want < 0:
        check(int(want), "ccvpe_conv_igemm_splitk_floats")
    if want > 0:          # small-batch GEMM: K cut into slices + deterministic second pass (csrc/conv_igemm.hip)
        global SPLIT_K_CALLS
        SPLIT_K_CALLS += 1
        scratch = _empty((want,), device=src0.device, dtype=torch.float32)
        if dt == torch.float32:
            check(lib.ccvpe_conv_igemm_splitk_f32(ctypes.byref(d), _ptr(scratch), _stream()), "ccvpe_conv_igemm_splitk_f32")
        else:
            check(lib.ccvpe_conv_igemm_splitk_bf16(ctypes.byref(d), int(bool(out_f32)), _ptr(scratch), _stream()),
                  "ccvpe_conv_igemm_splitk_bf16")
    elif dt == torch.float32:
        check(lib.ccvpe_conv_igemm_f32(ctypes.byref(d), _stream()), "ccvpe_conv_igemm_f32")
    else:
        check(lib.ccvpe_conv_igemm_bf16(ctypes.byref(d), int(bool(out_f32)), _stream()), "ccvpe_conv_igemm_bf16")
    if rec is not None:
        m = batch * ho * wo
        k_alg = algo_k if algo_k is not None else kh * kw * (c0 + c1)
        flops = 2.0 * m * n * k_alg
        # algorithmic bytes: input read once, output written once, weights once
        esz = 4.0 if dt == torch.float32 else 2.0
        nbytes = esz * (batch * in_h * in_w * (c0 + c1) + m * n + n * k_alg
                        + (m * n if residual is not None else 0))
        if want > 0:      # split-K: always the generic gather kernel with the tile pick_cfg() chose
            name = igemm_tile(n, False)
        else:             # ask the library which kernel it ran (no Python mirror of the dispatch rules)
            name = conv_route_name(d, dt != torch.float32, bool(out_f32))
        if want > 0 and dt != torch.float32:
            name = name.replace("_f32_kernel<", "_kernel<bf16,")
        rec.end(name, "%dx%d s%d M%d N%d K%d" % (kh, kw, stride, m, n, k_alg), flops, nbytes, ev0)
    return dst


def _wino_desc(src0, c0, u_packed, n, batch, in_h, in_w, shift, dst, ldd, ld0):
    d = ConvDesc()
    d.src0, d.src1, d.gate, d.w = _ptr(src0), None, None, _ptr(u_packed)
    d.scale, d.shift, d.residual, d.dst = None, _ptr(shift), None, _ptr(dst) if dst is not None else None
    d.c0, d.ld0, d.c1, d.ld1 = c0, ld0, 0, 0
    d.batch, d.in_h, d.in_w = batch, in_h, in_w
    d.kh, d.kw, d.stride, d.pad = 3, 3, 1, 1
    d.n, d.kpad = n, u_packed.shape[1]
    d.ldd, d.ldres = ldd, 0
    d.act, d.out_mode = ACT_NONE, OUT_NHWC
    return d


def conv3x3_wino_ok(src0, c0, u_packed, n, *, batch, in_h, in_w, ldd=None, ld0=None):
    """True if ccvpe_conv3x3_wino_f32 serves this layer (fp32 storage and the library's own shape rules)."""
    if src0.dtype != torch.float32 or u_packed is None:
        return False
    ld0 = ld0 if ld0 is not None else src0.shape[-1]
    d = _wino_desc(src0, c0, u_packed, n, batch, in_h, in_w, None, None, ldd if ldd is not None else n, ld0)
    return bool(_lib.load().ccvpe_conv3x3_wino_ok(ctypes.byref(d)))


def conv3x3_wino(src0, c0, u_packed, n, *, batch, in_h, in_w, shift=None, dst=None, ldd=None, ld0=None):
    """fp32 3x3 / stride 1 / pad 1 conv with bias by Winograd F(2x2,3x3) (ccvpe_conv3x3_wino_f32); u_packed from
    models._pack_wino.  Same result as conv_igemm(..., kh=3, kw=3, pad=1, shift=shift) to fp32 rounding, not bit for bit."""
    lib = _lib.load()
    for t, nm in ((src0, "src0"), (u_packed, "w"), (shift, "shift"), (dst, "dst")):
        _chk(t, nm)
    ld0 = ld0 if ld0 is not None else src0.shape[-1]
    if dst is None:
        ldd = ldd if ldd is not None else n
        dst = _empty((batch, in_h, in_w, ldd), device=src0.device)
    elif ldd is None:
        ldd = dst.shape[-1]
    d = _wino_desc(src0, c0, u_packed, n, batch, in_h, in_w, shift, dst, ldd, ld0)
    rec = _recorder
    ev0 = rec.begin() if rec is not None else None
    check(lib.ccvpe_conv3x3_wino_f32(ctypes.byref(d), _stream()), "ccvpe_conv3x3_wino_f32")
    if rec is not None:
        m = batch * in_h * in_w
        # the direct algorithm's FLOPs: the "TF" of this kernel in the bench tables can exceed the fp32 peak
        flops = 2.0 * m * n * 9 * c0
        nbytes = 4.0 * (m * c0 + m * n + n * 9 * c0)
        rec.end("conv3x3_wino_f32_kernel<16x16,32>", "3x3 s1 M%d N%d K%d" % (m, n, 9 * c0), flops, nbytes, ev0)
    return dst


def conv3x3_wino_n_ok(src0, c0, u_packed, n, *, batch, in_h, in_w, ldd=None, ld0=None):
    """ccvpe_conv3x3_wino_n_ok for this layer: 0 = not served, 1 = computed correctly, 2 = also a launch the probe showed a win at."""
    if src0.dtype != torch.float32 or u_packed is None:
        return 0
    ld0 = ld0 if ld0 is not None else src0.shape[-1]
    d = _wino_desc(src0, c0, u_packed, n, batch, in_h, in_w, None, None, ldd if ldd is not None else n, ld0)
    return int(_lib.load().ccvpe_conv3x3_wino_n_ok(ctypes.byref(d)))


def conv3x3_wino_n(src0, c0, u_packed, n, *, batch, in_h, in_w, shift=None, dst=None, ldd=None, ld0=None):
    """conv3x3_wino for 16 < n <= 80 with all output channels in one workgroup (ccvpe_conv3x3_wino_n_f32): bit-identical to
    conv3x3_wino.  A shape the kernel does not serve is an error."""
    lib = _lib.load()
    for t, nm in ((src0, "src0"), (u_packed, "w"), (shift, "shift"), (dst, "dst")):
        _chk(t, nm)
    ld0 = ld0 if ld0 is not None else src0.shape[-1]
    if dst is None:
        ldd = ldd if ldd is not None else n
        dst = _empty((batch, in_h, in_w, ldd), device=src0.device)
    elif ldd is None:
        ldd = dst.shape[-1]
    d = _wino_desc(src0, c0, u_packed, n, batch, in_h, in_w, shift, dst, ldd, ld0)
    rec = _recorder
    ev0 = rec.begin() if rec is not None else None
    check(lib.ccvpe_conv3x3_wino_n_f32(ctypes.byref(d), _stream()), "ccvpe_conv3x3_wino_n_f32")
    if rec is not None:
        m = batch * in_h * in_w
        flops = 2.0 * m * n * 9 * c0                   # the direct algorithm's, as conv3x3_wino
        nbytes = 4.0 * (m * c0 + m * n + n * 9 * c0)
        rec.end("conv3x3_wino_n_kernel<%d>" % (-(-n // 16)), "3x3 s1 M%d N%d K%d" % (m, n, 9 * c0), flops, nbytes, ev0)
    return dst


def _conv3x3_match1_f32(src0, c0, u_packed, n, g, L, shift, stride, ldo, batch, in_h, in_w, bias, window_offset, query_only):
    """fp32 storage: the Winograd kernel with all n <= 80 channels in one workgroup (ccvpe_conv3x3_wino_match1_f32); u_packed from
    models._pack_wino.  query_only returns the library's 0 / 1 / 2."""
    lib = _lib.load()
    if u_packed is None or u_packed.dtype != torch.float32 or src0.dtype != torch.float32:
        if query_only:
            return 0
        raise ValueError("conv3x3_match1: fp32 storage needs the Winograd U pack")
    _chk(src0, "src0")
    _chk(u_packed, "w")
    _chk(bias, "bias")
    d = _wino_desc(src0, c0, u_packed, n, batch, in_h, in_w, bias, None, ldo, src0.shape[-1])
    if query_only:
        return int(lib.ccvpe_conv3x3_wino_match1_ok(ctypes.byref(d), 1, L))
    if not g.is_cuda or g.dtype != torch.float32 or g.stride(-1) != 1:
        raise ValueError("g must be an fp32 device tensor with unit inner stride")
    scores = _empty((batch, 1, in_h, in_w), device=src0.device, dtype=torch.float32)
    cat = _empty((batch, in_h, in_w, ldo), device=src0.device, dtype=torch.float32)
    d.dst = _ptr(cat)
    rec = _recorder
    ev0 = rec.begin() if rec is not None else None
    check(lib.ccvpe_conv3x3_wino_match1_f32(ctypes.byref(d), 1, _ptr(g), g.stride(0), L, int(shift), int(stride),
                                            int(window_offset), _ptr(scores), _stream()), "ccvpe_conv3x3_wino_match1_f32")
    if rec is not None:
        m = batch * in_h * in_w
        rec.end("conv3x3_wino_n_kernel<%d,match>" % (-(-n // 16)), "3x3+match M%d N%d K%d" % (m, n, 9 * c0), 2.0 * m * n * 9 * c0,
                4.0 * m * c0 + 4.0 * m * ldo + 4.0 * m + 4.0 * n * 9 * c0, ev0)
    return scores, cat


def upconv3x3(src0, c0, w_packed, shift9, n, *, batch, h1, w1, src1=None, c1=0, act=ACT_NONE, algo_flops=None, route_only=False):
    """ConvTranspose2d(k2,s2) folded into the following 3x3 conv (ccvpe_upconv3x3_f32 / _bf16).
    src0 [B,h1,w1,ld0] low-res, src1 [B,2h1,2w1,ld1] skip; returns [B,2h1,2w1,n]."""
    lib = _lib.load()
    dt = _act_dtype(src0)
    for t, nm in ((src0, "src0"), (src1, "src1"), (w_packed, "w")):
        _chk(t, nm, dt)
    _chk(shift9, "shift9")
    dst = _empty((batch, 2 * h1, 2 * w1, n), device=src0.device, dtype=dt)
    d = _lib.UpconvDesc()
    d.src0, d.src1, d.w, d.shift9, d.dst = _ptr(src0), _ptr(src1), _ptr(w_packed), _ptr(shift9), _ptr(dst)
    d.c0, d.ld0, d.c1, d.ld1 = c0, src0.shape[-1], c1, (src1.shape[-1] if src1 is not None else 0)
    d.batch, d.h1, d.w1 = batch, h1, w1
    d.n, d.kpad, d.ldd, d.act = n, w_packed.shape[-1], n, act
    if route_only:
        return upconv_route(d, dt != torch.float32)
    rec = _recorder
    ev0 = rec.begin() if rec is not None else None
    fn = lib.ccvpe_upconv3x3_f32 if dt == torch.float32 else lib.ccvpe_upconv3x3_bf16
    check(fn(ctypes.byref(d), _stream()), "ccvpe_upconv3x3")
    if rec is not None:
        m = batch * h1 * w1 * 4
        k_eff = 4 * c0 + 9 * c1
        flops = algo_flops if algo_flops is not None else 2.0 * m * n * k_eff
        esz = 4.0 if dt == torch.float32 else 2.0
        nbytes = esz * (batch * h1 * w1 * c0 + m * c1 + m * n + 4 * n * k_eff)
        name = upconv_route_name(d, dt != torch.float32)                  # the library's own dispatch (ccvpe_upconv3x3_route)
        rec.end(name, "up3x3 M%d N%d Keff%d" % (m, n, k_eff), flops, nbytes, ev0)
    return dst


def _s3_desc(src0, c0, w3_packed, shift9, n, batch, h1, w1, src1, c1, act, dst, ldd, ld0, ld1):
    d = _lib.UpconvDesc()
    d.src0, d.src1, d.w, d.shift9 = _ptr(src0), _ptr(src1), _ptr(w3_packed), _ptr(shift9)
    d.dst = _ptr(dst) if dst is not None else None
    d.c0, d.ld0, d.c1, d.ld1 = c0, ld0, c1, ld1
    d.batch, d.h1, d.w1 = batch, h1, w1
    d.n, d.kpad, d.ldd, d.act = n, w3_packed.shape[1] * w3_packed.shape[3], ldd, act
    return d


def upconv3x3_s3_ok(src0, c0, w3_packed, n, *, batch, h1, w1, src1=None, c1=0, ldd=None, ld0=None, ld1=None):
    """ccvpe_upconv3x3_s3_ok for this layer: 0 = not served (also: anything but fp32 tensors, no three-plane pack), 1 = the
    kernel computes it, 2 = and the library's measured size rule prefers it to ccvpe_upconv3x3_f32.  Nothing is launched."""
    if w3_packed is None or src0.dtype != torch.float32 or (src1 is not None and src1.dtype != torch.float32):
        return 0
    if w3_packed.dtype != torch.bfloat16 or w3_packed.dim() != 4:
        return 0
    ld0 = ld0 if ld0 is not None else src0.shape[-1]
    ld1 = ld1 if ld1 is not None else (src1.shape[-1] if src1 is not None else 0)
    d = _s3_desc(src0, c0, w3_packed, None, n, batch, h1, w1, src1, c1, ACT_NONE, None, ldd if ldd is not None else n, ld0, ld1)
    return int(_lib.load().ccvpe_upconv3x3_s3_ok(ctypes.byref(d)))


def upconv3x3_s3_form_ok(src0, c0, w3_packed, n, form, *, batch, h1, w1, src1=None, c1=0, ldd=None, ld0=None, ld1=None):
    """ccvpe_upconv3x3_s3_form_ok: 0 = `form` (0 auto, 1 per-parity, 2 quad) cannot compute this layer, else the form that runs
    (for form 0: what the library's size rule picks).  Nothing is launched."""
    if not upconv3x3_s3_ok(src0, c0, w3_packed, n, batch=batch, h1=h1, w1=w1, src1=src1, c1=c1, ldd=ldd, ld0=ld0, ld1=ld1):
        return 0
    ld0 = ld0 if ld0 is not None else src0.shape[-1]
    ld1 = ld1 if ld1 is not None else (src1.shape[-1] if src1 is not None else 0)
    d = _s3_desc(src0, c0, w3_packed, None, n, batch, h1, w1, src1, c1, ACT_NONE, None, ldd if ldd is not None else n, ld0, ld1)
    return int(_lib.load().ccvpe_upconv3x3_s3_form_ok(ctypes.byref(d), form))


def upconv3x3_s3(src0, c0, w3_packed, shift9, n, *, batch, h1, w1, src1=None, c1=0, act=ACT_NONE, dst=None, ldd=None, ld0=None,
                 ld1=None, form=None):
    """ccvpe_upconv3x3_f32's layer with its products on the bf16 matrix cores, three bf16 planes per fp32 operand
    (ccvpe_upconv3x3_s3_f32); w3_packed from models._pack_upconv_s3.  Same result as upconv3x3 to fp32 rounding, not bit for
    bit.  fp32 tensors only; a layer the kernel does not serve is an error (no fallback).  form = None: the library chooses
    between its per-parity and quad kernels (ccvpe_upconv3x3_s3_f32); 1 / 2 force one (ccvpe_upconv3x3_s3_form_f32)."""
    lib = _lib.load()
    for t, nm in ((src0, "src0"), (src1, "src1"), (shift9, "shift9"), (dst, "dst")):
        _chk(t, nm)
    _chk(w3_packed, "w", torch.bfloat16)
    ld0 = ld0 if ld0 is not None else src0.shape[-1]
    ld1 = ld1 if ld1 is not None else (src1.shape[-1] if src1 is not None else 0)
    if dst is None:
        ldd = ldd if ldd is not None else n
        dst = _empty((batch, 2 * h1, 2 * w1, ldd), device=src0.device)
    elif ldd is None:
        ldd = dst.shape[-1]
    d = _s3_desc(src0, c0, w3_packed, shift9, n, batch, h1, w1, src1, c1, act, dst, ldd, ld0, ld1)
    rec = _recorder
    ev0 = rec.begin() if rec is not None else None
    if form is None:
        check(lib.ccvpe_upconv3x3_s3_f32(ctypes.byref(d), _stream()), "ccvpe_upconv3x3_s3_f32")
    else:
        check(lib.ccvpe_upconv3x3_s3_form_f32(ctypes.byref(d), form, _stream()), "ccvpe_upconv3x3_s3_form_f32")
    if rec is not None:
        # the fp32 layer's FLOPs and bytes (as upconv3x3): this kernel's "TF" in the bench tables can exceed the fp32 peak
        m = batch * h1 * w1 * 4
        k_eff = 4 * c0 + 9 * c1
        flops = 2.0 * m * n * k_eff
        nbytes = 4.0 * (batch * h1 * w1 * c0 + m * c1 + m * n + 4 * n * k_eff)
        rec.end(upconv_s3_route_name(d, form or 0), "up3x3 M%d N%d Keff%d" % (m, n, k_eff), flops, nbytes, ev0)
    return dst


def _pw_s3_desc(src0, c0, w3_packed, n, batch, in_h, in_w, two, gate, scale, shift, residual, act, dst, ldd, ld0):
    d = ConvDesc()
    d.src0, d.src1, d.gate, d.w = _ptr(src0), None, _ptr(gate), _ptr(w3_packed)
    d.scale, d.shift, d.residual = _ptr(scale), _ptr(shift), _ptr(residual)
    d.dst = _ptr(dst) if dst is not None else None
    d.c0, d.ld0, d.c1, d.ld1 = c0, ld0, 0, 0
    d.batch, d.in_h, d.in_w = batch, in_h, in_w
    d.kh, d.kw, d.stride, d.pad = (2, 2, 2, 0) if two else (1, 1, 1, 0)
    d.n, d.kpad = n, w3_packed.shape[0] * w3_packed.shape[2]
    d.ldd = ldd
    d.ldres = residual.shape[-1] if residual is not None else 0
    d.act, d.out_mode = act, OUT_NHWC
    return d


def pw_s3_ok(src0, c0, w3_packed, n, *, batch, in_h, in_w, two=False, gate=None, residual=None, act=ACT_NONE, ldd=None, ld0=None):
    """ccvpe_pw_s3_ok for this 1x1 (two: 2x2 stride-2) layer: 0 = not served (also: anything but fp32 tensors, no three-plane pack
    or one whose rows are not round_up(n, 16)), 1 = the kernel computes it, 2 = and the library's measured size rule prefers it to
    conv_igemm.  Nothing is launched."""
    if w3_packed is None or src0.dtype != torch.float32 or (residual is not None and residual.dtype != torch.float32):
        return 0
    if w3_packed.dtype != torch.bfloat16 or w3_packed.dim() != 3 or w3_packed.shape[1] != (n + 15) // 16 * 16 or w3_packed.shape[2] != 48:
        return 0
    ld0 = ld0 if ld0 is not None else src0.shape[-1]
    d = _pw_s3_desc(src0, c0, w3_packed, n, batch, in_h, in_w, two, gate, None, None, residual, act, None, ldd if ldd is not None else n, ld0)
    return int(_lib.load().ccvpe_pw_s3_ok(ctypes.byref(d)))


def pw_s3_route_name(desc):
    """Kernel name of ccvpe_pw_s3_f32(desc) as rocprofv3 prints it (minus namespace): ccvpe_pw_s3_route, no launch."""
    r = _lib.load().ccvpe_pw_s3_route(ctypes.byref(desc))
    if r <= 0:
        raise _lib.CcvpeError("ccvpe_pw_s3_route: the kernel does not compute this layer")
    return "pw_s3_kernel<%d,%d,%d,%d>" % ((r >> 8) & 0xf, (r >> 12) & 0xf, (r >> 16) & 0xf, (r >> 20) & 0xf)


def pw_s3(src0, c0, w3_packed, n, *, batch, in_h, in_w, two=False, gate=None, scale=None, shift=None, residual=None, act=ACT_NONE,
          dst=None, ldd=None, ld0=None):
    """conv_igemm's fp32 1x1 layer (two: the 2x2 stride-2 layer) with its products on the bf16 matrix cores, three bf16 planes per
    fp32 operand (ccvpe_pw_s3_f32); w3_packed from models._pack_pw_s3.  Same result as conv_igemm to fp32 rounding, not bit for bit.
    fp32 tensors only; a layer the kernel does not serve is an error (no fallback)."""
    lib = _lib.load()
    for t, nm in ((src0, "src0"), (gate, "gate"), (scale, "scale"), (shift, "shift"), (residual, "residual"), (dst, "dst")):
        _chk(t, nm)
    _chk(w3_packed, "w", torch.bfloat16)
    if w3_packed.dim() != 3 or w3_packed.shape[1] != (n + 15) // 16 * 16 or w3_packed.shape[2] != 48:
        raise ValueError("w is not the three-plane pack of models._pack_pw_s3 for n = %d" % n)
    ld0 = ld0 if ld0 is not None else src0.shape[-1]
    ho, wo = (in_h // 2, in_w // 2) if two else (in_h, in_w)
    if dst is None:
        ldd = ldd if ldd is not None else n
        dst = _empty((batch, ho, wo, ldd), device=src0.device)
    elif ldd is None:
        ldd = dst.shape[-1]
    d = _pw_s3_desc(src0, c0, w3_packed, n, batch, in_h, in_w, two, gate, scale, shift, residual, act, dst, ldd, ld0)
    rec = _recorder
    ev0 = rec.begin() if rec is not None else None
    check(lib.ccvpe_pw_s3_f32(ctypes.byref(d), _stream()), "ccvpe_pw_s3_f32")
    if rec is not None:
        # the fp32 layer's FLOPs and bytes (as conv_igemm): this kernel's "TF" in the bench tables can exceed the fp32 peak
        m = batch * ho * wo
        k_alg = (4 if two else 1) * c0
        flops = 2.0 * m * n * k_alg
        nbytes = 4.0 * (batch * in_h * in_w * c0 + m * n + n * k_alg + (m * n if residual is not None else 0))
        rec.end(pw_s3_route_name(d), "%s M%d N%d K%d" % ("2x2 s2" if two else "1x1 s1", m, n, k_alg), flops, nbytes, ev0)
    return dst


def tail512(x, c0, w_packed, shift9, w2, b2, cout, normalize, *, batch, h1, w1, split=False, want_softmax=False):
    """The whole 512 x 512 decoder level in one launch (ccvpe_tail512_f32 / _bf16): folded deconv + conv.0 + ReLU + conv.2
    (+ F.normalize for cout = 2).  x [B,h1,w1,ld0]; w_packed / shift9 from models._pack_upconv (n = 16, no skip);
    w2 [cout,3,3,16], b2 [cout] fp32; returns [B,cout,2h1,2w1] fp32.
    split (fp32 operands): 0 / False = exact fp32 products; 1 / True = two bf16 planes per operand (cout 1: the fp32 tail of the bf16
    storage path); 2 = three bf16 planes, six products, fp32-class (cout 1 and 2: the fp32 path)."""
    lib = _lib.load()
    dt = _act_dtype(x)
    _chk(x, "x", dt)
    _chk(w_packed, "w", dt)
    for t, nm in ((shift9, "shift9"), (w2, "w2"), (b2, "b2")):
        _chk(t, nm)
    if tuple(w2.shape) != (cout, 3, 3, 16) or tuple(shift9.shape) != (9, 16) or w_packed.shape[0] != 4 or w_packed.shape[1] != 16:
        raise ValueError("tail512: w [4,16,kpad], shift9 [9,16], w2 [cout,3,3,16] expected")
    out = _empty((batch, cout, 2 * h1, 2 * w1), device=x.device, dtype=torch.float32)
    d = _lib.TailDesc()
    d.x, d.w, d.shift9, d.w2, d.b2, d.out = _ptr(x), _ptr(w_packed), _ptr(shift9), _ptr(w2), _ptr(b2), _ptr(out)
    d.batch, d.h1, d.w1 = batch, h1, w1
    d.c0, d.ld0, d.kpad = c0, x.shape[-1], w_packed.shape[-1]
    split = int(split)                       # True -> 1
    d.cout, d.normalize, d.split = cout, int(bool(normalize)), split
    smx = None
    if want_softmax:                         # cout = 1: per-(tile, wave) softmax partials for softmax_apply()
        npart = lib.ccvpe_tail512_partials(ctypes.byref(d), int(dt != torch.float32))
        if npart <= 0:
            check(int(npart) if npart < 0 else -1, "ccvpe_tail512_partials")
        smx = _empty((batch, npart, 2), device=x.device, dtype=torch.float32)
        d.softmax_partial = _ptr(smx)
    rec = _recorder
    ev0 = rec.begin() if rec is not None else None
    fn = lib.ccvpe_tail512_f32 if dt == torch.float32 else lib.ccvpe_tail512_bf16
    check(fn(ctypes.byref(d), _stream()), "ccvpe_tail512")
    if rec is not None:
        m = batch * h1 * w1 * 4
        esz = 4.0 if dt == torch.float32 else 2.0
        rec.end("tail512_kernel<%s,%d>" % (("f32", "f32 as bf16 hi+lo", "f32 as bf16 hi+mid+lo")[split] if dt == torch.float32 else "bf16", cout), "tail M%d Keff%d" % (m, 4 * c0),
                2.0 * m * 16 * (4 * c0 + 9 * cout), esz * batch * h1 * w1 * c0 + 4.0 * m * cout, ev0)
    return (out, smx) if want_softmax else out


def softmax_apply(logits, partials):
    """Softmax(dim=-1) of logits [rows, n] from the (max, sum exp) partials tail512 wrote ([rows, P, 2])."""
    lib = _lib.load()
    _chk(logits, "logits")
    _chk(partials, "partials")
    rows, n = logits.shape
    out = _empty(logits.shape, device=logits.device, dtype=logits.dtype)
    check(lib.ccvpe_softmax_apply_f32(_ptr(logits), _ptr(partials), partials.shape[1], _ptr(out), rows, n, _stream()),
          "ccvpe_softmax_apply_f32")
    return out


def tail512_ok(h1, w1, n_a):
    """Shapes the fused 512 x 512 level handles (everything else runs ccvpe_upconv3x3 + ccvpe_head_conv3x3)."""
    return n_a == 16 and h1 % 16 == 0 and w1 % 16 == 0


def stem_conv(x_nchw, w, scale, shift, circular, out_dtype=torch.float32):
    lib = _lib.load()
    for t, nm in ((x_nchw, "x"), (w, "w"), (scale, "scale"), (shift, "shift")):
        _chk(t, nm)
    b, c, h, wd = x_nchw.shape
    if c != 3:
        raise ValueError("stem expects 3 input channels")
    ho, wo = (h + 1 - 3) // 2 + 1, (wd + 1 - 3) // 2 + 1
    y = _empty((b, ho, wo, 32), device=x_nchw.device, dtype=out_dtype)
    fn = lib.ccvpe_stem_conv_f32 if out_dtype == torch.float32 else lib.ccvpe_stem_conv_bf16
    check(fn(_ptr(x_nchw), _ptr(w), _ptr(scale), _ptr(shift), _ptr(y), b, h, wd, int(bool(circular)), _stream()),
          "ccvpe_stem_conv")
    return y


def stem_dw_supported(in_h, in_w, circular):
    """SE partial rows per sample of the fused stem + block-0 depthwise launch, 0 when the shape runs unfused."""
    return _lib.load().ccvpe_stem_dw_nblk(in_h, in_w, int(bool(circular)))


def stem_dw(x_nchw, w, s0, b0, w_dw, s1, b1, circular, out_dtype=torch.float32):
    """Stem conv + BN + swish -> block-0 depthwise 3x3 + BN + swish + SE squeeze partials, the stem tensor kept in LDS
    (csrc/stem_dw.hip); returns (y [B,Ho,Wo,32], se_partial [B,nblk,32])."""
    lib = _lib.load()
    for t, nm in ((x_nchw, "x"), (w, "w"), (s0, "s0"), (b0, "b0"), (w_dw, "w_dw"), (s1, "s1"), (b1, "b1")):
        _chk(t, nm)
    b, c, h, wd = x_nchw.shape
    if c != 3 or w_dw.numel() != 9 * 32:
        raise ValueError("stem_dw expects 3 input channels and a 3x3x32 depthwise weight")
    nblk = stem_dw_supported(h, wd, circular)
    if nblk <= 0:
        raise _lib.CcvpeError("stem_dw: unsupported shape %s" % (tuple(x_nchw.shape),))
    ho, wo = (h + 1 - 3) // 2 + 1, (wd + 1 - 3) // 2 + 1
    y = _empty((b, ho, wo, 32), device=x_nchw.device, dtype=out_dtype)
    part = _empty((b, nblk, 32), device=x_nchw.device, dtype=torch.float32)
    rec = _recorder
    ev0 = rec.begin() if rec is not None else None
    fn = lib.ccvpe_stem_dw_f32 if out_dtype == torch.float32 else lib.ccvpe_stem_dw_bf16
    check(fn(_ptr(x_nchw), _ptr(w), _ptr(s0), _ptr(b0), _ptr(w_dw), _ptr(s1), _ptr(b1), _ptr(y), _ptr(part), b, h, wd,
             int(bool(circular)), _stream()), "ccvpe_stem_dw")
    if rec is not None:
        flops = 2.0 * b * ho * wo * 32 * (27 + 9)
        nbytes = 4.0 * b * 3 * h * wd + (4.0 if out_dtype == torch.float32 else 2.0) * b * ho * wo * 32
        rec.end("stem_dw_kernel", "in %dx%dx3" % (h, wd), flops, nbytes, ev0)
    return y, part


def dwconv(x, w, scale, shift, k, stride, circular):
    """Depthwise conv + BN + swish; returns (y, se_partial [B,nblk,C])."""
    lib = _lib.load()
    dt = _act_dtype(x)
    _chk(x, "x", dt)
    for t, nm in ((w, "w"), (scale, "scale"), (shift, "shift")):
        _chk(t, nm)
    b, h, wd, c = x.shape
    tot = (k - 1) if stride == 1 else (k - 2)
    ho, wo = (h + tot - k) // stride + 1, (wd + tot - k) // stride + 1
    nblk = lib.ccvpe_dwconv_nblk(h, wd, c, stride)
    if nblk <= 0:
        raise _lib.CcvpeError("ccvpe_dwconv_nblk rejected shape %s" % (tuple(x.shape),))
    y = _empty((b, ho, wo, c), device=x.device, dtype=dt)
    part = _empty((b, nblk, c), device=x.device, dtype=torch.float32)
    fn = lib.ccvpe_dwconv_f32 if dt == torch.float32 else lib.ccvpe_dwconv_bf16
    check(fn(_ptr(x), _ptr(w), _ptr(scale), _ptr(shift), _ptr(y), _ptr(part), b, h, wd, c, k, stride,
             int(bool(circular)), _stream()), "ccvpe_dwconv")
    return y, part


def mbconv_front_supported(in_h, in_w, cin, mid, k, stride):
    n = _lib.load().ccvpe_mbconv_front_nblk(in_h, in_w, cin, mid, k, stride)
    if n < 0:
        raise _lib.CcvpeError("ccvpe_mbconv_front_nblk rejected k=%d stride=%d" % (k, stride))
    return n


def mbconv_band_plan(in_h, in_w, cin, mid, k, stride, batch):
    """dict(nkk, tpw, ry, cpg, ngrp) of the mbconv_band_kernel launch the bf16 fused front makes for a shape (ccvpe_mbconv_band_plan:
    the launcher's own helper), or None when the band kernel does not take it."""
    r = _lib.load().ccvpe_mbconv_band_plan(in_h, in_w, cin, mid, k, stride, batch)
    if r <= 0:
        return None
    return dict(nkk=r & 0xf, tpw=(r >> 4) & 0xf, ry=(r >> 8) & 0xf, cpg=(r >> 12) & 0xff, ngrp=(r >> 20) & 0xff)


def mbconv_front(x, w_exp, s0, b0, w_dw, s1, b1, mid, k, stride, circular):
    """Fused expand + depthwise (+BN+swish each) + SE squeeze partials; returns (y, se_partial)."""
    lib = _lib.load()
    dt = _act_dtype(x)
    _chk(x, "x", dt)
    _chk(w_exp, "w_exp", dt)
    for t, nm in ((s0, "s0"), (b0, "b0"), (w_dw, "w_dw"), (s1, "s1"), (b1, "b1")):
        _chk(t, nm)
    b, h, wd, cin = x.shape
    nblk = mbconv_front_supported(h, wd, cin, mid, k, stride)
    if nblk == 0:
        raise _lib.CcvpeError("mbconv_front: unsupported shape %s" % (tuple(x.shape),))
    tot = (k - 1) if stride == 1 else (k - 2)
    ho, wo = (h + tot - k) // stride + 1, (wd + tot - k) // stride + 1
    y = _empty((b, ho, wo, mid), device=x.device, dtype=dt)
    part = _empty((b, nblk, mid), device=x.device, dtype=torch.float32)
    rec = _recorder
    ev0 = rec.begin() if rec is not None else None
    fn = lib.ccvpe_mbconv_front_f32 if dt == torch.float32 else lib.ccvpe_mbconv_front_bf16
    check(fn(_ptr(x), _ptr(w_exp), w_exp.shape[1], _ptr(s0), _ptr(b0), _ptr(w_dw), _ptr(s1), _ptr(b1), _ptr(y),
             _ptr(part), b, h, wd, cin, mid, k, stride, int(bool(circular)), _stream()), "ccvpe_mbconv_front")
    if rec is not None:
        flops = 2.0 * b * h * wd * cin * mid + 2.0 * b * ho * wo * mid * k * k
        nbytes = (4.0 if dt == torch.float32 else 2.0) * (b * h * wd * cin + b * ho * wo * mid)
        route = lib.ccvpe_mbconv_front_route(h, wd, cin, mid, k, stride, int(dt != torch.float32), b)
        kname = {1: "mbconv_front_kernel", 2: "mbconv_plane_kernel", 3: "mbconv_band_kernel"}.get(route, "mbconv_front_kernel")
        rec.end("%s<%d,%d>" % (kname, k, stride), "in %dx%dx%d mid %d" % (h, wd, cin, mid), flops, nbytes, ev0)
    return y, part


def mbconv_front_s3_ok(x, w_exp3, mid, k, stride):
    """ccvpe_mbconv_front_s3_ok for this early block: 0 = not served (also: anything but an fp32 x, no three-plane pack or one that
    is not [ceil(cin / 16)][mid][48] bf16), 1 = the kernel computes it, 2 = and the library's measured size rule prefers it to
    ccvpe_mbconv_front_f32.  Nothing is launched."""
    if w_exp3 is None or x.dtype != torch.float32 or w_exp3.dtype != torch.bfloat16:
        return 0
    b, h, wd, cin = x.shape
    if w_exp3.dim() != 3 or tuple(w_exp3.shape) != ((cin + 15) // 16, mid, 48):
        return 0
    return int(_lib.load().ccvpe_mbconv_front_s3_ok(h, wd, cin, mid, k, stride, b))


def mbconv_front_s3(x, w_exp3, s0, b0, w_dw, s1, b1, mid, k, stride, circular):
    """mbconv_front's fp32 early block with the expand 1x1 on the bf16 matrix cores, three bf16 planes per fp32 operand
    (ccvpe_mbconv_front_s3_f32); w_exp3 from models._pack_pw_s3 of the fp32 expand pack.  Same result as mbconv_front to fp32
    rounding, not bit for bit; same se_partial rows.  A shape the kernel does not serve is an error (no fallback)."""
    lib = _lib.load()
    _chk(x, "x", torch.float32)
    _chk(w_exp3, "w_exp3", torch.bfloat16)
    for t, nm in ((s0, "s0"), (b0, "b0"), (w_dw, "w_dw"), (s1, "s1"), (b1, "b1")):
        _chk(t, nm)
    b, h, wd, cin = x.shape
    if w_exp3.dim() != 3 or tuple(w_exp3.shape) != ((cin + 15) // 16, mid, 48):
        raise ValueError("w_exp3 is not the three-plane pack of models._pack_pw_s3 for cin = %d, mid = %d" % (cin, mid))
    nblk = mbconv_front_supported(h, wd, cin, mid, k, stride)
    if nblk == 0 or not lib.ccvpe_mbconv_front_s3_ok(h, wd, cin, mid, k, stride, b):
        raise _lib.CcvpeError("mbconv_front_s3: unsupported shape %s k=%d stride=%d" % (tuple(x.shape), k, stride))
    tot = (k - 1) if stride == 1 else (k - 2)
    ho, wo = (h + tot - k) // stride + 1, (wd + tot - k) // stride + 1
    y = _empty((b, ho, wo, mid), device=x.device, dtype=torch.float32)
    part = _empty((b, nblk, mid), device=x.device, dtype=torch.float32)
    rec = _recorder
    ev0 = rec.begin() if rec is not None else None
    check(lib.ccvpe_mbconv_front_s3_f32(_ptr(x), _ptr(w_exp3), w_exp3.shape[0] * w_exp3.shape[2], _ptr(s0), _ptr(b0), _ptr(w_dw),
                                        _ptr(s1), _ptr(b1), _ptr(y), _ptr(part), b, h, wd, cin, mid, k, stride,
                                        int(bool(circular)), _stream()), "ccvpe_mbconv_front_s3_f32")
    if rec is not None:
        # the fp32 layer's FLOPs and bytes (as mbconv_front)
        flops = 2.0 * b * h * wd * cin * mid + 2.0 * b * ho * wo * mid * k * k
        nbytes = 4.0 * (b * h * wd * cin + b * ho * wo * mid)
        rec.end("mbconv_front_s3_kernel<%d,%d>" % (k, stride), "in %dx%dx%d mid %d" % (h, wd, cin, mid), flops, nbytes, ev0)
    return y, part


def se_gate(part, hw, w1, b1, w2, b2):
    lib = _lib.load()
    for t, nm in ((part, "part"), (w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2")):
        _chk(t, nm)
    b, nblk, c = part.shape
    cs = w1.shape[0]
    gate = _empty((b, c), device=part.device, dtype=torch.float32)
    check(lib.ccvpe_se_gate_f32(_ptr(part), nblk, 1.0 / float(hw), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2),
                                _ptr(gate), b, c, cs, _stream()), "ccvpe_se_gate_f32")
    return gate


def ground_descriptor(y1, wh, bh, cd):
    lib = _lib.load()
    for t, nm in ((y1, "y1"), (wh, "wh"), (bh, "bh")):
        _chk(t, nm)
    b, h, w, ld = y1.shape
    cd_arr = (ctypes.c_int * 6)(*cd)
    out = _empty((b, w * sum(cd)), device=y1.device, dtype=torch.float32)
    check(lib.ccvpe_ground_descriptor_f32(_ptr(y1), ld, _ptr(wh), _ptr(bh), cd_arr, _ptr(out), b, h, w,
                                          _stream()), "ccvpe_ground_descriptor_f32")
    return out


def conv3x3_match1(src0, c0, w_packed, n, g, L, shift, stride, ldo, *, batch, in_h, in_w, bias, window_offset=0, out_f32=False,
                   query_only=False):
    """convK.2 (3x3, bias, no activation) of a decoder level WITH the next level's one-hypothesis matching in its epilogue
    (ccvpe_conv3x3_match1_bf16, csrc/narrow_impl.h c3n_kernel<MATCH>): returns (scores [B,1,H,W] fp32, cat [B,H,W,ldo] bf16 / fp32)
    = what conv_igemm(...) followed by match_level(x, g, L, [shift], 1, 0, stride, ldo) returns; x is never written.
    query_only: True / False — does the library serve this layer and shape (else the caller runs the two ops).
    fp32 storage: w_packed is the Winograd U pack (models._pack_wino) and the launch is ccvpe_conv3x3_wino_match1_f32
    (csrc/conv3x3_wino_n.hip); query_only then returns that entry's 0 / 1 / 2 (served at all / ... and a measured win)."""
    lib = _lib.load()
    dt = _act_dtype(src0)
    if dt != torch.bfloat16:
        return _conv3x3_match1_f32(src0, c0, w_packed, n, g, L, shift, stride, ldo, batch, in_h, in_w, bias, window_offset, query_only)
    _chk(src0, "src0", dt)
    _chk(w_packed, "w", dt)
    _chk(bias, "bias")
    d = ConvDesc()
    d.src0, d.src1, d.gate, d.w = _ptr(src0), None, None, _ptr(w_packed)
    d.scale, d.shift, d.residual = None, _ptr(bias), None
    d.c0, d.ld0, d.c1, d.ld1 = c0, src0.shape[-1], 0, 0
    d.batch, d.in_h, d.in_w = batch, in_h, in_w
    d.kh, d.kw, d.stride, d.pad = 3, 3, 1, 1
    d.n, d.kpad, d.ldd, d.ldres = n, w_packed.shape[1], ldo, 0
    d.act, d.out_mode = ACT_NONE, OUT_NHWC
    if query_only:
        return lib.ccvpe_conv3x3_match1_ok(ctypes.byref(d), int(bool(out_f32)), L) == 1
    if not g.is_cuda or g.dtype != torch.float32 or g.stride(-1) != 1:
        raise ValueError("g must be an fp32 device tensor with unit inner stride")
    scores = _empty((batch, 1, in_h, in_w), device=src0.device, dtype=torch.float32)
    cat = _empty((batch, in_h, in_w, ldo), device=src0.device, dtype=torch.float32 if out_f32 else dt)
    d.dst = _ptr(cat)
    rec = _recorder
    ev0 = rec.begin() if rec is not None else None
    check(lib.ccvpe_conv3x3_match1_bf16(ctypes.byref(d), int(bool(out_f32)), _ptr(g), g.stride(0), L, int(shift), int(stride),
                                        int(window_offset), _ptr(scores), _stream()), "ccvpe_conv3x3_match1_bf16")
    if rec is not None:
        m = batch * in_h * in_w
        rec.end("c3n_kernel<bf16,%d,match>" % n, "3x3+match M%d N%d K%d" % (m, n, 9 * c0), 2.0 * m * n * 9 * c0,
                2.0 * m * c0 + (4.0 if out_f32 else 2.0) * m * ldo + 4.0 * m + 2.0 * n * 9 * c0, ev0)
    return scores, cat


def match_level(x, g, L, shifts, n_max, n_tail, stride, ldo, channels=None, window_offset=0):
    """Fused rotational matching.  x [B,H,W,ldx]; g [B,ldg] view with row stride ldg.
    Returns (scores [B,n_shifts,H,W], dstx [B,H,W,ldo])."""
    lib = _lib.load()
    dt = _act_dtype(x)
    _chk(x, "x", dt)
    if not g.is_cuda or g.dtype != torch.float32 or g.stride(-1) != 1:
        raise ValueError("g must be an fp32 device tensor with unit inner stride")
    b, h, w, ldx = x.shape
    c = channels if channels is not None else ldx
    n = len(shifts)
    sh = (ctypes.c_int * n)(*shifts)
    scores = _empty((b, n, h, w), device=x.device, dtype=torch.float32)
    dstx = _empty((b, h, w, ldo), device=x.device, dtype=dt)
    fn = lib.ccvpe_match_level_f32 if dt == torch.float32 else lib.ccvpe_match_level_bf16
    check(fn(_ptr(x), ldx, _ptr(g), g.stride(0), L, sh, n, n_max, n_tail, stride, window_offset, _ptr(scores), _ptr(dstx),
             ldo, b, h * w, c, _stream()), "ccvpe_match_level")
    return scores, dstx


def head_conv3x3(x, w, bias, cout, normalize):
    lib = _lib.load()
    dt = _act_dtype(x)
    _chk(x, "x", dt)
    for t, nm in ((w, "w"), (bias, "bias")):
        _chk(t, nm)
    b, h, wd, c = x.shape
    if c != 16:
        raise ValueError("head conv expects 16 input channels")
    out = _empty((b, cout, h, wd), device=x.device, dtype=torch.float32)
    fn = lib.ccvpe_head_conv3x3_f32 if dt == torch.float32 else lib.ccvpe_head_conv3x3_bf16
    check(fn(_ptr(x), _ptr(w), _ptr(bias), _ptr(out), b, h, wd, cout, int(bool(normalize)), _stream()),
          "ccvpe_head_conv3x3")
    return out


def cast_f32(x):
    """bf16 activation tensor -> fp32 (ccvpe_cast_bf16_f32); an fp32 tensor is returned as is."""
    if x.dtype == torch.float32:
        return x
    lib = _lib.load()
    _chk(x, "x", torch.bfloat16)
    out = _empty(x.shape, device=x.device, dtype=torch.float32)
    check(lib.ccvpe_cast_bf16_f32(_ptr(x), _ptr(out), x.numel(), _stream()), "ccvpe_cast_bf16_f32")
    return out


def softmax_rows(logits):
    lib = _lib.load()
    _chk(logits, "logits")
    rows, n = logits.shape
    out = _empty(logits.shape, device=logits.device, dtype=logits.dtype)
    check(lib.ccvpe_softmax_rows_f32(_ptr(logits), _ptr(out), rows, n, _stream()), "ccvpe_softmax_rows_f32")
    return out


# ----------------------------------------------------------------------------------------------
# train-mode pieces
# ----------------------------------------------------------------------------------------------
def stem_conv_raw(x_nchw, w, circular):
    """Stem convolution only (train mode: BN needs the batch statistics first)."""
    lib = _lib.load()
    _chk(x_nchw, "x")
    _chk(w, "w")
    b, c, h, wd = x_nchw.shape
    ho, wo = (h + 1 - 3) // 2 + 1, (wd + 1 - 3) // 2 + 1
    y = _empty((b, ho, wo, 32), device=x_nchw.device, dtype=torch.float32)
    check(lib.ccvpe_stem_conv_raw_f32(_ptr(x_nchw), _ptr(w), _ptr(y), b, h, wd, int(bool(circular)), _stream()),
          "ccvpe_stem_conv_raw_f32")
    return y


def dwconv_raw(x, w, k, stride, circular):
    lib = _lib.load()
    _chk(x, "x")
    _chk(w, "w")
    b, h, wd, c = x.shape
    tot = (k - 1) if stride == 1 else (k - 2)
    ho, wo = (h + tot - k) // stride + 1, (wd + tot - k) // stride + 1
    y = _empty((b, ho, wo, c), device=x.device, dtype=torch.float32)
    check(lib.ccvpe_dwconv_raw_f32(_ptr(x), _ptr(w), _ptr(y), b, h, wd, c, k, stride, int(bool(circular)), _stream()),
          "ccvpe_dwconv_raw_f32")
    return y


def bn_stats(x, run_mean=None, run_var=None, momentum=0.01):
    """Per-channel batch mean / biased variance of an NHWC tensor; updates the running statistics in place
    (momentum as torch: new = (1-m)*old + m*batch, unbiased variance)."""
    lib = _lib.load()
    _chk(x, "x")
    _chk(run_mean, "run_mean")
    _chk(run_var, "run_var")
    c = x.shape[-1]
    rows = x.numel() // c
    mean = _empty((c,), device=x.device, dtype=torch.float32)
    var = _empty((c,), device=x.device, dtype=torch.float32)
    scratch = _empty((lib.ccvpe_bn_stats_nblk(rows) * 3 * c,), device=x.device, dtype=torch.float32)
    check(lib.ccvpe_bn_stats_f32(_ptr(x), rows, c, _ptr(mean), _ptr(var), _ptr(run_mean), _ptr(run_var),
                                 float(momentum), _ptr(scratch), _stream()), "ccvpe_bn_stats_f32")
    return mean, var


def bn_act(x, mean, var, gamma, beta, eps, act, residual=None, dc_scale=None, want_se=False):
    """Normalise + activation (+ drop-connect scale, + residual); optionally SE squeeze partials."""
    lib = _lib.load()
    for t, nm in ((x, "x"), (mean, "mean"), (var, "var"), (gamma, "gamma"), (beta, "beta"), (residual, "residual"),
                  (dc_scale, "dc_scale")):
        _chk(t, nm)
    b, c = x.shape[0], x.shape[-1]
    rps = x.numel() // (b * c)
    y = _empty(x.shape, device=x.device, dtype=x.dtype)
    part = None
    if want_se:
        part = _empty((b, lib.ccvpe_bn_act_nblk(rps), c), device=x.device, dtype=torch.float32)
    check(lib.ccvpe_bn_act_f32(_ptr(x), _ptr(mean), _ptr(var), _ptr(gamma), _ptr(beta), float(eps), act, _ptr(residual),
                               _ptr(dc_scale), _ptr(y), _ptr(part), b, rps, c, _stream()), "ccvpe_bn_act_f32")
    return (y, part) if want_se else y


def eval_postprocess(heatmap, ori):
    """train_VIGOR.py:294-324 on the device: returns [B,6] = (y, x, cos, sin, angle_deg, prob)."""
    lib = _lib.load()
    _chk(heatmap, "heatmap")
    _chk(ori, "ori")
    b, _, h, w = heatmap.shape
    out = _empty((b, 6), device=heatmap.device, dtype=torch.float32)
    check(lib.ccvpe_eval_postprocess_f32(_ptr(heatmap), _ptr(ori), _ptr(out), b, h, w, _stream()),
          "ccvpe_eval_postprocess_f32")
    return out


def eval_metrics(heatmap, ori, gt, gt_ori, heading_deg, metres_per_pixel, out=None):
    """The reference test protocols' per-sample loop body on the device (train_KITTI.py:304-343, train_VIGOR.py:294-326):
    returns [B,12] float64 = (pred_y, pred_x, gt_y, gt_x, pixel distance, metres, longitudinal metres, lateral metres,
    predicted angle, orientation error, heatmap[pred], heatmap[gt]) — ccvpe_amd.evaluate.metrics_spec is the specification.
    heading_deg, metres_per_pixel: [B] float64 device tensors.  out: a caller's [B,12] float64 slice of a larger table."""
    lib = _lib.load()
    for t, nm in ((heatmap, "heatmap"), (ori, "ori"), (gt, "gt"), (gt_ori, "gt_ori")):
        _chk(t, nm)
    for t, nm in ((heading_deg, "heading_deg"), (metres_per_pixel, "metres_per_pixel"), (out, "out")):
        _chk(t, nm, torch.float64)
    b, _, h, w = heatmap.shape
    if ori.shape != (b, 2, h, w) or gt.shape != heatmap.shape or gt_ori.shape != ori.shape:
        raise ValueError("eval_metrics: heatmap/gt [B,1,h,w] and ori/gt_ori [B,2,h,w] expected")
    if heading_deg.numel() != b or metres_per_pixel.numel() != b:
        raise ValueError("eval_metrics: heading_deg and metres_per_pixel must hold one value per sample")
    if out is None:
        out = _empty((b, 12), device=heatmap.device, dtype=torch.float64)
    elif tuple(out.shape) != (b, 12):
        raise ValueError("eval_metrics: out must be [%d,12], got %s" % (b, tuple(out.shape)))
    check(lib.ccvpe_eval_metrics_f32(_ptr(heatmap), _ptr(ori), _ptr(gt), _ptr(gt_ori), _ptr(heading_deg),
                                     _ptr(metres_per_pixel), _ptr(out), b, h, w, _stream()), "ccvpe_eval_metrics_f32")
    return out


def belief_partials(h, w):
    """Doubles of scratch per track that belief_step needs for an h x w grid (launches nothing)."""
    n = _lib.load().ccvpe_belief_partials(int(h), int(w))
    if n <= 0:
        raise ValueError("belief_partials: bad grid %s x %s" % (h, w))
    return n


def belief_step(prior, heatmap, ori, offsets, taps, outlier=0.0, reset=None, post=None, scratch=None, out=None):
    """One histogram-filter step per track on the device (two launches; ccvpe_amd.tracking.step_spec is the specification):
    the prior moved by `offsets` [B,2] int32 (oy, ox) and blurred by `taps` [B,2,2R+1] fp32 (y then x, 0 <= R <= 32), times
    (1 - outlier) * heatmap + outlier / (h w), renormalised.  prior, heatmap [B,1,h,w]; ori [B,2,h,w]; reset [B] int32 or None
    (a non-zero entry starts that track from the measurement; its prior is not read).  post: a caller's [B,1,h,w] tensor that
    does not overlap prior; scratch: B * belief_partials(h, w) float64; out: a caller's [B,14] float64 slice of a larger table.
    Returns (rows [B,14] float64 — columns ccvpe_amd.tracking.PRED_Y ... SURVIVED, post)."""
    return _belief_step("belief_step", [(prior, "prior"), (heatmap, "heatmap")], ori, offsets, _OFFSETS, taps, outlier,
                        (reset, "reset"), [(post, "post")], scratch, out)


def belief_step_rigid(prior, heatmap, ori, motion, taps, outlier=0.0, reset=None, post=None, scratch=None, out=None):
    """belief_step with the predict replaced by a rigid motion of the grid (ccvpe_amd.tracking.step_rigid_spec is the
    specification): the prior resampled bilinearly through `motion` [B,6] float64 on the device — rows (a00, a01, a02, a10, a11,
    a12) of the INVERSE map, output pixel (y, x) reads the prior at ((a00 y + a01 x) + a02, (a10 y + a11 x) + a12), as
    tracking.rigid_motion and tracking.kitti_motions return them — then blurred by `taps` [B,2,2R+1] (centred:
    tracking.motion_taps(zeros, sigma, R)).  Every other argument, every check and the return value are belief_step's."""
    return _belief_step("belief_step_rigid", [(prior, "prior"), (heatmap, "heatmap")], ori, motion, _MOTION, taps, outlier,
                        (reset, "reset"), [(post, "post")], scratch, out)


def belief_viterbi_step(prior, heatmap, ori, offsets, taps, outlier=0.0, reset=None, post=None, scratch=None, out=None):
    """belief_step in its max-product form (ccvpe_amd.tracking.viterbi_step_spec is the specification): the sums of the
    predict become maxima, P[y,x] = max_i ky max_j kx prior[y - oy - i, x - ox - j]; the measure, the normalisation by the
    map's SUM, the reset rules and the 14 columns are belief_step's (SURVIVED = sum P).  The forward pass of the most likely
    path (tracking.MostLikelyPath).  Every argument, every check and the return value are belief_step's."""
    return _belief_step("belief_viterbi_step", [(prior, "prior"), (heatmap, "heatmap")], ori, offsets, _OFFSETS, taps, outlier,
                        (reset, "reset"), [(post, "post")], scratch, out)


def belief_backtrack(deltas, ori, offsets, taps, rows, reset=None, out=None):
    """The most likely path of every track over a whole drive in ONE launch (ccvpe_amd.tracking.backtrack_spec is the
    specification): deltas [T,B,1,h,w] or [T,B,h,w] the posts of a belief_viterbi_step forward pass, ori [T,B,2,h,w], offsets
    [T,B,2] int32 and taps [T,B,2,2R+1] the motion INTO each frame, rows [T,B,14] float64 the forward rows, reset [T,B] int32 or
    None (frame 0 always starts a segment).  out: a caller's [T,B,8] float64 tensor.
    Returns path [T,B,8] float64 — columns ccvpe_amd.tracking.PATH_Y ... PATH_SCORE."""
    lib = _lib.load()
    for t, nm in ((deltas, "deltas"), (ori, "ori"), (taps, "taps")):
        _chk(t, nm)
    _chk(offsets, "offsets", torch.int32)
    _chk(reset, "reset", torch.int32)
    for t, nm in ((rows, "rows"), (out, "out")):
        _chk(t, nm, torch.float64)
    if deltas.dim() == 5 and deltas.shape[2] == 1:
        deltas = deltas.reshape(deltas.shape[0], deltas.shape[1], deltas.shape[3], deltas.shape[4])
    if deltas.dim() != 4:
        raise ValueError("belief_backtrack: deltas [T,B,h,w] or [T,B,1,h,w] expected, got %s" % (tuple(deltas.shape),))
    n, b, h, w = deltas.shape
    if tuple(ori.shape) != (n, b, 2, h, w):
        raise ValueError("belief_backtrack: ori must be [%d,%d,2,%d,%d], got %s" % (n, b, h, w, tuple(ori.shape)))
    if taps.dim() != 4 or tuple(taps.shape[:3]) != (n, b, 2) or taps.shape[3] % 2 != 1:
        raise ValueError("belief_backtrack: taps must be [%d,%d,2,2R+1], got %s" % (n, b, tuple(taps.shape)))
    radius = (taps.shape[3] - 1) // 2
    if tuple(offsets.shape) != (n, b, 2):
        raise ValueError("belief_backtrack: offsets must be [%d,%d,2], got %s" % (n, b, tuple(offsets.shape)))
    if tuple(rows.shape) != (n, b, 14):
        raise ValueError("belief_backtrack: rows must be [%d,%d,14], got %s" % (n, b, tuple(rows.shape)))
    if reset is not None and tuple(reset.shape) != (n, b):
        raise ValueError("belief_backtrack: reset must be [%d,%d], got %s" % (n, b, tuple(reset.shape)))
    if out is None:
        out = _empty((n, b, 8), device=deltas.device, dtype=torch.float64)
    elif tuple(out.shape) != (n, b, 8):
        raise ValueError("belief_backtrack: out must be [%d,%d,8], got %s" % (n, b, tuple(out.shape)))
    check(lib.ccvpe_belief_backtrack_f32(_ptr(deltas), _ptr(ori), _ptr(offsets), _ptr(taps), radius, _ptr(rows), _ptr(reset),
                                         _ptr(out), n, b, h, w, _stream()), "ccvpe_belief_backtrack_f32")
    return out


_OFFSETS, _MOTION = ("offsets", torch.int32, 2), ("motion", torch.float64, 6)       # a step's move: name, dtype, columns


def _belief_step(who, ins, ori, move, move_spec, taps, outlier, skip, outs, scratch, out):
    """The checks, the defaults and the call of the five step functions (entry point ccvpe_<who>_f32).  ins: the input maps as
    (tensor, name), heatmap among them, in the entry point's order; outs: the output maps likewise, None = allocated here;
    skip: (reset or cut, its name).  Returns (rows, the output maps last to first)."""
    lib, entry = _lib.load(), "ccvpe_%s_f32" % who
    others = dict((nm, t) for t, nm in ins)
    heatmap = others.pop("heatmap")
    for t, nm in ins + [(ori, "ori"), (taps, "taps")] + outs:
        _chk(t, nm)
    move_name, move_dtype, move_cols = move_spec
    _chk(move, move_name, move_dtype)
    _chk(skip[0], skip[1], torch.int32)
    for t, nm in ((scratch, "scratch"), (out, "out")):
        _chk(t, nm, torch.float64)
    if heatmap.dim() != 4 or heatmap.shape[1] != 1:
        raise ValueError("%s: heatmap [B,1,h,w] expected, got %s" % (who, tuple(heatmap.shape)))
    b, _, h, w = heatmap.shape
    if any(t.shape != heatmap.shape for t in others.values()) or ori.shape != (b, 2, h, w):
        raise ValueError("%s: %s [B,1,h,w] like heatmap and ori [B,2,h,w] expected" % (who, " and ".join(others)))
    if taps.dim() != 3 or taps.shape[0] != b or taps.shape[1] != 2 or taps.shape[2] % 2 != 1:
        raise ValueError("%s: taps must be [%d,2,2R+1], got %s" % (who, b, tuple(taps.shape)))
    radius = (taps.shape[2] - 1) // 2
    if tuple(move.shape) != (b, move_cols):
        raise ValueError("%s: %s must be [%d,%d], got %s" % (who, move_name, b, move_cols, tuple(move.shape)))
    if skip[0] is not None and skip[0].numel() != b:
        raise ValueError("%s: %s must hold one flag per track" % (who, skip[1]))
    need = b * belief_partials(h, w)
    if scratch is None:
        scratch = _empty((need,), device=heatmap.device, dtype=torch.float64)
    elif scratch.numel() < need:
        raise ValueError("%s: scratch holds %d doubles, %d needed" % (who, scratch.numel(), need))
    maps = []
    for t, nm in outs:
        if t is None:
            t = _empty(tuple(heatmap.shape), device=heatmap.device)
        elif t.shape != heatmap.shape:
            raise ValueError("%s: %s must be %s, got %s" % (who, nm, tuple(heatmap.shape), tuple(t.shape)))
        maps.append(t)
    if out is None:
        out = _empty((b, 14), device=heatmap.device, dtype=torch.float64)
    elif tuple(out.shape) != (b, 14):
        raise ValueError("%s: out must be [%d,14], got %s" % (who, b, tuple(out.shape)))
    args = [_ptr(t) for t, _ in ins] + [_ptr(ori), _ptr(move), _ptr(taps), radius, float(outlier), _ptr(skip[0])]
    check(getattr(lib, entry)(*(args + [_ptr(t) for t in maps] + [_ptr(scratch), _ptr(out), b, h, w, _stream()])), entry)
    return (out,) + tuple(reversed(maps))


def belief_smooth_step(beta, heatmap, alpha, ori, offsets, taps, outlier=0.0, cut=None, beta_out=None, smooth=None, scratch=None,
                       out=None):
    """One backward step of the forward-backward smoother per track on the device (two launches;
    ccvpe_amd.tracking.smooth_step_spec is the specification), for the pair of frames (s, t = s + 1): beta [B,1,h,w] the
    backward message of frame t (any positive scale), heatmap [B,1,h,w] of frame t, alpha [B,1,h,w] the filter's posterior of
    frame s, ori [B,2,h,w] of frame s; offsets [B,2] int32 and taps [B,2,2R+1] the FORWARD step's own of frame t — the kernel
    applies the predict's adjoint (offsets the other way, taps reversed) itself.  cut [B] int32 or None: a non-zero entry marks
    frame s as the last of its segment (frame t is a start, a filter reset, or does not exist): its smoothed belief is alpha
    and the message restarts uniform.  beta_out, smooth: a caller's [B,1,h,w] tensors that overlap neither each other nor an
    input; scratch: B * belief_partials(h, w) float64; out: a caller's [B,14] float64 slice.
    Returns (rows [B,14] float64 — the columns of belief_step for the smoothed belief, RESET = the state, SURVIVED = sum B',
    smooth, beta_out)."""
    return _belief_step("belief_smooth_step", [(beta, "beta"), (heatmap, "heatmap"), (alpha, "alpha")], ori, offsets, _OFFSETS, taps,
                        outlier, (cut, "cut"), [(beta_out, "beta_out"), (smooth, "smooth")], scratch, out)


def belief_smooth_step_rigid(beta, heatmap, alpha, ori, motion, taps, outlier=0.0, cut=None, beta_out=None, smooth=None,
                             scratch=None, out=None):
    """belief_smooth_step for a rigid motion of the grid (ccvpe_amd.tracking.smooth_step_rigid_spec is the specification):
    `motion` [B,6] float64 on the device is the FORWARD rigid step's own rows of frame t (tracking.rigid_motion,
    tracking.kitti_motions); the kernel inverts them (tracking.invert_motion) and resamples M beta along the reverse motion
    before the reversed-tap blur.  Not the exact adjoint of the rigid predict — a bilinear gather's adjoint is a scatter — but
    the same continuous model discretised the other way; equal to belief_smooth_step for angle 0 or quarter turns with
    whole-pixel shifts.  Every other argument, every check and the return value are belief_smooth_step's."""
    return _belief_step("belief_smooth_step_rigid", [(beta, "beta"), (heatmap, "heatmap"), (alpha, "alpha")], ori, motion, _MOTION,
                        taps, outlier, (cut, "cut"), [(beta_out, "beta_out"), (smooth, "smooth")], scratch, out)


def _loss_common(fn, name, tensors, extra):
    lib = _lib.load()
    for i, t in enumerate(tensors):
        _chk(t, "%s arg %d" % (name, i))
    b = tensors[0].shape[0]
    loss = _empty((1,), device=tensors[0].device, dtype=torch.float32)
    scratch = _empty((2 * b,), device=tensors[0].device, dtype=torch.float32)
    return lib, loss, scratch, b


def infonce_loss(scores, labels, temperature=0.1, want_den=False, want_rows=False):
    """losses.py:4 infoNCELoss — forward value only (device scalar).  want_den: also return the batch's label mass
    sum(labels > 1e-2) (the loss's denominator, losses.py:18); want_rows: also return the per-sample statistics
    [4*B + 4] the backward kernel reads (ccvpe_infonce_loss_bwd_f32)."""
    lib = _lib.load()
    _chk(scores, "infonce scores")
    _chk(labels, "infonce labels")
    b, n = scores.shape
    loss = _empty((1,), device=scores.device, dtype=torch.float32)
    rows = _empty((4 * b + 4,), device=scores.device, dtype=torch.float32)
    nfl = lib.ccvpe_infonce_scratch_floats(b, n)
    if nfl <= 0:
        raise _lib.CcvpeError("ccvpe_infonce_scratch_floats rejected [%d, %d]" % (b, n))
    scratch = _empty((nfl,), device=scores.device, dtype=torch.float32)
    check(lib.ccvpe_infonce_loss_f32(_ptr(scores), _ptr(labels), float(temperature), _ptr(loss), _ptr(rows), _ptr(scratch),
                                     b, n, _stream()), "ccvpe_infonce_loss_f32")
    out = (loss[0],)
    if want_den:
        out = out + (rows[4 * b],)
    if want_rows:
        out = out + (rows,)
    return out if len(out) > 1 else out[0]


def cross_entropy_loss(logits, labels):
    """losses.py:23 cross_entropy_loss — forward value only."""
    lib, loss, scratch, b = _loss_common(None, "ce", (logits, labels), None)
    check(lib.ccvpe_cross_entropy_loss_f32(_ptr(logits), _ptr(labels), _ptr(loss), _ptr(scratch), b,
                                           logits.shape[1], _stream()), "ccvpe_cross_entropy_loss_f32")
    return loss[0]


def orientation_loss(ori, gt_orientation, gt):
    """losses.py:28 orientation_loss — forward value only.  ori/gt_orientation [B,2,H,W], gt [B,1,H,W]."""
    lib, loss, scratch, b = _loss_common(None, "ori", (ori, gt_orientation, gt), None)
    hw = ori.shape[2] * ori.shape[3]
    check(lib.ccvpe_orientation_loss_f32(_ptr(ori), _ptr(gt_orientation), _ptr(gt), _ptr(loss), _ptr(scratch),
                                         b, hw, _stream()), "ccvpe_orientation_loss_f32")
    return loss[0]
