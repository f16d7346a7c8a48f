// Generic implicit-GEMM gather kernel (1x1 with gather features, 2x2/s2, deconv-as-GEMM, split-K) and the dispatcher of
// ccvpe_conv_igemm_*: the pointwise / 3x3 / folded-deconv kernels live in conv_pw_*.hip, conv3x3_*.hip, upconv_*.hip.
// Shared machinery and the design notes: conv_common.h.
#include "conv_common.h"

namespace ccvpe {

template <typename T, int MT, int NT, int WN>
__global__ __launch_bounds__(256) void igemm_kernel(const IgemmParams p) {
  constexpr int E = ElemTraits<T>::E;      // elements per 16-byte load
  constexpr int SK = 4 * E;                // K elements per stage row (64 bytes)
  constexpr int CPS = SK / 8;              // 8-channel chunks per stage: 2 (fp32) or 4 (bf16)
  constexpr int WM = 4 / WN;
  constexpr int BM = 16 * MT * WM;
  constexpr int BN = 16 * NT * WN;
  constexpr int A_IT = BM / 64;            // float4 loads per thread per stage (A)
  constexpr int B_IT = (BN + 63) / 64;     // float4 loads per thread per stage (W)

  constexpr bool SWZ = PanelLayout<T>::SWZ;     // bf16: unpadded, XOR-swizzled panels (conv_common.h)
  constexpr int PLD = PanelLayout<T>::LD;
  __shared__ __attribute__((aligned(16))) float As[2][BM][PLD];
  __shared__ __attribute__((aligned(16))) float Bs[2][BN][PLD];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN;
  const int wn = wave % WN;

  const int tile = xcd_tile(blockIdx.x, p.tiles_total);
  const int tm = tile / p.tiles_n;
  const int tn = tile % p.tiles_n;
  const int m0 = tm * BM;
  const int n0 = tn * BN;

  // ---- per-thread staging coordinates -------------------------------------------------------
  const int srow = tid >> 2;   // 0..63
  const int ssub = tid & 3;    // which 16-byte piece of the 64-byte stage row
  const int scol = (SWZ ? (ssub ^ panel_swz(srow)) : ssub) * 4;       // staged piece -> (swizzled) float column
  const int chunk_in_stage = (ssub * E) >> 3;      // fp32: ssub>>1, bf16: ssub
  const int half = (ssub * E) & 7;                 // channel offset inside the 8-chunk: fp32 0|4, bf16 0
  const T* src0 = reinterpret_cast<const T*>(p.src0);
  const T* src1 = reinterpret_cast<const T*>(p.src1);
  const T* wp = reinterpret_cast<const T*>(p.w);

  int a_b[A_IT], a_y[A_IT], a_x[A_IT];
  bool a_ok[A_IT];
#pragma unroll
  for (int it = 0; it < A_IT; ++it) {
    const int m = m0 + srow + 64 * it;
    a_ok[it] = m < p.M;
    const int mm = a_ok[it] ? m : 0;
    const int hw = p.Ho * p.Wo;
    const int b = mm / hw;
    const int rem = mm - b * hw;
    const int oy = rem / p.Wo;
    const int ox = rem - oy * p.Wo;
    a_b[it] = b;
    a_y[it] = oy * p.stride - p.pad;
    a_x[it] = ox * p.stride - p.pad;
  }
  // chunk cursor of this thread: kc = CPS*stage + chunk_in_stage, decoded as (ky, kx, r)
  const int s_begin = p.ksplit > 1 ? blockIdx.y * p.sps : 0;
  const int s_end = p.ksplit > 1 ? min(p.stages, s_begin + p.sps) : p.stages;
  int kc = CPS * s_begin + chunk_in_stage;
  int r, ky, kx;
  {
    const int tap = kc / p.cpt;
    r = kc - tap * p.cpt;
    ky = tap / p.kw;
    kx = tap - ky * p.kw;
  }

  f32x4 a_reg[A_IT], b_reg[B_IT];
  // byte offset of this lane's 16-byte piece inside W, per staged row (rows past the tile / Npad: any valid row, never
  // stored): stage-invariant, so a W request is (scalar base + stage offset) + this register — no vector ALU work per stage
  unsigned wrow[B_IT];
#pragma unroll
  for (int it = 0; it < B_IT; ++it)
    wrow[it] = ((unsigned)min(n0 + srow + 64 * it, p.Npad - 1) * (unsigned)p.Kpad + (unsigned)(ssub * E)) * (unsigned)sizeof(T);
  unsigned a_keep = 0;                      // bit `it`: piece `it` of the stage in a_reg is inside the image and the K range
  f32x4 g_r0 = {0.f, 0.f, 0.f, 0.f}, g_r1 = g_r0;   // SE gate of the FIRST staged row's sample (rows of a tile nearly always share it)
  int g_ch = 0;                             // channel of the staged piece, for the rare rows of another sample
  const bool gated = p.gate != nullptr;     // (1x1, single-source convs only)
  const int ld0s = sgpr(p.ld0), ld1s = sgpr(p.ld1);
  // both sources below 4 GB (workgroup-uniform): 32-bit byte offsets, one v_mad per piece instead of 64-bit multiply-adds
  const bool small32 = (double)p.in_pixels * (double)(ld0s > ld1s ? ld0s : ld1s) * sizeof(T) < 4294967296.0;

  auto load_stage = [&](int s) {
    const bool kvalid = kc < p.total_chunks;
    const bool from0 = !kvalid || r < p.cpt0;
    const T* base = from0 ? src0 : src1;
    const int ld = from0 ? ld0s : ld1s;
    const int ch = kvalid ? (from0 ? r : r - p.cpt0) * 8 + half : 0;
    a_keep = 0;
#pragma unroll
    for (int it = 0; it < A_IT; ++it) {
      const int iy = a_y[it] + ky;
      const int ix = a_x[it] + kx;
      const bool ok = a_ok[it] && kvalid && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
      const int pix = ok ? (a_b[it] * p.H + iy) * p.W + ix : 0;
      if (small32) a_reg[it] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(base) + ((unsigned)pix * (unsigned)ld + (unsigned)ch) * (unsigned)sizeof(T));
      else a_reg[it] = *reinterpret_cast<const f32x4*>(base + (size_t)pix * ld + ch);
      a_keep |= ok ? (1u << it) : 0u;
    }
    if (gated) {
      g_ch = ch;
      gate_load<T>(p.gate + (size_t)a_b[0] * p.c0 + ch, g_r0, g_r1);
    }
    {
      const char* wb = reinterpret_cast<const char*>(wp) + (size_t)s * (SK * sizeof(T));   // scalar base + per-lane row offset
#pragma unroll
      for (int it = 0; it < B_IT; ++it) b_reg[it] = *reinterpret_cast<const f32x4*>(wb + wrow[it]);
    }
    kc += CPS;
    r += CPS;
    while (r >= p.cpt) {
      r -= p.cpt;
      if (++kx == p.kw) { kx = 0; ++ky; }
    }
  };

  auto store_stage = [&](int buf) {
#pragma unroll
    for (int it = 0; it < A_IT; ++it) {
      f32x4 v = a_reg[it];
      if (gated) {
        if (a_b[it] == a_b[0]) v = gate_apply<T>(v, g_r0, g_r1);
        else v = apply_gate<T>(v, p.gate + (size_t)a_b[it] * p.c0 + g_ch);
      }
      *reinterpret_cast<f32x4*>(&As[buf][srow + 64 * it][scol]) = keep_if(v, (a_keep >> it) & 1u);
    }
#pragma unroll
    for (int it = 0; it < B_IT; ++it) {
      const int nrow = srow + 64 * it;
      if (nrow < BN) *reinterpret_cast<f32x4*>(&Bs[buf][nrow][scol]) = b_reg[it];
    }
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15;
  const int fk = (SWZ ? ((lane >> 4) ^ panel_swz(frow)) : (lane >> 4)) * 4;

  load_stage(s_begin);
  store_stage(0);
  __syncthreads();

  for (int s = s_begin; s < s_end; ++s) {
    const int buf = (s - s_begin) & 1;
    const bool more = s + 1 < s_end;
    if (more) load_stage(s + 1);

    f32x4 af[MT], bf[NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
      af[i] = *reinterpret_cast<const f32x4*>(&As[buf][(wm * MT + i) * 16 + frow][fk]);
#pragma unroll
    for (int j = 0; j < NT; ++j)
      bf[j] = *reinterpret_cast<const f32x4*>(&Bs[buf][(wn * NT + j) * 16 + frow][fk]);
    if (sizeof(T) == 4) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[j][kk], af[i][kk], acc[i][j], 0, 0, 0);
    } else {
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = mfma_stage<T>(bf[j], af[i], acc[i][j]);
    }

    if (more) store_stage(buf ^ 1);
    __syncthreads();
  }

  // ---- epilogue: swapped roles => D rows = channels ((lane>>4)*4 + reg), D cols = pixels (lane&15)
  const int epix = lane & 15;
  const int en = (lane >> 4) * 4;
  if (p.ksplit > 1) {      // raw partial sums; the epilogue runs in splitk_finish_kernel
    float* part = p.partial + (size_t)blockIdx.y * p.M * p.Npad;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int m = m0 + (wm * MT + i) * 16 + epix;
      if (m >= p.M) continue;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int n = n0 + (wn * NT + j) * 16 + en;
        if (n < p.Npad) *reinterpret_cast<f32x4*>(part + (size_t)m * p.Npad + n) = acc[i][j];
      }
    }
    return;
  }
  float sc[NT][4], sh[NT][4];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = n0 + (wn * NT + j) * 16 + en + q;
      const bool ok = n < p.N;
      sc[j][q] = (ok && p.scale) ? p.scale[n] : 1.0f;
      sh[j][q] = (ok && p.shift) ? p.shift[n] : 0.0f;
    }
  auto epilogue = [&](auto act_tag) {
  constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int m = m0 + (wm * MT + i) * 16 + epix;
    if (m >= p.M) continue;
    size_t pbase = 0;
    if (p.out_mode == CCVPE_OUT_DECONV2X) {
      const int hw = p.Ho * p.Wo;
      const int b = m / hw;
      const int rem = m - b * hw;
      const int y = rem / p.Wo;
      const int x = rem - y * p.Wo;
      pbase = ((size_t)(b * 2 * p.Ho + 2 * y) * (2 * p.Wo) + 2 * x) * p.ldd;
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = n0 + (wn * NT + j) * 16 + en;
      if (n >= p.N) continue;
      size_t obase;
      if (p.out_mode == CCVPE_OUT_NHWC) {
        obase = (size_t)m * p.ldd + n;
      } else {
        const int quad = n / p.cout;
        const int co = n - quad * p.cout;
        obase = pbase + ((size_t)(quad >> 1) * (2 * p.Wo) + (quad & 1)) * p.ldd + co;
      }
      store4<T, ACT>(p, acc[i][j], n, obase, (size_t)m * p.ldres, sc[j], sh[j]);
    }
  }
  };
  CCVPE_ACT_DISPATCH(p.act, epilogue);
}

// split-K second pass: thread = (pixel m, 4 channels); adds the K slices in index order (deterministic) and applies
// the same epilogue as the one-pass kernel (scale/shift, activation, residual, NHWC or pixel-shuffle addressing)
template <typename T>
__global__ __launch_bounds__(256) void splitk_finish_kernel(const IgemmParams p) {
  const int n4 = p.Npad >> 2;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)p.M * n4) return;
  const int m = (int)(idx / n4);
  const int n = (int)(idx - (long)m * n4) * 4;
  if (n >= p.N) return;
  f32x4 v = *reinterpret_cast<const f32x4*>(p.partial + (size_t)m * p.Npad + n);
  for (int k = 1; k < p.ksplit; ++k) v += *reinterpret_cast<const f32x4*>(p.partial + ((size_t)k * p.M + m) * p.Npad + n);
  float sc[4], sh[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const bool ok = n + q < p.N;
    sc[q] = (ok && p.scale) ? p.scale[n + q] : 1.0f;
    sh[q] = (ok && p.shift) ? p.shift[n + q] : 0.0f;
  }
  size_t obase;
  if (p.out_mode == CCVPE_OUT_NHWC) {
    obase = (size_t)m * p.ldd + n;
  } else {
    const int hw = p.Ho * p.Wo;
    const int b = m / hw;
    const int rem = m - b * hw;
    const int y = rem / p.Wo;
    const int x = rem - y * p.Wo;
    const size_t pbase = ((size_t)(b * 2 * p.Ho + 2 * y) * (2 * p.Wo) + 2 * x) * p.ldd;
    const int quad = n / p.cout;
    const int co = n - quad * p.cout;
    obase = pbase + ((size_t)(quad >> 1) * (2 * p.Wo) + (quad & 1)) * p.ldd + co;
  }
  auto fin = [&](auto act_tag) { store4<T, decltype(act_tag)::value>(p, v, n, obase, (size_t)m * p.ldres, sc, sh); };
  CCVPE_ACT_DISPATCH(p.act, fin);
}

// K slices for a GEMM with `tiles` workgroups and `stages` K stages (1 = no split): only when the launch cannot fill
// the 256 CUs and the serial K walk is long; each slice keeps >= 12 stages
static int splitk_slices(int tiles, int stages) {
  if (tiles >= 320 || stages < 24) return 1;
  int s = (640 + tiles - 1) / tiles;
  if (s > stages / 12) s = stages / 12;
  if (s > 32) s = 32;
  return s < 2 ? 1 : s;
}

template <typename T, int MT, int NT, int WN>
static int launch(const IgemmParams& p0, hipStream_t stream, float* scratch) {
  constexpr int BM = 16 * MT * (4 / WN), BN = 16 * NT * WN;
  IgemmParams p = p0;
  p.tiles_n = (p.Npad + BN - 1) / BN;
  p.tiles_total = ((p.M + BM - 1) / BM) * p.tiles_n;
  p.ksplit = 1; p.sps = p.stages; p.partial = nullptr;
  const int S = scratch ? splitk_slices(p.tiles_total, p.stages) : 1;      // (splitk_want: the same question at planning time)
  if (S > 1) {
    p.sps = (p.stages + S - 1) / S;
    p.ksplit = (p.stages + p.sps - 1) / p.sps;
    p.partial = scratch;
    hipLaunchKernelGGL((igemm_kernel<T, MT, NT, WN>), dim3(p.tiles_total, p.ksplit), dim3(256), 0, stream, p);
    const long n = (long)p.M * (p.Npad / 4);
    hipLaunchKernelGGL((splitk_finish_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p);
    return check_launch("igemm_kernel (split-K)");
  }
  hipLaunchKernelGGL((igemm_kernel<T, MT, NT, WN>), dim3(p.tiles_total), dim3(256), 0, stream, p);
  return check_launch("igemm_kernel");
}

template <typename T>
static int igemm_dispatch(const IgemmParams& p, TileCfg c, hipStream_t stream, float* scratch) {
#define CCVPE_CASE(MT_, NT_, WN_) \
  if (c.mt == MT_ && c.nt == NT_ && c.wn == WN_) return launch<T, MT_, NT_, WN_>(p, stream, scratch);
  CCVPE_TILES(CCVPE_CASE)
#undef CCVPE_CASE
  return fail(CCVPE_EINVAL, "conv_igemm: no tile config");
}

}  // namespace ccvpe

using namespace ccvpe;

#ifdef CCVPE_ABLATE   // diagnostics build only: CCVPE_PW_GEMM=0 routes the pointwise convs through the generic kernel again
static const bool g_use_pw = !(getenv("CCVPE_PW_GEMM") && getenv("CCVPE_PW_GEMM")[0] == '0');
#else
constexpr bool g_use_pw = true;
#endif
// CCVPE_NARROW=0 (any build: an A/B switch kept for the evidence runs) sends the narrow 3x3 layers back to conv3x3_kernel
namespace ccvpe { bool g_use_narrow = true; }
extern "C" int ccvpe_set_narrow_kernels(int on) {
  const int prev = ccvpe::g_use_narrow ? 1 : 0;
  ccvpe::g_use_narrow = on != 0;
  return prev;
}

// the same kind of switch for the fp32 pointwise ring kernel (csrc/conv_pw2_f32.hip)
namespace ccvpe { bool g_use_pw2 = true; }
extern "C" int ccvpe_set_pw_ring_kernels(int on) {
  const int prev = ccvpe::g_use_pw2 ? 1 : 0;
  ccvpe::g_use_pw2 = on != 0;
  return prev;
}

// Validates `d` and fills the kernels' parameter block; every entry point below starts here.
template <typename T>
static int fill_params(const ccvpe_conv_desc* d, int out_f32, IgemmParams& p) {
  constexpr int E = ElemTraits<T>::E;
  constexpr int SK = 4 * E;
  if (!d) return fail(CCVPE_EINVAL, "conv_igemm: null desc");
  if (d->c0 <= 0 || d->c0 % 8 || d->c1 < 0 || d->c1 % 8)
    return fail(CCVPE_EINVAL, "conv_igemm: c0/c1 must be multiples of 8 (got %d,%d)", d->c0, d->c1);
  if (d->c1 > 0 && !d->src1) return fail(CCVPE_EINVAL, "conv_igemm: c1>0 but src1 null");
  if (d->ld0 % E || (d->c1 && d->ld1 % E) || d->kpad % SK || d->ldd % 4 || (d->residual && d->ldres % 4))
    return fail(CCVPE_EINVAL, "conv_igemm: ld0/ld1 %% %d, kpad %% %d, ldd/ldres %% 4 required", E, SK);
  if (!aligned16(d->src0) || (d->src1 && !aligned16(d->src1)) || !aligned16(d->w) ||
      (d->gate && !aligned16(d->gate)) || !aligned16(d->dst) || (d->residual && !aligned16(d->residual)))
    return fail(CCVPE_EINVAL, "conv_igemm: pointers must be 16-byte aligned");
  if (d->gate && (d->kh != 1 || d->c1 != 0)) return fail(CCVPE_EINVAL, "conv_igemm: gate only for 1x1 single-source");
  if (d->stride < 1 || d->kh < 1 || d->kw < 1) return fail(CCVPE_EINVAL, "conv_igemm: bad kernel/stride");
  if (d->act == CCVPE_ACT_RELU_MASK && (!d->residual || d->out_mode != CCVPE_OUT_NHWC))
    return fail(CCVPE_EINVAL, "conv_igemm: CCVPE_ACT_RELU_MASK needs the ReLU output in `residual` and an NHWC store");
  p = IgemmParams{};
  p.src0 = d->src0; p.src1 = d->src1; p.gate = d->gate; p.w = d->w;
  p.scale = d->scale; p.shift = d->shift; p.residual = d->residual; p.dst = d->dst;
  p.out_f32 = out_f32;
  p.c0 = d->c0; p.ld0 = d->ld0; p.c1 = d->c1; p.ld1 = d->ld1;
  p.H = d->in_h; p.W = d->in_w;
  p.in_pixels = (long)d->batch * d->in_h * d->in_w;
  p.Ho = (d->in_h + 2 * d->pad - d->kh) / d->stride + 1;
  p.Wo = (d->in_w + 2 * d->pad - d->kw) / d->stride + 1;
  p.kw = d->kw; p.stride = d->stride; p.pad = d->pad;
  p.N = d->n; p.Kpad = d->kpad; p.Npad = (d->n + 15) / 16 * 16;
  p.cpt0 = d->c0 / 8; p.cpt = (d->c0 + d->c1) / 8;
  p.total_chunks = p.cpt * d->kh * d->kw;
  if (p.total_chunks * 8 > p.Kpad) return fail(CCVPE_EINVAL, "conv_igemm: kpad %d < K %d", p.Kpad, p.total_chunks * 8);
  constexpr int CPS = SK / 8;
  p.stages = (p.total_chunks + CPS - 1) / CPS;
  p.ldd = d->ldd; p.ldres = d->ldres; p.act = d->act; p.out_mode = d->out_mode;
  p.cout = (d->out_mode == CCVPE_OUT_DECONV2X) ? d->n / 4 : d->n;
  if (d->out_mode == CCVPE_OUT_DECONV2X && (d->n % 16 || d->residual))
    return fail(CCVPE_EINVAL, "conv_igemm: deconv mode needs cout%%4==0 and no residual");
  const long M = (long)d->batch * p.Ho * p.Wo;
  if (M <= 0 || M > 0x7fffffffL) return fail(CCVPE_EINVAL, "conv_igemm: bad M");
  if ((long)d->batch * d->in_h * d->in_w > 0x7fffffffL) return fail(CCVPE_EINVAL, "conv_igemm: too many pixels");
  p.M = (int)M;
  return CCVPE_OK;
}

// ---- the route: which kernel family and tile serve a layer.  pick_route() alone knows the order of the families; the launch,
// ccvpe_conv_igemm_route / ccvpe_conv3x3_variant (tests and bench.py's launch recorder read them instead of mirroring the rules
// in Python) and the split-K planner go through it or through its predicates
struct ConvRoute { int fam, mt, nt, wn; };      // fam: CCVPE_ROUTE_*; the ABI's encoding is fam | mt << 8 | nt << 12 | wn << 16

static bool is3x3(const ccvpe_conv_desc* d) {
  return d->kh == 3 && d->kw == 3 && d->stride == 1 && d->pad == 1 && d->out_mode == CCVPE_OUT_NHWC && !d->gate;
}
// pointwise convs (1x1, stride 1, one source, plain NHWC store) take the deep-stage kernels; the residual / bf16 rows
// they touch with 16-byte accesses must be 16-byte aligned along the channel axis
template <typename T>
static bool is_pw(const ccvpe_conv_desc* d, const IgemmParams& p) {
  const int esz = (int)sizeof(T);
  const bool out32 = esz == 4 || p.out_f32;
  return g_use_pw && d->kh == 1 && d->kw == 1 && d->stride == 1 && d->pad == 0 && d->c1 == 0 &&
         d->act != CCVPE_ACT_RELU && d->act != CCVPE_ACT_RELU_MASK &&
         d->n > 48 &&      // narrow outputs (N <= 48: 16-48 column tiles) stay with the generic kernel
         d->out_mode == CCVPE_OUT_NHWC && (d->ldd * (out32 ? 4 : 2)) % 16 == 0 &&
         (!d->residual || (d->ldres * esz) % 16 == 0);
}
// the tile the pointwise kernels run where the table says `c` (nt == 0: none, `c` is no wider than 48 columns).  The 256 x 80 tile
// needs more than 256 VGPRs there (staging registers live across the epilogue): N = 65..80 layers take the 128 x 96 tile.
static TileCfg pw_tile(int mt, int nt, int wn) {
  if (16 * nt * wn <= 48) return TileCfg{0, 0, 0};
  if (mt == 4 && nt == 5 && wn == 1) return TileCfg{4, 3, 2};
  return TileCfg{mt, nt, wn};
}

// one-pass route of a validated layer (a split-K run is the generic kernel by definition)
template <typename T>
static ConvRoute pick_route(const ccvpe_conv_desc* d, const IgemmParams& p) {
  const int esz = (int)sizeof(T);
  // N <= 48, K <= 256 (fp32: 144) projections on large planes: weights (x SE gate) in registers; tile fields = N / 16, K bytes / 64
  if (pwn_supported(p, d->batch, esz)) return ConvRoute{CCVPE_ROUTE_PWN, p.Npad / 16, (p.Kpad * esz) / 64, 0};
  const TileCfg c = kCfgs[pick_cfg(p.Npad)];
  if (is3x3(d)) {
    if (esz == 2 && g_use_narrow && c3n_supported(p, d->batch)) return ConvRoute{CCVPE_ROUTE_C3N, c.mt, c.nt, c.wn};
    return ConvRoute{CCVPE_ROUTE_CONV3X3, c.mt, c.nt, c.wn};
  }
  const TileCfg t = pw_tile(c.mt, c.nt, c.wn);
  if (t.nt && is_pw<T>(d, p))
    return ConvRoute{pw2_supported<T>(p, t.mt, t.nt, t.wn) ? CCVPE_ROUTE_PW_RING : CCVPE_ROUTE_PW_GEMM, t.mt, t.nt, t.wn};
  return ConvRoute{CCVPE_ROUTE_IGEMM, c.mt, c.nt, c.wn};
}

// planning: the fp32 scratch words a split-K run needs, 0 = one pass.  Two bf16 "do not split" rules, else the generic kernel's
// own answer (also for a layer pwn_supported() would serve: planning does not consult that kernel)
template <typename T>
static long splitk_want(const ccvpe_conv_desc* d, const IgemmParams& p) {
  const TileCfg c = kCfgs[pick_cfg(p.Npad)];
  // bf16 3x3 on images >= 16 columns wide with at least 128 halo tiles: the LDS-DMA 3x3 kernel UN-split beats the split-K gather
  // kernel + its second pass (tools/conv3_probe.py bf16, 16 x 16 images: B = 32 257 -> 166 us at 1344 -> 640 and 140 -> 82 us at
  // 640 -> 640, B = 16 equal, B = 8 slower).  fp32 keeps the split (its 3x3 kernel needs two workgroups per CU to cover its latencies)
  if (sizeof(T) == 2 && is3x3(d) && p.W >= 16) {
    const int th = c.mt * (4 / c.wn), bn = 16 * c.nt * c.wn;
    const long tiles = (long)d->batch * ((p.H + th - 1) / th) * ((p.W + 15) / 16) * ((p.Npad + bn - 1) / bn);
    if (tiles >= 128) return 0;
  }
  // bf16 1x1 layers the ring / pointwise kernels take, with >= 200 of their tiles (B = 64: the late MBConv projections 1152 -> 192
  // / 320 at 16 x 16 and 10 x 20): one pass beats the split gather kernel + its second pass there (round 6, same-box A/B of the
  // C1 forward: 8.94 -> 8.87 ms; at B = 32 — 100-128 tiles — the split still wins: C2 5.17 vs 5.25 ms)
  const TileCfg t = pw_tile(c.mt, c.nt, c.wn);
  if (sizeof(T) == 2 && t.nt && is_pw<T>(d, p)) {
    const int bm = 16 * t.mt * (4 / t.wn), bn = 16 * t.nt * t.wn;
    const long tiles = (long)((p.M + bm - 1) / bm) * ((p.Npad + bn - 1) / bn);
    if (tiles >= 200) return 0;
  }
  const int bm = 16 * c.mt * (4 / c.wn), bn = 16 * c.nt * c.wn;          // the generic kernel's grid: launch<T, MT, NT, WN> above
  const int S = splitk_slices(((p.M + bm - 1) / bm) * ((p.Npad + bn - 1) / bn), p.stages);
  return S > 1 ? (long)S * p.M * p.Npad : 0;
}

// ---- the entry points: fill_params + one of the pieces above.  conv_run with `scratch` is a split-K run: everything, 3x3
// included, goes through the generic gather kernel
template <typename T>
static int conv_run(const ccvpe_conv_desc* d, int out_f32, void* stream, float* scratch = nullptr) {
  IgemmParams p;
  if (const int rc = fill_params<T>(d, out_f32, p)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (scratch && !aligned16(scratch)) return fail(CCVPE_EINVAL, "conv_igemm: scratch must be 16-byte aligned");
  if (scratch) return igemm_dispatch<T>(p, kCfgs[pick_cfg(p.Npad)], st, scratch);
  const ConvRoute r = pick_route<T>(d, p);
  switch (r.fam) {
    case CCVPE_ROUTE_PWN: return pwn_dispatch(p, d->batch, (int)sizeof(T), st);
    case CCVPE_ROUTE_C3N: return c3n_dispatch(p, d->batch, st);
    case CCVPE_ROUTE_CONV3X3: return conv3x3_dispatch<T>(p, d->batch, r.mt, r.nt, r.wn, st);
    case CCVPE_ROUTE_PW_RING: return pw2_dispatch<T>(p, r.mt, r.nt, r.wn, st);
    case CCVPE_ROUTE_PW_GEMM: return pw_dispatch<T>(p, r.mt, r.nt, r.wn, st);
    default: return igemm_dispatch<T>(p, TileCfg{r.mt, r.nt, r.wn}, st, nullptr);
  }
}

// the route conv_run() would take or, with `variant`, the form of conv3x3_kernel behind it (0 for another family); no launch
template <typename T>
static int conv_route(const ccvpe_conv_desc* d, int out_f32, bool variant) {
  IgemmParams p;
  if (const int rc = fill_params<T>(d, out_f32, p)) return rc;
  const ConvRoute r = pick_route<T>(d, p);
  if (variant) return r.fam == CCVPE_ROUTE_CONV3X3 ? conv3x3_variant_query<T>(p, d->batch, r.mt, r.nt, r.wn) : 0;
  return r.fam | (r.mt << 8) | (r.nt << 12) | (r.wn << 16);
}

extern "C" int ccvpe_conv_igemm_splitk_floats(const ccvpe_conv_desc* d, int is_bf16) {
  IgemmParams p;
  const int rc = is_bf16 ? fill_params<bf16_t>(d, 0, p) : fill_params<float>(d, 0, p);
  const long want = rc ? rc : is_bf16 ? splitk_want<bf16_t>(d, p) : splitk_want<float>(d, p);
  return want > 0x7fffffffL ? 0 : (int)want;      // would not fit the int return: do not split
}
extern "C" int ccvpe_conv_igemm_route(const ccvpe_conv_desc* d, int is_bf16, int out_f32) {
  return is_bf16 ? conv_route<bf16_t>(d, out_f32 ? 1 : 0, false) : conv_route<float>(d, 1, false);
}
extern "C" int ccvpe_conv3x3_variant(const ccvpe_conv_desc* d, int is_bf16) {
  return is_bf16 ? conv_route<bf16_t>(d, 0, true) : conv_route<float>(d, 1, true);
}

// the next level's one-hypothesis matching fused into a bf16 3x3 layer's epilogue (narrow_impl.h): 1 = served, 0 = not, < 0 = bad desc
static int match1_served(const ccvpe_conv_desc* d, int out_f32, int L, IgemmParams& p) {
  if (const int rc = fill_params<bf16_t>(d, out_f32 ? 1 : 0, p)) return rc;
  return is3x3(d) && g_use_narrow && c3n_match_supported(p, d->batch, L) ? 1 : 0;
}
static int match1_offset(int n, int shift, int stride, int window_offset) {
  long o = (-((long)shift * stride + window_offset)) % n;      // match_any()'s offset (csrc/matching.hip)
  return (int)(o < 0 ? o + n : o);
}
extern "C" int ccvpe_conv3x3_match1_ok(const ccvpe_conv_desc* d, int out_f32, int L) {
  IgemmParams p;
  const int rc = match1_served(d, out_f32, L, p);
  return rc < 0 ? 0 : rc;
}
extern "C" int ccvpe_conv3x3_match1_bf16(const ccvpe_conv_desc* d, int out_f32, const float* g, int ldg, int L, int shift, int stride,
                                         int window_offset, float* scores, void* stream) {
  if (!d || !g || !scores) return fail(CCVPE_EINVAL, "conv3x3_match1: null pointer");
  if (L > ldg) return fail(CCVPE_EINVAL, "conv3x3_match1: L > ldg");
  IgemmParams p;
  const int ok = match1_served(d, out_f32, L, p);
  if (ok < 0) return ok;
  if (!ok) return fail(CCVPE_EINVAL, "conv3x3_match1: this layer / shape is not served (ask ccvpe_conv3x3_match1_ok first)");
  return c3n_match_dispatch(p, d->batch, g, ldg, L, match1_offset(d->n, shift, stride, window_offset), scores, (hipStream_t)stream);
}
extern "C" int ccvpe_conv_igemm_splitk_bf16(const ccvpe_conv_desc* d, int out_f32, float* scratch, void* stream) {
  if (!scratch) return fail(CCVPE_EINVAL, "conv_igemm_splitk: scratch is NULL");
  return conv_run<bf16_t>(d, out_f32, stream, scratch);
}
extern "C" int ccvpe_conv_igemm_splitk_f32(const ccvpe_conv_desc* d, float* scratch, void* stream) {
  if (!scratch) return fail(CCVPE_EINVAL, "conv_igemm_splitk: scratch is NULL");
  return conv_run<float>(d, 0, stream, scratch);
}
extern "C" int ccvpe_conv_igemm_f32(const ccvpe_conv_desc* d, void* stream) { return conv_run<float>(d, 1, stream); }
extern "C" int ccvpe_conv_igemm_bf16(const ccvpe_conv_desc* d, int out_f32, void* stream) {
  return conv_run<bf16_t>(d, out_f32 ? 1 : 0, stream);
}
