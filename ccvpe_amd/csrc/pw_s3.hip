// pw_s3_kernel: the fp32 1x1 GEMMs behind the depthwise stage of the two encoders (MBConv project, _conv_head) and the two descriptor
// heads, with their matrix arithmetic on the bf16 matrix cores at fp32-class accuracy:
//   D[m, n] = epilogue(sum_k (A[m, k] * gate[b(m), k]) * W[n, k])
// fp32 NHWC activations in, fp32 NHWC out.  The arithmetic convention is upconv_s3.hip's, exactly: the same split3 (hi / mid / lo,
// round-to-nearest, split3_impl.h), the same six products hh, hm, mh, mm, hl, lh as three v_mfma_f32_16x16x32_bf16 per 16-channel
// block, fp32 accumulation in the matrix unit.  The K loop is phase B of upconv_s3_kernel without the taps:
//   * A: one stage = 16 channels of BM rows, read as fp32, multiplied by the SE gate IN fp32 (as conv_igemm.hip: the gate is per
//     (sample, channel) and a tile may straddle samples, so it is fetched per row), split in registers on the way to LDS; rows are 96
//     bytes [hi|mid|lo], double-buffered.  A row is either a plain pixel (1x1) or, for the 2x2 stride-2 aerial descriptor, the four
//     taps of output pixel (oy, ox): k = (ky * 2 + kx) * c0 + ch reads input pixel (2 oy + ky, 2 ox + kx) — per input row two
//     adjacent pixels, i.e. one contiguous run of 2 c0 floats when ld0 == c0.  c0 % 16 == 0, so no stage straddles a tap.
//   * W: split ONCE on the host (models._pack_pw_s3), [stage = k / 16][Npad][hi 16 | mid 16 | lo 16] bf16.  A stage's panel is BN
//     contiguous 96-byte rows: HBM -> LDS by global_load_lds_dwordx4 as a linear copy, double-buffered, requested one stage ahead.
//   * LDS layout and fragment picking are upconv_s3.hip's (conflict-free ds_read_b128, tests/test_upconv_s3.py).
//   * Tiles: for N <= 320 the whole of N sits in ONE workgroup, so A is staged and split once; wider layers (N = 1280) tile N with
//     the 320-column tile.  Wave tiles reuse fragments: per stage a wave issues 2 MT + 3 NT ds_read_b128 for 3 MT NT matrix
//     instructions (10-25 reads for 12-42 instructions), away from the one-read-per-instruction LDS roof.  No K split: every launch
//     is one pass, sums are in a fixed order and results are bit-identical run to run (no atomics).
//   * What bounds it (tools/pw_s3_probe.py): a workgroup alone on the chip takes ~0.65-0.8 us per 16-channel stage whatever M is — the
//     serial chain of a stage (requests, LDS round trips of the fragments, split, LDS store, barrier), not the matrix pipe (12-42
//     instructions of 16 cycles) — so throughput comes from waves that overlap each other: 2-3 workgroups per CU on the
//     /16-resolution layers, and eight waves per workgroup where a 64-row tile leaves one workgroup per CU.  A variant that fetched A
//     and the gate by LDS-DMA too, three stages ahead with counted waits, had the same time per stage and one workgroup per CU; it
//     lost on the /16 layers and is not kept.
//   * Epilogue: conv_igemm.hip's store4 — folded BN scale / shift, activation, then the residual (own pitch); columns >= n are
//     never written.
// Non-finite and overflowing inputs behave as documented at the top of upconv_s3.hip (Inf splits into (Inf, NaN, NaN), |v| above
// 3.39e38 rounds hi to Inf, bf16-subnormal planes may be flushed by the matrix unit), here for A * gate.  The forward never produces
// such values.
#include "split3_impl.h"

namespace ccvpe {

struct PwS3Params {
  const float* src;
  const float* gate;
  const void* w;
  const float* scale;
  const float* shift;
  const float* residual;
  float* dst;
  int c0, ld0;           // channels per tap, row pitch of src
  int H, W, Ho, Wo, two; // source plane; output plane; two: the 2x2 stride-2 form (else one tap, Ho x Wo = H x W)
  int M, N, Npad, nst;   // nst = K / 16
  int ldd, ldres, act;
  int tiles_n, tiles_total;
};

template <int MT, int NT, int WN, int NW>
struct PwS3Geom {
  static constexpr int WM = NW / WN;
  static constexpr int BM = 16 * MT * WM;
  static constexpr int BN = 16 * NT * WN;
  static constexpr int ROW = S3_ROW;
  static constexpr int ASTG_DW = 2 * BM * ROW;                    // A stage [2][BM]
  static constexpr int W_INSTR = (BN * 6 + 63) / 64;               // wave-wide 1 KB DMA instructions per W panel
  static constexpr int WBUF_DW = W_INSTR * 256;
  static constexpr int LDS_BYTES = (ASTG_DW + 2 * WBUF_DW) * 4;
};

template <int MT, int NT, int WN, int NW>
__global__ __launch_bounds__(64 * NW, 2) void pw_s3_kernel(const PwS3Params p) {
  using G = PwS3Geom<MT, NT, WN, NW>;
  constexpr int BM = G::BM, BN = G::BN, ROW = G::ROW;
  constexpr int APASS = 16 * NW;                   // rows the workgroup's threads stage per pass (4 threads a row)
  constexpr int A_IT = (BM + APASS - 1) / APASS;
  constexpr int WQ = (G::W_INSTR + NW - 1) / NW;
  static_assert(BM % APASS == 0 || BM < APASS, "pw_s3_kernel: a stage is whole passes of the threads, or the first waves' share of one");

  extern __shared__ __attribute__((aligned(16))) float pw3_sm[];
  float* As = pw3_sm;                              // [2][BM][ROW]
  float* Ws = pw3_sm + G::ASTG_DW;                 // [2][W_INSTR * 256] by DMA: BN rows of ROW dwords

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = sgpr(tid >> 6);
  const int wm = wave / WN;
  const int wn = wave % WN;

  const int tile = xcd_tile(blockIdx.x, p.tiles_total);
  const int tn = tile % p.tiles_n;
  const int m0 = (tile / p.tiles_n) * BM;
  const int n0 = tn * BN;
  const int srow = tid >> 2, ssub = tid & 3;
  const int c0s = sgpr(p.c0), ld0s = sgpr(p.ld0);
  const bool gated = p.gate != nullptr;
  const bool a_on = BM >= APASS || wave * 16 < BM;      // (wave-uniform) the 8-wave tiles have 64 rows: waves 0-3 stage A

  // ---- A staging coordinates: byte offset of the row's first tap, gate row.  Rows past M re-read row M - 1 (valid memory; the
  // accumulator rows they feed are never stored and rows do not mix in the matrix unit)
  unsigned a_off[A_IT], g_off[A_IT];
#pragma unroll
  for (int it = 0; it < A_IT; ++it) {
    const int m = min(m0 + min(srow + APASS * it, BM - 1), p.M - 1);
    const int hw = p.Ho * p.Wo;
    const int b = m / hw;
    unsigned pix = (unsigned)m;
    if (p.two) {
      const int rem = m - b * hw;
      const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
      pix = (unsigned)((b * p.H + 2 * oy) * p.W + 2 * ox);
    }
    a_off[it] = (pix * (unsigned)ld0s + (unsigned)(ssub * 4)) * 4u;
    g_off[it] = ((unsigned)b * (unsigned)c0s + (unsigned)(ssub * 4)) * 4u;
  }
  // raw loads (STAGING RULE, conv_common.h): the gate is applied when the registers go to LDS
  f32x4 a_reg[A_IT], g_reg[A_IT];
  int tap = 0, ch0 = 0;                            // cursor of the NEXT load_a: workgroup-uniform
  auto load_a = [&]() {
    const unsigned koff = (unsigned)(((tap >> 1) * p.W + (tap & 1)) * ld0s + ch0) * 4u;
#pragma unroll
    for (int it = 0; it < A_IT && a_on; ++it) {
      a_reg[it] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(p.src) + (a_off[it] + koff));
      if (gated) g_reg[it] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(p.gate) + (g_off[it] + (unsigned)ch0 * 4u));
    }
    ch0 += 16;
    if (ch0 == c0s) { ch0 = 0; ++tap; }
  };
  auto store_a = [&](int buf) {
#pragma unroll
    for (int it = 0; it < A_IT && a_on; ++it)
      store_planes(As + (buf * BM + srow + APASS * it) * ROW + ssub * 2, gated ? a_reg[it] * g_reg[it] : a_reg[it]);
  };

  // ---- W by LDS-DMA: a stage's panel is BN contiguous 96-byte rows = a linear copy of W_INSTR x 1 KB ------------------
  // (rows past Npad: the lanes re-read the panel's last valid piece; those LDS rows only feed output columns >= Npad)
  unsigned wvoff[WQ];
  {
    const int valid = min(BN, p.Npad - n0) * 6;            // 16-byte pieces of this panel inside the pack
#pragma unroll
    for (int q = 0; q < WQ; ++q) wvoff[q] = (unsigned)min((wave + NW * q) * 64 + lane, valid - 1) * 16u;
  }
  const unsigned ws_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)Ws;
  const size_t stage_bytes = (size_t)p.Npad * (ROW * 4);
  const char* wbase = reinterpret_cast<const char*>(p.w) + (size_t)n0 * (ROW * 4);
  auto dma_w = [&](int s, int dbuf) {                      // stage s -> Ws[dbuf]
    const char* sbase = wbase + (size_t)s * stage_bytes;
#pragma unroll
    for (int q = 0; q < WQ; ++q) {
      const int g = wave + NW * q;
      if (g < G::W_INSTR) {
        const unsigned lds = __builtin_amdgcn_readfirstlane(ws_lds + (unsigned)((dbuf * G::WBUF_DW + g * 256) * 4));
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds), "v"(wvoff[q]), "s"(sbase) : "memory", "m0");
      }
    }
  };
  auto dma_wait = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int frow = lane & 15;
  const S3Frag fr(lane >> 4);
  const int afrag = ((wm * MT) * 16 + frow) * ROW;
  const int wfrag = ((wn * NT) * 16 + frow) * ROW;

  auto mma = [&](int buf) {
    const float* ab = As + buf * (BM * ROW) + afrag;
    f32x4 a1[MT], a2[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      a1[i] = *reinterpret_cast<const f32x4*>(ab + i * 16 * ROW + fr.a1);
      a2[i] = *reinterpret_cast<const f32x4*>(ab + i * 16 * ROW + fr.a2);
    }
    const float* wb = Ws + buf * G::WBUF_DW + wfrag;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const f32x4 w1 = *reinterpret_cast<const f32x4*>(wb + j * 16 * ROW + fr.w1);
      const f32x4 w2 = *reinterpret_cast<const f32x4*>(wb + j * 16 * ROW + fr.w2);
      const f32x4 w3 = *reinterpret_cast<const f32x4*>(wb + j * 16 * ROW + fr.w3);
#pragma unroll
      for (int i = 0; i < MT; ++i) acc[i][j] = mfma_stage<bf16_t>(w1, a1[i], acc[i][j]);
#pragma unroll
      for (int i = 0; i < MT; ++i) acc[i][j] = mfma_stage<bf16_t>(w2, a1[i], acc[i][j]);
#pragma unroll
      for (int i = 0; i < MT; ++i) acc[i][j] = mfma_stage<bf16_t>(w3, a2[i], acc[i][j]);
    }
  };

  // ---- K loop: stage s computes from buffers s & 1 while stage s + 1 is fetched (A through registers, W by DMA) ----------
  const int nst = p.nst;
  load_a();
  dma_w(0, 0);
  store_a(0);
  dma_wait();
  __syncthreads();
  for (int s = 0; s < nst; ++s) {
    const bool more = s + 1 < nst;
    if (more) {
      load_a();
      dma_w(s + 1, (s + 1) & 1);
    }
    mma(s & 1);
    if (more) store_a((s + 1) & 1);
    dma_wait();
    __syncthreads();
  }

  // ---- epilogue (conv_igemm.hip's): D rows = channels ((lane >> 4) * 4 + reg), D columns = pixels (lane & 15) ----------------
  const int epix = lane & 15;
  const int en = (lane >> 4) * 4;
  IgemmParams ep{};
  ep.N = p.N; ep.act = p.act; ep.residual = p.residual; ep.dst = p.dst; ep.out_f32 = 1;
  auto epilogue = [&](auto act_tag) {
  constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = n0 + (wn * NT + j) * 16 + en;
    if (n >= p.N) continue;
    float sc[4], sh[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool ok = n + q < p.N;
      sc[q] = (ok && p.scale) ? p.scale[n + q] : 1.0f;
      sh[q] = (ok && p.shift) ? p.shift[n + q] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int m = m0 + (wm * MT + i) * 16 + epix;
      if (m >= p.M) continue;
      store4<float, ACT>(ep, acc[i][j], n, (size_t)m * p.ldd + n, (size_t)m * p.ldres, sc, sh);
    }
  }
  };
  if (p.act == CCVPE_ACT_SWISH) epilogue(std::integral_constant<int, CCVPE_ACT_SWISH>{});
  else epilogue(std::integral_constant<int, CCVPE_ACT_NONE>{});
}

template <int MT, int NT, int WN, int NW>
static int launch_pw3(PwS3Params p, hipStream_t stream) {
  using G = PwS3Geom<MT, NT, WN, NW>;
  static_assert(G::LDS_BYTES <= 80 * 1024, "pw_s3_kernel: two workgroups per CU");
  p.tiles_n = (p.Npad + G::BN - 1) / G::BN;
  const long total = (long)((p.M + G::BM - 1) / G::BM) * p.tiles_n;
  if (total > 0x7fffffffL) return fail(CCVPE_EINVAL, "pw_s3: grid too large");
  p.tiles_total = (int)total;
  static DevCache lds_set;                      // per tile instantiation
  if (int rc = ensure_dyn_lds(lds_set, pw_s3_kernel<MT, NT, WN, NW>, G::LDS_BYTES, "pw_s3_kernel")) return rc;
  hipLaunchKernelGGL((pw_s3_kernel<MT, NT, WN, NW>), dim3(p.tiles_total), dim3(64 * NW), G::LDS_BYTES, stream, p);
  return check_launch("pw_s3_kernel");
}

// The tiles, X(MT, NT, WN, NW): NW waves, workgroup = 16 MT (NW / WN) rows x 16 NT WN columns.  Narrow layers (N <= 112: the
// /16-resolution projections, M >= 51 200 at B = 64) take 128 rows, four waves with all the columns in each wave's tile; the wider
// ones (the /32-resolution layers and the heads: M <= 16 384, no more than one 64-row workgroup per CU) take 64 rows and EIGHT waves,
// 2 x 4 over rows x columns: a workgroup alone on its CU still has two waves per SIMD to overlap one wave's LDS round trips, split
// and barrier wait with the other's matrix instructions.
#define CCVPE_PW3_TILES(X) X(2, 5, 1, 4) X(2, 7, 1, 4) X(2, 2, 4, 8) X(2, 3, 4, 8) X(2, 5, 4, 8)

struct Pw3Route { int mt, nt, wn, nw; };

// the narrowest tile that holds all of Npad; wider layers tile N with the widest
static Pw3Route pw3_tile(int npad) {
  Pw3Route best{2, 5, 4, 8};
#define CCVPE_CASE(MT_, NT_, WN_, NW_) \
  if (npad <= 16 * NT_ * WN_ && 16 * NT_ * WN_ < 16 * best.nt * best.wn) best = Pw3Route{MT_, NT_, WN_, NW_};
  CCVPE_PW3_TILES(CCVPE_CASE)
#undef CCVPE_CASE
  return best;
}

// Size rule (measured per layer at B = 64, 8 and 1 with tools/pw_s3_probe.py; DESIGN section 4, profiles/r21/pw_probe.txt): a layer is
// routed only where the three-plane kernel beat today's route — ccvpe_conv_igemm_f32, with its split-K second pass where it has one — by
// more than the spread of the probe's passes, from the smallest measured M on from which every measured size won.  At B = 64 all
// eighteen layers won (s3 / f32 0.52-0.79, spreads 0.005-0.10).  The 80-column projections (K = 240, 480) and _conv_head (K = 320, N
// tiled) also won at B = 8 and B = 1 (0.70-0.82, M down to 800 and 200); the layers with K >= 480 behind a 112- to 320-column tile,
// the ground descriptors (K = 1280) and the aerial descriptor (K = 5120) lost there (1.04-7.9: conv_igemm splits K over the idle
// CUs, this kernel walks it in one workgroup per tile) and keep conv_igemm below their B = 64 sizes.  Nothing else was measured, so
// nothing else is routed.
static bool pw3_measured_size(const ccvpe_conv_desc* d, long m) {
  const int npad = (d->n + 15) / 16 * 16;
  if (d->kh == 2) return m >= 4096;                       // aerial descriptor: 8 x 8 outputs x 64
  if (npad <= 80) return m >= 800;                        // blocks 5-7
  if (npad <= 112) return m >= 51200;                     // blocks 8-10
  if (npad <= 320) return m >= 12800;                     // blocks 11-15, ground descriptors
  return d->c0 <= 320 && m >= 200;                        // N tiled: _conv_head
}

// nullptr, the tile and M if the kernel computes this layer, else why not
static const char* pw3_pick(const ccvpe_conv_desc* d, Pw3Route& r, long& m) {
  r = Pw3Route{};
  m = 0;
  if (!d) return "null desc";
  const bool one = d->kh == 1 && d->kw == 1 && d->stride == 1 && d->pad == 0;
  const bool two = d->kh == 2 && d->kw == 2 && d->stride == 2 && d->pad == 0;
  if (!one && !two) return "neither a 1x1 nor a 2x2 stride-2 layer";
  if (d->c1 != 0 || d->src1) return "one source only";
  if (d->out_mode != CCVPE_OUT_NHWC) return "NHWC store only";
  if (d->act != CCVPE_ACT_NONE && d->act != CCVPE_ACT_SWISH) return "activation must be none or swish";
  if (d->c0 <= 0 || d->c0 % 16) return "K must be a positive multiple of 16";
  if (d->gate && !one) return "gate only for 1x1";
  if (d->batch <= 0 || d->in_h <= 0 || d->in_w <= 0 || d->n <= 0) return "bad shape";
  if (two && (d->in_h < 2 || d->in_w < 2)) return "bad shape";
  if (d->n <= 48) return "N <= 48 is not served";
  if (d->ld0 < d->c0 || d->ld0 % 4 || d->ldd < d->n || d->ldd % 4 || (d->residual && (d->ldres < d->n || d->ldres % 4))) return "bad strides";
  const int taps = two ? 4 : 1;
  if (d->kpad != 3 * taps * d->c0) return "kpad is not that of the three-plane pack (models._pack_pw_s3)";
  const int ho = two ? d->in_h / 2 : d->in_h, wo = two ? d->in_w / 2 : d->in_w;
  m = (long)d->batch * ho * wo;
  // 32-bit byte offsets into the source, 31-bit pixel indices
  const double px = (double)d->batch * d->in_h * d->in_w;
  if (px * d->ld0 * 4.0 >= 4294967296.0 || px >= 2147483648.0 || (double)d->batch * d->c0 * 4.0 >= 4294967296.0) return "tensor too large";
  if ((d->src0 && !aligned16(d->src0)) || (d->w && !aligned16(d->w)) || (d->gate && !aligned16(d->gate)) || (d->dst && !aligned16(d->dst)) ||
      (d->residual && !aligned16(d->residual)))
    return "pointers must be 16-byte aligned";
  r = pw3_tile((d->n + 15) / 16 * 16);
  return nullptr;
}

}  // namespace ccvpe

using namespace ccvpe;

extern "C" int ccvpe_pw_s3_ok(const ccvpe_conv_desc* d) {
  Pw3Route r;
  long m;
  return pw3_pick(d, r, m) ? 0 : pw3_measured_size(d, m) ? 2 : 1;
}

extern "C" int ccvpe_pw_s3_route(const ccvpe_conv_desc* d) {
  Pw3Route r;
  long m;
  return pw3_pick(d, r, m) ? 0 : 1 | (r.mt << 8) | (r.nt << 12) | (r.wn << 16) | (r.nw << 20);
}

extern "C" int ccvpe_pw_s3_f32(const ccvpe_conv_desc* d, void* stream) {
  Pw3Route r;
  long m;
  if (const char* why = pw3_pick(d, r, m)) return fail(CCVPE_EINVAL, "pw_s3: %s", why);
  if (!d->src0 || !d->w || !d->dst) return fail(CCVPE_EINVAL, "pw_s3: null pointer");
  const bool two = d->kh == 2;
  PwS3Params p{};
  p.src = d->src0; p.gate = d->gate; p.w = d->w; p.scale = d->scale; p.shift = d->shift; p.residual = d->residual; p.dst = d->dst;
  p.c0 = d->c0; p.ld0 = d->ld0;
  p.H = d->in_h; p.W = d->in_w; p.Ho = two ? d->in_h / 2 : d->in_h; p.Wo = two ? d->in_w / 2 : d->in_w; p.two = two ? 1 : 0;
  p.M = (int)m; p.N = d->n; p.Npad = (d->n + 15) / 16 * 16; p.nst = (two ? 4 : 1) * d->c0 / 16;
  p.ldd = d->ldd; p.ldres = d->ldres; p.act = d->act;
  hipStream_t st = (hipStream_t)stream;
#define CCVPE_CASE(MT_, NT_, WN_, NW_) \
  if (r.mt == MT_ && r.nt == NT_ && r.wn == WN_) return launch_pw3<MT_, NT_, WN_, NW_>(p, st);
  CCVPE_PW3_TILES(CCVPE_CASE)
#undef CCVPE_CASE
  return fail(CCVPE_EINVAL, "pw_s3: no tile config");
}
