// upconv_s3_kernel: the fp32 folded deconv + 3x3 layer (see upconv_impl.h for the fold) with its matrix arithmetic on the bf16
// matrix cores, fp32-class accuracy.  Every fp32 operand is split, round-to-nearest, into three bf16 planes
//   hi = bf16(v),  mid = bf16(v - hi),  lo = bf16(v - hi - mid)          (both subtractions exact, v == hi + mid + lo: 8 + 8 + 8 bits)
// and x.w is evaluated as the six products  hi.hi + hi.mid + mid.hi + mid.mid + hi.lo + lo.hi,  accumulated in fp32 by the matrix
// unit (the three dropped products are each <= 2^-24 |x||w|).  One v_mfma_f32_16x16x32_bf16 holds TWO products of a 16-channel
// block: its 32-deep K is [plane P of channels 0-15 | plane Q of channels 0-15], so per 16 channels and 16 x 16 output tile
//   acc += [w_hi |w_hi ] . [x_hi|x_mid]
//   acc += [w_mid|w_mid] . [x_hi|x_mid]
//   acc += [w_hi |w_lo ] . [x_lo|x_hi ]
// three bf16 instructions (3 x 16 cycles) where the fp32 kernel issues four v_mfma_f32_16x16x4_f32 (4 x 32 cycles).
//
// Skeleton of upconv_dma_kernel (upconv_impl.h): TH x 16 low-res pixel tiles, one output parity per workgroup, the low-res halo
// staged once per 16-channel chunk (phase A: the four low-res taps), the skip gathered per (tap, 16-channel block) stage (phase
// B: nine taps), PAIR form for level 6 (two 8 x 8 images per tile), the same epilogue (shift9 by border class, activation,
// store4).  Activations are read as fp32 from HBM and split in registers on their way to LDS; the output is fp32 NHWC.
//   * Weights: split ONCE on the host (models._pack_upconv_s3), laid out [parity][stage][Npad][hi 16 | mid 16 | lo 16] bf16 in the
//     kernel's own stage order, every tap padded to 16-channel blocks (no block straddles a tap).  A stage's W panel is BN
//     contiguous 96-byte rows: it goes HBM -> LDS by global_load_lds_dwordx4 as a linear copy (no VGPR round trip, no ds_write),
//     double-buffered, requested one stage ahead.
//   * LDS rows (W row and activation pixel alike) are 96 bytes = 24 dwords, [hi|mid|lo], unswizzled: 24 r mod 64 takes eight
//     distinct multiples of 8 over any eight consecutive rows, and each 16-lane group of a ds_read_b128 reads two runs of eight
//     rows at 16-byte slots of different parity — conflict-free for every window base and for the PAIR halo, whose two images sit
//     16 slots apart (tests/test_upconv_s3.py checks the model of tools/lds_layout.py).  The fragments are picked per lane group
//     g = lane >> 4:  [P|Q] = slot of plane P at g < 2, of plane Q at g >= 2; one ds_read_b128 each.
// Non-finite and overflowing inputs behave differently from the fp32 kernel: Inf splits into (Inf, NaN, NaN), |v| above 3.39e38
// rounds hi to Inf, and bf16-subnormal planes (|v| below ~1e-38 x 2^16) may be flushed by the matrix unit.  The forward never
// produces such values.
#include "split3_impl.h"      // split3, store_planes, the fragment offsets

namespace ccvpe {

struct UpS3Params {
  const float* src0;
  const float* src1;
  const void* w;
  const float* shift9;
  float* dst;
  int c0, ld0, c1, ld1;
  int H1, W1, batch;
  int N, Npad;
  int nb0, nb1, nst;      // 16-channel blocks per low-res tap / per skip tap; stages = 4 nb0 + 9 nb1
  int ldd, act;
  int tiles_n, tiles_total;
};

template <int MT, int NT, int WN, bool PAIR>
struct UpS3Geom {
  static constexpr int WM = 4 / WN;
  static constexpr int BM = 16 * MT * WM;
  static constexpr int BN = 16 * NT * WN;
  static constexpr int TH = BM / 16;
  static constexpr int HR = TH + 2, HCP = PAIR ? 26 : 18;
  static constexpr int ROW = 24;                                   // dwords per LDS row: [hi 16 | mid 16 | lo 16] bf16
  static constexpr int HALO_DW = HR * HCP * ROW, ASTG_DW = 2 * BM * ROW;
  static constexpr int U_DW = HALO_DW > ASTG_DW ? HALO_DW : ASTG_DW;   // halo (phase A) | A stage [2][BM] (phase B)
  static constexpr int W_INSTR = (BN * 6 + 63) / 64;               // wave-wide 1 KB DMA instructions per W panel
  static constexpr int WBUF_DW = W_INSTR * 256;
  static constexpr int LDS_BYTES = (U_DW + 2 * WBUF_DW) * 4;
};

template <int MT, int NT, int WN, bool PAIR>
__global__ __launch_bounds__(256, 2) void upconv_s3_kernel(const UpS3Params p) {
  using G = UpS3Geom<MT, NT, WN, PAIR>;
  constexpr int BM = G::BM, BN = G::BN, TH = G::TH, HR = G::HR, HCP = G::HCP, ROW = G::ROW;
  constexpr int HC = PAIR ? 20 : 18, HPX = HR * HC;   // staged halo columns (PAIR: two 10-column halos)
  constexpr int H_IT = (HPX * 4 + 255) / 256;
  constexpr int A_IT = BM / 64;
  constexpr int WQ = (G::W_INSTR + 3) / 4;

  extern __shared__ __attribute__((aligned(16))) float s3_sm[];
  float* Us = s3_sm;                               // halo [HR][HCP][ROW]  |  phase-B A stage [2][BM][ROW]
  float* Ws = s3_sm + G::U_DW;                     // [2][W_INSTR * 256] by DMA: BN rows of ROW dwords

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = sgpr(tid >> 6);
  const int wm = wave / WN;
  const int wn = wave % WN;

  const int tile = xcd_tile(blockIdx.x, p.tiles_total);
  const int tn = tile % p.tiles_n;
  const int par = (tile / p.tiles_n) & 3;
  const int ts = tile / (p.tiles_n * 4);
  const int tiles_x = PAIR ? 1 : (p.W1 + 15) / 16;
  const int tiles_y = PAIR ? 1 : (p.H1 + TH - 1) / TH;
  const int tx = ts % tiles_x;
  const int ty = (ts / tiles_x) % tiles_y;
  const int b = PAIR ? 2 * ts : ts / (tiles_x * tiles_y);
  const int nbatch = p.batch;
  const int py = par >> 1, px = par & 1;
  const int y0 = ty * TH, x0 = tx * 16;
  const int n0 = tn * BN;
  const int H2 = 2 * p.H1, W2 = 2 * p.W1;
  const int srow = tid >> 2, ssub = tid & 3;
  const int ld0s = sgpr(p.ld0), ld1s = sgpr(p.ld1);

  // ---- halo staging coordinates (one f32x4 = 4 channels of the 16-channel chunk per piece) -------
  int h_off[H_IT], h_pix[H_IT], h_sub[H_IT];
#pragma unroll
  for (int it = 0; it < H_IT; ++it) {
    const int idx = tid + 256 * it;
    const int pxl = idx >> 2, sub = idx & 3;
    h_sub[it] = sub;
    if (pxl < HPX) {
      const int hy = pxl / HC, hc = pxl - hy * HC;
      const int img = PAIR ? hc / 10 : 0;
      const int lx = hc - 10 * img, hx = lx + 16 * img;              // column inside the image's halo, slot in the halo row
      const int iy = y0 - 1 + hy, ix = x0 - 1 + lx;
      h_off[it] = (hy * HCP + hx) * ROW + sub * 2;
      h_pix[it] = ((unsigned)iy < (unsigned)p.H1 && (unsigned)ix < (unsigned)p.W1 && b + img < nbatch) ? ((b + img) * p.H1 + iy) * p.W1 + ix : -1;
    } else {
      h_off[it] = -1;
      h_pix[it] = -1;
    }
  }
  f32x4 h_reg[H_IT];
  unsigned h_keep = 0;
  auto load_halo = [&](int chunk) {         // raw loads from clamped addresses; pieces outside are zeroed at the LDS store
    h_keep = 0;
#pragma unroll
    for (int it = 0; it < H_IT; ++it) {
      const int ch = chunk * 16 + h_sub[it] * 4;
      const bool ok = h_pix[it] >= 0 && ch < p.c0;
      h_reg[it] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(p.src0) + (ok ? ((unsigned)h_pix[it] * (unsigned)ld0s + (unsigned)ch) * 4u : 0u));
      h_keep |= ok ? (1u << it) : 0u;
    }
  };
  auto store_halo = [&]() {
#pragma unroll
    for (int it = 0; it < H_IT; ++it)
      if (h_off[it] >= 0) store_planes(Us + h_off[it], keep_if(h_reg[it], (h_keep >> it) & 1u));
  };

  // ---- W by LDS-DMA: a stage's panel is BN contiguous 96-byte rows = a linear copy of W_INSTR x 1 KB ------------------
  // (rows past Npad: the lanes re-read the panel's last valid piece; those LDS rows only feed output columns >= Npad)
  unsigned wvoff[WQ];
  {
    const int valid = min(BN, p.Npad - n0) * 6;            // 16-byte pieces of this panel inside the pack
#pragma unroll
    for (int q = 0; q < WQ; ++q) wvoff[q] = (unsigned)min((wave + 4 * q) * 64 + lane, valid - 1) * 16u;
  }
  const unsigned ws_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)Ws;
  const size_t stage_bytes = (size_t)p.Npad * (ROW * 4);
  const char* wpar = reinterpret_cast<const char*>(p.w) + ((size_t)par * p.nst * p.Npad + n0) * (ROW * 4);
  auto dma_w = [&](int s, int dbuf) {                      // stage s -> Ws[dbuf]
    const char* sbase = wpar + (size_t)s * stage_bytes;
#pragma unroll
    for (int q = 0; q < WQ; ++q) {
      const int g = wave + 4 * q;
      if (g < G::W_INSTR) {
        const unsigned lds = __builtin_amdgcn_readfirstlane(ws_lds + (unsigned)((dbuf * G::WBUF_DW + g * 256) * 4));
        asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds), "v"(wvoff[q]), "s"(sbase) : "memory", "m0");
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
  const int g4 = lane >> 4;
  // per-lane dword offsets of the fragments inside a 24-dword [hi|mid|lo] row (S3Frag of split3_impl.h holds the same five for
  // pw_s3.hip; they stay spelled out here because tests/test_upconv_s3.py reads them from this file for its bank model)
  const int a1off = 4 * g4;                                  // [x_hi | x_mid]
  const int a2off = g4 < 2 ? 16 + 4 * g4 : 4 * g4 - 8;       // [x_lo | x_hi ]
  const int w1off = 4 * (g4 & 1);                            // [w_hi | w_hi ]
  const int w2off = 8 + 4 * (g4 & 1);                        // [w_mid| w_mid]
  const int w3off = g4 < 2 ? 4 * g4 : 4 * g4 + 8;            // [w_hi | w_lo ]
  const int wfrag = ((wn * NT) * 16 + frow) * ROW;

  // one stage: the pixel fragments at abase + i * istride, the W panel in Ws[wbuf]
  auto mma = [&](const float* abase, int istride, int wbuf) {
    f32x4 a1[MT], a2[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      a1[i] = *reinterpret_cast<const f32x4*>(abase + i * istride + a1off);
      a2[i] = *reinterpret_cast<const f32x4*>(abase + i * istride + a2off);
    }
    const float* wb = Ws + wbuf * G::WBUF_DW + wfrag;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const f32x4 w1 = *reinterpret_cast<const f32x4*>(wb + j * 16 * ROW + w1off);
      const f32x4 w2 = *reinterpret_cast<const f32x4*>(wb + j * 16 * ROW + w2off);
      const f32x4 w3 = *reinterpret_cast<const f32x4*>(wb + j * 16 * ROW + w3off);
#pragma unroll
      for (int i = 0; i < MT; ++i) acc[i][j] = mfma_stage<bf16_t>(w1, a1[i], acc[i][j]);
#pragma unroll
      for (int i = 0; i < MT; ++i) acc[i][j] = mfma_stage<bf16_t>(w2, a1[i], acc[i][j]);
#pragma unroll
      for (int i = 0; i < MT; ++i) acc[i][j] = mfma_stage<bf16_t>(w3, a2[i], acc[i][j]);
    }
  };

  // ================= phase A: low-res source; per 16-channel chunk the halo is staged once, 4 one-tap stages =================
  const int nstA = 4 * p.nb0;
  const int hfrag = (wm * MT * HCP + frow + (PAIR ? 8 * (frow >> 3) : 0)) * ROW;
  load_halo(0);
  dma_w(0, 0);
  store_halo();
  dma_wait();
  __syncthreads();
  {
    int chunk = 0, tap = 0;
    for (int s = 0; s < nstA; ++s) {
      const bool more = s + 1 < p.nst;
      const bool next_halo = chunk + 1 < p.nb0;
      if (tap == 0 && next_halo) load_halo(chunk + 1);
      if (more) dma_w(s + 1, (s + 1) & 1);
      const int du = tap >> 1, dv = tap & 1;
      mma(Us + hfrag + ((du + py) * HCP + dv + px) * ROW, HCP * ROW, s & 1);
      dma_wait();
      __syncthreads();
      if (++tap == 4) {
        tap = 0;
        ++chunk;
        if (next_halo) {                                     // every wave is done reading the halo -> overwrite it
          store_halo();
          __syncthreads();
        }
      }
    }
  }

  // ================= phase B: skip, 9 taps (stride 2, parity offset), one (tap, 16-channel block) gather per stage ===========
  const int nstB = 9 * p.nb1;
  if (nstB > 0) {
    f32x4 a_reg[A_IT];
    unsigned a_keep = 0;
    int a_pix[A_IT], a_yy[A_IT], a_xx[A_IT], a_bb[A_IT];
#pragma unroll
    for (int it = 0; it < A_IT; ++it) {
      const int ml = srow + 64 * it;
      const int col = ml & 15;
      const int y1 = y0 + (ml >> 4), x1 = PAIR ? (col & 7) : x0 + col;
      a_bb[it] = PAIR ? b + (col >> 3) : b;
      a_pix[it] = (y1 < p.H1 && x1 < p.W1 && a_bb[it] < nbatch) ? 1 : 0;
      a_yy[it] = 2 * y1 + py - 1;
      a_xx[it] = 2 * x1 + px - 1;
    }
    auto load_a = [&](int t) {
      const int tapb = t / p.nb1;
      const int ch = (t - tapb * p.nb1) * 16 + ssub * 4;
      const bool cvalid = ch < p.c1;
      const int ky = tapb / 3, kx = tapb - 3 * ky;
      a_keep = 0;
#pragma unroll
      for (int it = 0; it < A_IT; ++it) {
        const int iy = a_yy[it] + ky, ix = a_xx[it] + kx;
        const bool ok = cvalid && a_pix[it] && (unsigned)iy < (unsigned)H2 && (unsigned)ix < (unsigned)W2;
        const unsigned off = ok ? ((unsigned)((a_bb[it] * H2 + iy) * W2 + ix) * (unsigned)ld1s + (unsigned)ch) * 4u : 0u;
        a_reg[it] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(p.src1) + off);
        a_keep |= ok ? (1u << it) : 0u;
      }
    };
    auto store_a = [&](int buf) {
#pragma unroll
      for (int it = 0; it < A_IT; ++it)
        store_planes(Us + (buf * BM + srow + 64 * it) * ROW + ssub * 2, keep_if(a_reg[it], (a_keep >> it) & 1u));
    };
    // the halo is dead (phase A ended on a barrier); the W panel of stage nstA was requested by phase A's last stage
    load_a(0);
    store_a(0);
    __syncthreads();
    const int afrag = ((wm * MT) * 16 + frow) * ROW;
    for (int t = 0; t < nstB; ++t) {
      const int s = nstA + t;
      const bool more = t + 1 < nstB;
      if (more) {
        load_a(t + 1);
        dma_w(s + 1, (s + 1) & 1);
      }
      mma(Us + (t & 1) * (BM * ROW) + afrag, 16 * ROW, s & 1);
      if (more) store_a((t + 1) & 1);
      dma_wait();
      __syncthreads();
    }
  }

  // ---- epilogue (as upconv_dma_kernel) -------------------------------------------------------------
  const int epix = lane & 15;
  const int en = (lane >> 4) * 4;
  IgemmParams ep{};
  ep.N = p.N; ep.act = p.act; ep.residual = nullptr; ep.dst = p.dst; ep.out_f32 = 1;
  const float one[4] = {1.f, 1.f, 1.f, 1.f};
  const int x1 = PAIR ? (epix & 7) : x0 + epix;
  const int eb = PAIR ? b + (epix >> 3) : b;
  auto epilogue = [&](auto act_tag) {
  constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int y1 = y0 + wm * MT + i;
    if (y1 >= p.H1 || x1 >= p.W1 || eb >= nbatch) continue;
    const int Y = 2 * y1 + py, X = 2 * x1 + px;
    const int rc = Y == 0 ? 0 : (Y == H2 - 1 ? 2 : 1);
    const int cc = X == 0 ? 0 : (X == W2 - 1 ? 2 : 1);
    const float* shp = p.shift9 + (size_t)(rc * 3 + cc) * p.N;
    const size_t pix = (size_t)(eb * H2 + Y) * W2 + X;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = n0 + (wn * NT + j) * 16 + en;
      if (n >= p.N) continue;
      float sh[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) sh[q] = (n + q < p.N) ? shp[n + q] : 0.f;
      store4<float, ACT>(ep, acc[i][j], n, pix * p.ldd + n, 0, one, sh);
    }
  }
  };
  CCVPE_ACT_DISPATCH(p.act, epilogue);
}

template <int MT, int NT, int WN, bool PAIR>
static int launch_s3(UpS3Params p, hipStream_t stream) {
  using G = UpS3Geom<MT, NT, WN, PAIR>;
  static_assert(G::LDS_BYTES <= 80 * 1024, "upconv_s3_kernel: two workgroups per CU");
  p.tiles_n = (p.Npad + G::BN - 1) / G::BN;
  const long tiles_m = PAIR ? (p.batch + 1) / 2 : (long)((p.W1 + 15) / 16) * ((p.H1 + G::TH - 1) / G::TH) * p.batch;
  const long total = tiles_m * p.tiles_n * 4;
  if (total > 0x7fffffffL) return fail(CCVPE_EINVAL, "upconv_s3: grid too large");
  p.tiles_total = (int)total;
  static DevCache lds_set;                      // per (tile, PAIR) instantiation
  if (int rc = ensure_dyn_lds(lds_set, upconv_s3_kernel<MT, NT, WN, PAIR>, G::LDS_BYTES, "upconv_s3_kernel")) return rc;
  hipLaunchKernelGGL((upconv_s3_kernel<MT, NT, WN, PAIR>), dim3(p.tiles_total), dim3(256), G::LDS_BYTES, stream, p);
  return check_launch("upconv_s3_kernel");
}

// The tiles upconv_s3_kernel is instantiated for: a deliberate SUBSET of the tile table (CCVPE_TILES, conv_common.h), written once —
// s3_pick() serves an n whose tile is in it, s3_run() launches from it.  X(MT, NT, WN) per row.
#define CCVPE_S3_TILES(X) X(4, 5, 2) X(4, 4, 2) X(4, 2, 2) X(4, 1, 2) X(4, 5, 1) X(4, 3, 1)

// ---- the route: s3_pick() alone validates, decides the form and the tile; the three queries and the launch read its answer
struct S3Route { int form, pair, mt, nt, wn; };      // form 1 = per-parity (pair: two 8 x 8 images per tile), 2 = quad (MT 2, NT = Npad / 16, WN 0)

static bool g_s3_quad = true;                     // ccvpe_set_s3_quad

// Size rule (measured per level at B = 64 with tools/up_probe.py).  profiles/r10/up_probe.txt: the three-plane kernel
// beat ccvpe_upconv3x3_f32 in isolation on all ten decoder layers (1.32x at N = 40 to 1.72x at N = 128), every tile family.
// profiles/r11/up_probe.txt: the quad form (upconv_s3q.hip) beat the per-parity kernel in isolation on all four levels it serves, by
// more than the spread of the probe's repetitions (quad / per-parity 0.79 at N = 32, 0.81 at N = 40, 0.88 at N = 64, 0.96 at N = 80;
// spreads 0.01-0.04).  The smallest of those layers has 4096 low-res pixels and nothing below that was measured, so smaller
// problems keep the fp32 kernel (ccvpe_upconv3x3_s3_ok answers 1, not 2) and, asked for auto, the per-parity form.
static bool s3_measured_size(const ccvpe_upconv_desc* d) { return (long)d->batch * d->h1 * d->w1 >= 4096; }

// nullptr and the route if `form` (0 = auto) computes this layer, else why not
static const char* s3_pick(const ccvpe_upconv_desc* d, int form, S3Route& r) {
  r = S3Route{};
  if (!d) return "null desc";
  if (d->c0 <= 0 || d->c0 % 8 || d->c1 <= 0 || d->c1 % 8) return "c0 / c1 must be positive multiples of 8 (a layer without a skip is not implemented)";
  if (d->batch <= 0 || d->h1 <= 0 || d->w1 <= 0 || d->n <= 0) return "bad shape";
  if (d->ld0 < d->c0 || d->ld0 % 4 || d->ld1 < d->c1 || d->ld1 % 4 || d->ldd < d->n || d->ldd % 4) return "bad strides";
  const int nst = 4 * ((d->c0 + 15) / 16) + 9 * ((d->c1 + 15) / 16);
  if (d->kpad != nst * 48) return "kpad is not that of the three-plane pack (models._pack_upconv_s3)";
  const bool pair = d->w1 == 8 && d->h1 == 8;      // level 6: two images side by side in one 8 x 16 tile
  if (d->w1 < 16 && !pair) return "low-res images narrower than 16 pixels (other than 8 x 8)";
  const int npad = (d->n + 15) / 16 * 16;
  const TileCfg c = kCfgs[pick_cfg(npad)];
  bool tile = false;
#define CCVPE_CASE(MT_, NT_, WN_) tile = tile || (c.mt == MT_ && c.nt == NT_ && c.wn == WN_);
  CCVPE_S3_TILES(CCVPE_CASE)
#undef CCVPE_CASE
  if (!tile) return "no tile for this n";
  if (pair && !(c.nt == 5 && c.wn == 2)) return "8 x 8 images need the 160-column tile";
  // 32-bit byte offsets into both sources, 31-bit pixel indices
  const double m = (double)d->batch * d->h1 * d->w1;
  if (m * d->ld0 * 4.0 >= 4294967296.0 || 4.0 * m * d->ld1 * 4.0 >= 4294967296.0 || 4.0 * m >= 2147483648.0) return "tensor too large";
  if (form < 0 || form > 2) return "form must be 0 (auto), 1 (per-parity) or 2 (quad)";
  const bool quad = upconv_s3q_serves(d);
  if (form == 2 && !quad) return "the quad form serves 16 < n <= 80 and images of 16 or more pixels a row";
  if (form == 0) form = g_s3_quad && quad && s3_measured_size(d) ? 2 : 1;
  r = form == 2 ? S3Route{2, 0, 2, npad / 16, 0} : S3Route{1, pair, c.mt, c.nt, c.wn};
  return nullptr;
}

}  // namespace ccvpe

using namespace ccvpe;

extern "C" int ccvpe_upconv3x3_s3_ok(const ccvpe_upconv_desc* d) {
  S3Route r;
  return s3_pick(d, 1, r) ? 0 : s3_measured_size(d) ? 2 : 1;
}

extern "C" int ccvpe_set_s3_quad(int on) {
  const int prev = g_s3_quad ? 1 : 0;
  g_s3_quad = on != 0;
  return prev;
}

extern "C" int ccvpe_upconv3x3_s3_form_ok(const ccvpe_upconv_desc* d, int form) {
  S3Route r;
  return s3_pick(d, form, r) ? 0 : r.form;
}

extern "C" int ccvpe_upconv3x3_s3_route(const ccvpe_upconv_desc* d, int form) {
  S3Route r;
  return s3_pick(d, form, r) ? 0 : r.form | (r.pair << 4) | (r.mt << 8) | (r.nt << 12) | (r.wn << 16);
}

static int s3_run(const ccvpe_upconv_desc* d, int form, void* stream) {
  S3Route r;
  if (const char* why = s3_pick(d, form, r)) return fail(CCVPE_EINVAL, "upconv3x3_s3: %s", why);
  if (!d->src0 || !d->src1 || !d->w || !d->shift9 || !d->dst) return fail(CCVPE_EINVAL, "upconv3x3_s3: null pointer");
  if (!aligned16(d->src0) || !aligned16(d->src1) || !aligned16(d->w) || !aligned16(d->dst))
    return fail(CCVPE_EINVAL, "upconv3x3_s3: pointers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (r.form == 2) return upconv_s3q_launch(d, st);
  UpS3Params p;
  s3_fill(d, p);
  p.Npad = (d->n + 15) / 16 * 16;      // (tiles_n, tiles_total: launch_s3)
  if (r.pair) return launch_s3<4, 5, 2, true>(p, st);      // (s3_pick: a pair layer has the 160-column tile)
#define CCVPE_CASE(MT_, NT_, WN_) \
  if (r.mt == MT_ && r.nt == NT_ && r.wn == WN_) return launch_s3<MT_, NT_, WN_, false>(p, st);
  CCVPE_S3_TILES(CCVPE_CASE)
#undef CCVPE_CASE
  return fail(CCVPE_EINVAL, "upconv3x3_s3: no tile config");
}

extern "C" int ccvpe_upconv3x3_s3_f32(const ccvpe_upconv_desc* d, void* stream) { return s3_run(d, 0, stream); }

extern "C" int ccvpe_upconv3x3_s3_form_f32(const ccvpe_upconv_desc* d, int form, void* stream) { return s3_run(d, form, stream); }
