// upconv_s3q_kernel: the "quad" form of the three-plane bf16 folded deconv + 3x3 layer (upconv_s3.hip has the arithmetic, the
// weight pack and the LDS row format; nothing of that changes here) for the narrow levels, Npad = 32 .. 80.  One workgroup
// computes ALL FOUR output parities of its 8 x 16 low-res pixel tile, with four accumulator sets, so that
//   * the low-res halo (10 x 18 pixels) is staged and split once per 16-channel chunk for all four parities, and
//   * the skip is staged and split ONCE per 16-channel block, as the (2 x 8 + 2) x 34 high-res halo of the tile, where the
//     per-parity kernel gathers and splits it once per (parity, tap): phase B has no gather at all.
// The skip halo lies in LDS as four de-interleaved parity planes of 9 x 17 pixels (plane = (row & 1, column & 1) of the halo):
// tap (ky, kx) of output parity (py, px) reads, with r = py + ky and c = px + kx, sixteen CONSECUTIVE pixels of plane
// (r & 1, c & 1) from (row + (r >> 1), column (c >> 1)) on — the conflict-free pattern of the 24-dword rows (tests/
// test_upconv_s3_quad.py runs the bank model over every window base).
// Waves: WM = 4, WN = 1, MT = 2: wave w owns low-res rows 2w, 2w + 1 of the tile and every column tile; acc[parity][2][NT].
// Stages (one s_waitcnt vmcnt(0) + barrier each, the W panel of the next stage requested by LDS-DMA at the top):
//   phase A  (chunk, parity): the four low-res taps, one linear 4 x Npad-row panel of the pack          24 NT MFMAs per wave
//   phase B  G taps of the sequence (parity, tap) per 16-channel block, one Npad-row panel per tap       6 NT G MFMAs per wave
// Order of products per accumulator: phase A chunk ascending, tap 0..3; phase B block ascending, tap 0..8.  With one skip block
// (c1 <= 16) that is the per-parity kernel's order and the output is bit-identical to it; with two blocks the per-parity kernel
// runs tap-major (tap 0..8, block inside), this form block-major, and the two differ in the last bits.
#include "conv_common.h"

namespace ccvpe {

struct UpS3qParams {
  const float* src0;
  const float* src1;
  const void* w;
  const float* shift9;
  float* dst;
  int c0, ld0, c1, ld1;
  int H1, W1, batch;
  int N;
  int nb0, nb1, nst;      // 16-channel blocks per low-res tap / per skip tap; pack stages per parity = 4 nb0 + 9 nb1
  int ldd, act;
  int tiles_total;
};

template <int NT>
struct UpS3qGeom {
  static constexpr int TH = 8, HR = TH + 2, HC = 18;               // low-res tile rows, halo rows / columns
  static constexpr int PR = TH + 1, PC = 17;                       // rows / columns of one skip parity plane
  static constexpr int ROW = 24;                                   // dwords per LDS row: [hi 16 | mid 16 | lo 16] bf16
  static constexpr int NP = 16 * NT;                               // Npad: one column tile covers it
  static constexpr int HALO_DW = HR * HC * ROW;
  static constexpr int PLANES_DW = 4 * PR * PC * ROW;
  static constexpr int WA_INSTR = 6 * NT;                          // wave-wide 1 KB DMA instructions per phase-A panel (4 NP rows)
  static constexpr int WA_DW = WA_INSTR * 256;
  static constexpr int WB_INSTR = (NP * 6 + 63) / 64;              // per phase-B panel (NP rows)
  static constexpr int WB_DW = WB_INSTR * 256;
  static constexpr int G = NT == 2 ? 3 : (NT == 3 ? 2 : 1);        // taps per phase-B stage: what two buffers of G panels leave of 80 KB
  static constexpr int A_DW = HALO_DW + 2 * WA_DW;                 // phase A: halo | W [2]
  static constexpr int B_DW = PLANES_DW + 2 * G * WB_DW;           // phase B: planes | W [2][G]
  static constexpr int LDS_BYTES = (A_DW > B_DW ? A_DW : B_DW) * 4;
};

__device__ __forceinline__ unsigned q_pk_bf16(float a, float b) {    // round-to-nearest-even pair (v_cvt_pk_bf16_f32)
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  bf16x2_t v;
  v[0] = (__bf16)a;
  v[1] = (__bf16)b;
  return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ float q_bf_lo(unsigned p) { return __builtin_bit_cast(float, p << 16); }
__device__ __forceinline__ float q_bf_hi(unsigned p) { return __builtin_bit_cast(float, p & 0xffff0000u); }

typedef unsigned q_u32x2 __attribute__((ext_vector_type(2)));
// four fp32 values -> their hi / mid / lo bf16 planes, stored into one 24-dword LDS row (as upconv_s3.hip's split3)
__device__ __forceinline__ void q_store_planes(float* at, f32x4 v) {
  q_u32x2 hi, mid, lo;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    float a = v[2 * h], b = v[2 * h + 1];
    const unsigned ph = q_pk_bf16(a, b);
    a -= q_bf_lo(ph);
    b -= q_bf_hi(ph);
    const unsigned pm = q_pk_bf16(a, b);
    a -= q_bf_lo(pm);
    b -= q_bf_hi(pm);
    hi[h] = ph;
    mid[h] = pm;
    lo[h] = q_pk_bf16(a, b);
  }
  *reinterpret_cast<q_u32x2*>(at) = hi;
  *reinterpret_cast<q_u32x2*>(at + 8) = mid;
  *reinterpret_cast<q_u32x2*>(at + 16) = lo;
}

template <int NT>
__global__ __launch_bounds__(256, 2) void upconv_s3q_kernel(const UpS3qParams p) {
  using G = UpS3qGeom<NT>;
  constexpr int TH = G::TH, HR = G::HR, HC = G::HC, PR = G::PR, PC = G::PC, ROW = G::ROW, NP = G::NP;
  constexpr int HPX = HR * HC;
  constexpr int H_IT = (HPX * 4 + 255) / 256;
  constexpr int SPX = (2 * TH + 2) * 34;                         // skip halo pixels
  constexpr int S_IT = 5, S_HALVES = (SPX * 4 + 256 * S_IT - 1) / (256 * S_IT);
  constexpr int NGRP = 36 / G::G;                                // phase-B stages per skip block

  extern __shared__ __attribute__((aligned(16))) float s3q_sm[];
  float* Us = s3q_sm;                              // phase A: halo [HR][HC][ROW]   phase B: planes [4][PR][PC][ROW]
  float* WsA = s3q_sm + G::HALO_DW;                // phase A: [2][WA_DW] by DMA, 4 NP rows each
  float* WsB = s3q_sm + G::PLANES_DW;              // phase B: [2][G][WB_DW] by DMA, NP rows each

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = sgpr(tid >> 6);

  const int tile = xcd_tile(blockIdx.x, p.tiles_total);
  const int tiles_x = (p.W1 + 15) / 16;
  const int tiles_y = (p.H1 + TH - 1) / TH;
  const int tx = tile % tiles_x;
  const int ty = (tile / tiles_x) % tiles_y;
  const int b = tile / (tiles_x * tiles_y);
  const int y0 = ty * TH, x0 = tx * 16;
  const int H2 = 2 * p.H1, W2 = 2 * p.W1;
  const int ld0s = sgpr(p.ld0), ld1s = sgpr(p.ld1);

  // ---- low-res halo staging (one f32x4 = 4 channels of the 16-channel chunk per piece) ----------------------------------
  int h_off[H_IT], h_pix[H_IT], h_sub[H_IT];
#pragma unroll
  for (int it = 0; it < H_IT; ++it) {
    const int idx = tid + 256 * it;
    const int pxl = idx >> 2, sub = idx & 3;
    h_sub[it] = sub;
    if (pxl < HPX) {
      const int hy = pxl / HC, hx = pxl - hy * HC;
      const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
      h_off[it] = (hy * HC + hx) * ROW + sub * 2;
      h_pix[it] = ((unsigned)iy < (unsigned)p.H1 && (unsigned)ix < (unsigned)p.W1) ? (b * p.H1 + iy) * p.W1 + ix : -1;
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
      if (h_off[it] >= 0) q_store_planes(Us + h_off[it], keep_if(h_reg[it], (h_keep >> it) & 1u));
  };

  // ---- skip halo of one 16-channel block -> the four parity planes (loaded, split and stored in S_HALVES batches) -------
  auto stage_planes = [&](int blk) {
#pragma unroll
    for (int half = 0; half < S_HALVES; ++half) {
      f32x4 r[S_IT];
      int off[S_IT];
      unsigned keep = 0;
#pragma unroll
      for (int it = 0; it < S_IT; ++it) {
        const int idx = tid + 256 * (half * S_IT + it);
        const int pxl = idx >> 2, sub = idx & 3;
        const int hy = pxl / 34, hx = pxl - hy * 34;
        const int iy = 2 * y0 - 1 + hy, ix = 2 * x0 - 1 + hx;
        const int ch = blk * 16 + sub * 4;
        const bool ok = pxl < SPX && (unsigned)iy < (unsigned)H2 && (unsigned)ix < (unsigned)W2 && ch < p.c1;
        const unsigned goff = ok ? ((unsigned)((b * H2 + iy) * W2 + ix) * (unsigned)ld1s + (unsigned)ch) * 4u : 0u;
        r[it] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(p.src1) + goff);
        keep |= ok ? (1u << it) : 0u;
        off[it] = pxl < SPX ? ((((hy & 1) * 2 + (hx & 1)) * PR + (hy >> 1)) * PC + (hx >> 1)) * ROW + sub * 2 : -1;
      }
#pragma unroll
      for (int it = 0; it < S_IT; ++it)
        if (off[it] >= 0) q_store_planes(Us + off[it], keep_if(r[it], (keep >> it) & 1u));
    }
  };

  // ---- W by LDS-DMA: linear copies of whole 1 KB pieces (Npad = NP, every panel lies inside the pack) -------------------
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)s3q_sm;
  const unsigned vlin = (unsigned)lane * 16u;
  const unsigned vlast = (unsigned)min(lane, 31) * 16u;     // odd NT: the last piece of an NP-row panel is half a KB (the rest re-reads it)
  const size_t stage_bytes = (size_t)NP * (ROW * 4);
  auto dma_one = [&](unsigned lds, unsigned voff, const char* sbase) {
    const unsigned l = __builtin_amdgcn_readfirstlane(lds);
    asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(l), "v"(voff), "s"(sbase) : "memory", "m0");
  };
  auto dma_a = [&](int chunk, int par, int buf) {          // the four taps of (chunk, parity) -> WsA[buf]
    const char* sbase = reinterpret_cast<const char*>(p.w) + ((size_t)par * p.nst + (size_t)chunk * 4) * stage_bytes;
#pragma unroll
    for (int q = 0; q < (G::WA_INSTR + 3) / 4; ++q) {
      const int g = wave + 4 * q;
      if (g < G::WA_INSTR) dma_one(lds0 + (unsigned)((G::HALO_DW + buf * G::WA_DW + g * 256) * 4), vlin, sbase + (size_t)g * 1024);
    }
  };
  auto dma_b = [&](int blk, int grp) {                     // taps grp * G .. of the (parity, tap) sequence -> WsB[grp & 1][..]
#pragma unroll
    for (int q = 0; q < (G::G * G::WB_INSTR + 3) / 4; ++q) {
      const int e = wave + 4 * q;
      if (e < G::G * G::WB_INSTR) {
        const int u = e / G::WB_INSTR, g = e - u * G::WB_INSTR;
        const int seq = grp * G::G + u;
        const int par = seq / 9, tap = seq - 9 * par;
        const char* sbase = reinterpret_cast<const char*>(p.w) + ((size_t)par * p.nst + (size_t)(4 * p.nb0 + tap * p.nb1 + blk)) * stage_bytes + (size_t)g * 1024;
        const bool half = (NT & 1) && g == G::WB_INSTR - 1;
        dma_one(lds0 + (unsigned)((G::PLANES_DW + ((grp & 1) * G::G + u) * G::WB_DW + g * 256) * 4), half ? vlast : vlin, sbase);
      }
    }
  };
  auto dma_wait = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };

  f32x4 acc[4][2][NT];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[q][i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int frow = lane & 15;
  const int g4 = lane >> 4;
  // per-lane dword offsets of the fragments inside a 24-dword [hi|mid|lo] row (as upconv_s3.hip)
  const int a1off = 4 * g4;                                  // [x_hi | x_mid]
  const int a2off = g4 < 2 ? 16 + 4 * g4 : 4 * g4 - 8;       // [x_lo | x_hi ]
  const int w1off = 4 * (g4 & 1);                            // [w_hi | w_hi ]
  const int w2off = 8 + 4 * (g4 & 1);                        // [w_mid| w_mid]
  const int w3off = g4 < 2 ? 4 * g4 : 4 * g4 + 8;            // [w_hi | w_lo ]

  // one tap of one parity: the pixel fragments at abase + i * istride, NP W rows at wb
#define CCVPE_S3Q_TAP(PAR, abase, istride, wb)                                                              \
  {                                                                                                         \
    f32x4 a1[2], a2[2];                                                                                     \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                         \
      a1[i] = *reinterpret_cast<const f32x4*>((abase) + i * (istride) + a1off);                             \
      a2[i] = *reinterpret_cast<const f32x4*>((abase) + i * (istride) + a2off);                             \
    }                                                                                                       \
    _Pragma("unroll") for (int j = 0; j < NT; ++j) {                                                        \
      const f32x4 w1 = *reinterpret_cast<const f32x4*>((wb) + j * 16 * ROW + w1off);                        \
      const f32x4 w2 = *reinterpret_cast<const f32x4*>((wb) + j * 16 * ROW + w2off);                        \
      const f32x4 w3 = *reinterpret_cast<const f32x4*>((wb) + j * 16 * ROW + w3off);                        \
      _Pragma("unroll") for (int i = 0; i < 2; ++i) acc[PAR][i][j] = mfma_stage<bf16_t>(w1, a1[i], acc[PAR][i][j]); \
      _Pragma("unroll") for (int i = 0; i < 2; ++i) acc[PAR][i][j] = mfma_stage<bf16_t>(w2, a1[i], acc[PAR][i][j]); \
      _Pragma("unroll") for (int i = 0; i < 2; ++i) acc[PAR][i][j] = mfma_stage<bf16_t>(w3, a2[i], acc[PAR][i][j]); \
    }                                                                                                       \
  }

  // ================= phase A: low-res source; the halo staged once per 16-channel chunk, one stage per parity ==============
  const float* hfrag = Us + (wave * 2 * HC + frow) * ROW;
  const float* wfrag_a = WsA + frow * ROW;
  load_halo(0);
  dma_a(0, 0, 0);
  store_halo();
  dma_wait();
  __syncthreads();
  for (int chunk = 0; chunk < p.nb0; ++chunk) {
    const bool next_halo = chunk + 1 < p.nb0;
    if (next_halo) load_halo(chunk + 1);
#pragma unroll
    for (int par = 0; par < 4; ++par) {
      if (par < 3) dma_a(chunk, par + 1, (par + 1) & 1);
      else if (next_halo) dma_a(chunk + 1, 0, 0);
      const int py = par >> 1, px = par & 1;
#pragma unroll
      for (int tap = 0; tap < 4; ++tap) {
        const int du = tap >> 1, dv = tap & 1;
        CCVPE_S3Q_TAP(par, hfrag + ((du + py) * HC + dv + px) * ROW, HC * ROW, wfrag_a + ((par & 1) * G::WA_DW + tap * NP * ROW));
      }
      dma_wait();
      __syncthreads();
    }
    if (next_halo) {                                       // every wave is done reading the halo -> overwrite it
      store_halo();
      __syncthreads();
    }
  }

  // ================= phase B: skip; per 16-channel block the planes staged once, then 36 (parity, tap) products ==============
  // (phase A ended on a barrier: the halo and both of its W buffers are dead)
  const float* pfrag = Us + (wave * 2 * PC + frow) * ROW;
  const float* wfrag_b = WsB + frow * ROW;
  for (int blk = 0; blk < p.nb1; ++blk) {
    dma_b(blk, 0);
    stage_planes(blk);
    dma_wait();
    __syncthreads();
#pragma unroll
    for (int grp = 0; grp < NGRP; ++grp) {
      if (grp + 1 < NGRP) dma_b(blk, grp + 1);
#pragma unroll
      for (int u = 0; u < G::G; ++u) {
        const int seq = grp * G::G + u;
        const int par = seq / 9, tap = seq % 9;
        const int r = (par >> 1) + tap / 3, c = (par & 1) + tap % 3;
        CCVPE_S3Q_TAP(par, pfrag + ((((r & 1) * 2 + (c & 1)) * PR + (r >> 1)) * PC + (c >> 1)) * ROW, PC * ROW,
                      wfrag_b + ((grp & 1) * G::G + u) * G::WB_DW);
      }
      dma_wait();
      __syncthreads();                                     // also: every wave is done with the planes before the next block's
    }
  }
#undef CCVPE_S3Q_TAP

  // ---- epilogue per parity (as upconv_s3_kernel) ------------------------------------------------------------------------
  const int epix = lane & 15;
  const int en = (lane >> 4) * 4;
  IgemmParams ep{};
  ep.N = p.N; ep.act = p.act; ep.residual = nullptr; ep.dst = p.dst; ep.out_f32 = 1;
  const float one[4] = {1.f, 1.f, 1.f, 1.f};
  const int x1 = x0 + epix;
  auto epilogue = [&](auto act_tag) {
  constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
  for (int par = 0; par < 4; ++par) {
    const int py = par >> 1, px = par & 1;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int y1 = y0 + wave * 2 + i;
      if (y1 >= p.H1 || x1 >= p.W1) continue;
      const int Y = 2 * y1 + py, X = 2 * x1 + px;
      const int rc = Y == 0 ? 0 : (Y == H2 - 1 ? 2 : 1);
      const int cc = X == 0 ? 0 : (X == W2 - 1 ? 2 : 1);
      const float* shp = p.shift9 + (size_t)(rc * 3 + cc) * p.N;
      const size_t pix = (size_t)(b * H2 + Y) * W2 + X;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int n = j * 16 + en;
        if (n >= p.N) continue;
        float sh[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) sh[q] = (n + q < p.N) ? shp[n + q] : 0.f;
        store4<float, ACT>(ep, acc[par][i][j], n, pix * p.ldd + n, 0, one, sh);
      }
    }
  }
  };
  CCVPE_ACT_DISPATCH(p.act, epilogue);
}

template <int NT>
static int launch_s3q(UpS3qParams p, hipStream_t stream) {
  using G = UpS3qGeom<NT>;
  static_assert(G::LDS_BYTES <= 80 * 1024, "upconv_s3q_kernel: two workgroups per CU");
  p.tiles_total = ((p.W1 + 15) / 16) * ((p.H1 + G::TH - 1) / G::TH) * p.batch;      // < 2^31: s3_pick() bounds the pixel count
  static DevCache lds_set;                      // per instantiation
  if (int rc = ensure_dyn_lds(lds_set, upconv_s3q_kernel<NT>, G::LDS_BYTES, "upconv_s3q_kernel")) return rc;
  hipLaunchKernelGGL((upconv_s3q_kernel<NT>), dim3(p.tiles_total), dim3(256), G::LDS_BYTES, stream, p);
  return check_launch("upconv_s3q_kernel");
}

// The NT = Npad / 16 the kernel is instantiated for, written once: the quad form's N range (16 < n <= 80) and its launch.
#define CCVPE_S3Q_NTS(X) X(2) X(3) X(4) X(5)

// the quad form's own shape conditions, for a desc upconv_s3.hip's s3_pick() has accepted
bool upconv_s3q_serves(const ccvpe_upconv_desc* d) {
  const int nt = (d->n + 15) / 16;
#define CCVPE_CASE(NT_) if (nt == NT_) return d->w1 >= 16;
  CCVPE_S3Q_NTS(CCVPE_CASE)
#undef CCVPE_CASE
  return false;
}

int upconv_s3q_launch(const ccvpe_upconv_desc* d, hipStream_t stream) {
  UpS3qParams p;
  s3_fill(d, p);
  const int nt = (d->n + 15) / 16;
#define CCVPE_CASE(NT_) if (nt == NT_) return launch_s3q<NT_>(p, stream);
  CCVPE_S3Q_NTS(CCVPE_CASE)
#undef CCVPE_CASE
  return fail(CCVPE_EINVAL, "upconv3x3_s3: no quad tile");
}

}  // namespace ccvpe
