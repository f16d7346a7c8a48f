// Fused MBConv front half: expand 1x1 + BN0 + swish -> depthwise KxK (stride S) + BN1 + swish, plus
// the SE squeeze partial sums.  efficientnet_pytorch/model.py:102-110,114.
//
// Why: the 6x-expanded tensor is the largest in the network (25 MB fp32 per aerial sample at block 1)
// and the unfused path writes it and reads it back (about half of all encoder HBM bytes).  Here it
// lives only in LDS.
//
// Round 3 mapping (the round-2 kernel owned 16 channels x a band of FULL-WIDTH rows and alternated a one-row expand phase
// with a one-row depthwise phase: two barriers per output row around a few hundred cycles of work each, and x re-fetched
// mid/16 times by different workgroups — 0.94 TB/s, 22 % MFMA-busy):
//   * a workgroup owns (sample, SPATIAL tile of TOH x 16 output pixels) and loops over ALL mid/16 channel chunks, so the
//     x halo tile ((TOH-1)*S+K) x (15*S+K) pixels is fetched by ONE workgroup (first chunk from HBM, the rest from L1/L2);
//   * per chunk ONE expand phase for the whole halo tile: its pixels are numbered linearly and cut into 16-pixel MFMA tiles
//     (no idle waves whatever the row width), x fragments are loaded straight from global memory in operand layout
//     (lane = pixel l&15, k group l>>4 -> 16 bytes; groups of tiles in flight together), v_mfma accumulates, BN0 + swish,
//     one ds_write_b128 per lane into the LDS tile [pixel][16 ch], pixel pitch 20 floats (conflict-free for the writes and
//     for the depthwise reads below).  Pixels outside the image are ZEROS (the depthwise conv pads the EXPANDED tensor);
//     circular padding is an index wrap of the source column;
//   * ONE depthwise phase per chunk: thread = (4 channels, 4/S adjacent output columns, row) slides the window through
//     registers — K + (4/S - 1)*S reads per kernel row instead of K per output (LDS bandwidth is the roof of this phase for
//     k = 5) — BN1 + swish, 16-byte stores, per-channel sums for the squeeze reduced by a fixed butterfly;
//   * two barriers per (tile, chunk) around ~10x the work of the old per-row phases; 3-4 workgroups per CU overlap each
//     other's phases.
// Halo recompute: ((TOH-1)*S+K)*(15*S+K) / (TOH*S*16*S) = 1.10 (k3 s2) ... 1.56 (k5 s1) of the expand work, which is the
// cheap part (MFMA).
#include "common.h"
#include "mbconv_plane.h"
#include "split3_impl.h"      // split3, the fragment offsets of the three-plane form
#include <type_traits>

namespace ccvpe {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int mbf_i32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 keepv(f32x4 v, bool keep) {       // v or all-zero bits, without a branch
  return __builtin_bit_cast(f32x4, __builtin_bit_cast(mbf_i32x4, v) & (keep ? -1 : 0));
}

struct MbFrontParams {
  const void* x;
  const void* w_exp;
  const float* s0;
  const float* b0;
  const float* w_dw;
  const float* s1;
  const float* b1;
  void* y;
  float* se_partial;
  int H, W, Cin, kpad, mid, Ho, Wo, circular;
  int tiles_x, tiles_y, nchunks, total_blocks;
  int ngroups, cpg;      // the chunk loop of a tile is cut into ngroups workgroups of cpg chunks when there are few tiles
};

constexpr int MBF_MAX_KK = 3;   // Cin <= 48 (fp32) / 96 (bf16)

// TOH = output rows of the tile (16 columns wide).  The x fragments of the whole halo tile stay in REGISTERS across the
// channel-chunk loop (TPW tiles x NKK pieces of 16 bytes per lane), so TOH is chosen per (k, stride, Cin) to keep that at
// <= ~14 registers-of-4 (mbf_toh below; the choice must not depend on the storage type: it fixes the squeeze-partial rows).
template <int K, int S, int TOH>
struct MbfGeom {
  static constexpr int NOUT = TOH / 4;               // adjacent output columns per depthwise thread (256 = 4 cg x 16/NOUT x TOH)
  static constexpr int IH = (TOH - 1) * S + K;
  static constexpr int IW = 15 * S + K;
  static constexpr int NPX = IH * IW;
  static constexpr int NT = (NPX + 15) / 16;         // 16-pixel MFMA tiles of the halo
  static constexpr int TPW = (NT + 3) / 4;           // tiles per wave
  // LDS pixel pitch (floats): neighbouring column groups of the depthwise phase are NOUT*S pixels apart; their 16-byte reads
  // are conflict-free when that distance is 16 or 48 floats modulo 64
  static constexpr int PITCH = (NOUT * S == 2) ? 24 : 20;
  static constexpr int LDS_FLOATS = NT * 16 * PITCH + 2 * K * K * 16 + 64;
};

// TE = storage type of x / w_exp / y (float or bf16).  NKK counts 64-byte K pieces: 16 fp32 or 32 bf16
// input channels each; the LDS tile (expanded tensor) and all depthwise math stay fp32 either way.
template <typename TE, int K, int S, int NKK, int TOH>
__global__ __launch_bounds__(256, 3) void mbconv_front_kernel(const MbFrontParams p) {
  using G = MbfGeom<K, S, TOH>;
  constexpr int E = 16 / sizeof(TE);
  constexpr int SK = 4 * E;
  constexpr int PB = (S == 1) ? (K - 1) / 2 : (K - 2) / 2;   // pad before (224-schedule SAME)
  constexpr int IW = G::IW, NPX = G::NPX, NT = G::NT, TPW = G::TPW, PITCH = G::PITCH;
  constexpr int KYU = 1;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* tile = sm;                                  // [NT*16][PITCH]
  float* wdw = sm + NT * 16 * PITCH;                 // [2][K*K][16]
  float* red = wdw + 2 * K * K * 16;                 // [4 waves][4 cg][4]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;

  int lb;
  {
    const int q = p.total_blocks / 8, r = p.total_blocks % 8;
    const int xcd = blockIdx.x % 8, loc = blockIdx.x / 8;
    lb = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
  }
  const int grp = lb % p.ngroups;                    // chunk groups of one tile are neighbours: they re-read the same x halo
  lb /= p.ngroups;
  const int tx = lb % p.tiles_x;                     // neighbouring tiles (shared halo) on one XCD
  const int ty = (lb / p.tiles_x) % p.tiles_y;
  const int b = lb / (p.tiles_x * p.tiles_y);
  const int oy0 = ty * TOH, ox0 = tx * 16;
  const int iy0 = oy0 * S - PB, ix0 = ox0 * S - PB;
  const int kq = (lane >> 4) * E;                    // first input channel of this lane's k group inside a 64-byte piece
  const int q4 = (lane >> 4) * 4;                    // D rows (channels) of this lane: q4 .. q4+3

  // ---- the x halo tile, ONCE: this wave's 16-pixel tiles t = wave + 4*i, lane -> pixel q = 16*t + (lane & 15), straight
  // from global memory in MFMA operand layout (16 bytes of k group lane>>4); all TPW*NKK loads in flight together.  Pixels
  // outside the image read a clamped address; their EXPANDED value is forced to zero below (the depthwise conv pads the
  // expanded tensor); k groups beyond Cin re-read the pixel's first channels and meet the zero padding of the packed weights.
  const TE* xb = reinterpret_cast<const TE*>(p.x) + (size_t)b * p.H * p.W * p.Cin;
  f32x4 xr[TPW][NKK];
  unsigned pvalid = 0;
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int q = 16 * (wave + 4 * i) + (lane & 15);
    const int hy = q / IW, hx = q - hy * IW;
    const int gy = iy0 + hy;
    int gx = ix0 + hx;
    if (p.circular) gx = gx < 0 ? gx + p.W : (gx >= p.W ? gx - p.W : gx);
    const bool ok = q < NPX && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
    pvalid |= ok ? (1u << i) : 0u;
    const unsigned off = ok ? (unsigned)((gy * p.W + gx) * p.Cin) * (unsigned)sizeof(TE) : 0u;
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) {
      const int ch = kk * SK + kq;
      xr[i][kk] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(xb) + off + (unsigned)(ch < p.Cin ? ch : 0) * (unsigned)sizeof(TE));
    }
  }

  // ---- depthwise-phase coordinates -----------------------------------------------------------------------------------------
  constexpr int NOUT = G::NOUT;
  constexpr int NCOLS = (NOUT - 1) * S + K;          // input columns read per kernel row
  constexpr int XG = 16 / NOUT;                      // column groups per tile row
  const int cg = tid & 3;
  const int oxg = (tid >> 2) % XG;
  const int oyl = (tid >> 2) / XG;                   // 0 .. TOH-1
  const int oy = oy0 + oyl;
  const int oxl = oxg * NOUT;
  const bool row_ok = oy < p.Ho;
  TE* yrow = reinterpret_cast<TE*>(p.y) + ((size_t)(b * p.Ho + (row_ok ? oy : 0)) * p.Wo) * p.mid;
  const float* trow = tile + ((oyl * S) * IW + oxl * S) * PITCH + cg * 4;

  // ---- per-chunk parameters: loaded one chunk AHEAD (under the previous chunk's depthwise phase) ------------------------------
  f32x4 wf[NKK], sc0, sh0, sc1, sh1, wdr;
  auto load_chunk_params = [&](int chunk) {
    const int c0 = chunk * 16;
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk)   // expand weights: MFMA A operand, row n = lane&15, k group = lane>>4
      wf[kk] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const TE*>(p.w_exp) + (size_t)(c0 + (lane & 15)) * p.kpad + kk * SK + kq);
    sc0 = *reinterpret_cast<const f32x4*>(p.s0 + c0 + q4);
    sh0 = *reinterpret_cast<const f32x4*>(p.b0 + c0 + q4);
    sc1 = *reinterpret_cast<const f32x4*>(p.s1 + c0 + cg * 4);
    sh1 = *reinterpret_cast<const f32x4*>(p.b1 + c0 + cg * 4);
    const int wi = tid < K * K * 4 ? tid : 0;        // depthwise weights [tap][16]: one 16-byte piece per thread
    wdr = *reinterpret_cast<const f32x4*>(p.w_dw + (size_t)(wi >> 2) * p.mid + c0 + (wi & 3) * 4);
  };
  const int chunk_begin = grp * p.cpg, chunk_end = min(p.nchunks, chunk_begin + p.cpg);
  load_chunk_params(chunk_begin);

  for (int chunk = chunk_begin; chunk < chunk_end; ++chunk) {
    const int c0 = chunk * 16;
    float* wd = wdw + (chunk & 1) * K * K * 16;
    if (tid < K * K * 4) *reinterpret_cast<f32x4*>(wd + tid * 4) = wdr;
    // ---- expand: registers -> MFMA -> BN0 + swish -> LDS tile (no global loads in this phase) ------------------------------
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
      if (wave + 4 * i < NT) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
          if (sizeof(TE) == 4) {
#pragma unroll
            for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[kk][r], xr[i][kk][r], acc, 0, 0, 0);
          } else {
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(cc_bf16x8, wf[kk]), __builtin_bit_cast(cc_bf16x8, xr[i][kk]),
                                                          acc, 0, 0, 0);
          }
        }
        // D: row = channel q4 + reg, col = pixel lane & 15
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = swishf(acc[r] * sc0[r] + sh0[r]);
        // one mask word per tile, made from its bit when it is needed (a vector `keep ? -1 : 0` select was hoisted out of the
        // chunk loop as FOUR mask registers per tile: 36 VGPRs for 9 tiles)
        const bool inside = (pvalid >> i) & 1u;      // a lane mask in scalar registers, four selects
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = inside ? o[r] : 0.f;
        *reinterpret_cast<f32x4*>(tile + (16 * (wave + 4 * i) + (lane & 15)) * PITCH + q4) = o;
      }
      // two tiles at a time (two independent accumulator chains); without the fence the scheduler issues the MFMAs of all
      // TPW tiles first and keeps every accumulator + swish temporary live
      if (i & 1) __builtin_amdgcn_sched_barrier(0);
    }
    const f32x4 sc1c = sc1, sh1c = sh1;              // this chunk's BN1 (the registers are re-loaded below)
    __syncthreads();
    if (chunk + 1 < chunk_end) load_chunk_params(chunk + 1);   // in flight under the depthwise phase

    // ---- depthwise: NOUT adjacent outputs of one row for 4 channels, window slid through registers -------------------------
    f32x4 acc[NOUT];
#pragma unroll
    for (int t = 0; t < NOUT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // one kernel row of window reads in flight at a time (fully unrolled the scheduler hoists all of them: 200+ VGPRs)
#pragma unroll KYU
    for (int ky = 0; ky < K; ++ky) {
      f32x4 col[NCOLS];
#pragma unroll
      for (int j = 0; j < NCOLS; ++j) col[j] = *reinterpret_cast<const f32x4*>(trow + (ky * IW + j) * PITCH);
#pragma unroll
      for (int kx = 0; kx < K; ++kx) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wd + (ky * K + kx) * 16 + cg * 4);
#pragma unroll
        for (int t = 0; t < NOUT; ++t) acc[t] += col[t * S + kx] * wv;
      }
    }
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NOUT; ++t) {
      const int ox = ox0 + oxl + t;
      f32x4 o = acc[t] * sc1c + sh1c;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = swishf(o[r]);
      if (row_ok && ox < p.Wo) {
        st4<TE>(yrow + (size_t)ox * p.mid + c0 + cg * 4, o);
        sum += o;
      }
    }
    // squeeze partial of this (tile, chunk): fixed butterfly over the 16 lanes of a wave that share cg, then the 4 waves
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) {
#pragma unroll
      for (int r = 0; r < 4; ++r) sum[r] += __shfl_xor(sum[r], o, 64);
    }
    if (lane < 4) *reinterpret_cast<f32x4*>(red + (wave * 4 + lane) * 4) = sum;
    __syncthreads();                                 // the tile is free for the next chunk; red is published
    if (tid < 4) {
      f32x4 t = *reinterpret_cast<const f32x4*>(red + tid * 4);
#pragma unroll
      for (int w = 1; w < 4; ++w) t += *reinterpret_cast<const f32x4*>(red + (w * 4 + tid) * 4);
      *reinterpret_cast<f32x4*>(p.se_partial + ((size_t)b * (p.tiles_x * p.tiles_y) + ty * p.tiles_x + tx) * p.mid + c0 + tid * 4) = t;
    }
    // (red is rewritten only after the NEXT chunk's first barrier)
  }
}

// ---- Three-plane form of the fp32 kernel (blocks 1-5 of the fp32 eval forward) -------------------------------------------------------
// Everything but the expand phase is the kernel above: tile geometry, LDS tile, depthwise phase, squeeze butterfly, partial rows.
// The expand 1x1 runs on the bf16 matrix pipe in the arithmetic of upconv_s3.hip (three bf16 planes per fp32 operand, six products,
// three v_mfma_f32_16x16x32_bf16 per 16 input channels instead of four v_mfma_f32_16x16x4_f32, which issue on the vector fp32 pipe
// beside the swishes this kernel is bounded by):
//   * x: a lane loads 8 consecutive fp32 channels (those of its k group, (lane >> 4 & 1) * 8 ..) of its pixel per 16-channel block and
//     splits them ONCE, before the chunk loop, into its two B fragments [x_hi|x_mid] and [x_lo|x_hi] (S3Frag's a1 / a2: lane groups
//     0-1 hold the first plane, 2-3 the second) — 8 registers per tile and block, re-used by all mid / 16 chunks;
//   * W: the host's three-plane pack [block][mid][hi 16 | mid 16 | lo 16] (models._pack_pw_s3 of the fp32 pack: the planes sum to it
//     exactly; channels beyond Cin are zero in all planes).  A chunk's rows (16 x 96 bytes per block) are fetched one chunk ahead
//     under the depthwise phase, parked in LDS before the chunk's closing barrier ([2] buffers) and read as the three A fragments
//     [w_hi|w_hi], [w_mid|w_mid], [w_hi|w_lo] per block at the top of the expand phase: they are live in registers only there.
typedef unsigned mbf_u32x4 __attribute__((ext_vector_type(4)));

template <int K, int S, int NKB, int TOH>
struct Mbf3Geom {
  using G = MbfGeom<K, S, TOH>;
  static constexpr int W_DW = NKB * 16 * S3_ROW;       // dwords of one chunk's W rows in LDS: [block][16 rows][24]
  static constexpr int W_OFF = G::LDS_FLOATS;           // behind the fp32 kernel's layout
  static constexpr int LDS_FLOATS = W_OFF + 2 * W_DW;
};

template <int K, int S, int NKB, int TOH, int WGS>
__global__ __launch_bounds__(256, WGS) void mbconv_front_s3_kernel(const MbFrontParams p) {
  using G = MbfGeom<K, S, TOH>;
  using G3 = Mbf3Geom<K, S, NKB, TOH>;
  constexpr int PB = (S == 1) ? (K - 1) / 2 : (K - 2) / 2;   // pad before (224-schedule SAME)
  constexpr int IW = G::IW, NPX = G::NPX, NT = G::NT, TPW = G::TPW, PITCH = G::PITCH;
  constexpr int KYU = 1;
  constexpr int W_DW = G3::W_DW, WPIECES = W_DW / 4, WPT = (WPIECES + 255) / 256;   // 16-byte pieces of a chunk's W; per thread
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* tile = sm;                                  // [NT*16][PITCH]
  float* wdw = sm + NT * 16 * PITCH;                 // [2][K*K][16]
  float* red = wdw + 2 * K * K * 16;                 // [4 waves][4 cg][4]
  float* wl = sm + G3::W_OFF;                        // [2][NKB][16][S3_ROW]: the chunk's three-plane expand weights

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int g4 = lane >> 4;

  int lb;
  {
    const int q = p.total_blocks / 8, r = p.total_blocks % 8;
    const int xcd = blockIdx.x % 8, loc = blockIdx.x / 8;
    lb = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
  }
  const int grp = lb % p.ngroups;
  lb /= p.ngroups;
  const int tx = lb % p.tiles_x;
  const int ty = (lb / p.tiles_x) % p.tiles_y;
  const int b = lb / (p.tiles_x * p.tiles_y);
  const int oy0 = ty * TOH, ox0 = tx * 16;
  const int iy0 = oy0 * S - PB, ix0 = ox0 * S - PB;
  const int q4 = g4 * 4;                             // D rows (channels) of this lane: q4 .. q4+3

  // ---- per-chunk parameters, one chunk AHEAD; the expand weights go through registers into LDS (load_w / park_w) ----------------
  f32x4 sc0, sh0, sc1, sh1, wdr, wr[WPT];
  const int cg = tid & 3;
  auto load_chunk_params = [&](int chunk) {
    const int c0 = chunk * 16;
#pragma unroll
    for (int j = 0; j < WPT; ++j) {
      const int idx = tid + 256 * j;                 // piece idx = block * 96 + (row * 6 + piece of the row): LDS order == pack order
      if (idx < WPIECES) {
        const int kb = idx / 96, pc = idx - kb * 96;
        wr[j] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.w_exp) + ((size_t)kb * p.mid + c0) * S3_ROW + pc * 4);
      }
    }
    sc0 = *reinterpret_cast<const f32x4*>(p.s0 + c0 + q4);
    sh0 = *reinterpret_cast<const f32x4*>(p.b0 + c0 + q4);
    sc1 = *reinterpret_cast<const f32x4*>(p.s1 + c0 + cg * 4);
    sh1 = *reinterpret_cast<const f32x4*>(p.b1 + c0 + cg * 4);
    const int wi = tid < K * K * 4 ? tid : 0;        // depthwise weights [tap][16]: one 16-byte piece per thread
    wdr = *reinterpret_cast<const f32x4*>(p.w_dw + (size_t)(wi >> 2) * p.mid + c0 + (wi & 3) * 4);
  };
  auto park_w = [&](int chunk) {
#pragma unroll
    for (int j = 0; j < WPT; ++j) {
      const int idx = tid + 256 * j;
      if (idx < WPIECES) *reinterpret_cast<f32x4*>(wl + (chunk & 1) * W_DW + idx * 4) = wr[j];
    }
  };
  const int chunk_begin = grp * p.cpg, chunk_end = min(p.nchunks, chunk_begin + p.cpg);
  load_chunk_params(chunk_begin);

  // ---- the x halo tile, ONCE: this wave's 16-pixel tiles t = wave + 4*i, lane -> pixel q = 16*t + (lane & 15); 32 bytes of fp32 per
  // lane and block, split into the two B fragments.  Pixels outside the image read a clamped address (their EXPANDED value is forced
  // to zero below); channel groups beyond Cin re-read the pixel's first channels and meet the zero planes of the packed weights.
  const float* xb = reinterpret_cast<const float*>(p.x) + (size_t)b * p.H * p.W * p.Cin;
  mbf_u32x4 xa1[TPW][NKB], xa2[TPW][NKB];
  unsigned pvalid = 0;
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int q = 16 * (wave + 4 * i) + (lane & 15);
    const int hy = q / IW, hx = q - hy * IW;
    const int gy = iy0 + hy;
    int gx = ix0 + hx;
    if (p.circular) gx = gx < 0 ? gx + p.W : (gx >= p.W ? gx - p.W : gx);
    const bool ok = q < NPX && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
    pvalid |= ok ? (1u << i) : 0u;
    const unsigned off = ok ? (unsigned)((gy * p.W + gx) * p.Cin) * 4u : 0u;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      const int ch = kb * 16 + (g4 & 1) * 8;
      const char* src = reinterpret_cast<const char*>(xb) + off + (unsigned)(ch < p.Cin ? ch : 0) * 4u;
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 16);
      u32x2 h0, m0, l0, h1, m1, l1;
      split3(v0, h0, m0, l0);
      split3(v1, h1, m1, l1);
      const mbf_u32x4 hi = {h0[0], h0[1], h1[0], h1[1]}, mi = {m0[0], m0[1], m1[0], m1[1]}, lo = {l0[0], l0[1], l1[0], l1[1]};
      xa1[i][kb] = g4 < 2 ? hi : mi;                 // [x_hi|x_mid]
      xa2[i][kb] = g4 < 2 ? lo : hi;                 // [x_lo|x_hi ]
    }
  }
  park_w(chunk_begin);
  __syncthreads();

  // ---- depthwise-phase coordinates -----------------------------------------------------------------------------------------
  constexpr int NOUT = G::NOUT;
  constexpr int NCOLS = (NOUT - 1) * S + K;          // input columns read per kernel row
  constexpr int XG = 16 / NOUT;                      // column groups per tile row
  const int oxg = (tid >> 2) % XG;
  const int oyl = (tid >> 2) / XG;                   // 0 .. TOH-1
  const int oy = oy0 + oyl;
  const int oxl = oxg * NOUT;
  const bool row_ok = oy < p.Ho;
  float* yrow = reinterpret_cast<float*>(p.y) + ((size_t)(b * p.Ho + (row_ok ? oy : 0)) * p.Wo) * p.mid;
  const float* trow = tile + ((oyl * S) * IW + oxl * S) * PITCH + cg * 4;
  const S3Frag fr(g4);

  for (int chunk = chunk_begin; chunk < chunk_end; ++chunk) {
    const int c0 = chunk * 16;
    float* wd = wdw + (chunk & 1) * K * K * 16;
    if (tid < K * K * 4) *reinterpret_cast<f32x4*>(wd + tid * 4) = wdr;
    // ---- expand: the chunk's A fragments from LDS, registers -> MFMA -> BN0 + swish -> LDS tile -----------------------------------
    cc_bf16x8 w1[NKB], w2[NKB], w3[NKB];
    {
      const float* wrow = wl + (chunk & 1) * W_DW + (lane & 15) * S3_ROW;
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
        w1[kb] = __builtin_bit_cast(cc_bf16x8, *reinterpret_cast<const f32x4*>(wrow + kb * 16 * S3_ROW + fr.w1));
        w2[kb] = __builtin_bit_cast(cc_bf16x8, *reinterpret_cast<const f32x4*>(wrow + kb * 16 * S3_ROW + fr.w2));
        w3[kb] = __builtin_bit_cast(cc_bf16x8, *reinterpret_cast<const f32x4*>(wrow + kb * 16 * S3_ROW + fr.w3));
      }
    }
    // two tiles at a time, software-pipelined: the MFMA chains of the next pair are issued before the BN0 + swish of this pair, so
    // the matrix pipe works under the vector work of the same wave (the fences keep the scheduler from hoisting every chain to the
    // top and holding all accumulators live).  Only a wave's LAST tile can lie beyond NT.
    auto has = [&](int i) { return i < TPW - 1 || wave + 4 * i < NT; };
    auto chain = [&](int i) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
        const cc_bf16x8 a1 = __builtin_bit_cast(cc_bf16x8, xa1[i][kb]), a2 = __builtin_bit_cast(cc_bf16x8, xa2[i][kb]);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1[kb], a1, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2[kb], a1, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w3[kb], a2, acc, 0, 0, 0);
      }
      return acc;
    };
    auto finish = [&](int i, f32x4 acc) {            // D: row = channel q4 + reg, col = pixel lane & 15
      f32x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = swishf(acc[r] * sc0[r] + sh0[r]);
      const bool inside = (pvalid >> i) & 1u;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = inside ? o[r] : 0.f;
      *reinterpret_cast<f32x4*>(tile + (16 * (wave + 4 * i) + (lane & 15)) * PITCH + q4) = o;
    };
    constexpr int NPAIR = (TPW + 1) / 2;
    f32x4 pacc[2][2];
    pacc[0][0] = chain(0);
    if (1 < TPW && has(1)) pacc[0][1] = chain(1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int pp = 0; pp < NPAIR; ++pp) {
      const int n0 = 2 * pp + 2, n1 = 2 * pp + 3;
      if (n0 < TPW && has(n0)) pacc[(pp + 1) & 1][0] = chain(n0);
      if (n1 < TPW && has(n1)) pacc[(pp + 1) & 1][1] = chain(n1);
      if (has(2 * pp)) finish(2 * pp, pacc[pp & 1][0]);
      if (2 * pp + 1 < TPW && has(2 * pp + 1)) finish(2 * pp + 1, pacc[pp & 1][1]);
      __builtin_amdgcn_sched_barrier(0);
    }
    const f32x4 sc1c = sc1, sh1c = sh1;              // this chunk's BN1 (the registers are re-loaded below)
    __syncthreads();
    const bool more = chunk + 1 < chunk_end;
    if (more) load_chunk_params(chunk + 1);          // in flight under the depthwise phase

    // ---- depthwise: NOUT adjacent outputs of one row for 4 channels, window slid through registers -------------------------
    f32x4 acc[NOUT];
#pragma unroll
    for (int t = 0; t < NOUT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll KYU
    for (int ky = 0; ky < K; ++ky) {
      f32x4 col[NCOLS];
#pragma unroll
      for (int j = 0; j < NCOLS; ++j) col[j] = *reinterpret_cast<const f32x4*>(trow + (ky * IW + j) * PITCH);
#pragma unroll
      for (int kx = 0; kx < K; ++kx) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wd + (ky * K + kx) * 16 + cg * 4);
#pragma unroll
        for (int t = 0; t < NOUT; ++t) acc[t] += col[t * S + kx] * wv;
      }
    }
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NOUT; ++t) {
      const int ox = ox0 + oxl + t;
      f32x4 o = acc[t] * sc1c + sh1c;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = swishf(o[r]);
      if (row_ok && ox < p.Wo) {
        st4<float>(yrow + (size_t)ox * p.mid + c0 + cg * 4, o);
        sum += o;
      }
    }
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) {
#pragma unroll
      for (int r = 0; r < 4; ++r) sum[r] += __shfl_xor(sum[r], o, 64);
    }
    if (lane < 4) *reinterpret_cast<f32x4*>(red + (wave * 4 + lane) * 4) = sum;
    if (more) park_w(chunk + 1);                     // the other buffer: last read before this chunk's first barrier
    __syncthreads();                                 // the tile is free for the next chunk; red and the next W are published
    if (tid < 4) {
      f32x4 t = *reinterpret_cast<const f32x4*>(red + tid * 4);
#pragma unroll
      for (int w = 1; w < 4; ++w) t += *reinterpret_cast<const f32x4*>(red + (w * 4 + tid) * 4);
      *reinterpret_cast<f32x4*>(p.se_partial + ((size_t)b * (p.tiles_x * p.tiles_y) + ty * p.tiles_x + tx) * p.mid + c0 + tid * 4) = t;
    }
  }
}

// output rows per tile for (k, stride, Cin): keeps TPW * ceil(Cin / 16) register fragments per lane small (see MbfGeom);
// depends on Cin through the fp32 piece count for BOTH storage types
static int mbf_toh(int k, int stride, int cin) {
  const int n = (cin + 15) / 16;
  if (stride == 2) return n == 1 ? 8 : 4;
  return (n == 1 && k == 3) ? 16 : 8;
}

// (k = 5, stride 2 with more than 32 input channels is not instantiated: 11 tiles x 3 pieces of x do not fit the register
// budget of 3 waves per SIMD; EfficientNet-B0 has no such block.)  `stride` < 0: any.
static bool mbf_supported(int W, int cin, int mid, int k, int sk = 16, int stride = -1) {
  (void)W;
  if (k == 5 && stride == 2 && cin > 32) return false;
  return cin % 8 == 0 && cin <= 16 * MBF_MAX_KK && cin <= sk * MBF_MAX_KK && mid % 16 == 0;
}

}  // namespace ccvpe

using namespace ccvpe;

// number of squeeze-partial rows per sample = spatial tiles per sample (0 => use the unfused kernels)
extern "C" int ccvpe_mbconv_front_nblk(int in_h, int in_w, int cin, int mid, int k, int stride) {
  if (!(k == 3 || k == 5) || !(stride == 1 || stride == 2)) return CCVPE_EINVAL;
  if (!mbf_supported(in_w, cin, mid, k, 16, stride))      // late blocks (small planes, wide inputs): csrc/mbconv_plane.hip
    return (g_mbplane_mode & 1) ? mbplane_nblk(in_h, in_w, cin, mid, k, stride) : 0;
  const int total_pad = (stride == 1) ? (k - 1) : (k - 2);
  const int Ho = (in_h + total_pad - k) / stride + 1, Wo = (in_w + total_pad - k) / stride + 1;
  const int toh = mbf_toh(k, stride, cin);
  return ((Ho + toh - 1) / toh) * ((Wo + 15) / 16);
}

// which kernel ccvpe_mbconv_front_* runs for a shape (reporting: bench.py's launch recorder, tests): 0 = not served (use the
// unfused calls), 1 = mbconv_front_kernel (early blocks), 2 = mbconv_plane_kernel (late blocks, one channel slice per workgroup),
// 3 = mbconv_band_kernel (late blocks, bf16: producer / consumer waves)
extern "C" int ccvpe_mbconv_front_route(int in_h, int in_w, int cin, int mid, int k, int stride, int is_bf16, int batch) {
  if (!(k == 3 || k == 5) || !(stride == 1 || stride == 2)) return CCVPE_EINVAL;
  if (mbf_supported(in_w, cin, mid, k, 16, stride)) return 1;
  if (!(g_mbplane_mode & 1) || mbplane_nblk(in_h, in_w, cin, mid, k, stride) <= 0) return 0;
  return (is_bf16 && (g_mbplane_mode & 4) && mbband_takes(in_h, in_w, cin, mid, k, stride, batch)) ? 3 : 2;
}

// the mbconv_band_kernel<k, stride, nkk, tpw class, ry> instantiation and the chunk grouping ccvpe_mbconv_front_bf16 launches for a
// shape, or 0 when another kernel (or none) serves it: the same helper the launcher runs (csrc/mbconv_plane.hip: mbband_plan)
extern "C" int ccvpe_mbconv_band_plan(int in_h, int in_w, int cin, int mid, int k, int stride, int batch) {
  if (ccvpe_mbconv_front_route(in_h, in_w, cin, mid, k, stride, 1, batch) != 3) return 0;
  return mbband_plan_packed(in_h, in_w, cin, mid, k, stride, batch);
}

// argument checks and the launch geometry shared by the fp32 / bf16 kernel and the three-plane form (esize: bytes per element of x / y)
static int mbf_fill(MbFrontParams& p, int& toh, size_t esize, const void* x, const void* w_exp, int kpad, const float* s0, const float* b0,
                    const float* w_dw, const float* s1, const float* b1, void* y, float* se_partial, int B, int H, int W, int cin,
                    int mid, int k, int stride, int circular) {
  if (!aligned16(x) || !aligned16(w_exp) || !aligned16(s0) || !aligned16(b0) || !aligned16(s1) || !aligned16(b1) ||
      !aligned16(y) || !aligned16(se_partial) || !aligned16(w_dw))
    return fail(CCVPE_EINVAL, "mbconv_front: pointers must be 16-byte aligned");
  if ((double)H * W * cin * esize >= 4294967296.0) return fail(CCVPE_EINVAL, "mbconv_front: sample larger than 4 GB");
  if (circular && W < k) return fail(CCVPE_EINVAL, "mbconv_front: W too small for circular wrap");
  p.x = x; p.w_exp = w_exp; p.s0 = s0; p.b0 = b0; p.w_dw = w_dw; p.s1 = s1; p.b1 = b1; p.y = y; p.se_partial = se_partial;
  p.H = H; p.W = W; p.Cin = cin; p.kpad = kpad; p.mid = mid; p.circular = circular;
  const int total_pad = (stride == 1) ? (k - 1) : (k - 2);
  p.Ho = (H + total_pad - k) / stride + 1;
  p.Wo = (W + total_pad - k) / stride + 1;
  toh = mbf_toh(k, stride, cin);
  p.tiles_x = (p.Wo + 15) / 16;
  p.tiles_y = (p.Ho + toh - 1) / toh;
  p.nchunks = mid / 16;
  // few tiles (small planes): cut the chunk loop so that the launch still has ~8 workgroups per CU
  const long tiles = (long)p.tiles_x * p.tiles_y * B;
  int ng = (int)((2048 + tiles - 1) / tiles);
  if (ng > p.nchunks) ng = p.nchunks;
  if (ng < 1) ng = 1;
  p.cpg = (p.nchunks + ng - 1) / ng;
  p.ngroups = (p.nchunks + p.cpg - 1) / p.cpg;
  const long total = tiles * p.ngroups;
  if (total > 0x7fffffffL) return fail(CCVPE_EINVAL, "mbconv_front: grid too large");
  p.total_blocks = (int)total;
  return CCVPE_OK;
}

template <typename TE>
static int mbconv_front_any(const void* x, const void* w_exp, int kpad, const float* s0, const float* b0,
                            const float* w_dw, const float* s1, const float* b1, void* y, float* se_partial, int B,
                            int H, int W, int cin, int mid, int k, int stride, int circular, void* stream) {
  constexpr int SK = 4 * (16 / (int)sizeof(TE));
  if (!(k == 3 || k == 5) || !(stride == 1 || stride == 2)) return fail(CCVPE_EINVAL, "mbconv_front: k/stride unsupported");
  if (!mbf_supported(W, cin, mid, k, 16, stride) && (g_mbplane_mode & 1) && mbplane_nblk(H, W, cin, mid, k, stride) > 0)
    return mbplane_launch(sizeof(TE) == 2, 1, x, w_exp, kpad, s0, b0, w_dw, s1, b1, y, se_partial, B, H, W, cin, mid, k, stride,
                          circular, stream);
  if (!mbf_supported(W, cin, mid, k, SK, stride)) return fail(CCVPE_EINVAL, "mbconv_front: shape not supported (W=%d cin=%d mid=%d)", W, cin, mid);
  if (kpad % SK || kpad < cin) return fail(CCVPE_EINVAL, "mbconv_front: bad kpad");
  MbFrontParams p;
  int toh;
  if (int rc0 = mbf_fill(p, toh, sizeof(TE), x, w_exp, kpad, s0, b0, w_dw, s1, b1, y, se_partial, B, H, W, cin, mid, k, stride, circular)) return rc0;
  hipStream_t st = (hipStream_t)stream;
  const int nkk = (cin + SK - 1) / SK;
  int rc = CCVPE_OK;
  auto go = [&](auto kern, int lds_floats) {
    const int lds = lds_floats * 4;
    static DevCache lds_set;                         // per instantiation (generic lambda)
    if ((rc = ensure_dyn_lds(lds_set, kern, lds, "mbconv_front"))) return;
    hipLaunchKernelGGL(kern, dim3(p.total_blocks), dim3(256), lds, st, p);
  };
  // instantiated: the big tile for Cin <= 16 (one K piece in either storage type), the small tile for 1-3 pieces
#define MBF_N(K_, S_, TOH_)                                                                                  \
  if (nkk == 1) go(mbconv_front_kernel<TE, K_, S_, 1, TOH_>, MbfGeom<K_, S_, TOH_>::LDS_FLOATS);                \
  else if (nkk == 2) go(mbconv_front_kernel<TE, K_, S_, 2, TOH_>, MbfGeom<K_, S_, TOH_>::LDS_FLOATS);           \
  else go(mbconv_front_kernel<TE, K_, S_, 3, TOH_>, MbfGeom<K_, S_, TOH_>::LDS_FLOATS)
#define MBF_T(K_, S_, BIG_, SMALL_)                                                                          \
  if (toh == BIG_) { go(mbconv_front_kernel<TE, K_, S_, 1, BIG_>, MbfGeom<K_, S_, BIG_>::LDS_FLOATS); } else { MBF_N(K_, S_, SMALL_); }
  if (k == 3 && stride == 1) { MBF_T(3, 1, 16, 8) }
  else if (k == 3 && stride == 2) { MBF_T(3, 2, 8, 4) }
  else if (k == 5 && stride == 1) { MBF_N(5, 1, 8); }
  else if (toh == 8) { go(mbconv_front_kernel<TE, 5, 2, 1, 8>, MbfGeom<5, 2, 8>::LDS_FLOATS); }
  else if (nkk == 1) { go(mbconv_front_kernel<TE, 5, 2, 1, 4>, MbfGeom<5, 2, 4>::LDS_FLOATS); }
  else { go(mbconv_front_kernel<TE, 5, 2, 2, 4>, MbfGeom<5, 2, 4>::LDS_FLOATS); }
#undef MBF_T
#undef MBF_N
  if (rc) return rc;
  return check_launch("mbconv_front_kernel");
}

extern "C" int ccvpe_mbconv_front_f32(const float* x, const float* w_exp, int kpad, const float* s0, const float* b0,
                                      const float* w_dw, const float* s1, const float* b1, float* y,
                                      float* se_partial, int B, int H, int W, int cin, int mid, int k, int stride,
                                      int circular, void* stream) {
  return mbconv_front_any<float>(x, w_exp, kpad, s0, b0, w_dw, s1, b1, y, se_partial, B, H, W, cin, mid, k, stride,
                                 circular, stream);
}
extern "C" int ccvpe_mbconv_front_bf16(const void* x, const void* w_exp, int kpad, const float* s0, const float* b0,
                                       const float* w_dw, const float* s1, const float* b1, void* y,
                                       float* se_partial, int B, int H, int W, int cin, int mid, int k, int stride,
                                       int circular, void* stream) {
  return mbconv_front_any<cc_bf16>(x, w_exp, kpad, s0, b0, w_dw, s1, b1, y, se_partial, B, H, W, cin, mid, k, stride,
                                   circular, stream);
}

// ---- the three-plane form: which shapes it serves, the measured size rule, the entry point ---------------------------------------------
// instantiated for the five early-block shapes of EfficientNet-B0: (k, stride, 16-channel blocks) = (3,2,1) (3,1,2) (5,2,2) (5,1,3) (3,2,3)
static bool mbf3_served(int in_w, int cin, int mid, int k, int stride) {
  if (!(k == 3 || k == 5) || !(stride == 1 || stride == 2) || !mbf_supported(in_w, cin, mid, k, 16, stride)) return false;
  const int nkb = (cin + 15) / 16;
  return (k == 3 && stride == 2 && (nkb == 1 || nkb == 3)) || (k == 3 && stride == 1 && nkb == 2) || (k == 5 && stride == 2 && nkb == 2) ||
         (k == 5 && stride == 1 && nkb == 3);
}

// the measured size rule (tools/mbf_s3_probe.py, profiles/r23/mbf_s3_probe.txt): a shape is preferred from the smallest launch, counted in
// spatial tiles, at which the three-plane form beat the fp32 kernel by more than the run-to-run spread of the probe.  Every form with
// two or three 16-channel blocks wins at B = 64 (0.84-0.94 of the fp32 kernel's time) and loses or ties at the next measured size
// below (B = 8: the x split is paid per workgroup, and small launches cut the chunk loop into groups that each repeat it); the
// one-block form (block 1: 4 fp32 MFMAs per tile to save, two workgroups per CU instead of three) loses at every size.
static bool mbf3_measured(int in_h, int in_w, int cin, int k, int stride, int batch) {
  const int nkb = (cin + 15) / 16;
  if (nkb == 1) return false;
  const int total_pad = (stride == 1) ? (k - 1) : (k - 2);
  const int Ho = (in_h + total_pad - k) / stride + 1, Wo = (in_w + total_pad - k) / stride + 1;
  const int toh = mbf_toh(k, stride, cin);
  const long tiles = (long)batch * ((Ho + toh - 1) / toh) * ((Wo + 15) / 16);
  if (k == 3 && stride == 1) return tiles >= 1024;       // block 2: wins at 1024 (B = 8 aerial), not at 800
  if (k == 5 && stride == 2) return tiles >= 3200;       // block 3: wins at 3200 / 4096, not at 512
  if (k == 5 && stride == 1) return tiles >= 1600;       // block 4: wins at 1600 / 2048, not at 256
  return tiles >= 960;                                   // block 5: wins at 960 / 1024, not at 128
}

extern "C" int ccvpe_mbconv_front_s3_ok(int in_h, int in_w, int cin, int mid, int k, int stride, int batch) {
  if (in_h <= 0 || in_w <= 0 || batch <= 0 || !mbf3_served(in_w, cin, mid, k, stride)) return 0;
  return mbf3_measured(in_h, in_w, cin, k, stride, batch) ? 2 : 1;
}

extern "C" int ccvpe_mbconv_front_s3_f32(const float* x, const void* w_exp3, int kpad, const float* s0, const float* b0,
                                         const float* w_dw, const float* s1, const float* b1, float* y, float* se_partial, int B, int H,
                                         int W, int cin, int mid, int k, int stride, int circular, void* stream) {
  if (!mbf3_served(W, cin, mid, k, stride)) return fail(CCVPE_EINVAL, "mbconv_front_s3: shape not served (W=%d cin=%d mid=%d k=%d s=%d)", W, cin, mid, k, stride);
  const int nkb = (cin + 15) / 16;
  if (kpad != 48 * nkb) return fail(CCVPE_EINVAL, "mbconv_front_s3: kpad %d is not the three-plane pack's (%d)", kpad, 48 * nkb);
  MbFrontParams p;
  int toh;
  if (int rc0 = mbf_fill(p, toh, 4, x, w_exp3, kpad, s0, b0, w_dw, s1, b1, y, se_partial, B, H, W, cin, mid, k, stride, circular)) return rc0;
  hipStream_t st = (hipStream_t)stream;
  int rc = CCVPE_OK;
  auto go = [&](auto kern, int lds_floats) {
    const int lds = lds_floats * 4;
    static DevCache lds_set;                         // per instantiation (generic lambda)
    if ((rc = ensure_dyn_lds(lds_set, kern, lds, "mbconv_front_s3"))) return;
    hipLaunchKernelGGL(kern, dim3(p.total_blocks), dim3(256), lds, st, p);
  };
#define MBF3(K_, S_, NKB_, TOH_, WGS_) if (toh != TOH_) return fail(CCVPE_EINVAL, "mbconv_front_s3: tile height"); else go(mbconv_front_s3_kernel<K_, S_, NKB_, TOH_, WGS_>, Mbf3Geom<K_, S_, NKB_, TOH_>::LDS_FLOATS)
  if (k == 3 && stride == 2 && nkb == 1) MBF3(3, 2, 1, 8, 2);
  else if (k == 3 && stride == 1) MBF3(3, 1, 2, 8, 3);
  else if (k == 5 && stride == 2) MBF3(5, 2, 2, 4, 2);
  else if (k == 5 && stride == 1) MBF3(5, 1, 3, 8, 2);
  else MBF3(3, 2, 3, 4, 2);
#undef MBF3
  if (rc) return rc;
  return check_launch("mbconv_front_s3_kernel");
}
