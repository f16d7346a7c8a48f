// Convolution weight gradient on the fp32 matrix cores:
//   dW[n][tap][c] = sum_{m = (b,oy,ox)} dY[m][n] * X[b, oy*stride - pad + ky, ox*stride - pad + kx][c]
// (backward of F.conv2d w.r.t. its weight for every dense conv of the path: models.py:42-47,57-104 and
// efficientnet_pytorch/model.py:62,86,209; ConvTranspose2d's weight gradient is the same reduction with
// the roles of input and output gradient swapped, see ccvpe_amd/backward.py).
//
// GEMM view: rows = output channels n, columns = input channels c, reduction = OUTPUT PIXELS (millions),
// one GEMM per tap.  Both operands are pixel-major in HBM (NHWC), i.e. the reduction index is the slow
// one, so fragments are read from LDS one dword per lane (lane = (channel, pixel-in-group)): with the
// 32-cycle fp32 MFMA that costs nothing.  The pixel range is split over S workgroups per (tile, tap);
// partials go to scratch and a second kernel adds them in fixed order (deterministic, no atomics).
#include "common.h"
#include <cstdlib>

namespace ccvpe {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct WgradParams {
  const float* src0;
  const float* src1;
  const float* dy;
  float* part;          // [S][N][taps][Ctot]
  int c0, ld0, c1, ld1;
  int H, W, Ho, Wo;
  int kw, stride, pad, taps;
  int N, ldy;
  int M;                // batch * Ho * Wo
  int S, pix_per_split;
  int tiles_n, tiles_c;
  float* bias_part;     // optional [S][N]: column sums of dY (the conv's bias gradient) from the tiles with tc == 0, else nullptr
  const float* gate;    // GATED kernels (1x1 convs only): x is multiplied by gate[sample][channel] while it is staged
  int ablate;           // diagnostics build only (-DCCVPE_ABLATE): 1 = no global loads, 2 = no LDS stores, 4 = no fragment reads
};

constexpr int WG_T = 64;    // tile: 64 output channels x 64 input channels
constexpr int WG_BP = 32;   // pixels per stage
// Row pitch of a staged [pixel][column] panel.  Square tiles read fragments as 32 consecutive floats of one row per half-wave
// (conflict-free for any pitch).  The 16x16x4 tiles read (column = lane & 15, pixel = lane >> 4) with ds_read_b32, whose bank is
// (address / 4) mod 32 and whose lane groups are the two 32-lane halves: two pixel rows share a group, so the pitch must be
// 16 mod 32 for their 16-float runs to land on different banks.  (Pitch width + 4 — 68, 84, ... — made every fragment read
// a 2-way conflict: SQ_LDS_BANK_CONFLICT = 40 % of the LDS-active cycles with the LDS arrays busy 46-64 % of these kernels.)
constexpr int wgrad_pitch(int width, bool square) { return square ? width + 4 : (width + 15) / 32 * 32 + 16; }

// TN x TC = output channels x columns per tile.  TN = 16 / 32 for the decoder's last levels (N = 16..32 and millions of
// pixels: a 64-row tile would spend 4-16x the MFMA work on padding); 128 x 128 for the wide layers, where a 64 x 64 tile
// (16 FLOP per byte staged) is bound by L2 -> LDS bandwidth: every dY panel is re-read by each column tile and vice versa.
// The tile columns index (tap, input channel) jointly: col = tap*Ctot + c, so narrow layers (Ctot = 16..48) fill the
// tile with several taps instead of zero columns.
// GATED: the conv's input is u * gate[b, c] (the squeeze-excite product in front of the MBConv projection,
// efficientnet_pytorch/model.py:118-121): the gate is applied to the X pieces as they are written to LDS, so the training
// step no longer materialises the gated tensor (gate_mul_kernel: one read + one write of every depthwise-conv output).
template <int TN, int TC, bool GATED = false>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const WgradParams p) {
  constexpr bool SQ = TN == 64 || TN == 128;          // 2 x 2 waves of (TN/2) x (TC/2); else 4 waves of TN x (TC/4)
  constexpr int NI = (SQ ? TN / 2 : TN) / 16;         // 16-row MFMA tiles per wave along n
  constexpr int NJ = (SQ ? TC / 2 : TC / 4) / 16;     // 16-col MFMA tiles per wave along columns
  constexpr int YP = (TN + 31) / 32;                  // float4 pieces per thread per stage (dY): columns (tid&7)*4 + 32*q
  constexpr int XP = TC / 32;                         // float4 pieces per thread per stage (X)
  constexpr int YLD = wgrad_pitch(TN, SQ), XLD = wgrad_pitch(TC, SQ);
  extern __shared__ __attribute__((aligned(16))) float wsm[];
  float* Ys = wsm;                                    // [2][WG_BP][YLD]   dY [pixel][n]
  float* Xs = wsm + 2 * WG_BP * YLD;                  // [2][WG_BP][XLD]   X  [pixel][col]
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wn = SQ ? wave >> 1 : 0;
  const int wc = SQ ? wave & 1 : wave;
  // XCD-aware order: workgroup ids round-robin over the 8 XCDs (private L2s).  All tiles of ONE pixel split re-read the same
  // dY / X pixel rows (each (row tile, column tile) pair streams both panels), so give each XCD a contiguous run of logical
  // blocks (tile fastest, then split): with the identity map the 8 column tiles of a split sat on 8 different L2s and
  // every panel was fetched from HBM / the Infinity Cache 8 times.
  int bid;
  {
    const int total = gridDim.x, q = total / 8, r = total % 8;
    const int xcd = blockIdx.x % 8, loc = blockIdx.x / 8;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
  }
  const int tc = bid % p.tiles_c; bid /= p.tiles_c;
  const int tn = bid % p.tiles_n;
  const int split = bid / p.tiles_n;
  const int n0 = tn * TN, cc0 = tc * TC;
  const int ctot = p.c0 + p.c1;
  const int ncols = p.taps * ctot;
  const int m_begin = split * p.pix_per_split;
  const int m_end = min(m_begin + p.pix_per_split, p.M);

  // staging: thread -> pixel row tid >> 3 (0..31), float4 pieces at tile column (tid & 7) * 4 + 32 * q
  const int prow = tid >> 3;
  const int pc = (tid & 7) * 4;
  int pch[XP];                                       // (GATED) channel of each X piece
  int pky[XP], pkx[XP], pld[XP];                     // per X piece: tap offsets, pixel stride of its source (stage-invariant)
  const float* pbase[XP];                            // ... and the source row base at its input channel (src0 or src1)
  bool pok[XP];
#pragma unroll
  for (int q = 0; q < XP; ++q) {
    const int col = cc0 + pc + 32 * q;
    pok[q] = col < ncols;
    const int tap = pok[q] ? col / ctot : 0;
    const int c = pok[q] ? col - tap * ctot : 0;
    pky[q] = tap / p.kw;
    pkx[q] = tap - pky[q] * p.kw;
    const bool first = c < p.c0;
    pbase[q] = first ? p.src0 + c : p.src1 + (c - p.c0);
    pld[q] = first ? p.ld0 : p.ld1;
    pch[q] = c;
  }
  // Staged pieces are kept RAW in registers across the stage's matrix work, with their validity as lane masks; the masks
  // are applied when the pieces go to LDS (store_stage).  Applying them at the load (`x = in ? t : 0`) made every stage
  // wait for its own prefetch before the first MFMA: vmcnt(3..0) right after the loads.
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  f32x4 yr[YP], xr[XP];
  f32x4 gr[GATED ? XP : 1];                          // gate values of the staged X pieces
  int ykeep = 0, xkeep[XP];
  // bias gradient = column sums of dY: the first column tile of every row tile adds up the dY pieces it stages anyway
  // (one pass over dY instead of a second kernel reading it again: ccvpe_colsum_f32 was 3.3 ms of the B = 64 training step)
  const bool bias_on = p.bias_part != nullptr && tc == 0;
  f32x4 ysum[YP];
#pragma unroll
  for (int q = 0; q < YP; ++q) ysum[q] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // Pixel cursor of this thread's staged row: decoded ONCE (two integer divisions) and then advanced by WG_BP pixels per
  // stage with compare-and-carry (the per-stage decode was ~80 VALU instructions next to 1 024 cycles of MFMA work).
  // All loads are BRANCH-FREE: out-of-range pixels / columns read a clamped valid address and are zeroed by a select, so
  // the 4-8 loads of a stage issue back to back instead of one exec-mask branch each.
  int cm = m_begin + prow, cb, coy, cox;
  {
    const int hw = p.Ho * p.Wo;
    const int mm = cm < p.M ? cm : 0;
    cb = mm / hw;
    const int rem = mm - cb * hw;
    coy = rem / p.Wo;
    cox = rem - coy * p.Wo;
  }
  const int lastpix = p.M - 1;
  // A stage's staging work is cut into per-piece TASKS so that the stage loop can spread it between its groups of matrix
  // instructions (one task per group) instead of running it as one burst in front of them: the ~160 vector-ALU instructions
  // of a stage (address arithmetic, bounds tests, masks) are ~800 cycles, and a wave that is not issuing MFMAs is not hidden
  // by its neighbour on the SIMD — both run the same loop in step.  Tasks 0 .. NPIECE-1 request piece k of the NEXT stage,
  // tasks NPIECE .. 2*NPIECE-1 mask piece k and write it to LDS.
  constexpr int NPIECE = YP + XP;
  const int ldyb = p.ldy * 4;
  auto load_piece = [&](int k) {          // k: compile-time after unrolling
    const int m = cm;
    const bool ok = m < m_end;
    if (k < YP) {
      const int q = k;
      const int nl = pc + 32 * q;
      if (q == 0) ykeep = ok ? -1 : 0;
      if (nl < TN) {
        // One 16-byte load per piece, no tail path: the pixel stride ldy is a multiple of 4 floats >= N, so the vector at
        // column n stays inside the row whenever n < ldy.  Columns >= N only feed output rows that are never stored.
        const int mc = m < p.M ? m : lastpix;
        const int n = n0 + nl;
        const int nc = n < p.ldy ? n : 0;
        yr[q] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(p.dy) + (size_t)mc * ldyb + nc * 4);
      }
    } else {
      const int q = k - YP;
      const int iy = coy * p.stride - p.pad + pky[q], ix = cox * p.stride - p.pad + pkx[q];
      const bool in = ok && pok[q] && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
      const int pix = in ? (cb * p.H + iy) * p.W + ix : 0;        // 32-bit: the launcher checks pixels * pitch < 2^31 floats
      xr[q] = *reinterpret_cast<const f32x4*>(pbase[q] + (size_t)(unsigned)(pix * pld[q]));
      if constexpr (GATED) gr[q] = *reinterpret_cast<const f32x4*>(p.gate + (size_t)(in ? cb : 0) * ctot + pch[q]);
      xkeep[q] = in ? -1 : 0;
    }
  };
  auto advance_cursor = [&]() {
    cm += WG_BP;
    cox += WG_BP;
    while (cox >= p.Wo) {
      cox -= p.Wo;
      if (++coy == p.Ho) { coy = 0; ++cb; }
    }
  };
  auto store_piece = [&](int k, int buf) {
    if (k < YP) {
      const int q = k;
      if (pc + 32 * q < TN) {
        const i32x4 kept = __builtin_bit_cast(i32x4, yr[q]) & ykeep;
        *reinterpret_cast<i32x4*>(&Ys[(buf * WG_BP + prow) * YLD + pc + 32 * q]) = kept;
        if (bias_on) ysum[q] += __builtin_bit_cast(f32x4, kept);
      }
    } else {
      const int q = k - YP;
      f32x4 xv = xr[q];
      if constexpr (GATED) xv *= gr[q];
      *reinterpret_cast<i32x4*>(&Xs[(buf * WG_BP + prow) * XLD + pc + 32 * q]) = __builtin_bit_cast(i32x4, xv) & xkeep[q];
    }
  };
  auto load_stage = [&](int /*m0*/) {
#pragma unroll
    for (int k = 0; k < NPIECE; ++k) load_piece(k);
    advance_cursor();
  };
  auto store_stage = [&](int buf) {
#pragma unroll
    for (int k = 0; k < NPIECE; ++k) store_piece(k, buf);
  };

  // Square tiles (TN >= 64) run on v_mfma_f32_32x32x2_f32: a wave owns (TN/2) x (TC/2) as 32 x 32 blocks.  Operand lanes
  // are (channel = lane & 31, pixel = lane >> 5): the 32 lanes of a half-wave read 32 CONSECUTIVE floats of one staged pixel
  // row — conflict-free for any row pitch (with 16x16x4 the four pixel groups of a ds_read_b32 collided on the 68-float
  // pitch: SQ_LDS_BANK_CONFLICT was 40 % of the LDS-active cycles) — and half as many matrix instructions are issued.
  constexpr bool M32 = SQ;
  constexpr int NI32 = M32 ? TN / 2 / 32 : 1, NJ32 = M32 ? TC / 2 / 32 : 1;
  typedef float f32x16 __attribute__((ext_vector_type(16)));
  f32x4 acc[NI][NJ];
  f32x16 acc32[NI32][NJ32];
  if constexpr (M32) {
#pragma unroll
    for (int i = 0; i < NI32; ++i)
#pragma unroll
      for (int j = 0; j < NJ32; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc32[i][j][r] = 0.f;
  } else {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  const int fi = lane & 15, fq = lane >> 4;       // fragment: channel-in-tile, pixel-in-group
  const int nstage = (m_end - m_begin + WG_BP - 1) / WG_BP;
  if (nstage > 0) {
    load_stage(m_begin);
    store_stage(0);
  }
  __syncthreads();
  for (int s = 0; s < nstage; ++s) {
    const int buf = s & 1;
    if constexpr (M32) {
      // pixel pairs: group g = pixels 2g, 2g+1 of the stage; fragments of group g+1 are read before the MFMAs of group g
      const int l31 = lane & 31, lh = lane >> 5;
      float a[2][NI32], bb[2][NJ32];
      auto read_pair = [&](int g, float* ad, float* bd) {
        const float* yrow = &Ys[(buf * WG_BP + g * 2 + lh) * YLD + wn * NI32 * 32 + l31];
        const float* xrow = &Xs[(buf * WG_BP + g * 2 + lh) * XLD + wc * NJ32 * 32 + l31];
#pragma unroll
        for (int i = 0; i < NI32; ++i) ad[i] = yrow[i * 32];
#pragma unroll
        for (int j = 0; j < NJ32; ++j) bd[j] = xrow[j * 32];
      };
      read_pair(0, a[0], bb[0]);
      constexpr int NG32 = WG_BP / 2;              // 16 groups of NI32 * NJ32 matrix instructions
      static_assert(2 * NPIECE <= NG32, "one staging task per MFMA group");
#pragma unroll
      for (int g = 0; g < NG32; ++g) {
        const int cur = g & 1;
#ifdef CCVPE_ABLATE
        if (g + 1 < NG32 && (!(p.ablate & 4) || s == 0)) read_pair(g + 1, a[cur ^ 1], bb[cur ^ 1]);
#else
        if (g + 1 < NG32) read_pair(g + 1, a[cur ^ 1], bb[cur ^ 1]);
#endif
        // staging tasks of the NEXT stage, one per group (see load_piece).  UNCONDITIONAL: after the last stage they fetch
        // clamped addresses and write a buffer nobody reads — under `if (more)` the two paths merge in front of every task
        // and the merged wait-count state makes each request wait for the previous one (vmcnt(0) per group).
#ifdef CCVPE_ABLATE
        if (g < NPIECE && !(p.ablate & 1)) load_piece(g);
        if (g == NPIECE) advance_cursor();
        if (g >= NG32 - NPIECE && !(p.ablate & 2)) store_piece(g - (NG32 - NPIECE), buf ^ 1);
#else
        if (g < NPIECE) load_piece(g);
        if (g == NPIECE) advance_cursor();
        if (g >= NG32 - NPIECE) store_piece(g - (NG32 - NPIECE), buf ^ 1);
#endif
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NI32; ++i)
#pragma unroll
          for (int j = 0; j < NJ32; ++j)
            acc32[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][i], bb[cur][j], acc32[i][j], 0, 0, 0);
      }
    } else {
    // fragments of pixel group g+1 are read from LDS BEFORE the MFMAs of group g are issued (two register sets): the
    // compiler's own schedule read a group, waited lgkmcnt(0), issued its NI*NJ MFMAs and only then read the next group —
    // with 4 MFMAs per group the LDS latency (~100 cycles) was exposed behind every 128 cycles of matrix work.
    float a[2][NI], bb[2][NJ];
    auto read_group = [&](int g, float* ad, float* bd) {
      const float* yrow = &Ys[(buf * WG_BP + g * 4 + fq) * YLD + wn * NI * 16 + fi];
      const float* xrow = &Xs[(buf * WG_BP + g * 4 + fq) * XLD + wc * NJ * 16 + fi];
#pragma unroll
      for (int i = 0; i < NI; ++i) ad[i] = yrow[i * 16];
#pragma unroll
      for (int j = 0; j < NJ; ++j) bd[j] = xrow[j * 16];
    };
    read_group(0, a[0], bb[0]);
    static_assert(NPIECE < WG_BP / 4, "one request task per MFMA group");
#pragma unroll
    for (int g = 0; g < WG_BP / 4; ++g) {
      const int cur = g & 1;
      if (g + 1 < WG_BP / 4) read_group(g + 1, a[cur ^ 1], bb[cur ^ 1]);
      // next stage's requests, one piece per group (unconditional, see above); written to LDS after the loop
      if (g < NPIECE) load_piece(g);
      if (g == NPIECE) advance_cursor();
      __builtin_amdgcn_sched_barrier(0);      // keep the reads of group g+1 ABOVE the MFMAs of group g (see above)
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur][i], bb[cur][j], acc[i][j], 0, 0, 0);
    }
    }
    if constexpr (!M32) store_stage(buf ^ 1);
    __syncthreads();
  }
  if (bias_on) {        // (workgroup-uniform) the 32 staging rows of a column -> one sum, fixed order; Ys is dead (loop ended on a barrier)
#pragma unroll
    for (int q = 0; q < YP; ++q)
      if (pc + 32 * q < TN) *reinterpret_cast<f32x4*>(&Ys[prow * YLD + pc + 32 * q]) = ysum[q];
    __syncthreads();
    for (int n = tid; n < TN; n += 256) {
      float t = 0.f;
#pragma unroll 8
      for (int r = 0; r < WG_BP; ++r) t += Ys[r * YLD + n];
      if (n0 + n < p.N) p.bias_part[(size_t)split * p.N + n0 + n] = t;
    }
  }
  // D (16x16): row (n) = (lane>>4)*4 + reg, col = lane&15; D (32x32): row = (reg&3) + 8*(reg>>2) + 4*(lane>>5), col = lane&31.
  // dw layout [n][tap][c] == [n][col]
  float* out = p.part + (size_t)split * p.N * ncols;
  if constexpr (M32) {
#pragma unroll
    for (int i = 0; i < NI32; ++i)
#pragma unroll
      for (int j = 0; j < NJ32; ++j) {
        const int col = cc0 + (wc * NJ32 + j) * 32 + (lane & 31);
        if (col >= ncols) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int n = n0 + (wn * NI32 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          if (n < p.N) out[(size_t)n * ncols + col] = acc32[i][j][r];
        }
      }
    return;
  }
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = cc0 + (wc * NJ + j) * 16 + (lane & 15);
      if (col >= ncols) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + (wn * NI + i) * 16 + (lane >> 4) * 4 + r;
        if (n < p.N) out[(size_t)n * ncols + col] = acc[i][j][r];
      }
    }
}

// per-channel column sums (bias gradients): partial per CS_ROWS-row block (all 256 threads busy: channel lanes x
// row lanes, combined through LDS in lane order), then the fixed-order parallel reduce
constexpr int CS_ROWS = 1024;
template <int V>   // V = 4: one 16-byte load per (row, 4 channels); V = 1: scalar (unaligned / odd channel counts)
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ x, int rows, int C, int ld,
                                                            float* __restrict__ part, int rpb) {
  __shared__ __attribute__((aligned(16))) float red[256 * V];
  const int cgn = C / V;
  const int cw = cgn < 256 ? cgn : 256;
  const int R = 256 / cw;
  const int cl = threadIdx.x % cw, rr = threadIdx.x / cw;
  const int r0 = blockIdx.x * rpb, r1 = min(r0 + rpb, rows);
  for (int c0 = 0; c0 < cgn; c0 += cw) {
    const int cg = c0 + cl;
    float s[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] = 0.f;
    if (rr < R && cg < cgn) {
      for (int r = r0 + rr; r < r1; r += R) {
        if (V == 4) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(x + (size_t)r * ld + cg * 4);
#pragma unroll
          for (int j = 0; j < V; ++j) s[j] += v[j];
        } else {
          s[0] += x[(size_t)r * ld + cg];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) red[threadIdx.x * V + j] = s[j];
    __syncthreads();
    if (rr == 0 && cg < cgn) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float t = red[cl * V + j];
        for (int q = 1; q < R; ++q) t += red[(q * cw + cl) * V + j];
        part[(size_t)blockIdx.x * C + cg * V + j] = t;
      }
    }
    __syncthreads();
  }
}

}  // namespace ccvpe

using namespace ccvpe;

static int wgrad_splits(int M, int tiles, int taps, bool big = false) {
  (void)taps;
  const int maxS = (M + WG_BP * 8 - 1) / (WG_BP * 8);
  (void)big;   // (128 x 128 tiles: the smallest split that fills a round — S = 1 at level 6 — measured 110 TF against 115.5 with S = 8)
  // ~4 K workgroups: the stage loop is a chain of (global load -> LDS -> 8 MFMAs) with one stage of prefetch, so the
  // narrow layers (1-3 tiles, millions of pixels) need many co-resident workgroups to hide the load latency
  int S = 4096 / (tiles > 0 ? tiles : 1);
  if (S < 1) S = 1;
  if (S > maxS) S = maxS;
  if (S > 1024) S = 1024;
  return S < 1 ? 1 : S;
}

// Row tile: minimise (padded MFMA rows) / (measured relative efficiency of the tile).  N = 40 -> 48 rows, N = 80 / 160 /
// 320 -> 80 rows (the 64-row tile spent 37.5 % of its matrix work on zero rows there); the 128 x 128 tile (needs >= 512
// columns to fill) wins whenever its padding stays small (N = 640, 672, 1152, 1280 ...).
static int wgrad_pick(int n, int ncols) {
  static const int cand[] = {16, 32, 48, 64, 80, 128};
  static const double eff[] = {0.45, 0.70, 0.75, 0.80, 0.90, 1.00};      // from tools/wgrad_probe.py, relative to 128 x 128
  int best = 64;
  double best_cost = 1e30;
  for (int i = 0; i < 6; ++i) {
    const int t = cand[i];
    if (t == 128 && (n < 128 || ncols < 512)) continue;
    const double cost = (double)((n + t - 1) / t * t) / eff[i];
    if (cost < best_cost) { best_cost = cost; best = t; }
  }
  return best;
}
static int wgrad_tn(int n, int ncols) { const int t = wgrad_pick(n, ncols); return t == 128 ? 64 : t; }
static bool wgrad_big(int n, int ncols) { return wgrad_pick(n, ncols) == 128; }
// (an 80 x 128 tile — 4 waves of 80 x 32, twice the matrix work per stage — measured SLOWER than 80 x 64: 93 vs 102 TF on
// the N = 80 3x3 layer, 94 vs 104 on N = 160: one workgroup less per CU costs more than the longer stage gains)
static int wgrad_tc(int n, int ncols) { return wgrad_big(n, ncols) ? 128 : WG_T; }
static int wgrad_tile_count(int n, int ncols) {
  if (wgrad_big(n, ncols)) return ((n + 127) / 128) * ((ncols + 127) / 128);
  const int tn = wgrad_tn(n, ncols), tcw = wgrad_tc(n, ncols);
  return ((n + tn - 1) / tn) * ((ncols + tcw - 1) / tcw);
}

// which tile the kernel will use for an [n] x [ncols = taps * channels] weight gradient: (rows << 16) | columns
// (reporting only: bench.py names its launch records after the instantiation that ran)
extern "C" int ccvpe_conv_wgrad_tile(int n, int ncols) {
  if (n <= 0 || ncols <= 0) return CCVPE_EINVAL;
  if (wgrad_big(n, ncols)) return (128 << 16) | 128;
  return (wgrad_tn(n, ncols) << 16) | wgrad_tc(n, ncols);
}

extern "C" int ccvpe_conv_wgrad_scratch_floats(int batch, int in_h, int in_w, int kh, int kw, int stride, int pad,
                                               int ctot, int n) {
  const int Ho = (in_h + 2 * pad - kh) / stride + 1, Wo = (in_w + 2 * pad - kw) / stride + 1;
  const long M = (long)batch * Ho * Wo;
  if (M <= 0 || M > 0x7fffffffL || ctot <= 0 || n <= 0) return CCVPE_EINVAL;
  const int tiles = wgrad_tile_count(n, kh * kw * ctot);
  const int S = wgrad_splits((int)M, tiles, kh * kw, wgrad_big(n, kh * kw * ctot));
  const long fl = (long)S * ((long)n * kh * kw * ctot + n);     // + the bias-gradient partials of ccvpe_conv_wgrad_bias_f32
  return fl > 0x7fffffffL ? CCVPE_EINVAL : (int)fl;
}

static int conv_wgrad_impl(const float* src0, int c0, int ld0, const float* src1, int c1, int ld1,
                           const float* dy, int ldy, float* dw, float* dbias, float* scratch, int batch, int in_h,
                           int in_w, int kh, int kw, int stride, int pad, int n, void* stream, const float* gate = nullptr) {
  if (c0 <= 0 || c0 % 4 || c1 < 0 || c1 % 4 || ld0 % 4 || (c1 && ld1 % 4)) return fail(CCVPE_EINVAL, "conv_wgrad: channels/ld %% 4");
  if (c1 > 0 && !src1) return fail(CCVPE_EINVAL, "conv_wgrad: c1>0 but src1 null");
  if (!aligned16(src0) || (src1 && !aligned16(src1)) || !aligned16(dy) || ldy % 4) return fail(CCVPE_EINVAL, "conv_wgrad: alignment");
  if ((double)batch * in_h * in_w * (double)(ld0 > ld1 ? ld0 : ld1) >= 2147483648.0)
    return fail(CCVPE_EINVAL, "conv_wgrad: source larger than 2^31 floats (32-bit pixel offsets)");
  WgradParams p;
  p.src0 = src0; p.src1 = src1; p.dy = dy; p.part = scratch;
  p.c0 = c0; p.ld0 = ld0; p.c1 = c1; p.ld1 = ld1;
  p.H = in_h; p.W = in_w;
  p.Ho = (in_h + 2 * pad - kh) / stride + 1;
  p.Wo = (in_w + 2 * pad - kw) / stride + 1;
  p.kw = kw; p.stride = stride; p.pad = pad; p.taps = kh * kw;
  p.N = n; p.ldy = ldy;
  const long M = (long)batch * p.Ho * p.Wo;
  if (M <= 0 || M > 0x7fffffffL) return fail(CCVPE_EINVAL, "conv_wgrad: bad M");
  p.M = (int)M;
  p.ablate = 0;
#ifdef CCVPE_ABLATE
  p.ablate = getenv("CCVPE_WG_ABLATE") ? atoi(getenv("CCVPE_WG_ABLATE")) : 0;
#endif
  const int ctot = c0 + c1;
  const bool big = wgrad_big(n, p.taps * ctot);
  const int tn = big ? 128 : wgrad_tn(n, p.taps * ctot);
  const int tcw = wgrad_tc(n, p.taps * ctot);
  p.tiles_n = (n + tn - 1) / tn;
  p.tiles_c = (p.taps * ctot + tcw - 1) / tcw;
  p.S = wgrad_splits(p.M, p.tiles_n * p.tiles_c, p.taps, big);
  p.pix_per_split = ((p.M + p.S - 1) / p.S + WG_BP - 1) / WG_BP * WG_BP;
  p.bias_part = dbias ? scratch + (size_t)p.S * n * p.taps * ctot : nullptr;
  p.gate = gate;
  if (gate && (kh != 1 || kw != 1 || stride != 1 || pad != 0 || c1 != 0 || big || !aligned16(gate)))
    return fail(CCVPE_EINVAL, "conv_wgrad: the gated form is for 1x1 single-source convs with fewer than 128 output channels");
  hipStream_t st = (hipStream_t)stream;
  const long blocks = (long)p.tiles_n * p.tiles_c * p.S;
  const bool sq = tn == 64 || big;
  const size_t lds = sizeof(float) * 2 * WG_BP * ((size_t)wgrad_pitch(tn, sq) + wgrad_pitch(tcw, sq));
  if (big) {
    static DevCache lds_set;
    if (int rc = ensure_dyn_lds(lds_set, conv_wgrad_kernel<128, 128>, (int)lds, "conv_wgrad")) return rc;
    hipLaunchKernelGGL((conv_wgrad_kernel<128, 128>), dim3((unsigned)blocks), dim3(256), lds, st, p);
  } else if (gate) {
    if (tn == 16) hipLaunchKernelGGL((conv_wgrad_kernel<16, 64, true>), dim3((unsigned)blocks), dim3(256), lds, st, p);
    else if (tn == 32) hipLaunchKernelGGL((conv_wgrad_kernel<32, 64, true>), dim3((unsigned)blocks), dim3(256), lds, st, p);
    else if (tn == 48) hipLaunchKernelGGL((conv_wgrad_kernel<48, 64, true>), dim3((unsigned)blocks), dim3(256), lds, st, p);
    else if (tn == 80) hipLaunchKernelGGL((conv_wgrad_kernel<80, 64, true>), dim3((unsigned)blocks), dim3(256), lds, st, p);
    else hipLaunchKernelGGL((conv_wgrad_kernel<64, 64, true>), dim3((unsigned)blocks), dim3(256), lds, st, p);
  } else if (tn == 16) hipLaunchKernelGGL((conv_wgrad_kernel<16, 64>), dim3((unsigned)blocks), dim3(256), lds, st, p);
  else if (tn == 32) hipLaunchKernelGGL((conv_wgrad_kernel<32, 64>), dim3((unsigned)blocks), dim3(256), lds, st, p);
  else if (tn == 48) hipLaunchKernelGGL((conv_wgrad_kernel<48, 64>), dim3((unsigned)blocks), dim3(256), lds, st, p);
  else if (tn == 80) hipLaunchKernelGGL((conv_wgrad_kernel<80, 64>), dim3((unsigned)blocks), dim3(256), lds, st, p);
  else hipLaunchKernelGGL((conv_wgrad_kernel<64, 64>), dim3((unsigned)blocks), dim3(256), lds, st, p);
  const long n_elem = (long)n * p.taps * ctot;
  launch_sum_parts(scratch, p.S, n_elem, (int)n_elem, dw, st);
  if (dbias) launch_sum_parts(p.bias_part, p.S, n, n, dbias, st);
  return check_launch("conv_wgrad");
}

extern "C" int ccvpe_conv_wgrad_f32(const float* src0, int c0, int ld0, const float* src1, int c1, int ld1,
                                    const float* dy, int ldy, float* dw, float* scratch, int batch, int in_h,
                                    int in_w, int kh, int kw, int stride, int pad, int n, void* stream) {
  return conv_wgrad_impl(src0, c0, ld0, src1, c1, ld1, dy, ldy, dw, nullptr, scratch, batch, in_h, in_w, kh, kw, stride, pad, n,
                         stream);
}
extern "C" int ccvpe_conv_wgrad_gated_f32(const float* x, int c, int ld, const float* gate, const float* dy, int ldy, float* dw,
                                          float* scratch, int batch, int in_h, int in_w, int n, void* stream) {
  if (!gate) return fail(CCVPE_EINVAL, "conv_wgrad_gated: gate is NULL");
  return conv_wgrad_impl(x, c, ld, nullptr, 0, 0, dy, ldy, dw, nullptr, scratch, batch, in_h, in_w, 1, 1, 1, 0, n, stream, gate);
}
extern "C" int ccvpe_conv_wgrad_bias_f32(const float* src0, int c0, int ld0, const float* src1, int c1, int ld1,
                                         const float* dy, int ldy, float* dw, float* dbias, float* scratch, int batch,
                                         int in_h, int in_w, int kh, int kw, int stride, int pad, int n, void* stream) {
  if (!dbias) return fail(CCVPE_EINVAL, "conv_wgrad_bias: dbias is NULL");
  return conv_wgrad_impl(src0, c0, ld0, src1, c1, ld1, dy, ldy, dw, dbias, scratch, batch, in_h, in_w, kh, kw, stride, pad, n,
                         stream);
}

extern "C" int ccvpe_colsum_f32(const float* x, int rows, int channels, int ld, float* out, float* scratch,
                                void* stream) {
  if (rows <= 0 || channels <= 0 || ld < channels) return fail(CCVPE_EINVAL, "colsum: bad shape");
  // rows per workgroup: CS_ROWS for big tensors, fewer for small ones so that at least ~256 workgroups share the walk
  // (the caller's scratch is sized for ceil(rows / 256) partial rows)
  int rpb = CS_ROWS;
  if (rows < CS_ROWS * 256) rpb = rows / 256 < 256 ? 256 : rows / 256;
  const int nblk = (rows + rpb - 1) / rpb;
  hipStream_t st = (hipStream_t)stream;
  if (channels % 4 == 0 && ld % 4 == 0 && aligned16(x))
    hipLaunchKernelGGL((colsum_partial_kernel<4>), dim3(nblk), dim3(256), 0, st, x, rows, channels, ld, scratch, rpb);
  else
    hipLaunchKernelGGL((colsum_partial_kernel<1>), dim3(nblk), dim3(256), 0, st, x, rows, channels, ld, scratch, rpb);
  launch_sum_parts(scratch, nblk, channels, channels, out, st);
  return check_launch("colsum");
}
