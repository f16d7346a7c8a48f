// conv3x3_wino_n_kernel<NT, MATCH>: conv3x3_wino_kernel's fp32 Winograd F(2x2,3x3) convolution for layers of at most 80 output
// channels, with ALL 16 NT >= N columns in one workgroup — and, with MATCH, the next decoder level's one-hypothesis rotational
// matching in its epilogue (what c3n_kernel<MATCH> does for bf16 storage, csrc/narrow_impl.h).
//
// conv3x3_wino_kernel is always 32 columns wide: N = 40 runs two column tiles (64 columns of matrix work for 40, the 18 x 18 halo
// staged and B^T d B formed twice), N = 80 three.  Here:
//   * 2 NS waves on a 16 x 4 NS pixel tile (NS = 4: 16 x 16 as before; NS = 2 for N <= 48, where two workgroups then share a CU).
//     Wave (s, G) = (wave % NS, wave / NS) owns pixel strip s (16 x 4 outputs = 8 x 2 tiles, as before) and component rows
//     2G, 2G + 1 of the 4 x 4 grid: 8 x NT accumulators instead of 16 x 2;
//   * a stage is (chunk, r): wave (s, G) forms component row 2G + r of B^T d B from the two patch rows it needs and issues
//     4 components x 4 k-steps x NT matrix instructions — every component row is formed once per workgroup and chunk;
//   * U of a stage (the 8 components the two halves need) x 16 NT rows by LDS-DMA with conv3x3_wino_kernel's swizzle, double-buffered;
//   * the same operands meet in the same order per accumulator (chunk ascending, k-step 0..3), and A^T M A + bias is evaluated with
//     the same expression: the output is bit-identical to conv3x3_wino_kernel's;
//   * epilogue: A^T M A needs component rows of both halves.  Per pair of 16-column blocks (2p, 2p + 1) half 1 hands its rows of
//     block 2p to half 0 and half 0 its rows of block 2p + 1 to half 1, through the LDS the K loop has left; both halves finish a block;
//   * MATCH: the finished blocks stay in registers; per pixel sum x^2, the window's x^2 and x . g over the lane's channels, then over
//     the four lane groups and the two halves; dst receives [x / max(|x|, 1e-12) | score | 0-pad] (pitch ldd), `scores` the score
//     plane — ccvpe_match_level's formulas with one rotation hypothesis; x itself is never written.
#include "conv_common.h"

namespace ccvpe {

struct WinoNParams {
  const float* src0;
  const float* w;      // packed U (models._pack_wino): [round_up(n, 32)][16][round_up(c0, 16)]
  const float* shift;  // bias [N] or nullptr
  float* dst;
  int c0, ld0, H, W, N, Kpad, ldd;
  int tiles_x, tiles_y, tiles_total;
  // MATCH
  const float* g;      // [B][ldg] ground descriptor of the next level (first L entries)
  float* scores;       // [B,1,H,W]
  int ldg, L, off;     // off = (-shift * stride - window_offset) mod N: channel c of x meets g[(c + off) mod N]
};

// NS pixel strips of 16 x 4 per workgroup (tile = 16 columns x 4 NS rows), 2 NS waves
static constexpr int WN_HC = 18;
static constexpr int WN_TAB = 176;                             // MATCH tables: g[80], window[80], |g|, pad (floats)
static constexpr int WN_XCH = 8 * 64 * 4;                      // exchange floats per wave (8 f32x4 per lane)
constexpr int wn_halo_floats(int ns) { return (4 * ns + 2) * WN_HC * LDS_LD; }
constexpr int wn_lds_bytes(int nt, int ns) {
  const int work = wn_halo_floats(ns) + 2 * 8 * 16 * nt * 16, xch = 2 * ns * WN_XCH;
  return (WN_TAB + (work > xch ? work : xch)) * 4;
}

template <int NT, bool MATCH, int NS>
__global__ __launch_bounds__(128 * NS, 2) void conv3x3_wino_n_kernel(const WinoNParams p) {
  constexpr int WN_NW = 2 * NS;
  constexpr int WN_HPX = (4 * NS + 2) * WN_HC;
  constexpr int WN_HS = wn_halo_floats(NS);
  constexpr int NTHR = 64 * WN_NW;
  constexpr int NPAD = 16 * NT;
  constexpr int H_IT = (WN_HPX * 4 + NTHR - 1) / NTHR;
  constexpr int NP = (NT + 1) / 2;                     // epilogue rounds (pairs of column blocks)
  extern __shared__ __attribute__((aligned(16))) float wn_sm[];
  float* mtab = wn_sm;                                 // [NPAD] g, [NPAD] window at 80, |g| at 160
  float* Hs = wn_sm + WN_TAB;                          // [4 NS + 2][HC][LDS_LD]
  float* Bs = Hs + WN_HS;                              // [2][8][NPAD][16], 16-byte pieces swizzled by w_swz(row)
  float* Xs = Hs;                                      // epilogue exchange: [2 NS waves][8][64 lanes] f32x4 over the dead halo / U

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = sgpr(tid >> 6);
  const int strip = wave % NS, G = wave / NS;

  const int tile = xcd_tile(blockIdx.x, p.tiles_total);
  const int tx = tile % p.tiles_x;
  const int ty = (tile / p.tiles_x) % p.tiles_y;
  const int b = tile / (p.tiles_x * p.tiles_y);
  const int y0 = ty * (4 * NS), x0 = tx * 16;
  const int ctot = p.c0;
  const int cpad = p.Kpad / 16;                        // channels per component row of U
  const int nchunks = (ctot + 15) / 16;
  const int nstages = nchunks * 2;
  const float* src0 = p.src0;
  const float* wp = p.w;

  int h_off[H_IT], h_pix[H_IT], h_sub[H_IT];
#pragma unroll
  for (int it = 0; it < H_IT; ++it) {
    const int idx = tid + NTHR * it;
    const int px = idx >> 2, sub = idx & 3;
    h_sub[it] = sub;
    if (px < WN_HPX) {
      const int hy = px / WN_HC, hx = px - hy * WN_HC;
      const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
      h_off[it] = px * LDS_LD + sub * 4;
      h_pix[it] = ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) ? (b * p.H + iy) * p.W + ix : -1;
    } else {
      h_off[it] = -1;
      h_pix[it] = -1;
    }
  }
  f32x4 h_reg[H_IT];
  int h_chunk = 0;
  const int ld0s = sgpr(p.ld0);
  auto load_halo = [&](int chunk) {        // raw loads from clamped addresses; masked in store_halo (STAGING RULE, conv_common.h)
    h_chunk = chunk;
#pragma unroll
    for (int it = 0; it < H_IT; ++it) {
      const int ch = chunk * 16 + h_sub[it] * 4;
      const bool ok = h_pix[it] >= 0 && ch < ctot;
      const size_t off = ok ? (size_t)h_pix[it] * ld0s + ch : 0;
      h_reg[it] = *reinterpret_cast<const f32x4*>(src0 + off);
    }
  };
  auto store_halo = [&]() {
#pragma unroll
    for (int it = 0; it < H_IT; ++it)
      if (h_off[it] >= 0)
        *reinterpret_cast<f32x4*>(Hs + h_off[it]) = keep_if(h_reg[it], h_pix[it] >= 0 && h_chunk * 16 + h_sub[it] * 4 < ctot);
  };

  // U panels by LDS-DMA: stage (chunk, r) is the 8 components (2h + r) * 4 + col, h = 0 / 1, x NPAD rows x 64 bytes = 8 NT
  // wave-instructions of 16 rows; wave w moves component slots w (+ 2 NS) = 4h + col, all NT row groups: the per-lane source offset is one
  // stage-invariant register, component / chunk / row group go into the scalar base (conv3x3_wino_kernel's load_w).
  const int rl = lane >> 2;
  const unsigned wvoff = ((unsigned)rl * (unsigned)p.Kpad + (unsigned)(((lane & 3) ^ w_swz(rl)) * 4)) * 4u;
  const unsigned bs_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)Bs;
  auto load_w = [&](int chunk, int r, int dbuf) {
#pragma unroll
    for (int i = 0; i < 8 / WN_NW; ++i) {
      const int slot = wave + i * WN_NW;
      const int comp = ((slot >> 2) * 2 + r) * 4 + (slot & 3);
#pragma unroll
      for (int q = 0; q < NT; ++q) {
        const char* sbase = reinterpret_cast<const char*>(wp) + ((size_t)comp * cpad + (size_t)chunk * 16 + (size_t)q * 16 * p.Kpad) * 4;
        const unsigned lds = __builtin_amdgcn_readfirstlane(bs_lds + (unsigned)(((dbuf * 8 + slot) * NPAD + q * 16) * 16 * 4));
        // inline assembly for the reason given at conv3x3_kernel's load_w; dma_wait() is the matching vmcnt(0)
        asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds), "v"(wvoff), "s"(sbase) : "memory", "m0");
      }
    }
  };
  auto dma_wait = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };

  f32x4 acc[2][4][NT];                                 // [r][column][block]: component (2G + r) * 4 + column
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[r][x][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15;
  const int fk = (lane >> 4) * 4;
  const int bcol = ((lane >> 4) ^ w_swz(frow)) * 4;
  const int ttx = frow & 7, tty = frow >> 3;           // this lane's tile inside the wave's 8 x 2 tile strip
  const int dbase = ((4 * strip + 2 * tty) * WN_HC + 2 * ttx) * LDS_LD + fk;   // patch origin (halo row / column of d[0][0])
  // B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1].  Component row 2G (r = 0): patch rows 2G - (2 - G), i.e. p0 - p2 / p2 - p1;
  // row 2G + 1 (r = 1): p1 + p2 (G = 0) / p1 - p3 (G = 1).  The same subtractions and additions as conv3x3_wino_kernel.
  const int rowa0 = 2 * G * WN_HC * LDS_LD, rowb0 = (2 - G) * WN_HC * LDS_LD;
  const int rowa1 = WN_HC * LDS_LD, rowb1 = (2 + G) * WN_HC * LDS_LD;

  load_halo(0);
  load_w(0, 0, 0);
  if constexpr (MATCH) {                               // this sample's tables (read after the K loop's barriers); loaded beside the halo
    if (tid < NPAD) {
      int k = tid + p.off;
      k = k >= p.N ? k - p.N : k;
      const bool in = tid < p.N && k < p.L;
      mtab[tid] = in ? p.g[(size_t)b * p.ldg + k] : 0.f;
      mtab[80 + tid] = in ? 1.f : 0.f;
    }
    if (wave == WN_NW - 1) {                           // |g| over the first L <= 80 entries
      const float v0 = lane < p.L ? p.g[(size_t)b * p.ldg + lane] : 0.f;
      const float v1 = lane + 64 < p.L ? p.g[(size_t)b * p.ldg + lane + 64] : 0.f;
      float s = fmaf(v1, v1, v0 * v0);
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
      if (lane == 0) mtab[160] = sqrtf(s);
    }
  }
  store_halo();
  dma_wait();
  __syncthreads();

  int chunk = 0;
  auto stage = [&](int s, auto rtag) {
    constexpr int R = decltype(rtag)::value;
    const bool more = s + 1 < nstages;
    if (R == 0 && chunk + 1 < nchunks) load_halo(chunk + 1);   // first: re-using h_reg waits for what is in flight
    if (more) load_w(R == 1 ? chunk + 1 : chunk, R ^ 1, (s + 1) & 1);

    f32x4 v[4];
    {
      f32x4 t[4];
      const float* pa = Hs + dbase + (R == 0 ? rowa0 : rowa1);
      const float* pb = Hs + dbase + (R == 0 ? rowb0 : rowb1);
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const f32x4 da = *reinterpret_cast<const f32x4*>(pa + x * LDS_LD);
        const f32x4 db = *reinterpret_cast<const f32x4*>(pb + x * LDS_LD);
        if (R == 1 && G == 0) t[x] = da + db;
        else t[x] = da - db;
      }
      v[0] = t[0] - t[2];
      v[1] = t[1] + t[2];
      v[2] = t[2] - t[1];
      v[3] = t[1] - t[3];
    }
    __builtin_amdgcn_sched_barrier(0);                 // the next stage's loads stay above the matrix work
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      f32x4 bf[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j)
        bf[j] = *reinterpret_cast<const f32x4*>(&Bs[(((s & 1) * 8 + G * 4 + x) * NPAD + j * 16 + frow) * 16 + bcol]);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[R][x][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[j][kk], v[x][kk], acc[R][x][j], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);                 // the closing wait / barrier stay below it
    dma_wait();
    __syncthreads();
    if (R == 1 && more) {                              // chunk boundary: every wave is done with the halo -> overwrite it
      store_halo();
      __syncthreads();
    }
  };
  for (int s = 0; s < nstages; s += 2, ++chunk) {
    stage(s, std::integral_constant<int, 0>{});
    stage(s + 1, std::integral_constant<int, 1>{});
  }
  // (the last stage closed with a barrier: halo and U are dead)

  // ---- epilogue: A^T M A (A^T = [1 1 1 0; 0 1 -1 -1]) + bias, per channel; lane = (tile, 4 consecutive channels) ----------
  const int oy = y0 + 4 * strip + 2 * tty, ox = x0 + 2 * ttx;
  const bool inside = oy < p.H && ox < p.W;            // (H, W even: a tile is all inside or all outside)
  const size_t m00 = (size_t)(b * p.H + oy) * p.W + ox;
  f32x4* xmine = reinterpret_cast<f32x4*>(Xs + wave * WN_XCH) + lane;
  const f32x4* xpeer = reinterpret_cast<const f32x4*>(Xs + (wave ^ NS) * WN_XCH) + lane;

  f32x4 yk[MATCH ? NP : 1][2][2];                      // MATCH: the finished block of round p (block 2p + G), kept for the scaling
  if constexpr (MATCH) {
#pragma unroll
    for (int q = 0; q < NP; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) yk[q][i >> 1][i & 1] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  auto send = [&](auto jtag) {
    constexpr int J = decltype(jtag)::value;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int x = 0; x < 4; ++x) xmine[(r * 4 + x) * 64] = acc[r][x][J];
  };
  // one block: m[row][column] (f32x4 = 4 channels) -> y[dy][dx]; conv3x3_wino_kernel's expressions, element by element
  auto finish = [&](const f32x4 (&m)[4][4], int j, f32x4 (&y)[2][2]) {
    const int n = j * 16 + fk;
    f32x4 q0[4], q1[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      q0[c] = m[0][c] + m[1][c] + m[2][c];
      q1[c] = m[1][c] - m[2][c] - m[3][c];
    }
    f32x4 bias;
#pragma unroll
    for (int r = 0; r < 4; ++r) bias[r] = (p.shift && n + r < p.N) ? p.shift[n + r] : 0.0f;
    y[0][0] = q0[0] + q0[1] + q0[2] + bias;
    y[0][1] = q0[1] - q0[2] - q0[3] + bias;
    y[1][0] = q1[0] + q1[1] + q1[2] + bias;
    y[1][1] = q1[1] - q1[2] - q1[3] + bias;
  };
  auto store_block = [&](int j, const f32x4 (&y)[2][2]) {     // channels < N of block j
    const int n = j * 16 + fk;
    if (!inside || n >= p.N) return;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const size_t o = (m00 + (size_t)dy * p.W + dx) * p.ldd + n;
        if (n + 3 < p.N) {
          *reinterpret_cast<f32x4*>(p.dst + o) = y[dy][dx];
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (n + r < p.N) p.dst[o + r] = y[dy][dx][r];
        }
      }
  };
  auto round = [&](auto ptag) {
    constexpr int P = decltype(ptag)::value;
    constexpr int JE = 2 * P, JO = 2 * P + 1;          // half 0 finishes block JE, half 1 block JO (if it exists)
    if (G == 0) {
      if constexpr (JO < NT) send(std::integral_constant<int, JO>{});
    } else {
      send(std::integral_constant<int, JE>{});
    }
    __syncthreads();
    f32x4 y[2][2];
    if (G == 0) {
      f32x4 m[4][4];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        m[0][x] = acc[0][x][JE];
        m[1][x] = acc[1][x][JE];
        m[2][x] = xpeer[x * 64];
        m[3][x] = xpeer[(4 + x) * 64];
      }
      finish(m, JE, y);
      if constexpr (!MATCH) store_block(JE, y);
    } else if constexpr (JO < NT) {
      f32x4 m[4][4];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        m[0][x] = xpeer[x * 64];
        m[1][x] = xpeer[(4 + x) * 64];
        m[2][x] = acc[0][x][JO];
        m[3][x] = acc[1][x][JO];
      }
      finish(m, JO, y);
      if constexpr (!MATCH) store_block(JO, y);
    }
    if constexpr (MATCH) {
      if (G == 0 || JO < NT) {
#pragma unroll
        for (int i = 0; i < 4; ++i) yk[P][i >> 1][i & 1] = y[i >> 1][i & 1];
      }
    }
    __syncthreads();                                   // the exchange slots are free again
  };
  round(std::integral_constant<int, 0>{});
  if constexpr (NP > 1) round(std::integral_constant<int, 1>{});
  if constexpr (NP > 2) round(std::integral_constant<int, 2>{});

  if constexpr (MATCH) {
    // this lane: 4 pixels (dy, dx) x the 4 channels n .. n + 3 of its blocks 2q + G.  Channels >= N are exact zeros (zero U rows,
    // no bias) and their table entries are zero.
    float s2[4], wn[4], dt[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) s2[i] = wn[i] = dt[i] = 0.f;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const int n = (2 * q + G) * 16 + fk;
      if (2 * q + G < NT) {
        const f32x4 gq = *reinterpret_cast<const f32x4*>(mtab + n);
        const f32x4 wq = *reinterpret_cast<const f32x4*>(mtab + 80 + n);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float x = yk[q][i >> 1][i & 1][r];
            const float x2 = x * x;
            s2[i] += x2;
            wn[i] = fmaf(x2, wq[r], wn[i]);
            dt[i] = fmaf(x, gq[r], dt[i]);
          }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {                      // the four lane groups (fixed order)
      s2[i] += __shfl_xor(s2[i], 16, 64); wn[i] += __shfl_xor(wn[i], 16, 64); dt[i] += __shfl_xor(dt[i], 16, 64);
      s2[i] += __shfl_xor(s2[i], 32, 64); wn[i] += __shfl_xor(wn[i], 32, 64); dt[i] += __shfl_xor(dt[i], 32, 64);
    }
    // the two halves: half 0's sum + half 1's, in that order in both
    float* rmine = Xs + wave * WN_XCH + lane;
    const float* rpeer = Xs + (wave ^ NS) * WN_XCH + lane;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      rmine[(i * 3 + 0) * 64] = s2[i];
      rmine[(i * 3 + 1) * 64] = wn[i];
      rmine[(i * 3 + 2) * 64] = dt[i];
    }
    __syncthreads();
    const float gnorm = mtab[160];
    float inv[4], score[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float a = rpeer[(i * 3 + 0) * 64], bw = rpeer[(i * 3 + 1) * 64], c = rpeer[(i * 3 + 2) * 64];
      const float ts = G == 0 ? s2[i] + a : a + s2[i];
      const float tw = G == 0 ? wn[i] + bw : bw + wn[i];
      const float td = G == 0 ? dt[i] + c : c + dt[i];
      inv[i] = 1.0f / fmaxf(sqrtf(ts), 1e-12f);
      score[i] = td / (sqrtf(tw) * gnorm);
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      if (2 * q + G < NT) {
        f32x4 y[2][2];
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i >> 1][i & 1] = yk[q][i >> 1][i & 1] * inv[i];
        store_block(2 * q + G, y);
      }
    }
    if (G == 0 && inside) {                            // [score | 0-pad] behind the N channels (N, ldd multiples of 4), and the score plane
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const size_t pix = m00 + (size_t)(i >> 1) * p.W + (i & 1);
        for (int k = p.N + fk; k < p.ldd; k += 16)
          *reinterpret_cast<f32x4*>(p.dst + pix * p.ldd + k) = (f32x4){k == p.N ? score[i] : 0.f, 0.f, 0.f, 0.f};
        if (fk == 0) p.scores[pix] = score[i];
      }
    }
  }
}

static int round_up_n(int v, int m) { return (v + m - 1) / m * m; }

static bool g_wino_n = true;                         // ccvpe_set_wino_n

// Routing by measurement (tools/wino_probe.py, profiles/r25/README.md): per tile width, the smallest launch (output pixels) that won
// there.  N = 80 (NT = 5): B = 8 at 128 x 128; N = 40 (NT = 3): B = 8 at 256 x 256.  Nothing smaller was measured.
static long wino_n_min_pixels(int nt) { return nt >= 4 ? 1L << 17 : 1L << 19; }

// 0 = not served, 1 = computed correctly, 2 = also a launch the Winograd route serves (wino_refusal's size rule) where the probe
// showed a win: N = 80 and N = 40 won in both forms at B = 64 and B = 8 (n/w 0.74 - 0.87), N = 64 and N = 32 lost (1.03 - 1.14) —
// the layers where conv3x3_wino_kernel's 32-column tiles pad N by a whole 16-column block
static int wino_n_level(const ccvpe_conv_desc* d, bool match) {
  if (wino_shape_refusal(d)) return 0;
  if (d->n <= 16 || d->n > 80) return 0;
  if (match && (d->n % 4 || d->ldd < d->n + 1)) return 0;
  if (!g_wino_n || wino_refusal(d)) return 1;
  if (round_up_n(d->n, 16) == round_up_n(d->n, 32)) return 1;
  return (long)d->batch * d->in_h * d->in_w >= wino_n_min_pixels(round_up_n(d->n, 16) / 16) ? 2 : 1;
}

template <bool MATCH>
static int wino_n_run(const ccvpe_conv_desc* d, WinoNParams& p, hipStream_t stream) {
  p.src0 = reinterpret_cast<const float*>(d->src0); p.w = reinterpret_cast<const float*>(d->w);
  p.shift = d->shift; p.dst = reinterpret_cast<float*>(d->dst);
  p.c0 = d->c0; p.ld0 = d->ld0;
  p.H = d->in_h; p.W = d->in_w;
  p.N = d->n; p.Kpad = d->kpad; p.ldd = d->ldd;
  p.tiles_x = (p.W + 15) / 16;
  const int nt = round_up_n(d->n, 16) / 16;
  const int ns = nt == 3 ? 2 : 4;      // (tools/wino_probe.py: N = 40 is 6 % faster in 16 x 8 tiles, two workgroups per CU; N = 32 8 % slower)
  p.tiles_y = (p.H + 4 * ns - 1) / (4 * ns);
  const long total = (long)p.tiles_x * p.tiles_y * d->batch;
  if (total > 0x7fffffffL) return fail(CCVPE_EINVAL, "conv3x3_wino_n: grid too large");
  p.tiles_total = (int)total;
  static DevCache lds_set[4];
  void (*kern)(const WinoNParams) = nullptr;
  switch (nt) {
    case 2: kern = conv3x3_wino_n_kernel<2, MATCH, 4>; break;
    case 3: kern = conv3x3_wino_n_kernel<3, MATCH, 2>; break;
    case 4: kern = conv3x3_wino_n_kernel<4, MATCH, 4>; break;
    case 5: kern = conv3x3_wino_n_kernel<5, MATCH, 4>; break;
    default: return fail(CCVPE_EINVAL, "conv3x3_wino_n: 16 < n <= 80 only");
  }
  const int lds = wn_lds_bytes(nt, ns);
  if (int rc = ensure_dyn_lds(lds_set[nt - 2], kern, lds, "conv3x3_wino_n")) return rc;
  hipLaunchKernelGGL(kern, dim3(p.tiles_total), dim3(128 * ns), lds, stream, p);
  return check_launch(MATCH ? "conv3x3_wino_n_kernel<match>" : "conv3x3_wino_n_kernel");
}

}  // namespace ccvpe

using namespace ccvpe;

extern "C" int ccvpe_set_wino_n(int on) {
  const int prev = g_wino_n ? 1 : 0;
  g_wino_n = on != 0;
  return prev;
}

extern "C" int ccvpe_conv3x3_wino_n_ok(const ccvpe_conv_desc* d) { return wino_n_level(d, false); }

extern "C" int ccvpe_conv3x3_wino_n_f32(const ccvpe_conv_desc* d, void* stream) {
  if (const char* why = wino_shape_refusal(d)) return fail(CCVPE_EINVAL, "conv3x3_wino_n: %s", why);
  if (!wino_n_level(d, false)) return fail(CCVPE_EINVAL, "conv3x3_wino_n: 16 < n <= 80 only");
  WinoNParams p{};
  return wino_n_run<false>(d, p, (hipStream_t)stream);
}

extern "C" int ccvpe_conv3x3_wino_match1_ok(const ccvpe_conv_desc* d, int out_f32, int L) {
  (void)out_f32;                                     // fp32 storage: the output is fp32 either way
  if (L <= 0 || !d || L > d->n) return 0;
  return wino_n_level(d, true);
}

extern "C" int ccvpe_conv3x3_wino_match1_f32(const ccvpe_conv_desc* d, int out_f32, const float* g, int ldg, int L, int shift, int stride,
                                             int window_offset, float* scores, void* stream) {
  (void)out_f32;
  if (!d || !g || !scores) return fail(CCVPE_EINVAL, "conv3x3_wino_match1: null pointer");
  if (L > ldg) return fail(CCVPE_EINVAL, "conv3x3_wino_match1: L > ldg");
  if (const char* why = wino_shape_refusal(d)) return fail(CCVPE_EINVAL, "conv3x3_wino_match1: %s", why);
  if (L <= 0 || L > d->n || !wino_n_level(d, true))
    return fail(CCVPE_EINVAL, "conv3x3_wino_match1: needs 16 < n <= 80, n %% 4 == 0, ldd >= n + 1, 0 < L <= n");
  WinoNParams p{};
  p.g = g; p.scores = scores; p.ldg = ldg; p.L = L;
  long o = (-((long)shift * stride + window_offset)) % d->n;      // match_any()'s offset (csrc/matching.hip)
  p.off = (int)(o < 0 ? o + d->n : o);
  return wino_n_run<true>(d, p, (hipStream_t)stream);
}
