// conv3x3_wino_kernel: fp32 3x3 / stride 1 / pad 1 convolution by Winograd F(2x2,3x3) (Lavin & Gray, 2016), the second conv
// of every decoder double_conv (convK.2: bias, no activation, models.py:42-47).
//
//   Y = A^T [ (G g G^T) (.) (B^T d B) ] A      per 2x2 output tile, 4x4 input patch d, 3x3 filter g
//
// 16 multiplies per tile and (input channel, output channel) instead of 36: the fp32 MFMA runs at the fp32 VALU rate, so this is
// the one way left to cut the matrix cycles of these layers without narrowing the operands.  Operands and
// accumulation stay fp32; U = G g G^T is computed on the host in fp64 and rounded once (models.py _pack_wino).
//
// Layout (4 waves, each a 16 x 4 output strip = 8 x 2 tiles; the workgroup a 16 x 16 pixel block x 32 output channels):
//   * halo: (16 + 2) x 18 pixels x 16 channels staged in LDS once per channel chunk, as conv3x3_kernel (round-3 pitch);
//   * input transform, lane-local: MFMA B-operand lane l = (tile l & 15, channels 4(l >> 4) .. +3).  A stage covers two rows
//     of the 4 x 4 component grid (8 components): the lane reads the three patch rows they need and forms B^T d B for them in
//     registers — V never leaves the lane, let alone reaches HBM;
//   * the 16 components are 16 accumulators per 16-column block: after the K loop each lane holds all 16 components of 4
//     channels of one tile, and A^T M A, the bias and the NHWC store are lane-local;
//   * U staged by LDS-DMA like conv3x3_kernel's W (global_load_lds_dwordx4, XOR-swizzled 64-byte rows), double-buffered per
//     stage.  Packed U: [round_up(n, 32)][16][round_up(c0, 16)] — row = output channel, k = component * Cpad + channel.
#include "conv_common.h"

namespace ccvpe {

static constexpr int WG_NW = 4;                   // waves, stacked vertically
static constexpr int WG_NT = 2;                   // 16-column blocks per wave (every wave covers the workgroup's columns)
static constexpr int WG_BN = 16 * WG_NT;          // output channels per workgroup
static constexpr int WG_XS = 8;                   // components per stage (two rows of the 4 x 4 grid)
static constexpr int WG_TH = 4 * WG_NW;           // output rows per workgroup
static constexpr int WG_HR = WG_TH + 2, WG_HC = 18;
static constexpr int WG_HPX = WG_HR * WG_HC;
static constexpr int WG_HS = WG_HPX * LDS_LD;                 // halo floats
static constexpr int WG_BS = 2 * WG_XS * WG_BN * 16;          // U floats (two stage buffers)
static constexpr int WG_LDS = (WG_HS + WG_BS) * 4;

__global__ __launch_bounds__(256, 2) void conv3x3_wino_kernel(const IgemmParams p) {
  constexpr int NTHR = 64 * WG_NW;
  constexpr int H_IT = (WG_HPX * 4 + NTHR - 1) / NTHR;
  extern __shared__ __attribute__((aligned(16))) float wg_sm[];
  float* Hs = wg_sm;                                   // [HR][HC][LDS_LD]
  float* Bs = wg_sm + WG_HS;                           // [2][XS][BN][16], 16-byte pieces swizzled by w_swz(row)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = sgpr(tid >> 6);

  const int tile = xcd_tile(blockIdx.x, p.tiles_total);
  const int tn = tile % p.tiles_n;
  const int ts = tile / p.tiles_n;
  const int tx = ts % p.tiles_x;
  const int ty = (ts / p.tiles_x) % p.tiles_y;
  const int b = ts / (p.tiles_x * p.tiles_y);
  const int y0 = ty * WG_TH, x0 = tx * 16;
  const int n0 = tn * WG_BN;
  const int ctot = p.c0;
  const int cpad = p.Kpad / 16;                        // channels per component row of U
  const int nchunks = (ctot + 15) / 16;
  const int nstages = nchunks * 2;
  const float* src0 = reinterpret_cast<const float*>(p.src0);
  const float* wp = reinterpret_cast<const float*>(p.w);

  int h_off[H_IT], h_pix[H_IT], h_sub[H_IT];
#pragma unroll
  for (int it = 0; it < H_IT; ++it) {
    const int idx = tid + NTHR * it;
    const int px = idx >> 2, sub = idx & 3;
    h_sub[it] = sub;
    if (px < WG_HPX) {
      const int hy = px / WG_HC, hx = px - hy * WG_HC;
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

  // U panels by LDS-DMA: a stage is 8 components x 32 rows x 64 bytes = 16 wave-instructions of 16 rows; wave w moves row
  // group w & 1 of components (w >> 1) + 2q, q = 0..3, so its per-lane source offset is one stage-invariant register and the
  // component / chunk offset goes into the scalar base (conv3x3_kernel's load_w).
  const int rl = lane >> 2;
  const int grp = wave & 1;
  const unsigned wvoff = ((unsigned)(n0 + grp * 16 + rl) * (unsigned)p.Kpad + (unsigned)(((lane & 3) ^ w_swz(rl)) * 4)) * 4u;
  const unsigned bs_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)Bs;
  auto load_w = [&](int chunk, int g, int dbuf) {       // components 8g .. 8g+7 of `chunk` -> Bs[dbuf]
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int t = (wave >> 1) + 2 * q;
      const char* sbase = reinterpret_cast<const char*>(wp) + ((size_t)(g * WG_XS + t) * cpad + (size_t)chunk * 16) * 4;
      const unsigned lds = __builtin_amdgcn_readfirstlane(bs_lds + (unsigned)(((dbuf * WG_XS + t) * WG_BN + grp * 16) * 16 * 4));
      // inline assembly for the reason given at conv3x3_kernel's load_w; dma_wait() is the matching vmcnt(0)
      asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds), "v"(wvoff), "s"(sbase) : "memory", "m0");
    }
  };
  auto dma_wait = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };

  f32x4 acc[16][WG_NT];
#pragma unroll
  for (int x = 0; x < 16; ++x)
#pragma unroll
    for (int j = 0; j < WG_NT; ++j) acc[x][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15;
  const int fk = (lane >> 4) * 4;
  const int bcol = ((lane >> 4) ^ w_swz(frow)) * 4;
  const int ttx = frow & 7, tty = frow >> 3;           // this lane's tile inside the wave's 8 x 2 tile strip
  const int dbase = ((4 * wave + 2 * tty) * WG_HC + 2 * ttx) * LDS_LD + fk;   // patch origin (halo row / column of d[0][0])

  load_halo(0);
  load_w(0, 0, 0);
  store_halo();
  dma_wait();
  __syncthreads();

  // one stage: component rows 2G, 2G+1 of `chunk`, U from Bs[s & 1]
  int chunk = 0;
  auto stage = [&](int s, auto gtag) {
    constexpr int G = decltype(gtag)::value;
    const bool more = s + 1 < nstages;
    if (G == 0 && chunk + 1 < nchunks) load_halo(chunk + 1);   // first: re-using h_reg waits for what is in flight
    if (more) load_w(G == 1 ? chunk + 1 : chunk, G ^ 1, (s + 1) & 1);

    // B^T d B, rows 2G and 2G+1.  B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]: rows 0 / 1 need patch rows 0-2, rows 2 / 3
    // patch rows 1-3.  Each value is 4 channels (one per MFMA k-step).
    f32x4 d[3][4];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int x = 0; x < 4; ++x) d[r][x] = *reinterpret_cast<const f32x4*>(Hs + dbase + ((G + r) * WG_HC + x) * LDS_LD);
    f32x4 v[2][4];
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const f32x4 t0 = G == 0 ? d[0][x] - d[2][x] : d[1][x] - d[0][x];
      const f32x4 t1 = G == 0 ? d[1][x] + d[2][x] : d[0][x] - d[2][x];
      if (x == 0) { v[0][0] = t0; v[1][0] = t1; }
      else if (x == 1) { v[0][1] = t0; v[1][1] = t1; }
      else if (x == 2) { v[0][2] = t0; v[1][2] = t1; }
      else { v[0][3] = t0; v[1][3] = t1; }
    }
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const f32x4 a0 = v[rr][0], a1 = v[rr][1], a2 = v[rr][2], a3 = v[rr][3];
      v[rr][0] = a0 - a2;
      v[rr][1] = a1 + a2;
      v[rr][2] = a2 - a1;
      v[rr][3] = a1 - a3;
    }
    __builtin_amdgcn_sched_barrier(0);                 // the next stage's loads stay above the matrix work
#pragma unroll
    for (int t = 0; t < WG_XS; ++t) {
      f32x4 bf[WG_NT];
#pragma unroll
      for (int j = 0; j < WG_NT; ++j)
        bf[j] = *reinterpret_cast<const f32x4*>(&Bs[(((s & 1) * WG_XS + t) * WG_BN + j * 16 + frow) * 16 + bcol]);
      const f32x4 vv = v[t >> 2][t & 3];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int j = 0; j < WG_NT; ++j)
          acc[G * WG_XS + t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[j][kk], vv[kk], acc[G * WG_XS + t][j], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);                 // the closing wait / barrier stay below it
    dma_wait();
    __syncthreads();
    if (G == 1 && more) {                              // chunk boundary: every wave is done with the halo -> overwrite it
      store_halo();
      __syncthreads();
    }
  };
  for (int s = 0; s < nstages; s += 2, ++chunk) {
    stage(s, std::integral_constant<int, 0>{});
    stage(s + 1, std::integral_constant<int, 1>{});
  }

  // ---- epilogue: A^T M A (A^T = [1 1 1 0; 0 1 -1 -1]) + bias, per channel; lane = (tile, 4 consecutive channels) ----------
  const int oy = y0 + 4 * wave + 2 * tty, ox = x0 + 2 * ttx;
  if (oy >= p.H || ox >= p.W) return;                  // (H, W even: a tile is all inside or all outside)
  float* dst = reinterpret_cast<float*>(p.dst);
  const size_t m00 = (size_t)(b * p.H + oy) * p.W + ox;
#pragma unroll
  for (int j = 0; j < WG_NT; ++j) {
    const int n = n0 + j * 16 + fk;
    if (n >= p.N) continue;
    f32x4 y[2][2];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float m[4][4];
#pragma unroll
      for (int x = 0; x < 16; ++x) m[x >> 2][x & 3] = acc[x][j][r];
      float q0[4], q1[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        q0[c] = m[0][c] + m[1][c] + m[2][c];
        q1[c] = m[1][c] - m[2][c] - m[3][c];
      }
      const float bias = (p.shift && n + r < p.N) ? p.shift[n + r] : 0.0f;
      y[0][0][r] = q0[0] + q0[1] + q0[2] + bias;
      y[0][1][r] = q0[1] - q0[2] - q0[3] + bias;
      y[1][0][r] = q1[0] + q1[1] + q1[2] + bias;
      y[1][1][r] = q1[1] - q1[2] - q1[3] + bias;
    }
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const size_t o = (m00 + (size_t)dy * p.W + dx) * p.ldd + n;
        if (n + 3 < p.N) {
          *reinterpret_cast<f32x4*>(dst + o) = y[dy][dx];
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (n + r < p.N) dst[o + r] = y[dy][dx][r];
        }
      }
  }
}

static int round_up(int v, int m) { return (v + m - 1) / m * m; }

// the shapes the kernels of this family compute correctly; the reason for a refusal (or nullptr)
const char* wino_shape_refusal(const ccvpe_conv_desc* d) {
  if (!d) return "null desc";
  if (d->kh != 3 || d->kw != 3 || d->stride != 1 || d->pad != 1 || d->out_mode != CCVPE_OUT_NHWC) return "3x3 / stride 1 / pad 1 / NHWC only";
  if (d->c1 != 0 || d->src1 || d->gate || d->scale || d->residual || d->act != CCVPE_ACT_NONE)
    return "one source, bias only (no gate, scale, residual or activation)";
  if (d->in_h <= 0 || d->in_w <= 0 || d->in_h % 2 || d->in_w % 2) return "H and W must be even";
  if (d->c0 < 32 || d->c0 % 4 || d->ld0 < d->c0 || d->ld0 % 4) return "c0 >= 32, c0 and ld0 multiples of 4";
  if (d->n <= 0 || d->ldd < d->n || d->ldd % 4) return "ldd >= n, ldd multiple of 4";
  if (d->kpad != 16 * round_up(d->c0, 16)) return "kpad must be 16 * round_up(c0, 16) (packed U)";
  if (d->batch <= 0) return "batch must be positive";
  if ((long)d->batch * d->in_h * d->in_w > 0x7fffffffL) return "too many pixels";
  if ((size_t)round_up(d->n, WG_BN) * d->kpad * 4 >= (1ull << 32)) return "U larger than 4 GB";
  if (!aligned16(d->src0) || !aligned16(d->w) || !aligned16(d->dst)) return "pointers must be 16-byte aligned";
  return nullptr;
}

// ... and the size rule on top: the launches where Winograd is the faster route (ccvpe_conv3x3_wino_ok; the launchers themselves
// run any shape they compute correctly)
const char* wino_refusal(const ccvpe_conv_desc* d) {
  if (const char* why = wino_shape_refusal(d)) return why;
  if ((long)d->batch * d->in_h * d->in_w < 16384) return "fewer than 16384 output pixels";
  // where the direct path would split K (small batch), the split wins: stay with it
  ccvpe_conv_desc dd = *d;
  dd.kpad = round_up(9 * d->c0, 16);
  if (ccvpe_conv_igemm_splitk_floats(&dd, 0) != 0) return "the direct path splits K at this shape";
  return nullptr;
}

}  // namespace ccvpe

using namespace ccvpe;

extern "C" int ccvpe_conv3x3_wino_ok(const ccvpe_conv_desc* d) { return wino_refusal(d) ? 0 : 1; }

extern "C" int ccvpe_conv3x3_wino_f32(const ccvpe_conv_desc* d, void* stream) {
  if (const char* why = wino_shape_refusal(d)) return fail(CCVPE_EINVAL, "conv3x3_wino: %s", why);
  IgemmParams p{};
  p.src0 = d->src0; p.w = d->w; p.shift = d->shift; p.dst = d->dst;
  p.c0 = d->c0; p.ld0 = d->ld0;
  p.H = d->in_h; p.W = d->in_w;
  p.N = d->n; p.Kpad = d->kpad; p.Npad = round_up(d->n, WG_BN);
  p.ldd = d->ldd;
  p.tiles_x = (p.W + 15) / 16;
  p.tiles_y = (p.H + WG_TH - 1) / WG_TH;
  p.tiles_n = p.Npad / WG_BN;
  const long total = (long)p.tiles_x * p.tiles_y * d->batch * p.tiles_n;
  if (total > 0x7fffffffL) return fail(CCVPE_EINVAL, "conv3x3_wino: grid too large");
  p.tiles_total = (int)total;
  static DevCache lds_set;
  if (int rc = ensure_dyn_lds(lds_set, conv3x3_wino_kernel, WG_LDS, "conv3x3_wino")) return rc;
  hipLaunchKernelGGL(conv3x3_wino_kernel, dim3(p.tiles_total), dim3(64 * WG_NW), WG_LDS, (hipStream_t)stream, p);
  return check_launch("conv3x3_wino_kernel");
}
