// Histogram filter over the heat-map grid (ccvpe_amd/tracking.py: step_spec is the specification): one recursive Bayes step
// per track in two launches — predict (integer shift + separable blur of the prior) x measure (the network's heat-map mixed
// with a uniform outlier floor), then renormalise and read the estimate off the posterior.
//
// Launch one, belief_step_kernel<MODE, WARP, VEC>: a workgroup owns a (track, 16 x 64 output tile) pair.  The tile plus its R
// halo is staged in LDS already moved, zero outside the grid; the row pass (16 B LDS reads, four outputs per lane) and the
// column pass (a four-deep register window down the column) run in fp32; the product with the second factor is written and
// the tile's sums (double), arg-max candidate and moment sums go to one record per workgroup — for the product and for the
// factor, so that a reset needs no third pass over the maps.  The one kernel has three axes:
//   MODE  BF_SUM   the filter (ccvpe_belief_step_f32 / _rigid_f32): U = blur(moved prior) M, M = (1 - a) heat + a / (h w).
//         BF_MAX   the max-product step (ccvpe_belief_viterbi_step_f32; tracking.viterbi_step_spec): bf_passes in its max form
//                  (sums over taps become maxima), everything else BF_SUM's.
//         BF_BACK  the backward step of the forward-backward smoother (ccvpe_belief_smooth_step_f32 / _rigid_f32;
//                  tracking.smooth_step_spec / smooth_step_rigid_spec): the staging forms G = fma(1 - a, heat, floor) beta on the
//                  way into LDS — the measurement enters BEFORE the blur — with the offsets added instead of subtracted (the
//                  rigid form walks the inverted motion); bf_passes indexes the taps in reverse, which together with the sign
//                  is the adjoint of the predict; bf_epilogue multiplies with the stored posterior alpha, writes B' and
//                  V = alpha B' and the forward record with alpha in M's place.
//   WARP  false    bf_stage_shift: the map moved by the track's whole-pixel offset.
//         true     bf_stage_warp (tracking.step_rigid_spec): the map resampled bilinearly through the track's inverse motion
//                  map; only the staging differs.  BF_SUM and BF_BACK only, and VEC does not apply.
//   VEC   16-byte loads of the staged maps (w % 4 == 0 and 16-byte aligned maps); the values in LDS are the scalar form's.
// Launch two, belief_finish_kernel<VEC, BACK>: every workgroup of a track merges the track's records in the same fixed order
// (bf_merge_records), decides the state, scales its slice of the map by (float)(1 / Z) — BACK: both maps, or the fallback
// written — and the first slice writes the row (bf_write_row).
// No floating-point atomics: two runs are bit-identical.
// What the modes do not share: the value a staged pixel takes (bf_src), the second output map, the state rule and the
// per-element update of launch two.
//
// The most likely path (ccvpe_belief_backtrack_f32; tracking.backtrack_spec): belief_backtrack_kernel walks a whole drive of
// BF_MAX maps in one launch, a workgroup per track, and recomputes each link's decision at the one pixel the path visits —
// there are no back-pointer maps.
#include "common.h"

namespace ccvpe {

constexpr int BF_TH = 16, BF_TW = 64;         // output tile; 256 threads
constexpr int BF_REC = 18;                     // doubles per workgroup record
// record layout: [0] sum Q | [1..6] U: s, sy, sx, syy, sxx, syx | [7..12] the same of M | [13] max U [14] its index |
//                [15] max M [16] its index | [17] unused
// the backward step: [0] sum B' | [1..6] V | [7..12] alpha | max V | max alpha
constexpr int BF_NSUM = 13;
constexpr int BF_NONE = 0x7fffffff;

// LDS pitch of the staged prior tile: the row pass reads 16-byte pieces up to column BF_TW + 4 (R / 2) + 7.  128 when that
// fits: rows then start on the same bank and the 16-lane groups of a 16-byte read (two tile rows each) do not collide.
__host__ __device__ inline int bf_pitch(int R) {
  const int need = BF_TW + 4 * (R / 2) + 8;
  return need <= 128 ? 128 : need;
}

struct BfArg {
  float v;
  int i;
  __device__ __forceinline__ void take(float ov, int oi) {       // oi > i always: a strict > keeps the first maximum
    if (ov > v) { v = ov; i = oi; }
  }
  __device__ __forceinline__ void merge(float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
  __device__ __forceinline__ void wave_merge() {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) merge(__shfl_xor(v, o, 64), __shfl_xor(i, o, 64));
  }
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// s, sy, sx, syy, sxx, syx of one value at integer pixel (y, x)
__device__ __forceinline__ void bf_moments(double* m, float v, int y, int x) {
  const double d = (double)v, dy = (double)y, dx = (double)x;
  m[0] += d;
  m[1] = fma(d, dy, m[1]);
  m[2] = fma(d, dx, m[2]);
  m[3] = fma(d * dy, dy, m[3]);
  m[4] = fma(d * dx, dx, m[4]);
  m[5] = fma(d * dy, dx, m[5]);
}

enum BfMode { BF_SUM, BF_MAX, BF_BACK };

// The measurement M = (1 - a) heat + a / (h w), one fused multiply-add wherever it is formed
__device__ __forceinline__ float bf_measure(float heat, float one_minus_a, float floor_m) {
  return fmaf(one_minus_a, heat, floor_m);
}

// The value a staged pixel takes from global memory: the prior itself (the forward step), or the backward step's
// G = M beta formed on the way into LDS (v = heat, v2 = beta).
template <bool SMOOTH>
__device__ __forceinline__ float bf_src(float v, float v2, float one_minus_a, float floor_m) {
  return SMOOTH ? __fmul_rn(bf_measure(v, one_minus_a, floor_m), v2) : v;
}

// Stage the tile plus its R halo of a map moved by whole pixels: T[r][c] = src(gy0 + r, gx0 + c), zero outside the grid.
// 64-bit coordinates: the offsets may be any int32.  VEC: w % 4 == 0 and 16-byte aligned maps, so aligned quads are wholly
// inside or wholly outside a row; the backward step loads two quads (heat, beta) per LDS quad.
template <bool VEC, bool SMOOTH>
__device__ __forceinline__ void bf_stage_shift(float* T, const float* __restrict__ pb, const float* __restrict__ pb2,
                                               float one_minus_a, float floor_m, long long gy0, long long gx0, int rows, int PW,
                                               int h, int w) {
  const int tid = threadIdx.x;
  if (VEC) {
    const long long gxa = gx0 & ~3LL;
    const int lead = (int)(gx0 - gxa);
    const int nq = (PW + lead + 3) >> 2;
    for (int idx = tid; idx < rows * nq; idx += 256) {
      const int r = idx / nq, q = idx - r * nq;
      const long long gy = gy0 + r, gx = gxa + 4 * q;
      cc_f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
        v = *reinterpret_cast<const cc_f32x4*>(pb + (size_t)gy * w + (size_t)gx);
        if (SMOOTH) {
          const cc_f32x4 v2 = *reinterpret_cast<const cc_f32x4*>(pb2 + (size_t)gy * w + (size_t)gx);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = bf_src<true>(v[e], v2[e], one_minus_a, floor_m);
        }
      }
      const int c = 4 * q - lead;
      if (lead == 0) {
        *reinterpret_cast<cc_f32x4*>(T + r * PW + c) = v;        // q < PW / 4 here
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (c + e >= 0 && c + e < PW) T[r * PW + c + e] = v[e];
      }
    }
  } else {
    for (int idx = tid; idx < rows * PW; idx += 256) {
      const int r = idx / PW, c = idx - r * PW;
      const long long gy = gy0 + r, gx = gx0 + c;
      float v = 0.f;
      if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
        const size_t e = (size_t)gy * w + (size_t)gx;
        v = bf_src<SMOOTH>(pb[e], SMOOTH ? pb2[e] : 0.f, one_minus_a, floor_m);
      }
      T[idx] = v;
    }
  }
}

// The barrier after the staging of T, the row pass and the column pass: q[o] is the blurred value of tile pixel
// (4 (tid / 64) + o, tid % 64).  REV indexes both tap vectors in reverse (the backward step's adjoint blur).  MAXP is the
// max-product form (tracking.viterbi_step_spec): every sum over taps becomes a maximum, acc = fmaxf(acc, k * w) from a zero
// start — a NaN product is ignored and negative values count as zero; staging, layout and barriers are the same:
// P[y,x] = max_i ky[i+R] max_j kx[j+R] delta[y - oy - i, x - ox - j].  Every product is rounded once and a maximum rounds
// nothing, so P carries the bits of __fmul_rn(ky, __fmul_rn(kx, delta)) at its winning source pixel — what
// belief_backtrack_kernel recomputes.
template <bool REV, bool MAXP = false>
__device__ __forceinline__ void bf_passes(const float* T, float* mid, const float* __restrict__ taps, int R, bool skip, int b,
                                          float* q) {
  const int tid = threadIdx.x;
  const int rows = BF_TH + 2 * R, PW = bf_pitch(R), K = 2 * R + 1;
  __syncthreads();
  if (!skip) {
    // row pass: mid[r][x] = sum_j kx[2R - j] T[r][x + j], four consecutive x per lane from 16-byte pieces of the row
    const float* kx = taps + ((size_t)b * 2 + 1) * K;
    for (int item = tid; item < rows * (BF_TW / 4); item += 256) {
      const int r = item >> 4, t = item & 15;
      const float* tr = T + r * PW + 4 * t;
      cc_f32x4 cur = *reinterpret_cast<const cc_f32x4*>(tr);
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      for (int m = 0; 4 * m < K; ++m) {
        const cc_f32x4 nxt = *reinterpret_cast<const cc_f32x4*>(tr + 4 * m + 4);
        const float wv[7] = {cur[0], cur[1], cur[2], cur[3], nxt[0], nxt[1], nxt[2]};
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int j = 4 * m + jj;
          if (j < K) {
            const float k = kx[REV ? j : 2 * R - j];
            a0 = MAXP ? fmaxf(a0, __fmul_rn(k, wv[jj])) : fmaf(k, wv[jj], a0);
            a1 = MAXP ? fmaxf(a1, __fmul_rn(k, wv[jj + 1])) : fmaf(k, wv[jj + 1], a1);
            a2 = MAXP ? fmaxf(a2, __fmul_rn(k, wv[jj + 2])) : fmaf(k, wv[jj + 2], a2);
            a3 = MAXP ? fmaxf(a3, __fmul_rn(k, wv[jj + 3])) : fmaf(k, wv[jj + 3], a3);
          }
        }
        cur = nxt;
      }
      *reinterpret_cast<cc_f32x4*>(mid + r * BF_TW + 4 * t) = (cc_f32x4){a0, a1, a2, a3};
    }
  }
  __syncthreads();
  // column pass: wave s owns tile rows 4s .. 4s + 3, lanes along x
  const int tx = tid & 63, s4 = (tid >> 6) * 4;
  q[0] = q[1] = q[2] = q[3] = 0.f;
  if (!skip) {
    const float* ky = taps + (size_t)b * 2 * K;
    const float* mc = mid + s4 * BF_TW + tx;
    float w0 = mc[0], w1 = mc[BF_TW], w2 = mc[2 * BF_TW];
    for (int i = 0; i < K; ++i) {
      const float w3 = mc[(i + 3) * BF_TW];
      const float k = ky[REV ? i : 2 * R - i];
      q[0] = MAXP ? fmaxf(q[0], __fmul_rn(k, w0)) : fmaf(k, w0, q[0]);
      q[1] = MAXP ? fmaxf(q[1], __fmul_rn(k, w1)) : fmaf(k, w1, q[1]);
      q[2] = MAXP ? fmaxf(q[2], __fmul_rn(k, w2)) : fmaf(k, w2, q[2]);
      q[3] = MAXP ? fmaxf(q[3], __fmul_rn(k, w3)) : fmaf(k, w3, q[3]);
      w0 = w1; w1 = w2; w2 = w3;
    }
  }
}

// The product, the output map(s) and the tile's record.  Forward: aux = heat, m = fma(1 - a, heat, floor), U = q m into post.
// SMOOTH: aux = alpha, m = alpha, V = q alpha into post and q itself into bout.
template <bool SMOOTH>
__device__ __forceinline__ void bf_epilogue(const float* q, const float* __restrict__ aux, float one_minus_a, float floor_m,
                                            bool skip, float* __restrict__ post, float* __restrict__ bout,
                                            double* __restrict__ scratch, int b, int tile, int ntiles, int y0, int x0, int h,
                                            int w) {
  __shared__ double red[4][BF_NSUM];
  __shared__ float rv[2][4];
  __shared__ int ri[2][4];
  const int tid = threadIdx.x;
  const int tx = tid & 63, s4 = (tid >> 6) * 4;
  const size_t n = (size_t)h * w;
  double acc[BF_NSUM];
#pragma unroll
  for (int k = 0; k < BF_NSUM; ++k) acc[k] = 0.0;
  BfArg au = {-INFINITY, BF_NONE}, am = {-INFINITY, BF_NONE};
  const int x = x0 + tx;
  if (x < w) {
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int y = y0 + s4 + o;
      if (y < h) {
        const size_t e = (size_t)y * w + x;
        const float av = aux[(size_t)b * n + e];
        const float mv = SMOOTH ? av : bf_measure(av, one_minus_a, floor_m);
        const float uv = q[o] * mv;
        if (!skip) {
          post[(size_t)b * n + e] = uv;
          if (SMOOTH) bout[(size_t)b * n + e] = q[o];
        }
        acc[0] += (double)q[o];
        bf_moments(acc + 1, uv, y, x);
        bf_moments(acc + 7, mv, y, x);
        au.take(uv, (int)e);
        am.take(mv, (int)e);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < BF_NSUM; ++k) acc[k] = wave_sum_f64(acc[k]);
  au.wave_merge();
  am.wave_merge();
  const int wave = tid >> 6;
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < BF_NSUM; ++k) red[wave][k] = acc[k];
    rv[0][wave] = au.v; ri[0][wave] = au.i;
    rv[1][wave] = am.v; ri[1][wave] = am.i;
  }
  __syncthreads();
  if (tid < BF_NSUM) {
    double* rec = scratch + ((size_t)b * ntiles + tile) * BF_REC;
    rec[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  } else if (tid == 64) {
    double* rec = scratch + ((size_t)b * ntiles + tile) * BF_REC;
    au = {rv[0][0], ri[0][0]};
    am = {rv[1][0], ri[1][0]};
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      au.merge(rv[0][k], ri[0][k]);
      am.merge(rv[1][k], ri[1][k]);
    }
    rec[13] = (double)au.v; rec[14] = (double)au.i;
    rec[15] = (double)am.v; rec[16] = (double)am.i;
    rec[17] = 0.0;
  }
}

// The most likely path of every track over a whole drive (tracking.backtrack_spec), one launch: a workgroup owns a track and
// walks the frames from the last to the first.  There are no back-pointer maps — the decision of a link is recomputed at the
// one pixel the path passes through: the lanes stride over the (2R+1)^2 source pixels of the current pixel, form
// ky (kx delta) in the forward kernel's association and merge (value first, then the smaller flat source index).  Only
// positive finite candidates compete.  deltas [T,B,h w], ori [T,B,2,h w], offsets [T,B,2], taps [T,B,2,2R+1], rows [T,B,14]
// of the forward pass, reset [T,B] or null, path [T,B,8].  Pixels read from `rows` are clamped to the grid.
constexpr int BF_PATH = 8;
__global__ __launch_bounds__(256) void belief_backtrack_kernel(const float* __restrict__ deltas, const float* __restrict__ ori,
                                                               const int* __restrict__ offsets, const float* __restrict__ taps,
                                                               int R, const double* __restrict__ rows,
                                                               const int* __restrict__ reset, double* __restrict__ path,
                                                               int frames, int batch, int h, int w) {
  __shared__ int cur[3];                                         // y, x, link of the frame being written
  __shared__ float cur_score;
  __shared__ float rv[4];
  __shared__ int ri[4];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int K = 2 * R + 1;
  const size_t n = (size_t)h * w;
  auto row_pixel = [&](int t, int* y, int* x) {                  // the arg-max of frame t's row, clamped (NaN gives 0)
    const double* r = rows + ((size_t)t * batch + b) * 14;
    const double ry = r[0], rx = r[1];
    *y = ry >= 0.0 ? (ry < (double)h ? (int)ry : h - 1) : 0;
    *x = rx >= 0.0 ? (rx < (double)w ? (int)rx : w - 1) : 0;
  };
  if (tid == 0) {
    int y, x;
    row_pixel(frames - 1, &y, &x);
    cur[0] = y; cur[1] = x; cur[2] = 1;
    cur_score = 0.f;
  }
  __syncthreads();
  for (int t = frames - 1; t >= 0; --t) {
    const int y = cur[0], x = cur[1];
    const size_t tb = (size_t)t * batch + b;
    if (tid == 0) {
      const size_t e = (size_t)y * w + x;
      const float c = ori[(tb * 2 + 0) * n + e], s = ori[(tb * 2 + 1) * n + e];
      double ang = NAN;
      if (fabsf(c) <= 1.0f && fabsf(s) <= 1.0f) ang = angle_deg_f64((double)c, s < 0.0f);
      double* p = path + tb * BF_PATH;
      p[0] = (double)y; p[1] = (double)x;
      p[2] = (double)deltas[tb * n + e];
      p[3] = (double)c; p[4] = (double)s; p[5] = ang;
      p[6] = (double)cur[2]; p[7] = (double)cur_score;
    }
    if (t == 0) break;
    const bool start = (reset != nullptr && reset[tb] != 0) || rows[tb * 14 + 7] != 0.0;      // uniform over the workgroup
    BfArg best = {-INFINITY, BF_NONE};
    if (!start) {
      const long long cy = (long long)y - offsets[2 * tb], cx = (long long)x - offsets[2 * tb + 1];
      const float* ky = taps + tb * 2 * K;
      const float* kx = ky + K;
      const float* dp = deltas + (tb - batch) * n;               // frame t - 1
      for (int c = tid; c < K * K; c += 256) {
        const int ii = c / K, jj = c - ii * K;
        const long long sy = cy - (ii - R), sx = cx - (jj - R);
        if (sy >= 0 && sy < h && sx >= 0 && sx < w) {
          const int e = (int)(sy * w + sx);
          const float v = __fmul_rn(ky[ii], __fmul_rn(kx[jj], dp[e]));
          if (v > 0.f && v < INFINITY) best.merge(v, e);
        }
      }
    }
    best.wave_merge();
    if ((tid & 63) == 0) { rv[tid >> 6] = best.v; ri[tid >> 6] = best.i; }
    __syncthreads();                                             // every lane has read cur; the waves' candidates are in LDS
    if (tid == 0) {
#pragma unroll
      for (int k = 1; k < 4; ++k) best.merge(rv[k], ri[k]);
      if (best.i != BF_NONE) {
        cur[0] = best.i / w; cur[1] = best.i % w; cur[2] = 0;
        cur_score = best.v;
      } else {
        int py, px;
        row_pixel(t - 1, &py, &px);
        cur[0] = py; cur[1] = px; cur[2] = start ? 1 : 2;
        cur_score = 0.f;
      }
    }
    __syncthreads();
  }
}

// (a0 y + a1 x) + a2 with every product and every sum rounded on its own, as numpy evaluates the specification's expression.
// The operators are written out under contract(off): __dmul_rn / __dadd_rn are plain inline `*` and `+` in this toolchain, and
// the compiler fuses them into a multiply-add across the call (seen in the ISA) — the pragma only governs what it encloses.
__device__ __forceinline__ double bf_affine(double a0, double a1, double a2, double y, double x) {
#pragma clang fp contract(off)
  const double p = a0 * y;
  const double q = a1 * x;
  const double s = p + q;
  return s + a2;
}

// tracking.invert_motion on the device, operation for operation: the general 2 x 2 inverse in double with every product, sum
// and quotient rounded on its own; NaN rows (which sample nothing) for a singular or non-finite row.
__device__ __forceinline__ void bf_invert_motion(const double* __restrict__ m, double* o) {
#pragma clang fp contract(off)
  const double a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[3], a11 = m[4], a12 = m[5];
  const double p = a00 * a11;
  const double r = a01 * a10;
  const double det = p - r;
  bool ok = fabs(det) < (double)INFINITY && det != 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) ok = ok && fabs(m[k]) < (double)INFINITY;
  const double b00 = a11 / det, b01 = -a01 / det, b10 = -a10 / det, b11 = a00 / det;
  const double t0 = b00 * a02, t1 = b01 * a12, t2 = b10 * a02, t3 = b11 * a12;
  const double s0 = t0 + t1, s1 = t2 + t3;
  o[0] = ok ? b00 : NAN; o[1] = ok ? b01 : NAN; o[2] = ok ? -s0 : NAN;
  o[3] = ok ? b10 : NAN; o[4] = ok ? b11 : NAN; o[5] = ok ? -s1 : NAN;
}

// Stage W, the bilinear sample of a map through an inverse map, on the (16 + 2R) x (64 + 2R) pixels the tile's blur reads — the
// halo is warped too, the blur runs over W.  The
// source coordinates are computed per sample in double from the integer pixel with separately rounded products and sums in the
// order of the specification (no contraction, no stepping), so floor() and the fp32 weights are the specification's; the range
// test is done on the doubles (any motion row, NaN and inf included, reads nothing outside the prior).  The four taps are
// gathered from global memory (1 MB per track at 512 x 512: L2-resident, 2-D local); columns of T beyond 64 + 2R are loaded by
// the row pass but enter no sum.  SMOOTH gathers the four taps of both maps (heat, beta) and samples G = M beta.
template <bool SMOOTH>
__device__ __forceinline__ void bf_stage_warp(float* T, const float* __restrict__ pb, const float* __restrict__ pb2,
                                              const double* m, float one_minus_a, float floor_m, int R, int y0, int x0, int h,
                                              int w) {
  const int tid = threadIdx.x;
  const int rows = BF_TH + 2 * R, cols = BF_TW + 2 * R, PW = bf_pitch(R);
  const double a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[3], a11 = m[4], a12 = m[5];
  const double hd = (double)h, wd = (double)w;
  for (int idx = tid; idx < rows * cols; idx += 256) {
    const int r = idx / cols, c = idx - r * cols;
    const double y = (double)(y0 + r - R), x = (double)(x0 + c - R);
    const double sy = bf_affine(a00, a01, a02, y, x), sx = bf_affine(a10, a11, a12, y, x);
    float v = 0.f;
    if (sy > -1.0 && sy < hd && sx > -1.0 && sx < wd) {        // false for NaN and inf; only then to int
      const double fy0 = floor(sy), fx0 = floor(sx);
      const double fy = sy - fy0, fx = sx - fx0;
      const int iy = (int)fy0, ix = (int)fx0;                  // -1 .. h - 1, -1 .. w - 1
      const float wy1 = (float)fy, wy0 = (float)(1.0 - fy);
      const float wx1 = (float)fx, wx0 = (float)(1.0 - fx);
      const bool ya = iy >= 0, yb = iy + 1 < h, xa = ix >= 0, xb = ix + 1 < w;
      const long long e = (long long)iy * w + ix;              // dereferenced only under the guards
      float v00 = 0.f, v01 = 0.f, v10 = 0.f, v11 = 0.f;
      if (ya && xa) v00 = bf_src<SMOOTH>(pb[e], SMOOTH ? pb2[e] : 0.f, one_minus_a, floor_m);
      if (ya && xb) v01 = bf_src<SMOOTH>(pb[e + 1], SMOOTH ? pb2[e + 1] : 0.f, one_minus_a, floor_m);
      if (yb && xa) v10 = bf_src<SMOOTH>(pb[e + w], SMOOTH ? pb2[e + w] : 0.f, one_minus_a, floor_m);
      if (yb && xb) v11 = bf_src<SMOOTH>(pb[e + w + 1], SMOOTH ? pb2[e + w + 1] : 0.f, one_minus_a, floor_m);
      const float top = fmaf(wx1, v01, __fmul_rn(wx0, v00));
      const float bot = fmaf(wx1, v11, __fmul_rn(wx0, v10));
      v = fmaf(wy1, bot, __fmul_rn(wy0, top));
    }
    T[r * PW + c] = v;
  }
}

// The arguments of launch one, by value.  prev: the prior (forward) or beta, the message of frame t (BF_BACK); alpha: the
// stored posterior (BF_BACK only); move: offsets int32 [B,2] or, WARP, motion double [B,6]; skip: reset (forward) or cut
// (BF_BACK) flags, or null; out: post / smooth; beta_out: BF_BACK only.
struct BfStep {
  const float *prev, *heat, *alpha;
  const void* move;
  const float* taps;
  const int* skip;
  float *out, *beta_out;
  double* scratch;
  int R, h, w, ntx, nty;
  float one_minus_a, floor_m;
};

// Launch one of every step.  Forward, shift: T[r][c] = prior(y0 + r - R - oy, x0 + c - R - ox).  BF_BACK, shift
// (tracking.smooth_step_spec): the forward step's own offsets and taps, used the other way round —
// T[r][c] = G(y0 + r - R + oy, x0 + c - R + ox) and the taps in reverse, B'[y,x] = sum_ij ky[i+R] kx[j+R]
// G[y + oy + i, x + ox + j].  The sign lives in the 64-bit index arithmetic: no offset is negated.  WARP: T[r][c] =
// W(y0 + r - R, x0 + c - R), c < 64 + 2R, the map resampled through the track's inverse map; BF_BACK
// (tracking.smooth_step_rigid_spec) resamples G = M beta of frame t along the REVERSE motion — the forward step's motion row,
// inverted here.  A bilinear gather's adjoint would be a scatter: this is the same continuous model discretised the other
// way, not the exact adjoint of the rigid predict (for whole-pixel shifts and quarter turns the two coincide).
template <int MODE, bool WARP, bool VEC>
__global__ __launch_bounds__(256) void belief_step_kernel(const BfStep a) {
  extern __shared__ cc_f32x4 bf_smem[];
  constexpr bool BACK = MODE == BF_BACK;
  const int R = a.R, h = a.h, w = a.w;
  const int ntiles = a.ntx * a.nty;
  const int b = blockIdx.x / ntiles, tile = blockIdx.x - b * ntiles;
  const int y0 = (tile / a.ntx) * BF_TH, x0 = (tile % a.ntx) * BF_TW;
  const int rows = BF_TH + 2 * R, PW = bf_pitch(R);
  float* T = reinterpret_cast<float*>(bf_smem);                  // [rows][PW]: the moved map
  float* mid = T + rows * PW;                                    // [rows][BF_TW]: the row pass
  // a reset track starts from the measurement: no predict; a cut frame is the last of its segment: no message to bring back
  const bool skip = a.skip != nullptr && a.skip[b] != 0;
  if (!skip) {
    const size_t n = (size_t)h * w;
    const float* src = (BACK ? a.heat : a.prev) + (size_t)b * n;
    const float* src2 = BACK ? a.prev + (size_t)b * n : nullptr;
    if (WARP) {
      const double* m = static_cast<const double*>(a.move) + (size_t)b * 6;
      double mm[6] = {m[0], m[1], m[2], m[3], m[4], m[5]};
      if (BACK) bf_invert_motion(m, mm);
      bf_stage_warp<BACK>(T, src, src2, mm, a.one_minus_a, a.floor_m, R, y0, x0, h, w);
    } else {
      const int* offsets = static_cast<const int*>(a.move);
      const long long oy = offsets[2 * b], ox = offsets[2 * b + 1];
      const long long gy0 = (long long)y0 - R, gx0 = (long long)x0 - R;
      bf_stage_shift<VEC, BACK>(T, src, src2, a.one_minus_a, a.floor_m, BACK ? gy0 + oy : gy0 - oy, BACK ? gx0 + ox : gx0 - ox,
                                rows, PW, h, w);
    }
  }
  float q[4];
  bf_passes<BACK, MODE == BF_MAX>(T, mid, a.taps, R, skip, b, q);
  bf_epilogue<BACK>(q, BACK ? a.alpha : a.heat, a.one_minus_a, a.floor_m, skip, a.out, a.beta_out, a.scratch, b, tile, ntiles,
                    y0, x0, h, w);
}

// The track's records, merged in a fixed order by every workgroup of launch two: lane-strided, butterfly, waves 0..3.  fin
// [BF_NSUM], fv [2], fi [2] are the caller's shared arrays; ends with a barrier.
__device__ __forceinline__ void bf_merge_records(const double* __restrict__ rec, int ntiles, double* fin, float* fv, int* fi) {
  __shared__ double red[4][BF_NSUM];
  __shared__ float rv[2][4];
  __shared__ int ri[2][4];
  const int tid = threadIdx.x;
  double acc[BF_NSUM];
#pragma unroll
  for (int k = 0; k < BF_NSUM; ++k) acc[k] = 0.0;
  BfArg au = {-INFINITY, BF_NONE}, am = {-INFINITY, BF_NONE};
  for (int t = tid; t < ntiles; t += 256) {
    const double* r = rec + (size_t)t * BF_REC;
#pragma unroll
    for (int k = 0; k < BF_NSUM; ++k) acc[k] += r[k];
    au.merge((float)r[13], (int)r[14]);
    am.merge((float)r[15], (int)r[16]);
  }
#pragma unroll
  for (int k = 0; k < BF_NSUM; ++k) acc[k] = wave_sum_f64(acc[k]);
  au.wave_merge();
  am.wave_merge();
  const int wave = tid >> 6;
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < BF_NSUM; ++k) red[wave][k] = acc[k];
    rv[0][wave] = au.v; ri[0][wave] = au.i;
    rv[1][wave] = am.v; ri[1][wave] = am.i;
  }
  __syncthreads();
  if (tid < BF_NSUM) {
    fin[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  } else if (tid == 64) {
    au = {rv[0][0], ri[0][0]};
    am = {rv[1][0], ri[1][0]};
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      au.merge(rv[0][k], ri[0][k]);
      am.merge(rv[1][k], ri[1][k]);
    }
    fv[0] = au.v; fi[0] = au.i == BF_NONE ? 0 : au.i;            // nothing but NaN: index 0, as eval_metrics_kernel
    fv[1] = am.v; fi[1] = am.i == BF_NONE ? 0 : am.i;
  }
  __syncthreads();
}

// The 14 columns of a track's row from the merged record: bi the arg-max index, best the unscaled value there, mom the six
// moment sums of the map the state selected, Z = mom[0], S the record's first sum.
__device__ __forceinline__ void bf_write_row(double* __restrict__ r, const float* __restrict__ ori, int b, size_t n, int w,
                                             int bi, float best, float inv, const double* mom, double Z, int state, double S) {
  const float c = ori[((size_t)b * 2 + 0) * n + bi], s = ori[((size_t)b * 2 + 1) * n + bi];
  double ang = NAN;
  if (fabsf(c) <= 1.0f && fabsf(s) <= 1.0f) ang = angle_deg_f64((double)c, s < 0.0f);
  const double my = mom[1] / Z, mx = mom[2] / Z;
  r[0] = (double)(bi / w); r[1] = (double)(bi % w);
  r[2] = (double)(best * inv);
  r[3] = (double)c; r[4] = (double)s; r[5] = ang;
  r[6] = Z; r[7] = (double)state;
  r[8] = my; r[9] = mx;
  r[10] = mom[3] / Z - my * my;
  r[11] = mom[4] / Z - mx * mx;
  r[12] = mom[5] / Z - my * mx;
  r[13] = S;
}

// Launch two.  Forward (aux = heat, out = post): state 1 for a reset track, 2 when not (Z > 0 and finite); state 0 scales U by
// (float)(1 / Z), otherwise post = M (float)(1 / sum M).  BACK (aux = alpha, out = smooth): state 1 for a cut track, 2 when not
// (Z > 0 and finite and S > 0 and finite); state 0 scales V by (float)(1 / Z) and B' by (float)(1 / S); otherwise smooth =
// alpha (float)(1 / sum alpha) and the message is uniform.
template <bool VEC, bool BACK>
__global__ __launch_bounds__(256) void belief_finish_kernel(const float* __restrict__ aux, const float* __restrict__ ori,
                                                            float one_minus_a, float floor_m, const int* __restrict__ skip,
                                                            float* __restrict__ out, float* __restrict__ beta_out,
                                                            const double* __restrict__ scratch, double* __restrict__ rows, int h,
                                                            int w, int ntiles, int slices, int slice_len) {
  __shared__ double fin[BF_NSUM];
  __shared__ float fv[2];
  __shared__ int fi[2];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / slices, sl = blockIdx.x - b * slices;
  bf_merge_records(scratch + (size_t)b * ntiles * BF_REC, ntiles, fin, fv, fi);
  int state = (skip != nullptr && skip[b] != 0) ? 1 : 0;
  const double S = fin[0];
  double Z = fin[1];
  if (!state && !(Z > 0.0 && Z < (double)INFINITY && (!BACK || (S > 0.0 && S < (double)INFINITY)))) state = 2;
  const int sel = state ? 1 : 0;                                 // the M / alpha record serves a reset / the fallback
  const double* mom = fin + 1 + 6 * sel;
  Z = mom[0];
  const size_t n = (size_t)h * w;
  const float inv = (float)(1.0 / Z);
  const float* ab = aux + (size_t)b * n;
  float* ob = out + (size_t)b * n;
  const size_t e0 = (size_t)sl * slice_len, e1 = e0 + slice_len < n ? e0 + slice_len : n;
  // The per-element update, one loop per mode: VEC means n % 4 == 0, slice_len % 4 == 0 and 16-byte aligned maps.  The
  // backward form issues both loads before either product (one merged loop serialised them: 5 % at B = 1).
  if constexpr (BACK) {
    const float invs = state ? (float)(1.0 / (double)n) : (float)(1.0 / S);
    float* bb = beta_out + (size_t)b * n;
    if (VEC) {
      for (size_t i = e0 + 4 * (size_t)tid; i < e1; i += 1024) {
        cc_f32x4 v, m;
        if (state) {
          v = *reinterpret_cast<const cc_f32x4*>(ab + i);
          m = (cc_f32x4){invs, invs, invs, invs};
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] *= inv;
        } else {
          v = *reinterpret_cast<const cc_f32x4*>(ob + i);
          m = *reinterpret_cast<const cc_f32x4*>(bb + i);
#pragma unroll
          for (int k = 0; k < 4; ++k) { v[k] *= inv; m[k] *= invs; }
        }
        *reinterpret_cast<cc_f32x4*>(ob + i) = v;
        *reinterpret_cast<cc_f32x4*>(bb + i) = m;
      }
    } else {
      for (size_t i = e0 + tid; i < e1; i += 256) {
        ob[i] = (state ? ab[i] : ob[i]) * inv;
        bb[i] = state ? invs : bb[i] * invs;
      }
    }
  } else if (VEC) {
    for (size_t i = e0 + 4 * (size_t)tid; i < e1; i += 1024) {
      cc_f32x4 v;
      if (state) {
        const cc_f32x4 hv = *reinterpret_cast<const cc_f32x4*>(ab + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = bf_measure(hv[k], one_minus_a, floor_m) * inv;
      } else {
        v = *reinterpret_cast<const cc_f32x4*>(ob + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] *= inv;
      }
      *reinterpret_cast<cc_f32x4*>(ob + i) = v;
    }
  } else {
    for (size_t i = e0 + tid; i < e1; i += 256) ob[i] = (state ? bf_measure(ab[i], one_minus_a, floor_m) : ob[i]) * inv;
  }
  if (sl != 0 || tid != 0) return;
  bf_write_row(rows + (size_t)b * 14, ori, b, n, w, fi[sel], fv[sel], inv, mom, Z, state, S);
}

static bool bf_tiles(int h, int w, int* ntx, int* nty) {
  if (h <= 0 || w <= 0 || (long long)h * w > 0x7ffffff0LL) return false;      // the finish kernel's slice length (h w rounded up to 4) is an int
  *ntx = (w + BF_TW - 1) / BF_TW;
  *nty = (h + BF_TH - 1) / BF_TH;
  return (long long)*ntx * *nty * BF_REC <= 0x7fffffffLL;
}

}  // namespace ccvpe

using namespace ccvpe;

extern "C" int ccvpe_belief_partials(int h, int w) {
  int ntx, nty;
  if (!bf_tiles(h, w, &ntx, &nty)) return CCVPE_EINVAL;
  return ntx * nty * BF_REC;
}


namespace ccvpe {

static bool bf_overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + bbytes && b0 < a0 + abytes;
}

// The argument checks the step entry points share; `move` is the step's own motion input (offsets / motion), `who` the entry's
// name in the message.  The backward step passes beta as prior, cut as reset and smooth as post.
static int bf_check(const char* who, const float* prior, const float* heat, const float* ori, const void* move, const float* taps,
                    int radius, float outlier, const int* reset, float* post, double* scratch, double* rows, int batch, int h,
                    int w, int* ntx, int* nty) {
  if (batch <= 0 || !bf_tiles(h, w, ntx, nty)) return fail(CCVPE_EINVAL, "%s: bad shape", who);
  const long long ntiles = (long long)*ntx * *nty;
  if (ntiles * batch > 0x7fffffffLL) return fail(CCVPE_EINVAL, "%s: batch x tiles > 2^31", who);
  if (radius < 0 || radius > 32) return fail(CCVPE_EINVAL, "%s: radius %d outside [0, 32]", who, radius);
  if (!(outlier >= 0.f && outlier <= 1.f)) return fail(CCVPE_EINVAL, "%s: outlier outside [0, 1]", who);
  if (!prior || !heat || !ori || !move || !taps || !post || !scratch || !rows)
    return fail(CCVPE_EINVAL, "%s: null pointer", who);
  if ((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(scratch)) & 7)
    return fail(CCVPE_EINVAL, "%s: rows and scratch must be 8-byte aligned", who);
  if ((reinterpret_cast<uintptr_t>(prior) | reinterpret_cast<uintptr_t>(heat) | reinterpret_cast<uintptr_t>(ori) |
       reinterpret_cast<uintptr_t>(post) | reinterpret_cast<uintptr_t>(move) | reinterpret_cast<uintptr_t>(taps) |
       reinterpret_cast<uintptr_t>(reset)) & 3)
    return fail(CCVPE_EINVAL, "%s: float and int arrays must be 4-byte aligned", who);
  const size_t n = (size_t)h * w, bytes = (size_t)batch * n * sizeof(float);
  if (bf_overlap(prior, bytes, post, bytes)) return fail(CCVPE_EINVAL, "%s: prior and post overlap", who);
  // launch one writes U into post and launch two reads heat (a reset recomputes M from it) and ori (the row) afterwards
  if (bf_overlap(heat, bytes, post, bytes)) return fail(CCVPE_EINVAL, "%s: heat and post overlap", who);
  if (bf_overlap(ori, 2 * bytes, post, bytes)) return fail(CCVPE_EINVAL, "%s: ori and post overlap", who);
  return CCVPE_OK;
}

// What the backward step checks beyond bf_check: alpha and beta_out, and that neither output shares memory with the other or
// with any input map — launch two reads alpha, heat's neighbours in launch one's halo and ori after launch one has written.
static int bf_check_smooth(const char* who, const float* beta, const float* heat, const float* alpha, const float* ori,
                           float* beta_out, float* smooth, int batch, int h, int w) {
  if (!alpha || !beta_out) return fail(CCVPE_EINVAL, "%s: null pointer", who);
  if ((reinterpret_cast<uintptr_t>(alpha) | reinterpret_cast<uintptr_t>(beta_out)) & 3)
    return fail(CCVPE_EINVAL, "%s: float and int arrays must be 4-byte aligned", who);
  const size_t bytes = (size_t)batch * h * w * sizeof(float);
  if (bf_overlap(alpha, bytes, smooth, bytes)) return fail(CCVPE_EINVAL, "%s: alpha and smooth overlap", who);
  if (bf_overlap(smooth, bytes, beta_out, bytes)) return fail(CCVPE_EINVAL, "%s: smooth and beta_out overlap", who);
  if (bf_overlap(beta, bytes, beta_out, bytes)) return fail(CCVPE_EINVAL, "%s: beta and beta_out overlap", who);
  if (bf_overlap(heat, bytes, beta_out, bytes)) return fail(CCVPE_EINVAL, "%s: heat and beta_out overlap", who);
  if (bf_overlap(alpha, bytes, beta_out, bytes)) return fail(CCVPE_EINVAL, "%s: alpha and beta_out overlap", who);
  if (bf_overlap(ori, 2 * bytes, beta_out, bytes)) return fail(CCVPE_EINVAL, "%s: ori and beta_out overlap", who);
  return CCVPE_OK;
}

// The slices of launch two: ~1024 workgroups scale the maps; each merges the track's records first
static int bf_slices(const char* who, int batch, size_t n, int* slices, int* slice_len) {
  int s = (1024 + batch - 1) / batch;
  s = s < 1 ? 1 : (s > 64 ? 64 : s);
  const size_t per = (n + s - 1) / s;
  *slice_len = (int)((per + 3) & ~(size_t)3);
  *slices = (int)((n + *slice_len - 1) / *slice_len);
  if ((long long)*slices * batch > 0x7fffffffLL) return fail(CCVPE_EINVAL, "%s: batch x slices > 2^31", who);
  return CCVPE_OK;
}

template <int MODE, bool WARP, bool VEC>
static int bf_launch_one(const char* who, const BfStep& a, unsigned grid, int smem, hipStream_t st) {
  auto kern = belief_step_kernel<MODE, WARP, VEC>;
  static DevCache lds_set;                                       // per instantiation, so per kernel
  if (int rc = ensure_dyn_lds(lds_set, kern, smem, who)) return rc;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), smem, st, a);
  return check_launch("belief_step_kernel");
}

// Both launches of a step whose arguments have passed bf_check (which gave a.ntx, a.nty).  `a` comes with everything but the
// two scalars of the measurement; `who` names the entry should the dynamic-LDS opt-in fail.
template <int MODE, bool WARP>
static int bf_run(const char* who, BfStep a, const float* ori, float outlier, double* rows, int batch, void* stream) {
  constexpr bool BACK = MODE == BF_BACK;
  hipStream_t st = (hipStream_t)stream;
  const long long ntiles = (long long)a.ntx * a.nty;
  const size_t n = (size_t)a.h * a.w;
  a.one_minus_a = 1.0f - outlier;
  a.floor_m = outlier / (float)n;
  const int smem = (int)sizeof(float) * (BF_TH + 2 * a.R) * (bf_pitch(a.R) + BF_TW);      // 64 000 B at R = 32
  const unsigned grid1 = (unsigned)(ntiles * batch);
  int rc;
  if constexpr (WARP) {                                          // the warp gathers single pixels: no vector form
    rc = bf_launch_one<MODE, true, false>(who, a, grid1, smem, st);
  } else {                                                       // quads of the map(s) the staging loads
    const bool vec1 = (a.w % 4) == 0 && aligned16(a.prev) && (!BACK || aligned16(a.heat));
    rc = vec1 ? bf_launch_one<MODE, false, true>(who, a, grid1, smem, st) : bf_launch_one<MODE, false, false>(who, a, grid1, smem, st);
  }
  if (rc) return rc;
  int slices, slice_len;
  if ((rc = bf_slices(BACK ? "belief_smooth_step" : "belief_step", batch, n, &slices, &slice_len))) return rc;
  const float* aux = BACK ? a.alpha : a.heat;
  const bool vec2 = (n % 4) == 0 && aligned16(aux) && aligned16(a.out) && (!BACK || aligned16(a.beta_out));
  hipLaunchKernelGGL((vec2 ? belief_finish_kernel<true, BACK> : belief_finish_kernel<false, BACK>), dim3((unsigned)(slices * batch)),
                     dim3(256), 0, st, aux, ori, a.one_minus_a, a.floor_m, a.skip, a.out, a.beta_out, a.scratch, rows, a.h, a.w,
                     (int)ntiles, slices, slice_len);
  return check_launch("belief_finish_kernel");
}

}  // namespace ccvpe

extern "C" int ccvpe_belief_step_f32(const float* prior, const float* heat, const float* ori, const int* offsets,
                                     const float* taps, int radius, float outlier, const int* reset, float* post,
                                     double* scratch, double* rows, int batch, int h, int w, void* stream) {
  const char* who = "belief_step";
  int ntx, nty;
  if (int rc = bf_check(who, prior, heat, ori, offsets, taps, radius, outlier, reset, post, scratch, rows, batch, h, w, &ntx, &nty))
    return rc;
  return bf_run<BF_SUM, false>(who, {prior, heat, nullptr, offsets, taps, reset, post, nullptr, scratch, radius, h, w, ntx, nty}, ori,
                               outlier, rows, batch, stream);
}

extern "C" int ccvpe_belief_step_rigid_f32(const float* prior, const float* heat, const float* ori, const double* motion,
                                           const float* taps, int radius, float outlier, const int* reset, float* post,
                                           double* scratch, double* rows, int batch, int h, int w, void* stream) {
  const char* who = "belief_step_rigid";
  int ntx, nty;                                                  // the shared checks report as belief_step
  if (int rc = bf_check("belief_step", prior, heat, ori, motion, taps, radius, outlier, reset, post, scratch, rows, batch, h, w,
                        &ntx, &nty))
    return rc;
  if (reinterpret_cast<uintptr_t>(motion) & 7) return fail(CCVPE_EINVAL, "%s: motion must be 8-byte aligned", who);
  return bf_run<BF_SUM, true>(who, {prior, heat, nullptr, motion, taps, reset, post, nullptr, scratch, radius, h, w, ntx, nty}, ori,
                              outlier, rows, batch, stream);
}

extern "C" int ccvpe_belief_viterbi_step_f32(const float* prior, const float* heat, const float* ori, const int* offsets,
                                             const float* taps, int radius, float outlier, const int* reset, float* post,
                                             double* scratch, double* rows, int batch, int h, int w, void* stream) {
  const char* who = "belief_viterbi_step";
  int ntx, nty;
  if (int rc = bf_check(who, prior, heat, ori, offsets, taps, radius, outlier, reset, post, scratch, rows, batch, h, w, &ntx, &nty))
    return rc;
  return bf_run<BF_MAX, false>(who, {prior, heat, nullptr, offsets, taps, reset, post, nullptr, scratch, radius, h, w, ntx, nty}, ori,
                               outlier, rows, batch, stream);
}

extern "C" int ccvpe_belief_smooth_step_f32(const float* beta, const float* heat, const float* alpha, const float* ori,
                                            const int* offsets, const float* taps, int radius, float outlier, const int* cut,
                                            float* beta_out, float* smooth, double* scratch, double* rows, int batch, int h,
                                            int w, void* stream) {
  const char* who = "belief_smooth_step";
  int ntx, nty;
  if (int rc = bf_check(who, beta, heat, ori, offsets, taps, radius, outlier, cut, smooth, scratch, rows, batch, h, w, &ntx, &nty))
    return rc;
  if (int rc = bf_check_smooth(who, beta, heat, alpha, ori, beta_out, smooth, batch, h, w)) return rc;
  return bf_run<BF_BACK, false>(who, {beta, heat, alpha, offsets, taps, cut, smooth, beta_out, scratch, radius, h, w, ntx, nty}, ori,
                                outlier, rows, batch, stream);
}

extern "C" int ccvpe_belief_smooth_step_rigid_f32(const float* beta, const float* heat, const float* alpha, const float* ori,
                                                  const double* motion, const float* taps, int radius, float outlier,
                                                  const int* cut, float* beta_out, float* smooth, double* scratch, double* rows,
                                                  int batch, int h, int w, void* stream) {
  const char* who = "belief_smooth_step_rigid";
  int ntx, nty;
  if (int rc = bf_check(who, beta, heat, ori, motion, taps, radius, outlier, cut, smooth, scratch, rows, batch, h, w, &ntx, &nty))
    return rc;
  if (int rc = bf_check_smooth(who, beta, heat, alpha, ori, beta_out, smooth, batch, h, w)) return rc;
  if (reinterpret_cast<uintptr_t>(motion) & 7) return fail(CCVPE_EINVAL, "%s: motion must be 8-byte aligned", who);
  return bf_run<BF_BACK, true>(who, {beta, heat, alpha, motion, taps, cut, smooth, beta_out, scratch, radius, h, w, ntx, nty}, ori,
                               outlier, rows, batch, stream);
}

extern "C" int ccvpe_belief_backtrack_f32(const float* deltas, const float* ori, const int* offsets, const float* taps, int radius,
                                          const double* rows, const int* reset, double* path, int frames, int batch, int h, int w,
                                          void* stream) {
  const char* who = "belief_backtrack";
  int ntx, nty;
  if (frames <= 0 || batch <= 0 || !bf_tiles(h, w, &ntx, &nty)) return fail(CCVPE_EINVAL, "%s: bad shape", who);
  if ((long long)frames * batch > 0x7fffffffLL) return fail(CCVPE_EINVAL, "%s: frames x batch > 2^31", who);
  if (radius < 0 || radius > 32) return fail(CCVPE_EINVAL, "%s: radius %d outside [0, 32]", who, radius);
  if (!deltas || !ori || !offsets || !taps || !rows || !path) return fail(CCVPE_EINVAL, "%s: null pointer", who);
  if ((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(path)) & 7)
    return fail(CCVPE_EINVAL, "%s: rows and path must be 8-byte aligned", who);
  if ((reinterpret_cast<uintptr_t>(deltas) | reinterpret_cast<uintptr_t>(ori) | reinterpret_cast<uintptr_t>(offsets) |
       reinterpret_cast<uintptr_t>(taps) | reinterpret_cast<uintptr_t>(reset)) & 3)
    return fail(CCVPE_EINVAL, "%s: float and int arrays must be 4-byte aligned", who);
  const size_t tb = (size_t)frames * batch, maps = tb * (size_t)h * w * sizeof(float), out = tb * BF_PATH * sizeof(double);
  if (bf_overlap(deltas, maps, path, out)) return fail(CCVPE_EINVAL, "%s: deltas and path overlap", who);
  if (bf_overlap(ori, 2 * maps, path, out)) return fail(CCVPE_EINVAL, "%s: ori and path overlap", who);
  if (bf_overlap(rows, tb * 14 * sizeof(double), path, out)) return fail(CCVPE_EINVAL, "%s: rows and path overlap", who);
  if (bf_overlap(offsets, tb * 2 * sizeof(int), path, out)) return fail(CCVPE_EINVAL, "%s: offsets and path overlap", who);
  if (bf_overlap(taps, tb * 2 * (2 * (size_t)radius + 1) * sizeof(float), path, out))
    return fail(CCVPE_EINVAL, "%s: taps and path overlap", who);
  if (reset && bf_overlap(reset, tb * sizeof(int), path, out)) return fail(CCVPE_EINVAL, "%s: reset and path overlap", who);
  hipLaunchKernelGGL(belief_backtrack_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, deltas, ori, offsets, taps,
                     radius, rows, reset, path, frames, batch, h, w);
  return check_launch("belief_backtrack_kernel");
}
