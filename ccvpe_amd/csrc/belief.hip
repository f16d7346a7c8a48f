// Histogram filter over the heat-map grid (ccvpe_amd/tracking.py: step_spec is the specification): one recursive Bayes step
// per track in two launches — predict (integer shift + separable blur of the prior) x measure (the network's heat-map mixed
// with a uniform outlier floor), then renormalise and read the estimate off the posterior.
//
// Launch one, belief_predict_kernel: a workgroup owns a (track, 16 x 64 output tile) pair.  The prior tile plus its R halo is
// staged in LDS already shifted by the track's integer offset, zero outside the grid; the row pass (16 B LDS reads, four
// outputs per lane) and the column pass (a four-deep register window down the column) run in fp32; the product with
// M = (1 - a) heat + a / (h w) is written as U and the tile's sums (double), arg-max candidate and moment sums go to one
// record per workgroup — for U and for M, so that a reset needs no third pass over the maps.
// Launch two, belief_finish_kernel: every workgroup of a track merges the track's records in the same fixed order, decides
// the reset, scales its slice of the map by (float)(1 / Z), and the first slice writes the row.
// No floating-point atomics: two runs are bit-identical.
#include "common.h"

namespace ccvpe {

constexpr int BF_TH = 16, BF_TW = 64;         // output tile; 256 threads
constexpr int BF_REC = 18;                     // doubles per workgroup record
// record layout: [0] sum Q | [1..6] U: s, sy, sx, syy, sxx, syx | [7..12] the same of M | [13] max U [14] its index |
//                [15] max M [16] its index | [17] unused
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

template <bool VEC>
__global__ __launch_bounds__(256) void belief_predict_kernel(const float* __restrict__ prior, const float* __restrict__ heat,
                                                             const int* __restrict__ offsets, const float* __restrict__ taps,
                                                             int R, float one_minus_a, float floor_m,
                                                             const int* __restrict__ reset, float* __restrict__ post,
                                                             double* __restrict__ scratch, int h, int w, int ntx, int nty) {
  extern __shared__ cc_f32x4 bf_smem[];
  __shared__ double red[4][BF_NSUM];
  __shared__ float rv[2][4];
  __shared__ int ri[2][4];
  const int tid = threadIdx.x;
  const int ntiles = ntx * nty;
  const int b = blockIdx.x / ntiles, tile = blockIdx.x - b * ntiles;
  const int y0 = (tile / ntx) * BF_TH, x0 = (tile % ntx) * BF_TW;
  const int rows = BF_TH + 2 * R, PW = bf_pitch(R), K = 2 * R + 1;
  float* T = reinterpret_cast<float*>(bf_smem);                  // [rows][PW]: T[r][c] = prior(y0 + r - R - oy, x0 + c - R - ox)
  float* mid = T + rows * PW;                                    // [rows][BF_TW]: the row pass
  const bool skip = reset != nullptr && reset[b] != 0;           // a reset track starts from the measurement: no predict
  const size_t n = (size_t)h * w;
  const float* pb = prior + (size_t)b * n;

  if (!skip) {
    // 64-bit coordinates: the offsets may be any int32
    const long long oy = offsets[2 * b], ox = offsets[2 * b + 1];
    const long long gy0 = (long long)y0 - R - oy, gx0 = (long long)x0 - R - ox;
    if (VEC) {                                                   // w % 4 == 0 and a 16-byte aligned prior: aligned quads are
      const long long gxa = gx0 & ~3LL;                          // wholly inside or wholly outside a row
      const int lead = (int)(gx0 - gxa);
      const int nq = (PW + lead + 3) >> 2;
      for (int idx = tid; idx < rows * nq; idx += 256) {
        const int r = idx / nq, q = idx - r * nq;
        const long long gy = gy0 + r, gx = gxa + 4 * q;
        cc_f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) v = *reinterpret_cast<const cc_f32x4*>(pb + (size_t)gy * w + (size_t)gx);
        const int c = 4 * q - lead;
        if (lead == 0) {
          *reinterpret_cast<cc_f32x4*>(T + r * PW + c) = v;      // q < PW / 4 here
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
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) v = pb[(size_t)gy * w + (size_t)gx];
        T[idx] = v;
      }
    }
  }
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
            const float k = kx[2 * R - j];
            a0 = fmaf(k, wv[jj], a0);
            a1 = fmaf(k, wv[jj + 1], a1);
            a2 = fmaf(k, wv[jj + 2], a2);
            a3 = fmaf(k, wv[jj + 3], a3);
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
  float q[4] = {0.f, 0.f, 0.f, 0.f};
  if (!skip) {
    const float* ky = taps + (size_t)b * 2 * K;
    const float* mc = mid + s4 * BF_TW + tx;
    float w0 = mc[0], w1 = mc[BF_TW], w2 = mc[2 * BF_TW];
    for (int i = 0; i < K; ++i) {
      const float w3 = mc[(i + 3) * BF_TW];
      const float k = ky[2 * R - i];
      q[0] = fmaf(k, w0, q[0]);
      q[1] = fmaf(k, w1, q[1]);
      q[2] = fmaf(k, w2, q[2]);
      q[3] = fmaf(k, w3, q[3]);
      w0 = w1; w1 = w2; w2 = w3;
    }
  }
  // measure, write U, tile record
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
        const float mv = fmaf(one_minus_a, heat[(size_t)b * n + e], floor_m);
        const float uv = q[o] * mv;
        if (!skip) post[(size_t)b * n + e] = uv;
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

template <bool VEC>
__global__ __launch_bounds__(256) void belief_finish_kernel(const float* __restrict__ heat, const float* __restrict__ ori,
                                                            float one_minus_a, float floor_m, const int* __restrict__ reset,
                                                            float* __restrict__ post, const double* __restrict__ scratch,
                                                            double* __restrict__ rows, int h, int w, int ntiles, int slices,
                                                            int slice_len) {
  __shared__ double red[4][BF_NSUM];
  __shared__ float rv[2][4];
  __shared__ int ri[2][4];
  __shared__ double fin[BF_NSUM];
  __shared__ float fv[2];
  __shared__ int fi[2];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / slices, sl = blockIdx.x - b * slices;
  const double* rec = scratch + (size_t)b * ntiles * BF_REC;
  // the track's records, merged in a fixed order: lane-strided, butterfly, waves 0..3
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
  int rst = (reset != nullptr && reset[b] != 0) ? 1 : 0;
  double Z = fin[1];
  if (!rst && !(Z > 0.0 && Z < (double)INFINITY)) rst = 2;
  const int sel = rst ? 1 : 0;                                   // the M record serves a reset
  const double* mom = fin + 1 + 6 * sel;
  Z = mom[0];
  const float inv = (float)(1.0 / Z);
  const size_t n = (size_t)h * w;
  const float* hb = heat + (size_t)b * n;
  float* pb = post + (size_t)b * n;
  const size_t e0 = (size_t)sl * slice_len, e1 = e0 + slice_len < n ? e0 + slice_len : n;
  if (VEC) {                                                     // n % 4 == 0, slice_len % 4 == 0, 16-byte aligned maps
    for (size_t i = e0 + 4 * (size_t)tid; i < e1; i += 1024) {
      cc_f32x4 v;
      if (rst) {
        const cc_f32x4 hv = *reinterpret_cast<const cc_f32x4*>(hb + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = fmaf(one_minus_a, hv[k], floor_m) * inv;
      } else {
        v = *reinterpret_cast<const cc_f32x4*>(pb + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] *= inv;
      }
      *reinterpret_cast<cc_f32x4*>(pb + i) = v;
    }
  } else {
    for (size_t i = e0 + tid; i < e1; i += 256) pb[i] = (rst ? fmaf(one_minus_a, hb[i], floor_m) : pb[i]) * inv;
  }
  if (sl != 0 || tid != 0) return;
  const int bi = fi[sel];
  const float c = ori[((size_t)b * 2 + 0) * n + bi], s = ori[((size_t)b * 2 + 1) * n + bi];
  double ang = NAN;
  if (fabsf(c) <= 1.0f && fabsf(s) <= 1.0f) ang = angle_deg_f64((double)c, s < 0.0f);
  const double my = mom[1] / Z, mx = mom[2] / Z;
  double* r = rows + (size_t)b * 14;
  r[0] = (double)(bi / w); r[1] = (double)(bi % w);
  r[2] = (double)(fv[sel] * inv);
  r[3] = (double)c; r[4] = (double)s; r[5] = ang;
  r[6] = Z; r[7] = (double)rst;
  r[8] = my; r[9] = mx;
  r[10] = mom[3] / Z - my * my;
  r[11] = mom[4] / Z - mx * mx;
  r[12] = mom[5] / Z - my * mx;
  r[13] = fin[0];
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

extern "C" int ccvpe_belief_step_f32(const float* prior, const float* heat, const float* ori, const int* offsets,
                                     const float* taps, int radius, float outlier, const int* reset, float* post,
                                     double* scratch, double* rows, int batch, int h, int w, void* stream) {
  int ntx, nty;
  if (batch <= 0 || !bf_tiles(h, w, &ntx, &nty)) return fail(CCVPE_EINVAL, "belief_step: bad shape");
  const long long ntiles = (long long)ntx * nty;
  if (ntiles * batch > 0x7fffffffLL) return fail(CCVPE_EINVAL, "belief_step: batch x tiles > 2^31");
  if (radius < 0 || radius > 32) return fail(CCVPE_EINVAL, "belief_step: radius %d outside [0, 32]", radius);
  if (!(outlier >= 0.f && outlier <= 1.f)) return fail(CCVPE_EINVAL, "belief_step: outlier outside [0, 1]");
  if (!prior || !heat || !ori || !offsets || !taps || !post || !scratch || !rows)
    return fail(CCVPE_EINVAL, "belief_step: null pointer");
  if ((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(scratch)) & 7)
    return fail(CCVPE_EINVAL, "belief_step: rows and scratch must be 8-byte aligned");
  if ((reinterpret_cast<uintptr_t>(prior) | reinterpret_cast<uintptr_t>(heat) | reinterpret_cast<uintptr_t>(ori) |
       reinterpret_cast<uintptr_t>(post) | reinterpret_cast<uintptr_t>(offsets) | reinterpret_cast<uintptr_t>(taps) |
       reinterpret_cast<uintptr_t>(reset)) & 3)
    return fail(CCVPE_EINVAL, "belief_step: float and int arrays must be 4-byte aligned");
  const size_t n = (size_t)h * w, bytes = (size_t)batch * n * sizeof(float);
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(prior), q0 = reinterpret_cast<uintptr_t>(post);
  if (p0 < q0 + bytes && q0 < p0 + bytes) return fail(CCVPE_EINVAL, "belief_step: prior and post overlap");
  // launch one writes U into post and launch two reads heat (a reset recomputes M from it) and ori (the row) afterwards
  const uintptr_t h0 = reinterpret_cast<uintptr_t>(heat), o0 = reinterpret_cast<uintptr_t>(ori);
  if (h0 < q0 + bytes && q0 < h0 + bytes) return fail(CCVPE_EINVAL, "belief_step: heat and post overlap");
  if (o0 < q0 + bytes && q0 < o0 + 2 * bytes) return fail(CCVPE_EINVAL, "belief_step: ori and post overlap");
  hipStream_t st = (hipStream_t)stream;
  const float one_minus_a = 1.0f - outlier, floor_m = outlier / (float)n;
  const int smem = (int)sizeof(float) * (BF_TH + 2 * radius) * (bf_pitch(radius) + BF_TW);      // 64 000 B at R = 32
  const bool vec1 = (w % 4) == 0 && aligned16(prior);
  const dim3 grid1((unsigned)(ntiles * batch));
  if (vec1) {
    auto kern = belief_predict_kernel<true>;
    static DevCache lds_set;
    if (int rc = ensure_dyn_lds(lds_set, kern, smem, "belief_step")) return rc;
    hipLaunchKernelGGL(kern, grid1, dim3(256), smem, st, prior, heat, offsets, taps, radius, one_minus_a, floor_m, reset, post,
                       scratch, h, w, ntx, nty);
  } else {
    auto kern = belief_predict_kernel<false>;
    static DevCache lds_set;
    if (int rc = ensure_dyn_lds(lds_set, kern, smem, "belief_step")) return rc;
    hipLaunchKernelGGL(kern, grid1, dim3(256), smem, st, prior, heat, offsets, taps, radius, one_minus_a, floor_m, reset, post,
                       scratch, h, w, ntx, nty);
  }
  if (int rc = check_launch("belief_predict_kernel")) return rc;
  // ~1024 workgroups scale the maps; each merges the track's records first
  int slices = (1024 + batch - 1) / batch;
  slices = slices < 1 ? 1 : (slices > 64 ? 64 : slices);
  const size_t per = (n + slices - 1) / slices;
  const int slice_len = (int)((per + 3) & ~(size_t)3);
  slices = (int)((n + slice_len - 1) / slice_len);
  if ((long long)slices * batch > 0x7fffffffLL) return fail(CCVPE_EINVAL, "belief_step: batch x slices > 2^31");
  const bool vec2 = (n % 4) == 0 && aligned16(heat) && aligned16(post);
  const dim3 grid2((unsigned)(slices * batch));
  if (vec2)
    hipLaunchKernelGGL(belief_finish_kernel<true>, grid2, dim3(256), 0, st, heat, ori, one_minus_a, floor_m, reset, post, scratch,
                       rows, h, w, (int)ntiles, slices, slice_len);
  else
    hipLaunchKernelGGL(belief_finish_kernel<false>, grid2, dim3(256), 0, st, heat, ori, one_minus_a, floor_m, reset, post, scratch,
                       rows, h, w, (int)ntiles, slices, slice_len);
  return check_launch("belief_finish_kernel");
}
