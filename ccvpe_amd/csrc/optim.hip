// Device-side optimizer (ccvpe_amd/optim.py, the capturable path): Adam / AdamW with global-norm clipping where every
// per-step number — step counts, bias corrections, the clip coefficient, the skip decision — lives in device memory, so a
// step is two or three launches with no host arithmetic, no upload and no read-back, and captures into a hipGraph.
//
// All kernels run over adam_kernel's table (train_glue.hip): one row (param, grad, exp_avg, exp_avg_sq, numel) per tensor
// and a workgroup -> (tensor, chunk of ADAM_CHUNK elements) map.
//
//   1. grad_sqnorm_kernel   one workgroup per chunk: sum of (grad_scale * g)^2 -> one fp32 partial per chunk
//   2. adam_prepare_kernel  ONE workgroup: partials -> total L2 norm, clip coefficient, finite flag; then, unless the step
//                           is skipped, step[t] += 1 and the derived hyper row of every tensor with a gradient
//   3. adam_update_kernel   adam_kernel's arithmetic with the gradient scaled by grad_scale * clip_coef and weight decay
//
// The step counts move in (2), not in (3): the many chunk workgroups of one tensor then all read a settled row.
// Fixed summation order everywhere (no atomics): two runs on the same gradients give the same bits.
#include <cmath>

#include "common.h"

namespace ccvpe {

constexpr int OPT_CHUNK = 4096;    // = ADAM_CHUNK (train_glue.hip); ccvpe_adam_chunk_elems() is the one the host reads
constexpr int OPT_CONST = 6;       // doubles per tensor: lr, beta1, beta2, eps, weight_decay, decoupled (0 / 1)
constexpr int OPT_HYPER = 10;      // floats per tensor: adam_kernel's first seven, then L2 weight decay, decoupled factor, reserved
constexpr int OPT_SCALARS = 4;     // floats: total_norm, clip_coef, finite (1 / 0), skipped_steps

typedef float f4 __attribute__((ext_vector_type(4)));

// Summation depth of one partial: <= 16 dependent fp32 additions per lane (the scalar path: 4096 / 256 elements on one
// accumulator; the 16-byte path: 4 per accumulator), 2 to merge the four accumulators, 6 butterfly steps, 2 across the waves.
__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const long long* __restrict__ table, const int* __restrict__ chunk_tensor,
                                                          const int* __restrict__ chunk_off, float grad_scale,
                                                          float* __restrict__ partials) {
  __shared__ float sh[4];
  const long long* row = table + (size_t)chunk_tensor[blockIdx.x] * 5;
  const float* g = reinterpret_cast<const float*>(row[1]);
  const long long n = row[4];
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (g != nullptr) {                                     // a tensor without a gradient contributes 0
    const long long base = (long long)chunk_off[blockIdx.x] * OPT_CHUNK;
    const long long end = min(base + OPT_CHUNK, n);
    if (((n | base) & 3) == 0 && ((size_t)g & 15) == 0) {                                             // 16-byte path
      for (long long i = base + 4 * threadIdx.x; i < end; i += 1024) {
        const f4 gi = *reinterpret_cast<const f4*>(g + i) * grad_scale;
        s0 += gi[0] * gi[0];
        s1 += gi[1] * gi[1];
        s2 += gi[2] * gi[2];
        s3 += gi[3] * gi[3];
      }
    } else {
      for (long long i = base + threadIdx.x; i < end; i += 256) {
        const float gi = g[i] * grad_scale;
        s0 += gi * gi;
      }
    }
  }
  float s = wave_sum((s0 + s1) + (s2 + s3));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// beta^k for an integer k >= 1 by repeated squaring in double: a few double roundings, no libm pow (and no scratch)
__device__ __forceinline__ double powi(double b, unsigned k) {
  double r = 1.0;
  while (k) {
    if (k & 1u) r *= b;
    b *= b;
    k >>= 1;
  }
  return r;
}

__global__ __launch_bounds__(256) void adam_prepare_kernel(const long long* __restrict__ table, const double* __restrict__ consts,
                                                           float* __restrict__ steps, float* __restrict__ hyper, int n_tensors,
                                                           const float* __restrict__ partials, int n_partials, float max_norm,
                                                           float* __restrict__ scalars) {
  __shared__ double red[256];
  __shared__ int finite_sh;
  // the partials in double, lane-strided then an LDS tree: fixed order, and no fp32 depth beyond the partials' own
  double a = 0.0;
  for (int k = threadIdx.x; k < n_partials; k += 256) a += (double)partials[k];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float total = (float)sqrt(red[0]);              // n_partials == 0 (no norm pass): 0, finite, coefficient 1
    const bool finite = isfinite(total);
    float coef = 1.0f;
    if (finite && max_norm > 0.f) coef = fminf(1.0f, max_norm / (total + 1e-6f));       // torch.nn.utils.clip_grad_norm_
    scalars[0] = total;
    scalars[1] = coef;
    scalars[2] = finite ? 1.0f : 0.0f;
    if (!finite) scalars[3] += 1.0f;
    finite_sh = finite ? 1 : 0;
  }
  __syncthreads();
  if (!finite_sh) return;                                 // skipped step: counts and rows stay, the update kernel returns early
  for (int t = threadIdx.x; t < n_tensors; t += 256) {
    if (table[(size_t)t * 5 + 1] == 0) continue;
    const float k = steps[t] + 1.0f;
    steps[t] = k;
    const double* c = consts + (size_t)t * OPT_CONST;
    const double lr = c[0], b1 = c[1], b2 = c[2], eps = c[3], wd = c[4];
    const bool decoupled = c[5] != 0.0;
    float* hy = hyper + (size_t)t * OPT_HYPER;
    hy[0] = (float)(lr / (1.0 - powi(b1, (unsigned)k)));
    hy[1] = (float)b1;
    hy[2] = (float)b2;
    hy[3] = (float)(1.0 - b1);
    hy[4] = (float)(1.0 - b2);
    hy[5] = (float)eps;
    hy[6] = (float)sqrt(1.0 - powi(b2, (unsigned)k));
    hy[7] = decoupled ? 0.0f : (float)wd;                 // torch.optim.Adam: g += wd * p
    hy[8] = decoupled ? (float)(1.0 - lr * wd) : 1.0f;    // torch.optim.AdamW: p *= 1 - lr * wd
    hy[9] = 0.0f;
  }
}

__global__ __launch_bounds__(256) void adam_update_kernel(const long long* __restrict__ table /*[n][5]: p, g, m, v, numel*/,
                                                          const float* __restrict__ hyper /*[n][OPT_HYPER]*/,
                                                          const int* __restrict__ chunk_tensor, const int* __restrict__ chunk_off,
                                                          float grad_scale, const float* __restrict__ scalars) {
  const int t = chunk_tensor[blockIdx.x];
  const long long* row = table + (size_t)t * 5;
  float* p = reinterpret_cast<float*>(row[0]);
  const float* g = reinterpret_cast<const float*>(row[1]);
  float* m = reinterpret_cast<float*>(row[2]);
  float* v = reinterpret_cast<float*>(row[3]);
  const long long n = row[4];
  if (g == nullptr || scalars[2] == 0.0f) return;         // no gradient, or a non-finite norm: the whole step is skipped
  const float gs = grad_scale * scalars[1];
  const float* hy = hyper + (size_t)t * OPT_HYPER;
  const float step = hy[0], b1 = hy[1], b2 = hy[2], omb1 = hy[3], omb2 = hy[4], eps = hy[5], bc2_sqrt = hy[6];
  const float l2 = hy[7], decay = hy[8];
  const long long base = (long long)chunk_off[blockIdx.x] * OPT_CHUNK;
  const long long end = min(base + OPT_CHUNK, n);
  if (((n | base) & 3) == 0 && ((((size_t)p | (size_t)g | (size_t)m | (size_t)v) & 15) == 0)) {     // 16-byte path
    for (long long i = base + 4 * threadIdx.x; i < end; i += 1024) {
      f4 gi = *reinterpret_cast<const f4*>(g + i) * gs;
      f4 mi = *reinterpret_cast<const f4*>(m + i), vi = *reinterpret_cast<const f4*>(v + i), pi = *reinterpret_cast<const f4*>(p + i);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (l2 != 0.0f) gi[q] += l2 * pi[q];
        if (decay != 1.0f) pi[q] *= decay;
        mi[q] = b1 * mi[q] + omb1 * gi[q];
        vi[q] = b2 * vi[q] + omb2 * gi[q] * gi[q];
        pi[q] -= step * mi[q] / (sqrtf(vi[q]) / bc2_sqrt + eps);
      }
      *reinterpret_cast<f4*>(m + i) = mi;
      *reinterpret_cast<f4*>(v + i) = vi;
      *reinterpret_cast<f4*>(p + i) = pi;
    }
    return;
  }
  for (long long i = base + threadIdx.x; i < end; i += 256) {
    float gi = g[i] * gs, pi = p[i];
    if (l2 != 0.0f) gi += l2 * pi;
    if (decay != 1.0f) pi *= decay;
    const float mi = b1 * m[i] + omb1 * gi;
    const float vi = b2 * v[i] + omb2 * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] = pi - step * mi / (sqrtf(vi) / bc2_sqrt + eps);
  }
}

}  // namespace ccvpe

using namespace ccvpe;

extern "C" int ccvpe_adam_device_layout(int what) {
  switch (what) {
    case 0: return OPT_HYPER;
    case 1: return OPT_CONST;
    case 2: return OPT_SCALARS;
  }
  return fail(CCVPE_EINVAL, "adam_device_layout: what must be 0 (hyper floats), 1 (const doubles) or 2 (scalar floats)");
}

extern "C" int ccvpe_grad_sqnorm_f32(const void* table, const int* chunk_tensor, const int* chunk_off, int n_chunks,
                                     float grad_scale, float* partials, void* stream) {
  if (n_chunks <= 0 || !table || !chunk_tensor || !chunk_off || !partials) return fail(CCVPE_EINVAL, "grad_sqnorm: bad args");
  if (!std::isfinite(grad_scale)) return fail(CCVPE_EINVAL, "grad_sqnorm: grad_scale not finite");
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(table), chunk_tensor, chunk_off, grad_scale, partials);
  return check_launch("grad_sqnorm_kernel");
}

extern "C" int ccvpe_adam_prepare_f32(const void* table, const double* consts, float* steps, float* hyper, int n_tensors,
                                      const float* partials, int n_partials, float max_norm, float* scalars, void* stream) {
  if (n_tensors <= 0 || !table || !consts || !steps || !hyper || !scalars) return fail(CCVPE_EINVAL, "adam_prepare: bad args");
  if (n_partials < 0 || (n_partials > 0 && !partials)) return fail(CCVPE_EINVAL, "adam_prepare: n_partials without partials");
  if (std::isnan(max_norm)) return fail(CCVPE_EINVAL, "adam_prepare: max_norm is NaN");
  if (max_norm > 0.f && n_partials == 0) return fail(CCVPE_EINVAL, "adam_prepare: clipping needs the norm partials");
  hipLaunchKernelGGL(adam_prepare_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const long long*>(table),
                     consts, steps, hyper, n_tensors, partials, n_partials, max_norm, scalars);
  return check_launch("adam_prepare_kernel");
}

extern "C" int ccvpe_adam_update_f32(const void* table, const float* hyper, const int* chunk_tensor, const int* chunk_off,
                                     int n_chunks, float grad_scale, const float* scalars, void* stream) {
  if (n_chunks <= 0 || !table || !hyper || !chunk_tensor || !chunk_off || !scalars) return fail(CCVPE_EINVAL, "adam_update: bad args");
  if (!std::isfinite(grad_scale)) return fail(CCVPE_EINVAL, "adam_update: grad_scale not finite");
  hipLaunchKernelGGL(adam_update_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(table), hyper, chunk_tensor, chunk_off, grad_scale, scalars);
  return check_launch("adam_update_kernel");
}
