// Input side of the path: what the reference does per image on the host after JPEG decoding —
//   transforms.Resize([h, w]) on a PIL image (= PIL.Image.resize(..., BILINEAR): antialiased, 8-bit fixed point),
//   ToTensor (uint8 HWC -> float CHW / 255), Normalize(mean, std)             train_VIGOR.py:57-70, train_KITTI.py:93-100
//   torch.roll along W by round(rotation * W)                                  datasets.py:112-121
//   FoV crop grd[:, :, :, :int(W * FoV / 360)]                                 train_VIGOR.py:177-178,272-273
// — as two kernels on the decoded uint8 image resident in HBM.
//
// Pillow's resampler (src/libImaging/Resample.c, the algorithm torchvision's Resize delegates to for PIL inputs) is
// reproduced bit for bit: horizontal pass then vertical pass, each output = clip8((2^21 + sum_k px_k * kk_k) >> 22)
// with the per-output windows / integer coefficients precomputed on the host in double precision exactly as
// precompute_coeffs() + normalize_coeffs_8bpc() do (ccvpe_amd/preprocess.py), the intermediate image in uint8.
// HBM-bound byte work: lanes along output columns (coalesced), coefficient rows are wave-uniform or per-lane L1 hits.
#include "common.h"

namespace ccvpe {

constexpr int PRECISION_BITS = 32 - 8 - 2;

__device__ __forceinline__ unsigned char clip8(int v) {
  v >>= PRECISION_BITS;                       // arithmetic shift, as the C code's lookup index
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// horizontal pass: src [H][W][3] u8 -> tmp [H][wo][3] u8
__global__ __launch_bounds__(256) void resample_h_kernel(const unsigned char* __restrict__ src, int H, int W,
                                                         const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                         unsigned char* __restrict__ tmp, int wo) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)H * wo) return;
  const int y = (int)(idx / wo), xx = (int)(idx - (long)y * wo);
  const int xmin = bounds[2 * xx], xn = bounds[2 * xx + 1];
  const int* k = kk + (size_t)xx * ksize;
  int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
  const unsigned char* row = src + ((size_t)y * W + xmin) * 3;
  for (int x = 0; x < xn; ++x) {
    const int c = k[x];
    s0 += row[3 * x] * c;
    s1 += row[3 * x + 1] * c;
    s2 += row[3 * x + 2] * c;
  }
  unsigned char* o = tmp + (size_t)idx * 3;
  o[0] = clip8(s0);
  o[1] = clip8(s1);
  o[2] = clip8(s2);
}

// vertical pass + ToTensor + Normalize + roll + crop: tmp [H][wo][3] u8 -> dst [3][ho][keep] f32
__global__ __launch_bounds__(256) void resample_v_norm_kernel(const unsigned char* __restrict__ tmp, int wo,
                                                              const int* __restrict__ bounds, const int* __restrict__ kk,
                                                              int ksize, float* __restrict__ dst, int ho, int keep, int roll,
                                                              float m0, float m1, float m2, float d0, float d1, float d2) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)ho * keep) return;
  const int yy = (int)(idx / keep), xo = (int)(idx - (long)yy * keep);
  int xs = xo - roll;                          // torch.roll(x, r, W): out[..., j] = in[..., (j - r) mod W]
  xs %= wo;
  if (xs < 0) xs += wo;
  const int ymin = bounds[2 * yy], yn = bounds[2 * yy + 1];
  const int* k = kk + (size_t)yy * ksize;
  int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
  const unsigned char* col = tmp + ((size_t)ymin * wo + xs) * 3;
  for (int y = 0; y < yn; ++y) {
    const int c = k[y];
    const unsigned char* p = col + (size_t)y * wo * 3;
    s0 += p[0] * c;
    s1 += p[1] * c;
    s2 += p[2] * c;
  }
  const size_t plane = (size_t)ho * keep;
  // ToTensor: float(v) / 255 ; Normalize: (t - mean) / std   (IEEE divisions, fp32, same order as torchvision)
  dst[idx] = ((float)clip8(s0) / 255.0f - m0) / d0;
  dst[plane + idx] = ((float)clip8(s1) / 255.0f - m1) / d1;
  dst[2 * plane + idx] = ((float)clip8(s2) / 255.0f - m2) / d2;
}

// vertical pass alone, for the device image cache: tmp [H][wo][3] u8 -> dst [ho][wo][3] u8, full width, no roll.  One lane
// per output BYTE: a row of tmp and a row of dst are both wo * 3 contiguous bytes, so loads and stores coalesce.
__global__ __launch_bounds__(256) void resample_v_u8_kernel(const unsigned char* __restrict__ tmp, int wo,
                                                            const int* __restrict__ bounds, const int* __restrict__ kk,
                                                            int ksize, unsigned char* __restrict__ dst, int ho) {
  const long pitch = (long)wo * 3;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)ho * pitch) return;
  const int yy = (int)(idx / pitch);
  const long xc = idx - (long)yy * pitch;
  const int ymin = bounds[2 * yy], yn = bounds[2 * yy + 1];
  const int* k = kk + (size_t)yy * ksize;
  int s = 1 << (PRECISION_BITS - 1);
  const unsigned char* col = tmp + (size_t)ymin * pitch + xc;
  for (int y = 0; y < yn; ++y) s += col[(size_t)y * pitch] * k[y];
  dst[idx] = clip8(s);
}

// Batch assembly from the device image cache: srcs[b] = device address of a resized [h][w][3] u8 image,
//   dst[b][c][y][x] = ((float)src_b[y][(x - roll_b) mod w][c] / 255 - mean[c]) / std[c],   x < keep
// — the ToTensor / Normalize arithmetic of resample_v_norm_kernel, operation for operation (two IEEE divisions, nothing to
// contract).  Pure streaming: 3 B read, 12 B written per pixel.  blockIdx.y = sample.
// VEC: a lane owns four consecutive output columns of one row (keep % 4 == 0, so a group never straddles rows and every
// plane row is 16-byte aligned) and writes one 16-byte store per channel plane, lanes along x.  The source bytes are read
// per lane, one byte load each: the roll shifts the source by an arbitrary number of 3-byte pixels, so no wider load is
// aligned, and neighbouring lanes read neighbouring 12-byte runs of the same cache lines.  The wrap
// can fall INSIDE a group, so the modulo is taken per element.
template <bool VEC>
__global__ __launch_bounds__(256) void gather_norm_kernel(const long long* __restrict__ srcs, const int* __restrict__ rolls,
                                                          int h, int w, int keep, float* __restrict__ dst, float m0, float m1,
                                                          float m2, float d0, float d1, float d2) {
  constexpr int NX = VEC ? 4 : 1;
  const int per_row = keep / NX;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)h * per_row) return;
  const int b = blockIdx.y;
  const int y = (int)(idx / per_row), x0 = (int)(idx - (long)y * per_row) * NX;
  int r = rolls[b] % w;                        // torch.roll(x, r, W): out[..., j] = in[..., (j - r) mod W]
  if (r < 0) r += w;
  const unsigned char* row = reinterpret_cast<const unsigned char*>(srcs[b]) + (size_t)y * w * 3;
  float v0[NX], v1[NX], v2[NX];
#pragma unroll
  for (int j = 0; j < NX; ++j) {
    int xs = x0 + j - r;                       // x0 + j < keep <= w and 0 <= r < w: -w < xs < w
    if (xs < 0) xs += w;
    const unsigned char* p = row + (size_t)xs * 3;
    v0[j] = ((float)p[0] / 255.0f - m0) / d0;
    v1[j] = ((float)p[1] / 255.0f - m1) / d1;
    v2[j] = ((float)p[2] / 255.0f - m2) / d2;
  }
  const size_t plane = (size_t)h * keep;
  float* o = dst + (size_t)b * 3 * plane + (size_t)y * keep + x0;
  if constexpr (VEC) {
    *reinterpret_cast<cc_f32x4*>(o) = (cc_f32x4){v0[0], v0[1], v0[2], v0[3]};
    *reinterpret_cast<cc_f32x4*>(o + plane) = (cc_f32x4){v1[0], v1[1], v1[2], v1[3]};
    *reinterpret_cast<cc_f32x4*>(o + 2 * plane) = (cc_f32x4){v2[0], v2[1], v2[2], v2[3]};
  } else {
    o[0] = v0[0];
    o[plane] = v1[0];
    o[2 * plane] = v2[0];
  }
}

}  // namespace ccvpe

using namespace ccvpe;

extern "C" int ccvpe_preprocess_u8_f32(const unsigned char* src, int in_h, int in_w, const int* xbounds, const int* xcoef,
                                       int xksize, const int* ybounds, const int* ycoef, int yksize, unsigned char* tmp,
                                       float* dst, int out_h, int out_w, int keep_w, int roll, const float* mean,
                                       const float* stdv, void* stream) {
  if (in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0 || keep_w <= 0 || keep_w > out_w || xksize <= 0 || yksize <= 0)
    return fail(CCVPE_EINVAL, "preprocess: bad shape");
  if (!src || !tmp || !dst || !xbounds || !xcoef || !ybounds || !ycoef || !mean || !stdv) return fail(CCVPE_EINVAL, "preprocess: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const long n1 = (long)in_h * out_w;
  hipLaunchKernelGGL(resample_h_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, st, src, in_h, in_w, xbounds, xcoef, xksize,
                     tmp, out_w);
  const long n2 = (long)out_h * keep_w;
  hipLaunchKernelGGL(resample_v_norm_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, st, tmp, out_w, ybounds, ycoef, yksize,
                     dst, out_h, keep_w, roll, mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2]);
  return check_launch("preprocess");
}

extern "C" int ccvpe_resize_u8(const unsigned char* src, int in_h, int in_w, const int* xbounds, const int* xcoef, int xksize,
                               const int* ybounds, const int* ycoef, int yksize, unsigned char* tmp, unsigned char* dst_u8,
                               int out_h, int out_w, void* stream) {
  if (in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0 || xksize <= 0 || yksize <= 0) return fail(CCVPE_EINVAL, "resize_u8: bad shape");
  if (!src || !tmp || !dst_u8 || !xbounds || !xcoef || !ybounds || !ycoef) return fail(CCVPE_EINVAL, "resize_u8: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const long n1 = (long)in_h * out_w;
  hipLaunchKernelGGL(resample_h_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, st, src, in_h, in_w, xbounds, xcoef, xksize,
                     tmp, out_w);
  const long n2 = (long)out_h * out_w * 3;
  hipLaunchKernelGGL(resample_v_u8_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, st, tmp, out_w, ybounds, ycoef, yksize,
                     dst_u8, out_h);
  return check_launch("resize_u8");
}

extern "C" int ccvpe_gather_norm_u8_f32(const long long* srcs, const int* rolls, int batch, int h, int w, int keep_w,
                                        const float* mean, const float* stdv, float* dst, void* stream) {
  if (batch < 0 || batch > 65535 || h <= 0 || w <= 0 || keep_w <= 0 || keep_w > w) return fail(CCVPE_EINVAL, "gather_norm: bad shape");
  if ((long)h * w * 3 > 0x7fffffffL) return fail(CCVPE_EINVAL, "gather_norm: image above 2 GB");
  if (!mean || !stdv) return fail(CCVPE_EINVAL, "gather_norm: null pointer");
  if (batch == 0) return CCVPE_OK;                       // an empty batch has empty (possibly null) tables and nothing to write
  if (!srcs || !rolls || !dst) return fail(CCVPE_EINVAL, "gather_norm: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (keep_w % 4 == 0 && aligned16(dst)) {
    const long n = (long)h * (keep_w / 4);
    hipLaunchKernelGGL((gather_norm_kernel<true>), dim3((unsigned)((n + 255) / 256), (unsigned)batch), dim3(256), 0, st, srcs, rolls, h, w,
                       keep_w, dst, mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2]);
  } else {
    const long n = (long)h * keep_w;
    hipLaunchKernelGGL((gather_norm_kernel<false>), dim3((unsigned)((n + 255) / 256), (unsigned)batch), dim3(256), 0, st, srcs, rolls, h, w,
                       keep_w, dst, mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2]);
  }
  return check_launch("gather_norm");
}
