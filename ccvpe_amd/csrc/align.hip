// KITTI aerial alignment on the device (the reference: datasets.py:443-464 training, :577-596 test).
// Per sample the reference runs four Pillow passes over the WHOLE aerial map and keeps the centre 512 x 512:
//   sat.rotate(-heading)                                   NEAREST   pass 1
//   sat.transform(size, AFFINE, (1,0,tx1, 0,1,ty1))        BILINEAR  pass 2   (GPS antenna -> camera)
//   sat.transform(size, AFFINE, (1,0,tx2, 0,1,ty2))        BILINEAR  pass 3   (the sample's shift)
//   sat.rotate(ori)                                        NEAREST   pass 4,  then center_crop
// Here every pixel of the crop is evaluated lazily, one launch per batch, and the intermediate images never exist:
//   pass 4's 16.16 fixed-point walk names ONE pixel of pass 3 (or 0 outside), that pixel is the float64 bilinear of up to
//   four pass-2 pixels, each of those the bilinear of up to four pass-1 pixels, each of those one fixed-point NEAREST fetch
//   from the source: sixteen fetches (nine distinct; the repeats hit L1).  Every pass applies its own inside and clip
//   rules at its own coordinates and truncates to uint8, exactly as Pillow 12.2 does (Geometry.c: affine_fixed,
//   affine_transform, bilinear_filter32RGB).  ccvpe_amd/align.py restates the same chain in numpy (align_reference) and
//   computes the per-sample parameter row on the host; the result equals Pillow's bit for bit (tests/test_kitti_align*.py).
// Two kernels share that chain (align_pixel): kitti_align_kernel writes the uint8 crop from a packed upload, and
// kitti_align_norm_kernel reads each map through a table of device addresses (the device image cache's raw slots,
// ccvpe_amd/cache.py) and writes the normalised fp32 NCHW batch side itself (tests/test_kitti_map_cache*.py).
//
// Pillow's x86-64 build rounds the product and the sum of  a + (b - a) * d  separately and the truncation makes one ulp
// visible, so nothing in this file may be contracted into a fused multiply-add:
#pragma clang fp contract(off)
#include "common.h"

namespace ccvpe {

constexpr int ALIGN_ROW = 20;        // int64 per sample: pass-1 a0..a5, pass-4 a0..a5, tx1 ty1 tx2 ty2 (double bits), w h left top
constexpr int ALIGN_MAX_SIDE = 32767;   // Pillow's fixed-point walk is only taken below 32768

struct AlignSample {
  const unsigned char* src;
  const long long* row;
  int w, h;
};

struct AlignAxis {          // one axis of a bilinear tap pair: Pillow's BILINEAR_HEAD for a pure translation
  bool inside;
  int i0, i1;
  double d;
};

__device__ __forceinline__ AlignAxis align_axis(int x, double t, int n) {
  AlignAxis r;
  double v = ((double)x + 0.5) + t;
  r.inside = !(v < 0.0 || v >= (double)n);
  v -= 0.5;
  const double f = floor(v);
  r.d = v - f;
  const int i = (int)fmin(fmax(f, -1.0), (double)n);        // inside: -1 <= f <= n - 1; the clamp keeps any input in range
  r.i0 = min(max(i, 0), n - 1);
  r.i1 = min(max(i + 1, 0), n - 1);
  return r;
}

// pass 1: one fixed-point NEAREST fetch from the source
__device__ __forceinline__ void align_p1(const AlignSample& s, int x, int y, double o[3]) {
  const long long* a = s.row;
  const long long u = (a[2] + a[0] * x + a[1] * y) >> 16;
  const long long v = (a[5] + a[3] * x + a[4] * y) >> 16;
  if (u < 0 || u >= s.w || v < 0 || v >= s.h) {
    o[0] = o[1] = o[2] = 0.0;
    return;
  }
  const unsigned char* p = s.src + ((size_t)v * s.w + (size_t)u) * 3;
  o[0] = (double)p[0];
  o[1] = (double)p[1];
  o[2] = (double)p[2];
}

// bilinear_filter32RGB on one pixel: v = a + (b - a) * d three times, the byte truncated
template <typename Fetch>
__device__ __forceinline__ void align_bilinear(const AlignSample& s, int x, int y, double tx, double ty, Fetch fetch, double o[3]) {
  const AlignAxis ax = align_axis(x, tx, s.w), ay = align_axis(y, ty, s.h);
  if (!(ax.inside && ay.inside)) {
    o[0] = o[1] = o[2] = 0.0;
    return;
  }
  double p00[3], p01[3], p10[3], p11[3];
  fetch(ax.i0, ay.i0, p00);
  fetch(ax.i1, ay.i0, p01);
  fetch(ax.i0, ay.i1, p10);
  fetch(ax.i1, ay.i1, p11);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double v1 = p00[c] + (p01[c] - p00[c]) * ax.d;
    const double v2 = p10[c] + (p11[c] - p10[c]) * ax.d;
    const double v = v1 + (v2 - v1) * ay.d;
    o[c] = (double)(int)v;                                  // (UINT8)v: 0 <= v <= 255
  }
}

// One pixel of the crop, shared by both kernels: pass 4's fixed-point walk at (X, Y) of the window names one pixel of
// pass 3 (0 outside), which the lazy chain evaluates.  px = the three bytes Pillow writes there, as exact doubles.
__device__ __forceinline__ void align_pixel(const AlignSample& s, int X, int Y, double px[3]) {
  const long long* row = s.row;
  const double tx1 = __longlong_as_double(row[12]), ty1 = __longlong_as_double(row[13]);
  const double tx2 = __longlong_as_double(row[14]), ty2 = __longlong_as_double(row[15]);
  // pass 4: the fixed-point walk at the crop pixel's position in the whole image
  const long long x = row[18] + X, y = row[19] + Y;
  const long long u = (row[8] + row[6] * x + row[7] * y) >> 16;
  const long long v = (row[11] + row[9] * x + row[10] * y) >> 16;
  px[0] = px[1] = px[2] = 0.0;
  if (x >= 0 && x < s.w && y >= 0 && y < s.h && u >= 0 && u < s.w && v >= 0 && v < s.h) {   // (a crop past the image is 0, as PIL's crop)
    auto p1 = [&](int xx, int yy, double* q) { align_p1(s, xx, yy, q); };
    auto p2 = [&](int xx, int yy, double* q) { align_bilinear(s, xx, yy, tx1, ty1, p1, q); };
    align_bilinear(s, (int)u, (int)v, tx2, ty2, p2, px);
  }
}

// lanes along the crop's columns, 32 x 8 pixels per workgroup, one sample per blockIdx.z
__global__ __launch_bounds__(256) void kitti_align_kernel(const unsigned char* __restrict__ src, long src_bytes,
                                                          const long long* __restrict__ offsets,
                                                          const long long* __restrict__ rows, unsigned char* __restrict__ dst,
                                                          int crop_h, int crop_w) {
  const int b = blockIdx.z;
  const int X = blockIdx.x * 32 + (threadIdx.x & 31), Y = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (X >= crop_w || Y >= crop_h) return;
  const long long* row = rows + (size_t)b * ALIGN_ROW;
  unsigned char* o = dst + (((size_t)b * crop_h + Y) * crop_w + X) * 3;
  const long long w = row[16], h = row[17], off = offsets[b];
  // a sample that does not lie inside the packed buffer is written as zeros and never read
  if (w <= 0 || w > ALIGN_MAX_SIDE || h <= 0 || h > ALIGN_MAX_SIDE || off < 0 || off > (long long)src_bytes ||
      w * h * 3 > (long long)src_bytes - off) {
    o[0] = o[1] = o[2] = 0;
    return;
  }
  AlignSample s;
  s.src = src + off;
  s.row = row;
  s.w = (int)w;
  s.h = (int)h;
  double px[3];
  align_pixel(s, X, Y, px);
  o[0] = (unsigned char)(int)px[0];
  o[1] = (unsigned char)(int)px[1];
  o[2] = (unsigned char)(int)px[2];
}

// The same crop, straight into the model's input: srcs[b] = device address of sample b's decoded [h][w][3] map (a pointer
// table as in gather_norm_kernel: cache slots, a staged upload, repeats), and the byte of every pixel goes through the
// ToTensor / Normalize arithmetic of gather_norm_kernel, operation for operation (two IEEE fp32 divisions), into
// dst [batch][3][crop_h][crop_w] fp32.  The uint8 crop never exists.  Same tiling: lanes along the crop's columns, so each
// channel plane's store is one contiguous 128-byte run per wavefront row.  A row with address 0, or with w / h outside
// 1..ALIGN_MAX_SIDE, is the all-zero crop (the normalised zero byte per channel) and nothing is dereferenced.
__global__ __launch_bounds__(256) void kitti_align_norm_kernel(const long long* __restrict__ srcs,
                                                               const long long* __restrict__ rows, float* __restrict__ dst,
                                                               int crop_h, int crop_w, float m0, float m1, float m2, float d0,
                                                               float d1, float d2) {
  const int b = blockIdx.z;
  const int X = blockIdx.x * 32 + (threadIdx.x & 31), Y = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (X >= crop_w || Y >= crop_h) return;
  const long long* row = rows + (size_t)b * ALIGN_ROW;
  const long long w = row[16], h = row[17], addr = srcs[b];
  double px[3] = {0.0, 0.0, 0.0};
  if (addr != 0 && w > 0 && w <= ALIGN_MAX_SIDE && h > 0 && h <= ALIGN_MAX_SIDE) {
    AlignSample s;
    s.src = reinterpret_cast<const unsigned char*>(addr);
    s.row = row;
    s.w = (int)w;
    s.h = (int)h;
    align_pixel(s, X, Y, px);
  }
  const size_t plane = (size_t)crop_h * crop_w;
  float* o = dst + (size_t)b * 3 * plane + (size_t)Y * crop_w + X;
  o[0] = ((float)(int)px[0] / 255.0f - m0) / d0;
  o[plane] = ((float)(int)px[1] / 255.0f - m1) / d1;
  o[2 * plane] = ((float)(int)px[2] / 255.0f - m2) / d2;
}

}  // namespace ccvpe

using namespace ccvpe;

extern "C" int ccvpe_kitti_align_u8(const unsigned char* src, long src_bytes, const long long* offsets, const long long* rows,
                                    int batch, unsigned char* dst, int crop_h, int crop_w, void* stream) {
  if (batch <= 0 || batch > 65535 || crop_h <= 0 || crop_w <= 0 || crop_h > ALIGN_MAX_SIDE || crop_w > ALIGN_MAX_SIDE ||
      src_bytes <= 0)
    return fail(CCVPE_EINVAL, "kitti_align: bad shape");
  if (!src || !offsets || !rows || !dst) return fail(CCVPE_EINVAL, "kitti_align: null pointer");
  hipLaunchKernelGGL(kitti_align_kernel, dim3((unsigned)((crop_w + 31) / 32), (unsigned)((crop_h + 7) / 8), (unsigned)batch),
                     dim3(256), 0, (hipStream_t)stream, src, src_bytes, offsets, rows, dst, crop_h, crop_w);
  return check_launch("kitti_align");
}

extern "C" int ccvpe_kitti_align_norm_u8_f32(const long long* srcs, const long long* rows, int batch, const float* mean,
                                             const float* stdv, float* dst, int crop_h, int crop_w, void* stream) {
  if (batch < 0 || batch > 65535 || crop_h <= 0 || crop_w <= 0 || crop_h > ALIGN_MAX_SIDE || crop_w > ALIGN_MAX_SIDE)
    return fail(CCVPE_EINVAL, "kitti_align_norm: bad shape");
  if (!mean || !stdv) return fail(CCVPE_EINVAL, "kitti_align_norm: null pointer");
  if (batch == 0) return CCVPE_OK;                       // an empty batch has empty (possibly null) tables and nothing to write
  if (!srcs || !rows || !dst) return fail(CCVPE_EINVAL, "kitti_align_norm: null pointer");
  hipLaunchKernelGGL(kitti_align_norm_kernel, dim3((unsigned)((crop_w + 31) / 32), (unsigned)((crop_h + 7) / 8), (unsigned)batch),
                     dim3(256), 0, (hipStream_t)stream, srcs, rows, dst, crop_h, crop_w, mean[0], mean[1], mean[2], stdv[0],
                     stdv[1], stdv[2]);
  return check_launch("kitti_align_norm");
}
