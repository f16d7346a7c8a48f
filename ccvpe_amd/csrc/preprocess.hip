// Input side of the path: what the reference does per image on the host after JPEG decoding —
//   transforms.Resize([h, w]) on a PIL image (= PIL.Image.resize(..., BILINEAR): antialiased, 8-bit fixed point),
//   ToTensor (uint8 HWC -> float CHW / 255), Normalize(mean, std)             train_VIGOR.py:57-70, train_KITTI.py:93-100
//   torch.roll along W by round(rotation * W)                                  datasets.py:112-121
//   FoV crop grd[:, :, :, :int(W * FoV / 360)]                                 train_VIGOR.py:177-178,272-273
// — as two kernels on the decoded uint8 image resident in HBM; for the device image cache the resize alone, kept as bytes, and one
// gather launch per batch side; for the Oxford RobotCar aerial side (datasets.py:296-330: an 800 x 800 patch of ONE large map per
// sample) the crop and both passes of a whole batch in one kernel on the map resident in HBM (window_resize_norm_kernel).
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

// Device-resident aerial map (Oxford RobotCar): crop + Pillow-exact resize + ToTensor + Normalize of a whole batch side in ONE
// launch.  map [map_h][map_w][3] u8 stays in HBM; origins [batch][2] = (x0, y0) of each sample's window, any sign:
//   W_b[i][j] = map[y0 + i][x0 + j] inside the map, else 0 (PIL.Image.crop of an RGB image), never materialised;
//   dst[b] = resample_v_norm_kernel(resample_h_kernel(W_b)), bit for bit, neither intermediate in HBM.
// A workgroup owns one WIN_TY x WIN_TX output tile of one sample (blockIdx = tile x, tile y, sample).  Phase 1: the horizontal
// pass for the window rows [lo, hi) the tile's vertical taps reach, straight from the map into LDS as clipped bytes — lanes
// along the output columns, so neighbouring lanes read neighbouring map bytes, four taps per three dword loads (win_mac4); a tap
// outside the map contributes 0 and is not read (border tiles take a per-tap checked byte path); every byte offset into the map
// is 64-bit.  Phase 2: the vertical pass out of LDS.  VEC (out_w % 4 == 0): a lane owns
// four consecutive columns = 12 staged bytes per tap row, 4-byte aligned (the LDS pitch and 4 pixels are both multiples of
// 12 B), read as three dwords at a lane stride of 3 dwords (conflict-free), and writes one 16-byte store per channel plane.
// Nothing the tables hold can take an access out of bounds: counts are clamped to ksize, staged rows to `cap_rows` (what
// the launcher sized the LDS for), map reads are range-checked whenever the tap run is not wholly inside.
constexpr int WIN_TX = 128, WIN_TY = 16, WIN_PITCH = WIN_TX * 3;

// four taps of the horizontal pass: 12 map bytes at ANY byte address (a pixel is 3 bytes) as three dword loads — global memory
// takes unaligned dwords — into the three channel sums.  R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3.
__device__ __forceinline__ void win_mac4(const unsigned char* __restrict__ p, const int (&c)[4], int& s0, int& s1, int& s2) {
  unsigned w[3];
  __builtin_memcpy(w, p, 12);
  s0 += (int)(w[0] & 255u) * c[0] + (int)(w[0] >> 24) * c[1] + (int)((w[1] >> 16) & 255u) * c[2] + (int)((w[2] >> 8) & 255u) * c[3];
  s1 += (int)((w[0] >> 8) & 255u) * c[0] + (int)(w[1] & 255u) * c[1] + (int)(w[1] >> 24) * c[2] + (int)((w[2] >> 16) & 255u) * c[3];
  s2 += (int)((w[0] >> 16) & 255u) * c[0] + (int)((w[1] >> 8) & 255u) * c[1] + (int)(w[2] & 255u) * c[2] + (int)(w[2] >> 24) * c[3];
}

template <bool VEC>
__global__ __launch_bounds__(256) void window_resize_norm_kernel(
    const unsigned char* __restrict__ map, int map_h, int map_w, const int* __restrict__ origins, const int* __restrict__ xbounds,
    const int* __restrict__ xk, int xksize, const int* __restrict__ ybounds, const int* __restrict__ yk, int yksize, int cap_rows,
    float* __restrict__ dst, int ho, int wo, float m0, float m1, float m2, float d0, float d1, float d2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char win_sm[];   // [cap_rows][WIN_TX][3] u8
  const int b = blockIdx.z;
  const int tx0 = blockIdx.x * WIN_TX, ty0 = blockIdx.y * WIN_TY;
  const int tw = min(WIN_TX, wo - tx0), th = min(WIN_TY, ho - ty0);
  const long ox = origins[2 * b], oy = origins[2 * b + 1];
  // window rows the tile's vertical taps reach (workgroup-uniform): Pillow's windows move monotonically with the output row,
  // so the first row's start and the last row's end bound them all (phase 2 skips any tap another table would put outside)
  const long lo = ybounds[2 * ty0];
  const long hi = (long)ybounds[2 * (ty0 + th - 1)] + min(max(ybounds[2 * (ty0 + th - 1) + 1], 0), yksize);
  const int nrows = (int)min(hi - lo, (long)cap_rows);

  // phase 1: horizontal pass of rows lo .. lo + nrows into LDS
  {
    const int tx = threadIdx.x & (WIN_TX - 1);
    if (tx < tw) {
      const int xx = tx0 + tx;
      const int xn = min(max(xbounds[2 * xx + 1], 0), xksize);
      const long sx = ox + xbounds[2 * xx];
      const int* k = xk + (size_t)xx * xksize;
      // taps go four pixels = 12 bytes = three dword loads at a time (a count that is no multiple of 4 is padded with zero
      // coefficients; the first group is read even for an empty window): the fast path needs the padded run inside the ROW,
      // so no load leaves the map
      const bool x_inside = sx >= 0 && sx + max((xn + 3) & ~3, 4) <= map_w;
      int c0[4];                                             // the first four coefficients do not depend on the row
#pragma unroll
      for (int j = 0; j < 4; ++j) c0[j] = j < xn ? k[j] : 0;
      const int r_first = threadIdx.x / WIN_TX;
      if (x_inside && xn <= 4 && oy + lo >= 0 && oy + lo + nrows <= map_h) {
        // interior tile, one tap group (enlargements, and reductions whose windows span at most four pixels: 800 -> 512 is
        // one): no test per row, so the loop unrolls and a lane keeps four rows' loads in flight (eight took 108 VGPRs and ran slower)
        const unsigned char* p = map + ((size_t)(oy + lo) * (size_t)map_w + (size_t)sx) * 3;
        const size_t pitch = (size_t)map_w * 3;
#pragma unroll 4
        for (int r = r_first; r < nrows; r += 256 / WIN_TX) {
          int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
          win_mac4(p + (size_t)r * pitch, c0, s0, s1, s2);
          unsigned char* o = win_sm + r * WIN_PITCH + tx * 3;
          o[0] = clip8(s0);
          o[1] = clip8(s1);
          o[2] = clip8(s2);
        }
      } else for (int r = r_first; r < nrows; r += 256 / WIN_TX) {
        int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
        const long sy = oy + lo + r;
        if (sy >= 0 && sy < map_h) {
          const unsigned char* row = map + (size_t)sy * (size_t)map_w * 3;
          if (x_inside) {
            const unsigned char* p = row + (size_t)sx * 3;
            win_mac4(p, c0, s0, s1, s2);
            for (int x = 4; x < xn; x += 4) {
              int c[4];
#pragma unroll
              for (int j = 0; j < 4; ++j) c[j] = x + j < xn ? k[x + j] : 0;
              win_mac4(p + 3 * x, c, s0, s1, s2);
            }
          } else {
            for (int x = 0; x < xn; ++x) {
              const long gx = sx + x;
              if (gx < 0 || gx >= map_w) continue;
              const unsigned char* p = row + (size_t)gx * 3;
              const int c = k[x];
              s0 += p[0] * c;
              s1 += p[1] * c;
              s2 += p[2] * c;
            }
          }
        }
        unsigned char* o = win_sm + r * WIN_PITCH + tx * 3;
        o[0] = clip8(s0);
        o[1] = clip8(s1);
        o[2] = clip8(s2);
      }
    }
  }
  __syncthreads();

  // phase 2: vertical pass out of LDS + ToTensor + Normalize
  constexpr int NX = VEC ? 4 : 1;
  constexpr int PER_ROW = WIN_TX / NX;
  const int x = (threadIdx.x % PER_ROW) * NX;
  if (x >= tw) return;
  const size_t plane = (size_t)ho * wo;
  for (int t = threadIdx.x / PER_ROW; t < th; t += 256 / PER_ROW) {
    const int yy = ty0 + t;
    const long r0 = (long)ybounds[2 * yy] - lo;
    const int yn = min(max(ybounds[2 * yy + 1], 0), yksize);
    const int* k = yk + (size_t)yy * yksize;
    int s0[NX], s1[NX], s2[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) s0[j] = s1[j] = s2[j] = 1 << (PRECISION_BITS - 1);
    for (int y = 0; y < yn; ++y) {
      const long r = r0 + y;
      if (r < 0 || r >= nrows) continue;                     // only with tables the launcher's LDS bound does not cover
      const int c = k[y];
      const unsigned char* p = win_sm + (int)r * WIN_PITCH + x * 3;
      if constexpr (VEC) {
        const unsigned* q = reinterpret_cast<const unsigned*>(p);
        const unsigned w0 = q[0], w1 = q[1], w2 = q[2];      // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
        s0[0] += (int)(w0 & 255u) * c;
        s1[0] += (int)((w0 >> 8) & 255u) * c;
        s2[0] += (int)((w0 >> 16) & 255u) * c;
        s0[1] += (int)(w0 >> 24) * c;
        s1[1] += (int)(w1 & 255u) * c;
        s2[1] += (int)((w1 >> 8) & 255u) * c;
        s0[2] += (int)((w1 >> 16) & 255u) * c;
        s1[2] += (int)(w1 >> 24) * c;
        s2[2] += (int)(w2 & 255u) * c;
        s0[3] += (int)((w2 >> 8) & 255u) * c;
        s1[3] += (int)((w2 >> 16) & 255u) * c;
        s2[3] += (int)(w2 >> 24) * c;
      } else {
        s0[0] += p[0] * c;
        s1[0] += p[1] * c;
        s2[0] += p[2] * c;
      }
    }
    float v0[NX], v1[NX], v2[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      // ToTensor: float(v) / 255 ; Normalize: (t - mean) / std   (IEEE divisions, as resample_v_norm_kernel)
      v0[j] = ((float)clip8(s0[j]) / 255.0f - m0) / d0;
      v1[j] = ((float)clip8(s1[j]) / 255.0f - m1) / d1;
      v2[j] = ((float)clip8(s2[j]) / 255.0f - m2) / d2;
    }
    float* o = dst + (size_t)b * 3 * plane + (size_t)yy * wo + tx0 + x;
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
}

// ksize of Pillow's BILINEAR tables for in -> out (ccvpe_amd/preprocess.py resample_tables)
static int pillow_ksize(int in_size, int out_size) {
  const double scale = (double)in_size / out_size;
  return (int)ceil(scale < 1.0 ? 1.0 : scale) * 2 + 1;
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

extern "C" int ccvpe_window_resize_norm_u8_f32(const unsigned char* map, int map_h, int map_w, const int* origins, int batch,
                                               int box_h, int box_w, const int* xbounds, const int* xcoef, int xksize,
                                               const int* ybounds, const int* ycoef, int yksize, const float* mean,
                                               const float* stdv, float* dst, int out_h, int out_w, void* stream) {
  if (batch < 0 || batch > 65535 || map_h <= 0 || map_w <= 0 || box_h <= 0 || box_w <= 0 || out_h <= 0 || out_w <= 0)
    return fail(CCVPE_EINVAL, "window_resize_norm: bad shape");
  if (!mean || !stdv) return fail(CCVPE_EINVAL, "window_resize_norm: null pointer");
  if (batch == 0) return CCVPE_OK;                       // an empty batch has empty (possibly null) tables and nothing to write
  if (!map || !origins || !xbounds || !xcoef || !ybounds || !ycoef || !dst) return fail(CCVPE_EINVAL, "window_resize_norm: null pointer");
  if (xksize != pillow_ksize(box_w, out_w) || yksize != pillow_ksize(box_h, out_h))
    return fail(CCVPE_EINVAL, "window_resize_norm: ksize %d / %d is not Pillow's for %dx%d -> %dx%d", xksize, yksize, box_h, box_w,
                out_h, out_w);
  // window rows one tile's vertical taps can reach: hi - lo < (WIN_TY - 1) * scale + 2 * support + 1 <= (WIN_TY - 1) * scale + ksize
  const long cap_rows = (long)(WIN_TY - 1) * box_h / out_h + yksize + 1;
  if (cap_rows * WIN_PITCH > 65536)
    return fail(CCVPE_EINVAL, "window_resize_norm: unsupported geometry: %d -> %d rows stages %ld rows of %d bytes, above 64 KB of LDS",
                box_h, out_h, cap_rows, WIN_PITCH);
  const long gy = ((long)out_h + WIN_TY - 1) / WIN_TY;
  if (gy > 65535) return fail(CCVPE_EINVAL, "window_resize_norm: bad shape (out_h above %d)", 65535 * WIN_TY);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((out_w + WIN_TX - 1) / WIN_TX), (unsigned)gy, (unsigned)batch);
  const unsigned lds = (unsigned)(cap_rows * WIN_PITCH);
  if (out_w % 4 == 0 && aligned16(dst)) {
    hipLaunchKernelGGL((window_resize_norm_kernel<true>), grid, dim3(256), lds, st, map, map_h, map_w, origins, xbounds, xcoef, xksize,
                       ybounds, ycoef, yksize, (int)cap_rows, dst, out_h, out_w, mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2]);
  } else {
    hipLaunchKernelGGL((window_resize_norm_kernel<false>), grid, dim3(256), lds, st, map, map_h, map_w, origins, xbounds, xcoef, xksize,
                       ybounds, ycoef, yksize, (int)cap_rows, dst, out_h, out_w, mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2]);
  }
  return check_launch("window_resize_norm");
}
