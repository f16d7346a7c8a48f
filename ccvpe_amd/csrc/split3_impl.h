// What the three-plane bf16 kernels share (upconv_s3.hip, pw_s3.hip): the split of an fp32 value into hi / mid / lo bf16 planes and
// the per-lane fragment offsets inside a 24-dword [hi 16 | mid 16 | lo 16] LDS row.  The arithmetic convention is described at the
// top of upconv_s3.hip.
#pragma once
#include "conv_common.h"

namespace ccvpe {

__device__ __forceinline__ unsigned pk_bf16(float a, float b) {      // round-to-nearest-even pair (v_cvt_pk_bf16_f32)
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  bf16x2_t v;
  v[0] = (__bf16)a;
  v[1] = (__bf16)b;
  return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ float bf_lo(unsigned p) { return __builtin_bit_cast(float, p << 16); }
__device__ __forceinline__ float bf_hi(unsigned p) { return __builtin_bit_cast(float, p & 0xffff0000u); }

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
// four fp32 values -> their hi / mid / lo bf16 planes (4 bf16 = 8 bytes each)
__device__ __forceinline__ void split3(f32x4 v, u32x2& hi, u32x2& mid, u32x2& lo) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    float a = v[2 * h], b = v[2 * h + 1];
    const unsigned ph = pk_bf16(a, b);
    a -= bf_lo(ph);
    b -= bf_hi(ph);
    const unsigned pm = pk_bf16(a, b);
    a -= bf_lo(pm);
    b -= bf_hi(pm);
    hi[h] = ph;
    mid[h] = pm;
    lo[h] = pk_bf16(a, b);
  }
}

constexpr int S3_ROW = 24;      // dwords per LDS row: [hi 16 | mid 16 | lo 16] bf16

// four channels of one row -> their planes at dword `at` (+ 8, + 16) of that row's piece
__device__ __forceinline__ void store_planes(float* at, f32x4 v) {
  u32x2 hi, mid, lo;
  split3(v, hi, mid, lo);
  *reinterpret_cast<u32x2*>(at) = hi;
  *reinterpret_cast<u32x2*>(at + 8) = mid;
  *reinterpret_cast<u32x2*>(at + 16) = lo;
}

// per-lane dword offsets of the fragments inside a row, by lane group g4 = lane >> 4: one ds_read_b128 each.  Per 16 channels
//   acc += [w_hi |w_hi ] . [x_hi|x_mid]   (w1, a1)
//   acc += [w_mid|w_mid] . [x_hi|x_mid]   (w2, a1)
//   acc += [w_hi |w_lo ] . [x_lo|x_hi ]   (w3, a2)
struct S3Frag {
  int a1, a2, w1, w2, w3;
  __device__ __forceinline__ explicit S3Frag(int g4)
      : a1(4 * g4), a2(g4 < 2 ? 16 + 4 * g4 : 4 * g4 - 8), w1(4 * (g4 & 1)), w2(8 + 4 * (g4 & 1)), w3(g4 < 2 ? 4 * g4 : 4 * g4 + 8) {}
};

}  // namespace ccvpe
