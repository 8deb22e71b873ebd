// Batch norm's backward, the arithmetic that TWO kernels must do bit for bit alike: hb_apply_kernel (kernels.hip) and the fused
// epilogue of the fp32-emulating dual launch (gemm_bf16.hip: EPI_DACT_BN), which does hb_apply's work inside the dA blocks when
// it is safe to wait for the other row tiles of a block column.  Everything whose rounding or association could differ between
// two translation units is spelled out HERE and nowhere else:
//   * dz of one element -- every rounding named, contraction switched off around them (hipcc's __fmul_rn / __fsub_rn are plain
//     `*` / `-` that -ffp-contract=fast may fuse with a neighbour).  The roundings are the ones hb_apply_kernel compiled to with
//     contraction on before this header existed (gfx950 ISA: v_pk_add (z - mu), v_pk_add (du - m1), v_pk_mul by rstd,
//     v_pk_fma with the negated mean, v_pk_mul by rstd);
//   * the sum over the 8 row lanes of a column tile: lanes 0 .. 7 in order, from 0.f;
//   * the column means from the per-tile partial sums: lane y takes chunks y, y + 8, .. from 0.f, lanes summed as above, then a
//     product with 1.f / T;
//   * the three-plane store of a dz quad.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "x3_layout.h"

namespace tfk {
namespace hb {

constexpr int kLanes = 8;   // row lanes of a column tile (CT_Y of kernels.hip)
constexpr int kQuads = 32;  // float4 columns of a column tile (CT_X)

// dz = rstd * (du - mean(du) - xhat * mean(du * xhat)), xhat = (z - mu) * rstd
__device__ __forceinline__ float dz(float du, float z, float mu, float rsd, float m1, float m2) {
#pragma clang fp contract(off)
  const float xhat = __fmul_rn(rsd, __fsub_rn(z, mu));
  return __fmul_rn(rsd, __fmaf_rn(-m2, xhat, __fsub_rn(du, m1)));
}
__device__ __forceinline__ float4 dz4(float4 du, float4 z, float4 mu, float4 rsd, float4 m1, float4 m2) {
  return make_float4(dz(du.x, z.x, mu.x, rsd.x, m1.x, m2.x), dz(du.y, z.y, mu.y, rsd.y, m1.y, m2.y),
                     dz(du.z, z.z, mu.z, rsd.z, m1.z, m2.z), dz(du.w, z.w, mu.w, rsd.w, m1.w, m2.w));
}
__device__ __forceinline__ void add4(float4& s, float4 v) {
#pragma clang fp contract(off)
  s.x = __fadd_rn(s.x, v.x); s.y = __fadd_rn(s.y, v.y); s.z = __fadd_rn(s.z, v.z); s.w = __fadd_rn(s.w, v.w);
}
__device__ __forceinline__ float4 scale4(float4 v, float f) {
#pragma clang fp contract(off)
  return make_float4(__fmul_rn(v.x, f), __fmul_rn(v.y, f), __fmul_rn(v.z, f), __fmul_rn(v.w, f));
}

// Sum a float4 over the 8 row lanes of column quad x (every thread of the block calls this: two block barriers); the result is
// valid in row lane 0.
__device__ __forceinline__ float4 sum_lanes(float4 v, float4 (*sm)[kQuads], int x, int y) {
  sm[y][x] = v;
  __syncthreads();
  float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
  if (y == 0) {
#pragma unroll
    for (int k = 0; k < kLanes; ++k) add4(t, sm[k][x]);
  }
  __syncthreads();
  return t;
}

// the three planes of a dz quad (x3_layout.h; col a multiple of 4: the four values share a unit), plain or streaming stores
typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));
template <bool STREAM>
__device__ __forceinline__ void store_x3(uint16_t* p, int ld, size_t row, int col, float4 v) {
  uint16_t a[4], b[4], c[4];
  x3::split3(v.x, a[0], b[0], c[0]); x3::split3(v.y, a[1], b[1], c[1]);
  x3::split3(v.z, a[2], b[2], c[2]); x3::split3(v.w, a[3], b[3], c[3]);
  u16x4 q1, q2, q3;
  q1.x = a[0]; q1.y = a[1]; q1.z = a[2]; q1.w = a[3];
  q2.x = b[0]; q2.y = b[1]; q2.z = b[2]; q2.w = b[3];
  q3.x = c[0]; q3.y = c[1]; q3.z = c[2]; q3.w = c[3];
  uint16_t* d = p + x3::at(row, col, ld);
  if constexpr (STREAM) {
    __builtin_nontemporal_store(q1, reinterpret_cast<u16x4*>(d));
    __builtin_nontemporal_store(q2, reinterpret_cast<u16x4*>(d + 64));
    __builtin_nontemporal_store(q3, reinterpret_cast<u16x4*>(d + 128));
  } else {
    *reinterpret_cast<u16x4*>(d) = q1;
    *reinterpret_cast<u16x4*>(d + 64) = q2;
    *reinterpret_cast<u16x4*>(d + 128) = q3;
  }
}

}  // namespace hb
}  // namespace tfk
