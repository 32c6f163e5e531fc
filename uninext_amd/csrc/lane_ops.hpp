// Lane-level primitives of the MSDeformAttn kernels (and linear.hip's LayerNorm epilogue): DPP moves, lane-group butterflies,
// the LDS integer add and the fixed-point conversions around it.  Internal, device only.
// A namespace of its own, not pulled into msda_common.hpp: the sources under experiments/ define a qb, a wave_max ... of theirs in
// namespace msda.  A translation unit that needs these includes this header and qualifies its calls or names them with `using`.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lane_ops {

typedef float v2f __attribute__((ext_vector_type(2)));        // packed fp32 math: v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32

// the value of the lane that the DPP control CTRL names (all rows and banks, 0 where the control has no source lane)
template <int CTRL>
__device__ __forceinline__ int dppi(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
template <int CTRL>
__device__ __forceinline__ float dpp(float v) { return __int_as_float(dppi<CTRL>(__float_as_int(v))); }

// value held by lane SRC of this lane's quad
template <int SRC>
__device__ __forceinline__ uint32_t quad_bcast(uint32_t v) { return (uint32_t)dppi<SRC * 0x55>((int)v); }
template <int SRC>
__device__ __forceinline__ float quad_bcast(float v) { return __uint_as_float(quad_bcast<SRC>(__float_as_uint(v))); }

// Sum over the G lanes of a lane-group (G = 2 .. 64, aligned groups); every lane ends up with the total.
template <int G>
__device__ __forceinline__ float group_sum(float v) {
  if constexpr (G >= 2) v += dpp<0xB1>(v);    // quad_perm [1,0,3,2]
  if constexpr (G >= 4) v += dpp<0x4E>(v);    // quad_perm [2,3,0,1]
  if constexpr (G >= 8) v += dpp<0x141>(v);   // row_half_mirror: lane i <- 7-i within 8
  if constexpr (G >= 16) v += dpp<0x140>(v);  // row_mirror: lane i <- 15-i within 16
  if constexpr (G >= 32) v += __shfl_xor(v, 16, 64);
  if constexpr (G >= 64) v += __shfl_xor(v, 32, 64);
  return v;
}
// The same steps with fmaxf.
template <int G>
__device__ __forceinline__ float group_max(float v) {
  if constexpr (G >= 2) v = fmaxf(v, dpp<0xB1>(v));
  if constexpr (G >= 4) v = fmaxf(v, dpp<0x4E>(v));
  if constexpr (G >= 8) v = fmaxf(v, dpp<0x141>(v));
  if constexpr (G >= 16) v = fmaxf(v, dpp<0x140>(v));
  if constexpr (G >= 32) v = fmaxf(v, __shfl_xor(v, 16, 64));
  if constexpr (G >= 64) v = fmaxf(v, __shfl_xor(v, 32, 64));
  return v;
}

typedef int __attribute__((address_space(3)))* lds_int_ptr;
__device__ __forceinline__ void lds_add(uint32_t lds_byte_addr, int v) {   // ds_add_u32, no return value
  __hip_atomic_fetch_add(reinterpret_cast<lds_int_ptr>((uintptr_t)lds_byte_addr), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ int cvt_rn_i32(float x) {   // floor(x + 0.5): one VALU instruction
  int r;
  asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(r) : "v"(x));
  return r;
}
__device__ __forceinline__ float abs_or_inf(float x) {  // |x|, +inf for NaN / Inf (so that a max() sees it)
  const float a = fabsf(x);
  return (a <= 3.402823466e+38f) ? a : __builtin_inff();
}
__device__ __forceinline__ uint32_t mad_u24(uint32_t a, uint32_t b, uint32_t c) {   // (a & 0xffffff) * (b & 0xffffff) + c
  uint32_t r;
  asm volatile("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));   // volatile: stays out of branches
  return r;
}

}  // namespace lane_ops
