// Register fragments of the 32 x 32 MFMA kernels (the GEMM family -- conv3x3*, patch_embed*, linear, query_select -- and, through
// attn_tile.hpp, the attention cores).  Internal: device code only, not part of the C ABI.
//
// Here: the vector types of an accumulator and of a split-bf16 operand, the accumulator-register -> row map and accumulator
// clearing.  The fp32 -> (bf16 hi, bf16 lo) operand split, the one order of the three split products (small terms first:
// hi lo, lo hi, hi hi) with its two operand forms, the packed weights and the fp32 stage are in gemm_core.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mfma_frag {

typedef float f32x16 __attribute__((__vector_size__(64)));      // a lane's 16 accumulator registers of a 32 x 32 tile
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));      // a lane's operand of v_mfma_f32_32x32x16_bf16
typedef uint32_t u32x4v __attribute__((__vector_size__(16)));   // the same 8 bf16 as four words (LDS / global transfers)

// row of accumulator register v in a 32 x 32 tile: for lane half 0, and for lane half `half` (= lane / 32)
__device__ __forceinline__ constexpr int acc_row(int v) { return 8 * (v / 4) + (v % 4); }
__device__ __forceinline__ constexpr int acc_row(int v, int half) { return 8 * (v / 4) + 4 * half + (v % 4); }

__device__ __forceinline__ void zero_acc(f32x16& acc) {
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
}
// ... of an array of accumulators, of any rank
template <typename T, int N>
__device__ __forceinline__ void zero_acc(T (&acc)[N]) {
#pragma unroll
  for (int n = 0; n < N; ++n) zero_acc(acc[n]);
}

}  // namespace mfma_frag
