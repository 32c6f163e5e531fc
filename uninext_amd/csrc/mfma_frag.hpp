// Register fragments of the 32 x 32 MFMA kernels (the GEMM family -- conv3x3*, patch_embed*, linear, query_select -- and, through
// attn_tile.hpp, the attention cores).  Internal: device code only, not part of the C ABI.
//
// Here: the vector types of an accumulator and of a split-bf16 operand, the accumulator-register -> row map, accumulator
// clearing, and the fp32 -> (bf16 hi, bf16 lo) operand split.  The order in which a kernel issues its three split products
// differs from kernel to kernel and stays in the kernels.
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

// 8 floats -> 8 bf16 hi (the upper 16 bits) and 8 bf16 lo (the remainder, rounded to nearest), two to a word
__device__ __forceinline__ void split8(const float (&v)[8], u32x4v& hi, u32x4v& lo) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const uint32_t a = __float_as_uint(v[2 * p]), b = __float_as_uint(v[2 * p + 1]);
    const uint32_t ah = a & 0xffff0000u, bh = b & 0xffff0000u;
    const uint32_t al = __float_as_uint(v[2 * p] - __uint_as_float(ah));
    const uint32_t bl = __float_as_uint(v[2 * p + 1] - __uint_as_float(bh));
    hi[p] = (ah >> 16) | bh;
    lo[p] = ((al + 0x8000u) >> 16) | ((bl + 0x8000u) & 0xffff0000u);   // lo rounded to nearest
  }
}

}  // namespace mfma_frag
