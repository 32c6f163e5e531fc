// What the GEMM family (conv3x3*, patch_embed*, linear) shares on top of the register fragments of mfma_frag.hpp.
// Internal: device code only, not part of the C ABI.
//
// Split-bf16 products: x = hi + lo with hi = the upper 16 bits of x and lo = bf16(x - hi) rounded to nearest, and
// a b ~ hi_a lo_b + lo_a hi_b + hi_a hi_b with v_mfma_f32_32x32x16_bf16 -- ONE order, small terms first, in two operand
// forms: activations first (rows = activation rows: linear, patch_embed NHWC) or weights first (the transposed tile:
// patch_embed NCHW, conv3x3).  The weights are split once into [K / 16 chunks][hi, lo][N padded to 128][16 k] bf16
// (conv3x3: one such group per chunk of 16 input channels and tap), so a lane's operand of a group is 16 contiguous bytes.
// Every packed kernel splits, loads and multiplies through the functions below: they compute the same bits.
//
// fp32 products: the stage of the tile kernels -- one ds_read_b128 per operand row and half-wave feeds four
// v_mfma_f32_32x32x2_f32.
#pragma once

#include "mfma_frag.hpp"
#include "msda_common.hpp"

namespace gemm_core {

using namespace mfma_frag;
using msda::f32x4;

constexpr int kChunk = 16;   // k per v_mfma_f32_32x32x16_bf16 and per group of the packed weights

// hi in the upper half of its word; lo as the fp32 remainder, which (+ kRound) >> 16 rounds to the nearest bf16
constexpr uint32_t kRound = 0x8000u;
__device__ __forceinline__ uint32_t bf16_hi(float x) { return __float_as_uint(x) & 0xffff0000u; }
__device__ __forceinline__ uint32_t bf16_lo(float x, uint32_t hi) { return __float_as_uint(x - __uint_as_float(hi)); }

// 2 P floats -> P words of bf16 hi and P words of bf16 lo, two to a word (V, W: anything indexable -- arrays, vectors)
template <int P, typename V, typename W>
__device__ __forceinline__ void split_pairs(const V& v, W& hi, W& lo) {
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const float fa = v[2 * p], fb = v[2 * p + 1];
    const uint32_t ah = bf16_hi(fa), bh = bf16_hi(fb);
    const uint32_t al = bf16_lo(fa, ah), bl = bf16_lo(fb, bh);
    hi[p] = (ah >> 16) | bh;
    lo[p] = ((al + kRound) >> 16) | ((bl + kRound) & 0xffff0000u);
  }
}

// a lane's weight operands of one packed group for WJ column tiles of 32
template <int WJ>
struct WFrag {
  u32x4v hi[WJ], lo[WJ];
};

// w_lane: the lane's words of group 0, column tile 0; idx: the group (clamped by the caller: a ring runs past the end)
template <int WJ>
__device__ __forceinline__ void load_w(const uint32_t* w_lane, int idx, int64_t idx_stride, int64_t part_stride, WFrag<WJ>& f) {
  const uint32_t* p = w_lane + idx * idx_stride;
#pragma unroll
  for (int jn = 0; jn < WJ; ++jn) {
    f.hi[jn] = *reinterpret_cast<const u32x4v*>(p + jn * 32 * 8);
    f.lo[jn] = *reinterpret_cast<const u32x4v*>(p + part_stride + jn * 32 * 8);
  }
}

// acc += a w over 16 k; W_FIRST: the weights are the first operand (accumulator rows = weight rows)
template <bool W_FIRST>
__device__ __forceinline__ void mfma_split(f32x16& acc, u32x4v a_hi, u32x4v a_lo, u32x4v w_hi, u32x4v w_lo) {
  const bf16x8 ah = __builtin_bit_cast(bf16x8, a_hi), al = __builtin_bit_cast(bf16x8, a_lo);
  const bf16x8 wh = __builtin_bit_cast(bf16x8, w_hi), wl = __builtin_bit_cast(bf16x8, w_lo);
  if constexpr (W_FIRST) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, ah, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, al, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, ah, acc, 0, 0, 0);
  } else {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, wl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, wh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, wh, acc, 0, 0, 0);
  }
}

inline int padded128(int n) { return (n + 127) / 128 * 128; }

// weight [N][K] fp32 -> packed [K / 16 groups][hi, lo][n_pad][16] bf16, rows past N zero.  TAPS = 1: group g is k 16 g ..
// 16 g + 15; TAPS = 9 (conv3x3, k = (channel, tap)): group g is tap g % 9 of channels 16 (g / 9) .. + 15.
template <int TAPS>
__global__ void pack_weight_kernel(const float* __restrict__ w, int N, int K, int n_pad, uint16_t* __restrict__ packed) {
  const int64_t total = (int64_t)(K / kChunk) * n_pad * kChunk;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int kl = (int)(idx % kChunk);
    const int n = (int)((idx / kChunk) % n_pad);
    const int group = (int)(idx / kChunk / n_pad);
    const int k = ((group / TAPS) * kChunk + kl) * TAPS + group % TAPS;
    const float v = n < N ? w[(int64_t)n * K + k] : 0.f;
    const uint32_t hi = bf16_hi(v), lo = bf16_lo(v, hi);
    const int64_t o = ((int64_t)group * 2 * n_pad + n) * kChunk + kl;
    packed[o] = (uint16_t)(hi >> 16);
    packed[o + (int64_t)n_pad * kChunk] = (uint16_t)((lo + kRound) >> 16);
  }
}

// acc[i][j] += sum over four k of a[i] b[j]; B_FIRST: b is the first operand (the transposed tile)
template <bool B_FIRST, int TI, int TJ>
__device__ __forceinline__ void mfma_f32x4(const f32x4 (&a)[TI], const f32x4 (&b)[TJ], f32x16 (&acc)[TI][TJ]) {
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        if constexpr (B_FIRST) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[j][t], a[i][t], acc[i][j], 0, 0, 0);
        else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][t], b[j][t], acc[i][j], 0, 0, 0);
      }
}

// The fp32 stage: rows wr .. of Rs x rows wc .. of Cs over 16 reduction indices, tiles stored [row][PITCH floats].  In each
// 8-deep step lanes 0-31 take k 0..3 and lanes 32-63 k 4..7 (the k order is free as long as both operands agree).
template <bool B_FIRST, int TI, int TJ, int PITCH>
__device__ __forceinline__ void mfma_stage(const float (*Rs)[PITCH], const float (*Cs)[PITCH], int wr, int wc, int r32,
                                           int half, f32x16 (&acc)[TI][TJ]) {
#pragma unroll
  for (int ss = 0; ss < 2; ++ss) {
    f32x4 af[TI], bf[TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i) af[i] = *reinterpret_cast<const f32x4*>(&Rs[wr + i * 32 + r32][ss * 8 + half * 4]);
#pragma unroll
    for (int j = 0; j < TJ; ++j) bf[j] = *reinterpret_cast<const f32x4*>(&Cs[wc + j * 32 + r32][ss * 8 + half * 4]);
    mfma_f32x4<B_FIRST>(af, bf, acc);
  }
}

}  // namespace gemm_core
