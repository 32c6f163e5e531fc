// The row-tile routine of the kernels that run Linear layers over rows of 256 features (query_select.hip, pred_heads.hip).
// Internal: device code only, not part of the C ABI.
//
// A workgroup (4 waves) owns a tile of 32 rows, 256 features each, in LDS.  Y = X W^T with v_mfma_f32_32x32x2_f32: wave w owns
// output features [64 w, 64 w + 64) as two 32 x 32 accumulator tiles (row of the tile in the registers, feature on the lane).
// The weight ([out, in] row-major, as nn.Linear keeps it) is streamed through LDS in chunks of 16 input features; the next chunk
// travels in registers while the current one is multiplied.  Every row sees the same k order (the MFMA's), so a row's result does
// not depend on its place in the tile.  With BOUNDED the weight has n_out <= 256 rows: rows past n_out read as zeros (nothing
// past the weight is touched) and a 32-column group without a live column is not multiplied.
#pragma once

#include "mfma_frag.hpp"
#include "msda_common.hpp"

namespace row_tile {

using namespace mfma_frag;
using msda::f32x4;

constexpr int kThreads = 256;
constexpr int kD = 256;                 // features of a row
constexpr int kRows = 32;               // rows per tile
constexpr int kPitch = kD + 4;          // floats per LDS row of the tile (rows stay 16-byte aligned, b128 reads conflict-free)
constexpr int kKC = 16;                 // input features per streamed weight chunk
constexpr int kWPitch = kKC + 4;
constexpr int kPre = kD * kKC / 4 / kThreads;   // float4 items per thread and chunk
constexpr int kRowsPerWave = kRows / (kThreads / 64);

template <bool BOUNDED>
__device__ __forceinline__ void w_load(f32x4 (&pre)[kPre], const float* __restrict__ W, int n_out, int chunk, int tid) {
#pragma unroll
  for (int r = 0; r < kPre; ++r) {
    const int f = tid + r * kThreads, j = f / (kKC / 4), q = f % (kKC / 4);
    if (BOUNDED && j >= n_out)
      pre[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    else
      pre[r] = *reinterpret_cast<const f32x4*>(W + j * kD + chunk * kKC + q * 4);
  }
}

__device__ __forceinline__ void w_store(float (*Ws)[kWPitch], const f32x4 (&pre)[kPre], int tid) {
#pragma unroll
  for (int r = 0; r < kPre; ++r) {
    const int f = tid + r * kThreads, j = f / (kKC / 4), q = f % (kKC / 4);
    *reinterpret_cast<f32x4*>(&Ws[j][q * 4]) = pre[r];
  }
}

// acc <- Xs W^T, W [n_out, kD] row-major (n_out = kD unless BOUNDED).  Entered with every thread's writes to Xs issued (the first
// barrier below orders them).  Xs is only read; Ws is still being read by other waves on return.
template <bool BOUNDED>
__device__ __forceinline__ void matmul_tile(f32x16 (&acc)[2], float (*Xs)[kPitch], float (*Ws)[kWPitch],
                                            const float* __restrict__ W, int n_out, int tid) {
  const int lane = tid & 63, wv = tid >> 6, r32 = lane & 31, half = lane >> 5;
  zero_acc(acc);
  f32x4 pre[kPre];
  w_load<BOUNDED>(pre, W, n_out, 0, tid);
  for (int c = 0; c < kD / kKC; ++c) {
    __syncthreads();                       // the previous chunk has been multiplied (first round: Xs is complete)
    w_store(Ws, pre, tid);
    __syncthreads();
    if (c + 1 < kD / kKC) w_load<BOUNDED>(pre, W, n_out, c + 1, tid);
#pragma unroll
    for (int ss = 0; ss < kKC / 8; ++ss) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(&Xs[r32][c * kKC + ss * 8 + half * 4]);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        if (BOUNDED && wv * 64 + nt * 32 >= n_out) continue;      // wave-uniform
        const f32x4 bv = *reinterpret_cast<const f32x4*>(&Ws[wv * 64 + nt * 32 + r32][ss * 8 + half * 4]);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], bv[t], acc[nt], 0, 0, 0);
      }
    }
  }
}

// Xs <- act(Xs W^T + bias), W [kD, kD] row-major.  Entered like matmul_tile; left with the new Xs visible to the workgroup.
template <bool RELU>
__device__ __forceinline__ void linear_tile(float (*Xs)[kPitch], float (*Ws)[kWPitch], const float* __restrict__ W,
                                            const float* __restrict__ bias, int tid) {
  const int lane = tid & 63, wv = tid >> 6, r32 = lane & 31, half = lane >> 5;
  f32x16 acc[2];
  matmul_tile<false>(acc, Xs, Ws, W, kD, tid);
  __syncthreads();                         // every wave has read all of Xs
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int col = wv * 64 + nt * 32 + r32;
    const float bj = bias[col];
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const float y = acc[nt][v] + bj;
      Xs[acc_row(v) + 4 * half][col] = RELU ? fmaxf(y, 0.f) : y;
    }
  }
  __syncthreads();
}

__device__ __forceinline__ float dot4(const f32x4 a, const f32x4 b) { return (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]); }

}  // namespace row_tile
