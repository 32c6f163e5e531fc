// The streamed-attention tile scheme of the fused attention cores (biattn.hip, vit_attn.hip, dec_attn.hip).  Internal: device
// code only, not part of the C ABI.
//
// A wave OWNS 32 tokens of one side, whose operand rows (D floats each, scaled first) stay in its registers, and the tokens of
// the other side are STREAMED through LDS in tiles of 32 rows.  v_mfma_f32_32x32x2_f32 takes the streamed rows as A and the
// owned rows as B, so a score tile has the owned token on the lane (column l % 32) and the streamed tokens in the 16 registers:
// register v of lane l holds row 8 (v / 4) + 4 (l / 32) + v % 4.  Each reduction step of the product takes two floats per row,
// one from each lane half: of every 8 consecutive floats of a row, lane half 0 supplies the first 4 and half 1 the last 4.
//
// The softmax over the streamed side is therefore a reduction over a lane's 16 registers plus ONE exchange between the two lane
// halves (__shfl_xor 32), kept as a running max / sum; a streamed row that does not exist is -inf in the tile, so it enters
// neither.  The second product, out^T[d, i] += V^T[d, j] P[j, i], sums over the tile's ROW index: the tile of probabilities is
// its B operand exactly as the registers hold it, with no lane movement, and the accumulator again has the owned token on the
// lane -- the rescale factor of a column is the lane's own.
//
// Exact fp32 products, fp32 accumulation, and every sum in one fixed order: registers 0..15, then the other lane half.
//
// Here: the types and the register-to-row map (from mfma_frag.hpp, which the GEMM kernels share), the register-staged tile
// load / store, the owned-row load, the score product, the running-softmax step, the rescale and the second product.  In
// attn_bwd_tile.hpp: what the recomputing backwards (vit_attn_bwd.hip, dec_attn_bwd.hip) add.  In dec_attn_launch.hpp,
// vit_attn_launch.hpp and biattn_common.hpp: what a forward shares with its own training route (the decoder's whole forward
// text; the ViT's tile configuration, relative-position terms and row store; the bi-attention core's whole image-side text,
// its A-operand product and row store, and the text side's range combine).  In the kernels: the grid and what a wave owns, what is added to a
// score before the softmax (clamp, mask, relative-position terms, -inf for tail rows), how partial results are combined.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mfma_frag.hpp"

namespace attn_tile {

typedef float f32x4 __attribute__((__vector_size__(16)));
using mfma_frag::f32x16;
using mfma_frag::acc_row;             // row of accumulator register v in a 32 x 32 tile, for lane half 0 (half 1: + 4)
using mfma_frag::zero_acc;

constexpr int kTile = 32;             // rows of a streamed tile, owned tokens of a wave

// float4 items of a tile of 32 rows x D floats that each of THREADS threads carries
template <int D, int THREADS>
constexpr int kTileItems = (kTile * D / 4 + THREADS - 1) / THREADS;

// global -> registers: rows [0, nvalid) of a tile of 32 rows x D floats (row stride `stride` floats), item f = tid + r THREADS
// being float4 f % (D / 4) of row f / (D / 4); other rows are zero and not read
template <int D, int THREADS>
__device__ __forceinline__ void tile_load(f32x4 (&pre)[(kTileItems<D, THREADS>)], const float* __restrict__ base, int64_t stride,
                                          int nvalid, int tid) {
#pragma unroll
  for (int r = 0; r < kTileItems<D, THREADS>; ++r) {
    const int f = tid + r * THREADS, row = f / (D / 4), c4 = f % (D / 4);
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
    pre[r] = (f < kTile * D / 4 && row < nvalid) ? *reinterpret_cast<const f32x4*>(base + (int64_t)row * stride + c4 * 4) : z;
  }
}

// registers -> LDS, the same items
template <int D, int THREADS, int PITCH>
__device__ __forceinline__ void tile_store(float (*Ts)[PITCH], const f32x4 (&pre)[(kTileItems<D, THREADS>)], int tid) {
#pragma unroll
  for (int r = 0; r < kTileItems<D, THREADS>; ++r) {
    const int f = tid + r * THREADS, row = f / (D / 4), c4 = f % (D / 4);
    if (f < kTile * D / 4) *reinterpret_cast<f32x4*>(&Ts[row][c4 * 4]) = pre[r];
  }
}

// The lane's share of reduction step ss of the owned token's operand row, scaled first: floats [8 ss + 4 half, + 4) of `row`;
// zero when !valid (`row` must still be readable).
__device__ __forceinline__ f32x4 own_part(const float* __restrict__ row, bool valid, float scale, int half, int ss) {
  f32x4 z = {0.f, 0.f, 0.f, 0.f};
  return valid ? *reinterpret_cast<const f32x4*>(row + ss * 8 + half * 4) * scale : z;
}

// the owned token's operand row of D floats, as the lane's share of every reduction step
template <int D>
__device__ __forceinline__ void own_load(f32x4 (&own)[D / 8], const float* __restrict__ row, bool valid, float scale, int half) {
#pragma unroll
  for (int ss = 0; ss < D / 8; ++ss) own[ss] = own_part(row, valid, scale, half, ss);
}

// reduction step ss of the score product: X[streamed row, owned token] += Ts[streamed row, 8 ss ..] . own_ss, as four MFMAs
template <int PITCH>
__device__ __forceinline__ void score_step(const float (*Ts)[PITCH], const f32x4& own_ss, f32x16& X, int r32, int half, int ss) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(&Ts[r32][ss * 8 + half * 4]);
#pragma unroll
  for (int t = 0; t < 4; ++t) X = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], own_ss[t], X, 0, 0, 0);
}

// X[streamed row, owned token] += Ts[streamed row, :D] . own[:D]
template <int D, int PITCH>
__device__ __forceinline__ void scores(const float (*Ts)[PITCH], const f32x4 (&own)[D / 8], f32x16& X, int r32, int half) {
#pragma unroll
  for (int ss = 0; ss < D / 8; ++ss) score_step(Ts, own[ss], X, r32, half, ss);
}

// One step of the running softmax over the streamed rows of the lane's owned token.  X holds the tile's scores as the kernel
// wants them in the softmax (everything added, rows that do not exist -inf) and leaves as the tile of probabilities against
// the new running max; m_run / l_run are updated, and the factor that brings what was accumulated against the old max to the
// new one is returned.
//   GUARD_EMPTY: the owned token may have met nothing but -inf so far; the exponentials are then taken against 0 (every term
//                is exp(-inf) = 0), never against -inf (exp(-inf - -inf) is NaN).  Without it the max must be finite.
//   FLOOR:       the exponent is kept at or above -floor.
template <bool GUARD_EMPTY, bool FLOOR>
__device__ __forceinline__ float softmax_step(f32x16& X, float& m_run, float& l_run, float floor = 0.f) {
  float tmax = -INFINITY;
#pragma unroll
  for (int v = 0; v < 16; ++v) tmax = fmaxf(tmax, X[v]);
  tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
  const float m_new = fmaxf(m_run, tmax);
  const float m_use = GUARD_EMPTY && m_new == -INFINITY ? 0.f : m_new;
  const float alpha = expf(m_run - m_use);
  float psum = 0.f;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const float p = FLOOR ? expf(fmaxf(X[v] - m_use, -floor)) : expf(X[v] - m_use);
    X[v] = p;
    psum += p;
  }
  psum += __shfl_xor(psum, 32);
  l_run = l_run * alpha + psum;
  m_run = m_new;
  return alpha;
}

// acc *= alpha, skipped when no lane of the wave has a factor other than 1: a factor of 1 changes no bit, so skipping is not
// a different result
template <int DB>
__device__ __forceinline__ void rescale(f32x16 (&acc)[DB], float alpha) {
  if (__any(alpha != 1.f)) {
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[db][v] *= alpha;
  }
}

// the second product: acc[db][d, owned token] += Ts[streamed row, 32 db + d] P[streamed row, owned token], rows in register
// order
template <int DB, int PITCH>
__device__ __forceinline__ void pv(const float (*Ts)[PITCH], const f32x16& P, f32x16 (&acc)[DB], int r32, int half) {
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const float* vrow = &Ts[acc_row(v) + 4 * half][r32];
#pragma unroll
    for (int db = 0; db < DB; ++db) acc[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[db * 32], P[v], acc[db], 0, 0, 0);
  }
}

}  // namespace attn_tile
