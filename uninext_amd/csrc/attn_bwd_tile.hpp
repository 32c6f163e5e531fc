// What the recomputing attention backwards (vit_attn_bwd.hip, dec_attn_bwd.hip) add to attn_tile.hpp's scheme.  Internal: device
// code only, not part of the C ABI.
//
// Both passes hold one 32 x 32 tile per wave with the OWNED token on the lane and the STREAMED tokens in the 16 registers:
// the query pass owns queries (scaled q and g in registers, delta = g . o taken from the owned rows), the key pass owns keys and
// streams the scaled q and g tiles.  From the tile of probabilities p and of dp = g . v, ds = p (dp - delta) is the B operand
// of attn_tile's second product as the registers hold it.
//
// Here: the owned rows of the query pass, the scaled tile of the key pass and its ds^T step.  In the kernels: the grid and what a
// wave owns, the mask or relative-position terms, which tiles are skipped, how p is taken from the score, the width and height
// bins, the two-wave hand-over and every store.
#pragma once

#include "attn_tile.hpp"

namespace attn_bwd_tile {

using namespace attn_tile;

// The owned rows of the query pass, as the lane's share of every reduction step: the scaled q as the forward rounds it, and g.
// Returns delta = g . o of the lane's token: each lane half sums its floats in step order, then one exchange.  Zero rows, and
// delta 0, when !valid (the rows must still be readable).
template <int D>
__device__ __forceinline__ float own_rows(f32x4 (&ownq)[D / 8], f32x4 (&owng)[D / 8], const float* __restrict__ qrow,
                                          const float* __restrict__ grow, const float* __restrict__ orow, bool valid, float scale,
                                          int half) {
  float dl = 0.f;
#pragma unroll
  for (int ss = 0; ss < D / 8; ++ss) {
    ownq[ss] = own_part(qrow, valid, scale, half, ss);
    owng[ss] = own_part(grow, valid, 1.f, half, ss);
    const f32x4 o = own_part(orow, valid, 1.f, half, ss);
#pragma unroll
    for (int u = 0; u < 4; ++u) dl = fmaf(owng[ss][u], o[u], dl);
  }
  return dl + __shfl_xor(dl, 32);
}

// global -> LDS: tile_load's rows times `scale` (the scaled row, rounded as the forward's owned row is), through `pre`
template <int D, int THREADS, int PITCH>
__device__ __forceinline__ void stage_scaled(float (*Ts)[PITCH], f32x4 (&pre)[(kTileItems<D, THREADS>)], const float* __restrict__ base,
                                             int64_t stride, int nvalid, float scale, int tid) {
  tile_load<D, THREADS>(pre, base, stride, nvalid, tid);
#pragma unroll
  for (int r = 0; r < kTileItems<D, THREADS>; ++r) pre[r] = pre[r] * scale;
  tile_store<D, THREADS>(Ts, pre, tid);
}

// P <- ds^T = p^T (dp^T - delta), the owned token a key: the delta of each register's streamed query.  (The query pass's
// ds = p (dp - delta) stays in its loop over p: taken out of it, dec_attn_bwd::bwd_q compiled to 137 | 142 | 144 VGPRs for its
// 122 | 140 | 140.)
__device__ __forceinline__ void ds_t(f32x16& P, const f32x16& DP, const float (&delta)[16]) {
#pragma unroll
  for (int v = 0; v < 16; ++v) P[v] = P[v] * (DP[v] - delta[v]);
}

}  // namespace attn_bwd_tile
