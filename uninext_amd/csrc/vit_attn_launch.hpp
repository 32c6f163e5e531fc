// What vit_attn.hip shares with its training route (vit_attn_bwd.hip).  Internal: not part of the C ABI.
//   device  the tile configuration Cfg<D>, the zero-fill of a tile's pad columns, the divide by q_w, the relative-position terms
//           of a score, and the store of an accumulator's row;
//   host    the geometry check, the size of the relative-position terms, the divide-by-q_w constant and the launch of the
//           rel_terms kernel (defined in vit_attn.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "attn_tile.hpp"

namespace vit_attn {

using namespace attn_tile;            // kTile = 32: streamed rows per LDS tile, owned tokens per wave

constexpr int kThreads = 256;
constexpr int kGroup = 4 * kTile;     // owned tokens per workgroup

template <int D>
struct Cfg {
  static constexpr int kDB = (D + 31) / 32;          // 32-wide blocks of d in the second product
  static constexpr int kDP = kDB * 32;               // tile columns the second product reads (D = 80: 96, the last 16 zero)
  static constexpr int kPitch = kDP + 4;             // floats per LDS row: rows 16-byte aligned, 4-bank step between rows
  static constexpr int kPre = kTileItems<D, kThreads>;   // float4 items of a tile per thread
};

// the columns of a tile past D: zero once, no tile_store touches them
template <int D>
__device__ __forceinline__ void zero_pad_columns(float (*Ts)[Cfg<D>::kPitch], int tid) {
  using C = Cfg<D>;
  if (C::kDP > D) {
    for (int f = tid; f < kTile * (C::kDP - D); f += kThreads) Ts[f / (C::kDP - D)][D + f % (C::kDP - D)] = 0.f;
  }
}

__device__ __forceinline__ int div_w(int x, int Wq, unsigned wq_magic) {   // x / Wq (exact: host limits)
  return Wq == 1 ? x : (int)__umulhi((unsigned)x, wq_magic);
}

// The relative-position terms of one score for the lane's query (relp = &rel[bh, 0, i]): column jh and column Hq + jw of the key
// (jh, jw).  A key past S takes the last key's columns; its score is excluded by the caller.  (One register at a time: the loop
// over a tile's 16 registers inside this function cost vit_attn::attn<64, true> and <80, true> a VGPR each, 181 and 187.)
__device__ __forceinline__ void rel_term(float& rh, float& rw, const float* relp, int key, int S, int Hq, int Wq, unsigned wq_magic,
                                         int SP) {
  key = key < S ? key : S - 1;
  const int jh = div_w(key, Wq, wq_magic), jw = key - jh * Wq;
  rh = relp[jh * SP];
  rw = relp[(Hq + jw) * SP];
}

// dst[d] = acc[d, lane's token] * factor for the lane's d (accumulator layout of attn_tile's second product: four consecutive d
// per register quad, the token on the lane)
template <int D>
__device__ __forceinline__ void store_row(float* __restrict__ dst, const f32x16 (&acc)[Cfg<D>::kDB], int half, float factor = 1.f) {
#pragma unroll
  for (int db = 0; db < Cfg<D>::kDB; ++db)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int d = db * 32 + g4 * 8 + half * 4;
      if (d < D) {
        f32x4 r = {acc[db][g4 * 4] * factor, acc[db][g4 * 4 + 1] * factor, acc[db][g4 * 4 + 2] * factor, acc[db][g4 * 4 + 3] * factor};
        *reinterpret_cast<f32x4*>(dst + d) = r;
      }
    }
}

// ---- host side ----------------------------------------------------------------------------------
// 0, or a negative PATCH_EMBED_ERR_* (message set)
int geometry(int batch, int num_heads, int q_h, int q_w, int head_dim);
// bytes of rel[batch * num_heads, q_h + q_w, roundup(S, 32)]: the forward's whole workspace (at least 256)
size_t rel_bytes(int batch, int num_heads, int q_h, int q_w);
// x / q_w == __umulhi(x, div_magic(q_w)) inside the geometry limits (q_w == 1: unused)
unsigned div_magic(int q_w);
// enqueues rel_terms<head_dim> (head_dim 64 or 80, geometry checked by the caller); 0 or the launch's status
int launch_rel_terms(int head_dim, hipStream_t stream, const float* qkv, const float* rel_h_table, const float* rel_w_table, int batch,
                     int num_heads, int q_h, int q_w, float* rel);

}  // namespace vit_attn
