// What dec_attn.hip and its training route (dec_attn_bwd.hip) share: the constants of the scheme, the mask's element, the ONE
// text of the forward (dec_attn::attn and dec_attn_bwd::attn_lse are thin kernels around it, so the training `out` cannot
// drift from the inference `out`), and the host-side argument checks.  Internal: not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "../../include/biattn_hip.h"
#include "attn_tile.hpp"
#include "launch_glue.hpp"
#include "msda_common.hpp"

namespace dec_attn {

using namespace attn_tile;            // kTile = 32: streamed rows per LDS tile, owned tokens per workgroup

constexpr int kD = 32;                // head dimension
constexpr int kWaves = 2;             // streamed ranges of a workgroup, one wave each
constexpr int kThreads = 64 * kWaves;
constexpr int kPitch = kD + 4;        // floats per LDS row: rows 16-byte aligned, 4-bank step between rows
constexpr int kPre = kTileItems<kD, 64>;   // float4 items of a tile per lane: every wave loads its own tiles
constexpr int kMaxLen = 65535;

// what the mask adds to the score of (query, key) at element `at` of the [L, L] mask
template <int MASK>
__device__ __forceinline__ float mask_add(const void* __restrict__ mask, size_t at) {
  if (MASK == BIATTN_MASK_BOOL) return static_cast<const unsigned char*>(mask)[at] ? -INFINITY : 0.f;
  if (MASK == BIATTN_MASK_F32) return static_cast<const float*>(mask)[at];
  return 0.f;
}

// The forward, for a grid of (batch * heads * NG) workgroups of kThreads, NG = groups of 32 queries.  MASK: BIATTN_MASK_NONE /
// _BOOL / _F32.  LSE: wave 0 also stores lse[bh, i] = max + log(sum) of the combined key ranges for i < SP = 32 NG (-inf for a
// query with every key excluded, 0 for the rows past L, which the key pass reads); without it SP and lse are not looked at.
template <int MASK, bool LSE>
__device__ __forceinline__ void fwd(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int64_t qs,
                                    int64_t ks, int64_t vs, const void* __restrict__ mask, int heads, int L, int SP, int NG,
                                    float scale, float* __restrict__ out, float* __restrict__ lse) {
  __shared__ __attribute__((aligned(16))) float Ts[kWaves][kTile][kPitch];
  __shared__ float Part[18][64];      // wave 1's accumulator registers, running max and sum, by lane

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r32 = lane & 31, half = lane >> 5;
  const int bh = blockIdx.x / NG, grp = blockIdx.x - bh * NG, b = bh / heads, h = bh - b * heads;
  const int i = grp * kTile + r32;
  const int ic = i < L ? i : L - 1;                                 // queries past L: the last row's addresses, nothing stored

  // the owned query's row, scaled first (in fp32, as F.multi_head_attention_forward does).  Queries past L are zero rows.
  f32x4 own[kD / 8];
  {
    const float* row = q + ((int64_t)b * L + ic) * qs + h * kD;
    own_load<kD>(own, row, i < L, scale, half);
  }

  const float* kbase = k + (int64_t)b * L * ks + h * kD;
  const float* vbase = v + (int64_t)b * L * vs + h * kD;
  const int tiles = (L + kTile - 1) / kTile;
  const int per_wave = (tiles + kWaves - 1) / kWaves;               // the same trip count in both waves: the barriers meet
  const int t0 = wv * per_wave;
  auto rows_of = [&](int t) { const int n = L - t * kTile; return n < kTile ? n : kTile; };   // <= 0 past the last tile
  float (*T)[kPitch] = Ts[wv];

  float m_run = -INFINITY, l_run = 0.f;
  f32x16 acc[1];
#pragma unroll
  for (int u = 0; u < 16; ++u) acc[0][u] = 0.f;

  f32x4 pre[kPre];
  tile_load<kD, 64>(pre, kbase + (int64_t)t0 * kTile * ks, ks, rows_of(t0), lane);
  tile_store<kD, 64>(T, pre, lane);
  __syncthreads();

  for (int it = 0; it < per_wave; ++it) {
    const int t = t0 + it;
    const int nv = rows_of(t);                                      // wave-uniform; <= 0: this wave has no tile left
    tile_load<kD, 64>(pre, vbase + (int64_t)t * kTile * vs, vs, nv, lane);

    // what is added to the scores of the lane's query: the mask's element, -inf for keys past the end
    float add[16];
    bool open = false;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int kr = acc_row(u) + 4 * half;
      float a = 0.f;
      if (MASK != BIATTN_MASK_NONE && kr < nv) a = mask_add<MASK>(mask, (size_t)ic * (size_t)L + (size_t)(t * kTile + kr));
      a = kr < nv ? a : -INFINITY;
      add[u] = a;
      open = open || !(a == -INFINITY);
    }
    const bool live = __any(open) != 0;                             // wave-uniform: some query of the wave has an open key here

    f32x16 X;
#pragma unroll
    for (int u = 0; u < 16; ++u) X[u] = 0.f;
    if (live) {
      scores<kD>(T, own, X, r32, half);
#pragma unroll
      for (int u = 0; u < 16; ++u) X[u] += add[u];
      rescale(acc, softmax_step<true, false>(X, m_run, l_run));     // guarded: nothing may be open yet for this query
    }
    __syncthreads();
    tile_store<kD, 64>(T, pre, lane);
    __syncthreads();
    if (it + 1 < per_wave) tile_load<kD, 64>(pre, kbase + (int64_t)(t + 1) * kTile * ks, ks, rows_of(t + 1), lane);
    if (live) pv(T, X, acc, r32, half);
    __syncthreads();
    if (it + 1 < per_wave) tile_store<kD, 64>(T, pre, lane);
    __syncthreads();
  }

  // the two key ranges, combined in range order by wave 0
  if (wv == 1) {
#pragma unroll
    for (int u = 0; u < 16; ++u) Part[u][lane] = acc[0][u];
    Part[16][lane] = m_run;
    Part[17][lane] = l_run;
  }
  __syncthreads();
  if (wv == 0 && i < L) {
    const float m1 = Part[16][lane], l1 = Part[17][lane];
    const float m = fmaxf(m_run, m1);
    const float m_use = m == -INFINITY ? 0.f : m;
    const float a0 = expf(m_run - m_use), a1 = expf(m1 - m_use);
    const float l = l_run * a0 + l1 * a1;
    const float inv = 1.f / l;                                      // every key excluded: 1 / 0, and 0 * inf below is NaN
    // out[i, h D + d]: d in the registers (four consecutive d per register quad), the query on the lane
    float* o = out + ((int64_t)b * L + i) * ((int64_t)heads * kD) + h * kD;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      f32x4 r;
#pragma unroll
      for (int u = 0; u < 4; ++u) r[u] = (acc[0][g4 * 4 + u] * a0 + Part[g4 * 4 + u][lane] * a1) * inv;
      *reinterpret_cast<f32x4*>(o + g4 * 8 + half * 4) = r;
    }
    if (LSE && half == 0) lse[(int64_t)bh * SP + i] = m + logf(l);  // every key excluded: -inf + log(0) = -inf
  }
  if (LSE && wv == 0 && i >= L && half == 0) lse[(int64_t)bh * SP + i] = 0.f;   // i < SP
}

// ---- host side ----------------------------------------------------------------------------------
// sets "<who>: <what>" as the thread's last error (msda::set_error copies the text) and returns `code`
inline int refuse(const char* who, int code, const char* what) {
  char text[160];
  snprintf(text, sizeof(text), "%s: %s", who, what);
  return msda::set_error(code, text);
}

// 0, or a negative BIATTN_ERR_* (message set): the limits on the dimensions, the mask kind and every row stride
inline int geometry(const char* who, int batch, int num_heads, int len, int head_dim, int mask_kind,
                    std::initializer_list<long long> strides) {
  if (batch < 0 || num_heads <= 0 || len <= 0 || head_dim <= 0) return refuse(who, BIATTN_ERR_BAD_DIMS, "bad dimensions");
  if (len > kMaxLen) return refuse(who, BIATTN_ERR_BAD_DIMS, "len must be at most 65535");
  if (head_dim != kD) return refuse(who, BIATTN_ERR_UNSUPPORTED, "head_dim must be 32");
  if (mask_kind != BIATTN_MASK_NONE && mask_kind != BIATTN_MASK_BOOL && mask_kind != BIATTN_MASK_F32)
    return refuse(who, BIATTN_ERR_UNSUPPORTED, "unknown mask kind (none, bool or fp32)");
  const long long E = (long long)num_heads * kD, NG = msda::ceil_div(len, kTile);
  for (long long s : strides) {
    if (s < E) return refuse(who, BIATTN_ERR_BAD_DIMS, "a row stride is smaller than num_heads * head_dim");
    if (s % 4 != 0) return refuse(who, BIATTN_ERR_UNSUPPORTED, "row strides must be multiples of 4 floats");
    if (s >= (1ll << 31) || (long long)batch * len * s >= (1ll << 42)) return refuse(who, BIATTN_ERR_BAD_DIMS, "problem too large");
  }
  if ((long long)batch * num_heads * NG >= (1ll << 31)) return refuse(who, BIATTN_ERR_BAD_DIMS, "problem too large");
  return 0;
}

// 0, or a negative BIATTN_ERR_* (message set): a mask of a kind other than none is there, an fp32 one on a float's boundary
inline int mask_pointer(const char* who, const void* mask, int mask_kind) {
  if (mask_kind != BIATTN_MASK_NONE && !mask) return refuse(who, BIATTN_ERR_NULL_POINTER, "null pointer argument");
  if (mask_kind == BIATTN_MASK_F32 && reinterpret_cast<uintptr_t>(mask) % 4 != 0)
    return refuse(who, BIATTN_ERR_UNSUPPORTED, "an fp32 mask must be 4-byte aligned");
  return 0;
}

}  // namespace dec_attn
