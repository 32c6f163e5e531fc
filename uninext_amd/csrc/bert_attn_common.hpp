// What bert.hip's attention kernel and its training route (bert_attn_bwd.hip) share: the constants of the scheme, the keep test
// of a streamed tile, the ONE text of the forward (bert::attn and bert_attn_bwd::attn_train are thin kernels around it, so the
// training `out` cannot drift from the inference `out`), and the host-side argument checks.  Internal: not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "../../include/dynmask_hip.h"
#include "attn_tile.hpp"
#include "launch_glue.hpp"
#include "msda_common.hpp"
#include "philox.hpp"

namespace bert {

using namespace attn_tile;            // kTile = 32: streamed rows per LDS tile, owned tokens per workgroup

constexpr int kD = 64;                // head dimension
constexpr int kDB = kD / 32;          // 32-wide blocks of d in the second product
constexpr int kWaves = 2;             // streamed ranges of a workgroup, one wave each
constexpr int kThreads = 64 * kWaves;
constexpr int kPitch = kD + 4;        // floats per LDS row: rows 16-byte aligned, 4-bank step between rows
constexpr int kPre = kTileItems<kD, 64>;   // float4 items of a tile per lane: every wave loads its own tiles
constexpr int kMaxLen = 512;

// What the mask adds to the scores of the lane's query ic against tile t (0 kept, -inf excluded or past the end; nv rows of the
// tile exist, <= 0: none).  Returns whether any query of the wave keeps a key of the tile: wave-uniform.
template <int MASK>
__device__ __forceinline__ bool tile_keep(float (&add)[16], const void* __restrict__ mask, int b, int ic, int T, int t, int nv,
                                          int r32, int half) {
  if (MASK == BERT_MASK_FULL_U8) {
    const unsigned char* row = static_cast<const unsigned char*>(mask) + ((size_t)b * T + ic) * (size_t)T + (size_t)t * kTile;
    bool open = false;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int kr = acc_row(u) + 4 * half;
      const bool keep = kr < nv && row[kr] != 0;
      add[u] = keep ? 0.f : -INFINITY;
      open = open || keep;
    }
    return __any(open) != 0;
  }
  bool flag = r32 < nv;
  if (flag && MASK == BERT_MASK_KEY_I64) flag = static_cast<const long long*>(mask)[(size_t)b * T + t * kTile + r32] != 0;
  if (flag && MASK == BERT_MASK_KEY_U8) flag = static_cast<const unsigned char*>(mask)[(size_t)b * T + t * kTile + r32] != 0;
  const unsigned bits = (unsigned)__ballot(flag);   // lanes 0..31: the tile's 32 flags (lanes 32..63 repeat them)
#pragma unroll
  for (int u = 0; u < 16; ++u) add[u] = (bits >> (acc_row(u) + 4 * half)) & 1u ? 0.f : -INFINITY;
  return bits != 0;
}

// The forward, for a grid of (batch * heads * NG) workgroups of kThreads, NG = groups of 32 queries.
//   LSE:  wave 0 also stores lse[bh, i] = max + log(sum) of the combined key ranges for i < SP = 32 NG (-inf for a query that
//         keeps no key, 0 for the rows past T, which the key pass reads); without it SP and lse are not looked at.
//   DROP: the tile of probabilities is multiplied by c m (philox.hpp) between the running softmax, whose max and sum stay those
//         of all kept keys, and the second product; without it `drop` is not looked at.
template <int MASK, bool LSE, bool DROP>
__device__ __forceinline__ void fwd(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int64_t qs,
                                    int64_t ks, int64_t vs, const void* __restrict__ mask, int heads, int T, int SP, int NG,
                                    float scale, float* __restrict__ out, float* __restrict__ lse,
                                    const philox::Dropout& drop = philox::Dropout()) {
  __shared__ __attribute__((aligned(16))) float Ts[kWaves][kTile][kPitch];
  __shared__ float Part[16 * kDB + 2][64];   // wave 1's accumulator registers, running max and sum, by lane

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r32 = lane & 31, half = lane >> 5;
  const int bh = blockIdx.x / NG, grp = blockIdx.x - bh * NG, b = bh / heads, h = bh - b * heads;
  const int i = grp * kTile + r32;
  const int ic = i < T ? i : T - 1;                                 // queries past T: the last row's addresses, nothing stored

  f32x4 own[kD / 8];                                                // the owned query's row, scaled first in fp32
  own_load<kD>(own, q + ((int64_t)b * T + ic) * qs + h * kD, i < T, scale, half);

  const float* kbase = k + (int64_t)b * T * ks + h * kD;
  const float* vbase = v + (int64_t)b * T * vs + h * kD;
  const int tiles = (T + kTile - 1) / kTile;
  const int per_wave = (tiles + kWaves - 1) / kWaves;               // the same trip count in both waves: the barriers meet
  const int t0 = wv * per_wave;
  auto rows_of = [&](int t) { const int n = T - t * kTile; return n < kTile ? n : kTile; };   // <= 0 past the last tile
  float (*Tw)[kPitch] = Ts[wv];

  float m_run = -INFINITY, l_run = 0.f;
  f32x16 acc[kDB];
#pragma unroll
  for (int db = 0; db < kDB; ++db)
#pragma unroll
    for (int u = 0; u < 16; ++u) acc[db][u] = 0.f;

  float add[16];
  bool live = tile_keep<MASK>(add, mask, b, ic, T, t0, rows_of(t0), r32, half);
  f32x4 pre[kPre];
  tile_load<kD, 64>(pre, kbase + (int64_t)t0 * kTile * ks, ks, live ? rows_of(t0) : 0, lane);
  tile_store<kD, 64>(Tw, pre, lane);
  __syncthreads();

  for (int it = 0; it < per_wave; ++it) {
    const int t = t0 + it;
    const bool more = it + 1 < per_wave;
    tile_load<kD, 64>(pre, vbase + (int64_t)t * kTile * vs, vs, live ? rows_of(t) : 0, lane);   // a dead tile: nothing is read

    uint32_t keep = 0;                                              // drawn before the score fragment is live
    if (DROP && live) keep = philox::keep_bits_row_owner(philox::stream_of(drop), drop.threshold, bh, ic, t * kTile, half);

    f32x16 X;
#pragma unroll
    for (int u = 0; u < 16; ++u) X[u] = 0.f;
    if (live) {
      scores<kD>(Tw, own, X, r32, half);
#pragma unroll
      for (int u = 0; u < 16; ++u) X[u] += add[u];
      rescale(acc, softmax_step<true, false>(X, m_run, l_run));     // guarded: this query may have kept nothing yet
      if (DROP) {
#pragma unroll
        for (int u = 0; u < 16; ++u) X[u] *= philox::keep_factor(keep, u, drop.scale);
      }
    }
    __syncthreads();
    tile_store<kD, 64>(Tw, pre, lane);
    __syncthreads();
    float add_next[16];
    bool live_next = false;
    if (more) {
      live_next = tile_keep<MASK>(add_next, mask, b, ic, T, t + 1, rows_of(t + 1), r32, half);
      tile_load<kD, 64>(pre, kbase + (int64_t)(t + 1) * kTile * ks, ks, live_next ? rows_of(t + 1) : 0, lane);
    }
    if (live) pv(Tw, X, acc, r32, half);
    __syncthreads();
    if (more) {
      tile_store<kD, 64>(Tw, pre, lane);
#pragma unroll
      for (int u = 0; u < 16; ++u) add[u] = add_next[u];
    }
    live = live_next;
    __syncthreads();
  }

  // the two key ranges, combined in range order by wave 0
  if (wv == 1) {
#pragma unroll
    for (int db = 0; db < kDB; ++db)
#pragma unroll
      for (int u = 0; u < 16; ++u) Part[db * 16 + u][lane] = acc[db][u];
    Part[16 * kDB][lane] = m_run;
    Part[16 * kDB + 1][lane] = l_run;
  }
  __syncthreads();
  if (wv == 0 && i < T) {
    const float m1 = Part[16 * kDB][lane], l1 = Part[16 * kDB + 1][lane];
    const float m = fmaxf(m_run, m1);
    const float m_use = m == -INFINITY ? 0.f : m;
    const float a0 = expf(m_run - m_use), a1 = expf(m1 - m_use);
    const float l = l_run * a0 + l1 * a1;
    const float inv = l > 0.f ? 1.f / l : 0.f;                      // no key kept: sum 0, accumulator 0, a row of zeros
    // out[i, h D + d]: d in the registers (four consecutive d per register quad), the query on the lane
    float* o = out + ((int64_t)b * T + i) * ((int64_t)heads * kD) + h * kD;
#pragma unroll
    for (int db = 0; db < kDB; ++db)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        f32x4 r;
#pragma unroll
        for (int u = 0; u < 4; ++u) r[u] = (acc[db][g4 * 4 + u] * a0 + Part[db * 16 + g4 * 4 + u][lane] * a1) * inv;
        *reinterpret_cast<f32x4*>(o + db * 32 + g4 * 8 + half * 4) = r;
      }
    if (LSE && half == 0) lse[(int64_t)bh * SP + i] = m + logf(l);  // no key kept: -inf + log(0) = -inf
  }
  if (LSE && wv == 0 && i >= T && half == 0) lse[(int64_t)bh * SP + i] = 0.f;   // i < SP
}

// ---- host side ----------------------------------------------------------------------------------
// sets "<who>: <what>" as the thread's last error (msda::set_error copies the text) and returns `code`
inline int refuse(const char* who, int code, const char* what) {
  char text[160];
  snprintf(text, sizeof(text), "%s: %s", who, what);
  return msda::set_error(code, text);
}

// 0, or a negative BERT_ERR_* (message set): the limits on the dimensions, the mask kind and every row stride
inline int geometry(const char* who, int batch, int num_heads, int len, int head_dim, int mask_kind,
                    std::initializer_list<long long> strides) {
  if (batch < 0 || num_heads <= 0 || len <= 0 || head_dim <= 0) return refuse(who, BERT_ERR_BAD_DIMS, "bad dimensions");
  if (head_dim != kD) return refuse(who, BERT_ERR_UNSUPPORTED, "head_dim must be 64");
  if (len > kMaxLen) return refuse(who, BERT_ERR_UNSUPPORTED, "len must be at most 512");
  if (mask_kind != BERT_MASK_NONE && mask_kind != BERT_MASK_KEY_I64 && mask_kind != BERT_MASK_KEY_U8 && mask_kind != BERT_MASK_FULL_U8)
    return refuse(who, BERT_ERR_UNSUPPORTED, "unknown mask kind (none, key int64, key u8 or full u8)");
  const long long E = (long long)num_heads * kD, NG = msda::ceil_div(len, kTile);
  for (long long s : strides) {
    if (s < E) return refuse(who, BERT_ERR_BAD_DIMS, "a row stride is smaller than num_heads * head_dim");
    if (s % 4 != 0) return refuse(who, BERT_ERR_UNSUPPORTED, "row strides must be multiples of 4 floats");
    if (s >= (1ll << 31) || (long long)batch * len * s >= (1ll << 42)) return refuse(who, BERT_ERR_BAD_DIMS, "problem too large");
  }
  if ((long long)batch * num_heads * NG >= (1ll << 31)) return refuse(who, BERT_ERR_BAD_DIMS, "problem too large");
  return 0;
}

// 0, or a negative BERT_ERR_* (message set): a mask of a kind other than none is there, an int64 one on its boundary
inline int mask_pointer(const char* who, const void* mask, int mask_kind) {
  if (mask_kind != BERT_MASK_NONE && !mask) return refuse(who, BERT_ERR_NULL_POINTER, "null pointer argument");
  if (mask_kind == BERT_MASK_KEY_I64 && reinterpret_cast<uintptr_t>(mask) % 8 != 0)
    return refuse(who, BERT_ERR_UNSUPPORTED, "an int64 mask must be 8-byte aligned");
  return 0;
}

inline const char* kind_name(int mask_kind) {
  return mask_kind == BERT_MASK_NONE ? "none" : mask_kind == BERT_MASK_KEY_I64 ? "key_i64" : mask_kind == BERT_MASK_KEY_U8 ? "key_u8" : "full_u8";
}

}  // namespace bert
