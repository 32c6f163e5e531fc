// What the inference kernels of the bi-directional attention core (biattn.hip) share with its training route (biattn_bwd.hip):
// the constants, the split of S into ranges, the file's own tile pair, the clamp, what the text mask adds to a score, the
// product with the probabilities as the A operand and its row store, the text side's range combine, the ONE
// text of the image-side forward (image_fwd: biattn::biattn_image and biattn_bwd::image_train are thin kernels around it, so
// the training out_v cannot drift from the inference out_v), the NJ dispatch and the argument checks of the C ABI
// (include/biattn_hip.h).  Internal: not part of the C ABI.
#pragma once

#include "../../include/biattn_hip.h"

#include <math.h>

#include <initializer_list>
#include <type_traits>

#include "attn_tile.hpp"
#include "launch_glue.hpp"
#include "msda_common.hpp"
#include "philox.hpp"

namespace biattn {

using namespace attn_tile;            // kTile = 32: streamed rows per LDS tile

constexpr int kThreads = 256;
constexpr int kD = 256;               // head dimension
constexpr int kMaxT = 256;            // text tokens
constexpr int kPitch = kD + 4;        // floats per LDS row (rows stay 16-byte aligned)
constexpr int kPre = kTileItems<kD, kThreads>;   // float4 items per thread and tile
constexpr int kTargetGroups = 256;    // text-side workgroups a launch aims at (one per CU of the MI355X)
constexpr int kMaxChunks = 64;
constexpr float kClamp = 50000.f;
constexpr float kMasked = -9e15f;

struct Plan {
  int TP;       // text tokens rounded up to 32
  int NG;       // groups of four 32-token blocks
  int NC;       // ranges of S
  size_t bytes;
};

inline Plan plan(long long BH, int S, int T) {
  Plan p;
  p.TP = msda::round_up(T, kTile);
  p.NG = (p.TP + 4 * kTile - 1) / (4 * kTile);
  const long long tiles = ((long long)S + kTile - 1) / kTile;
  long long per = BH * p.NG;
  long long nc = per > 0 ? (kTargetGroups + per - 1) / per : 1;
  if (nc > kMaxChunks) nc = kMaxChunks;
  if (nc > tiles) nc = tiles;
  if (nc < 1) nc = 1;
  p.NC = (int)nc;
  p.bytes = (size_t)BH * p.NC * (kD + 2) * p.TP * sizeof(float);
  if (p.bytes < 256) p.bytes = 256;
  return p;
}

// This file's own tile pair (not attn_tile's): a row is one wave-wide load, which allows 32-bit lane offsets, and the store
// takes a factor (the Q tile of biattn_text is scaled on its way in).
// global -> registers: rows [0, nvalid) of a tile of 32 rows x 256 floats (row stride `stride` floats); other rows are zero.
__device__ __forceinline__ void tile_load(f32x4 (&pre)[kPre], const float* __restrict__ base, int64_t stride, int nvalid, int tid) {
  const uint32_t lane_off = (uint32_t)(tid >> 6) * (uint32_t)stride + (uint32_t)(tid & 63) * 4u;   // H <= 65535 (host check): fits
#pragma unroll
  for (int r = 0; r < kPre; ++r) {
    const int row = (tid >> 6) + r * (kThreads / 64);
    const float* tile_rows = base + (int64_t)r * (kThreads / 64) * stride;   // uniform
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
    pre[r] = row < nvalid ? *reinterpret_cast<const f32x4*>(tile_rows + lane_off) : z;
  }
}

__device__ __forceinline__ void tile_store(float (*Ts)[kPitch], const f32x4 (&pre)[kPre], float scale, int tid) {
#pragma unroll
  for (int r = 0; r < kPre; ++r) {
    const int f = tid + r * kThreads;
    *reinterpret_cast<f32x4*>(&Ts[f >> 6][(f & 63) * 4]) = pre[r] * scale;
  }
}

__device__ __forceinline__ float clamp_score(float s) { return fminf(fmaxf(s, -kClamp), kClamp); }

// what the text mask adds to the scores of text token j < T of batch b: nothing, -9e15f where it is 0, its own value elsewhere
__device__ __forceinline__ float mask_term(const void* __restrict__ mask, int mask_kind, int b, int T, int j) {
  if (mask_kind == BIATTN_MASK_INT64) {
    const long long m = static_cast<const long long*>(mask)[(int64_t)b * T + j];
    return m == 0 ? kMasked : (float)m;
  }
  if (mask_kind == BIATTN_MASK_F32) {
    const float m = static_cast<const float*>(mask)[(int64_t)b * T + j];
    return m == 0.f ? kMasked : m;
  }
  return 0.f;
}

// acc[i, d] += P[i, j] Ts[j, d] over the tile's 32 rows j: P as the A operand, so the owned token is in the registers and d on
// the lanes
__device__ __forceinline__ void rows_times_tile(const float (*Ts)[kPitch], const f32x16& P, f32x16 (&acc)[kD / 32], int r32, int half) {
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const float* vrow = &Ts[acc_row(v) + 4 * half][r32];
#pragma unroll
    for (int db = 0; db < kD / 32; ++db) acc[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(P[v], vrow[db * 32], acc[db], 0, 0, 0);
  }
}

// dst[b, i, h, d] = acc[i, d] * scale for the wave's tokens below S: the token in the registers, d on the lanes, so rows are
// stored in 128-byte runs
__device__ __forceinline__ void store_rows(float* __restrict__ dst, const f32x16 (&acc)[kD / 32], int64_t b, int h, int64_t E, int S,
                                           int i_wave, float scale, int r32, int half) {
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int i = i_wave + acc_row(v) + 4 * half;
    if (i < S) {
      float* o = dst + (b * S + i) * E + h * kD + r32;
#pragma unroll
      for (int db = 0; db < kD / 32; ++db) o[db * 32] = acc[db][v] * scale;
    }
  }
}

// The NC ranges of a text token's forward statistics, combined in range order: M = the largest of the running maxima m_c
// (row kD of a slab) and L = the sum of l_c w_c (row kD + 1) with w_c = exp(m_c - M).  `slab` is range 0's at the token's
// column, the ranges `step` floats apart; each(c, w_c) is called in the same order for what else is summed with these weights
// (biattn_combine's accumulator; text_stats has nothing).
struct RangeStats { float M, L; };
template <typename F>
__device__ __forceinline__ RangeStats combine_ranges(const float* slab, int NC, int64_t step, int TP, F each) {
  float M = -INFINITY;
  for (int c = 0; c < NC; ++c) M = fmaxf(M, slab[c * step + (int64_t)kD * TP]);
  float L = 0.f;
  for (int c = 0; c < NC; ++c) {
    const float w = expf(slab[c * step + (int64_t)kD * TP] - M);
    L += slab[c * step + (int64_t)(kD + 1) * TP] * w;
    each(c, w);
  }
  return {M, L};
}

// The image side of the forward, for a grid of (tiles of 128 image tokens, B * H) workgroups of kThreads.  NJ = number of
// 32-token text tiles (T <= 32 NJ).  A wave owns 32 image tokens and streams K, then V_l; all T scores of a token are kept (NJ
// accumulator tiles), clamped, masked, normalised and multiplied as the A operand with the V_l tiles.  STATS: the row's two
// numbers are stored as well, stat_v[bh, 0, i] = the maximum and stat_v[bh, 1, i] = the log of the sum for i < SP = S rounded
// up to 32 (0 for the rows past S, which the backward's text-owner passes read); without it SP and stat_v are not looked at.
// DROP: the normalised probabilities are multiplied by c m_v (philox.hpp) on their way into the product, a tile's keep bits
// drawn as it is taken up; the statistics are those of the undropped softmax.  Without it `drop` is not looked at.
template <int NJ, bool STATS, bool DROP = false>
__device__ __forceinline__ void image_fwd(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ vl,
                                          const void* __restrict__ mask, int mask_kind, int H, int S, int T, int SP, float q_scale,
                                          float* __restrict__ out_v, float* __restrict__ stat_v,
                                          const philox::Dropout& drop = philox::Dropout()) {
  __shared__ __attribute__((aligned(16))) float Ts[kTile][kPitch];
  __shared__ float addv[kMaxT];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r32 = lane & 31, half = lane >> 5;
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const int64_t E = (int64_t)H * kD;
  const int i_wave = blockIdx.x * (4 * kTile) + wv * kTile;

  addv[tid] = tid < T ? mask_term(mask, mask_kind, b, T, tid) : -INFINITY;   // what is added to the scores of text token tid

  f32x4 own[kD / 8];
  {
    const int i = i_wave + r32 < S ? i_wave + r32 : S - 1;   // rows past S repeat the last one; they are not stored
    own_load<kD>(own, q + ((int64_t)b * S + i) * E + h * kD, true, q_scale, half);
  }

  const float* kbase = k + (int64_t)b * T * E + h * kD;
  const float* vbase = vl + (int64_t)b * T * E + h * kD;
  auto rows_of = [&](int jt) { const int n = T - jt * kTile; return n < kTile ? n : kTile; };

  f32x4 pre[kPre];
  tile_load(pre, kbase, E, rows_of(0), tid);
  tile_store(Ts, pre, 1.f, tid);
  __syncthreads();

  f32x16 X[NJ];
#pragma unroll
  for (int jt = 0; jt < NJ; ++jt) {
    zero_acc(X[jt]);
    if (jt + 1 < NJ) tile_load(pre, kbase + (int64_t)(jt + 1) * kTile * E, E, rows_of(jt + 1), tid);
    else tile_load(pre, vbase, E, rows_of(0), tid);
    scores<kD>(Ts, own, X[jt], r32, half);
    __syncthreads();
    tile_store(Ts, pre, 1.f, tid);
    __syncthreads();
  }

  // softmax over the text tokens of the lane's image token: 16 NJ registers here, the other half of the rows 32 lanes away
  float mx = -INFINITY;
#pragma unroll
  for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const float s = clamp_score(X[jt][v]) + addv[jt * kTile + acc_row(v) + 4 * half];
      X[jt][v] = s;
      mx = fmaxf(mx, s);
    }
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  float sum = 0.f;
#pragma unroll
  for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const float p = expf(X[jt][v] - mx);
      X[jt][v] = p;
      sum += p;
    }
  sum += __shfl_xor(sum, 32);
  const float inv = 1.f / sum;

  if constexpr (STATS) {   // the grid covers SP
    if (half == 0 && i_wave + r32 < SP) {
      const bool real = i_wave + r32 < S;
      float* st = stat_v + (int64_t)bh * 2 * SP + i_wave + r32;
      st[0] = real ? mx : 0.f;
      st[SP] = real ? logf(sum) : 0.f;
    }
  }

  f32x16 acc[kD / 32];
  zero_acc(acc);
#pragma unroll
  for (int jt = 0; jt < NJ; ++jt) {
    if (jt + 1 < NJ) tile_load(pre, vbase + (int64_t)(jt + 1) * kTile * E, E, rows_of(jt + 1), tid);
    if constexpr (DROP) {
      const int i = i_wave + r32 < S ? i_wave + r32 : S - 1;
      const uint32_t keep = philox::keep_bits_image_owner(philox::stream_of(drop), drop.threshold, philox::kSideV, bh, i, jt * kTile, half);
      f32x16 P = X[jt] * inv;
#pragma unroll
      for (int v = 0; v < 16; ++v) P[v] *= philox::keep_factor(keep, v, drop.scale);
      rows_times_tile(Ts, P, acc, r32, half);
    } else {
      rows_times_tile(Ts, X[jt] * inv, acc, r32, half);   // normalised before the product, stored unscaled
    }
    if (jt + 1 < NJ) {
      __syncthreads();
      tile_store(Ts, pre, 1.f, tid);
      __syncthreads();
    }
  }
  store_rows(out_v, acc, b, h, E, S, i_wave, 1.f, r32, half);
}

// ---- host side ----------------------------------------------------------------------------------
// 0, or a negative BIATTN_ERR_* (message set)
inline int geometry(int batch, int num_heads, int image_len, int text_len, int head_dim) {
  if (batch < 0 || num_heads <= 0 || image_len <= 0 || text_len <= 0 || head_dim <= 0)
    return msda::set_error(BIATTN_ERR_BAD_DIMS, "biattn: bad dimensions");
  if (head_dim != kD) return msda::set_error(BIATTN_ERR_UNSUPPORTED, "biattn: head_dim must be 256");
  if (text_len > kMaxT) return msda::set_error(BIATTN_ERR_UNSUPPORTED, "biattn: text_len must be at most 256");
  const long long BH = (long long)batch * num_heads;
  if (BH > 65535 || image_len >= (1 << 30) || BH * image_len * head_dim >= (1ll << 42))
    return msda::set_error(BIATTN_ERR_BAD_DIMS, "biattn: problem too large");
  return 0;
}

// What every entry point refuses first, in this order: the geometry and the mask kind, before it looks at a pointer, then a
// null pointer among `ptrs` or a mask kind without a mask
inline int check_args(int batch, int num_heads, int image_len, int text_len, int head_dim, int mask_kind, const void* mask,
                      std::initializer_list<const void*> ptrs) {
  const int rc = geometry(batch, num_heads, image_len, text_len, head_dim);
  if (rc) return rc;
  if (mask_kind != BIATTN_MASK_NONE && mask_kind != BIATTN_MASK_INT64 && mask_kind != BIATTN_MASK_F32)
    return msda::set_error(BIATTN_ERR_UNSUPPORTED, "biattn: unknown mask kind");
  bool null = mask_kind != BIATTN_MASK_NONE && !mask;
  for (const void* ptr : ptrs) null = null || !ptr;
  return null ? msda::set_error(BIATTN_ERR_NULL_POINTER, "biattn: null pointer argument") : 0;
}

// ... and what both forwards refuse next: a workspace smaller than the plan's, which is left in `p`
inline int forward_args(int batch, int num_heads, int image_len, int text_len, int head_dim, int mask_kind, const void* mask,
                        std::initializer_list<const void*> ptrs, size_t workspace_bytes, Plan& p) {
  const int rc = check_args(batch, num_heads, image_len, text_len, head_dim, mask_kind, mask, ptrs);
  if (rc) return rc;
  p = plan((long long)batch * num_heads, image_len, text_len);
  if (workspace_bytes < p.bytes)
    return msda::set_error(BIATTN_ERR_WORKSPACE, "biattn: workspace smaller than biattn_hip_workspace_bytes");
  return 0;
}

// the grid of the image-owner kernels: (tiles of 128 image tokens, B * H)
inline dim3 image_grid(int S, long long BH) { return dim3((unsigned)((S + 4 * kTile - 1) / (4 * kTile)), (unsigned)BH); }

// f(std::integral_constant<int, NJ>) for the smallest NJ of 1 | 2 | 4 | 8 with TP <= 32 NJ: the instantiation of the
// image-side forward that holds all TP / 32 score tiles of a token
template <typename F>
inline void with_nj(int TP, F&& f) {
  const int nj = TP / kTile;
  if (nj <= 1) f(std::integral_constant<int, 1>{});
  else if (nj <= 2) f(std::integral_constant<int, 2>{});
  else if (nj <= 4) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, 8>{});
}

// Enqueues the text side of the forward, biattn_text and biattn_combine (biattn.hip), which the training forward runs
// unchanged; 0 or the launch's HIP error.
// With `drop` the text kernel multiplies its probabilities by c m_l (philox.hpp); the sums and the combine are the same.
int enqueue_text_side(const float* q, const float* k, const float* vv, int H, int S, int T, float q_scale, const Plan& p,
                      long long BH, float* ws, float* out_l, hipStream_t st, const philox::Dropout* drop = nullptr);

// The dropout arguments of the C ABI: a null seed and a probability outside [0, 1) are refused (message set); else `d` is filled
// with the threshold (uint32) llrint(p 2^32) and the scale 1.0f / (1.0f - p).
inline int dropout_args(float dropout_p, const unsigned long long* seed, philox::Dropout& d) {
  if (!seed) return msda::set_error(BIATTN_ERR_NULL_POINTER, "biattn: null seed");
  if (!(dropout_p >= 0.f && dropout_p < 1.f)) return msda::set_error(BIATTN_ERR_BAD_DIMS, "biattn: dropout_p must be in [0, 1)");
  d.seed = seed;
  d.threshold = (uint32_t)llrint((double)dropout_p * 4294967296.0);
  d.scale = 1.0f / (1.0f - dropout_p);
  return 0;
}

}  // namespace biattn
