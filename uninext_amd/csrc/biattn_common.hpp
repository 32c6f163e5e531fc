// What the inference kernels of the bi-directional attention core (biattn.hip) share with its training route (biattn_bwd.hip):
// the constants, the split of S into ranges, the file's own tile pair, the clamp, what the text mask adds to a score, and the
// argument checks of the C ABI (include/biattn_hip.h).  Internal: not part of the C ABI.
#pragma once

#include "../../include/biattn_hip.h"

#include <math.h>

#include "attn_tile.hpp"
#include "launch_glue.hpp"
#include "msda_common.hpp"

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

// the geometry and the mask kind: what every entry point refuses before it looks at a pointer
inline int check_dims(int batch, int num_heads, int image_len, int text_len, int head_dim, int mask_kind) {
  const int rc = geometry(batch, num_heads, image_len, text_len, head_dim);
  if (rc) return rc;
  if (mask_kind != BIATTN_MASK_NONE && mask_kind != BIATTN_MASK_INT64 && mask_kind != BIATTN_MASK_F32)
    return msda::set_error(BIATTN_ERR_UNSUPPORTED, "biattn: unknown mask kind");
  return 0;
}

// Enqueues the text side of the forward, biattn_text and biattn_combine (biattn.hip), which the training forward runs
// unchanged; 0 or the launch's HIP error.
int enqueue_text_side(const float* q, const float* k, const float* vv, int H, int S, int T, float q_scale, const Plan& p,
                      long long BH, float* ws, float* out_l, hipStream_t st);

}  // namespace biattn
