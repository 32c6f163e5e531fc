// Self-attention core of the decoder layers (nn.MultiheadAttention(256, 8) among the queries) with an [Lq, Lq] mask -- see
// include/biattn_hip.h (biattn_hip_self_forward_f32).
//
// The streamed-attention tile scheme (attn_tile.hpp) as self-attention for head dimension 32: a wave OWNS 32 queries of one
// (b, h), and the keys, then the values, of the same (b, h) are STREAMED through LDS in tiles of 32 rows (4 KB), one running
// softmax with rescaling over them.
//
// The grid.  batch * heads is 16 at the workload (bs 2, 8 heads), so a workgroup takes only 32 queries, and its TWO waves own
// the SAME 32 queries and split the key tiles between them: wave 0 the first ceil(tiles / 2), wave 1 the rest, each through an
// LDS tile of its own.  At the end wave 1 hands its (max, sum, accumulator) over through LDS and wave 0 combines the two in that
// fixed order and stores.  bs 2 x 900 queries: 16 * 29 = 464 workgroups = 928 waves for the card's 1024 SIMDs, each wave over 15
// or 14 key tiles (128 queries per workgroup over all keys, as vit_attn has it, would be 128 workgroups of 29 tiles a wave).
//
// The mask.  Element [i, j] of the lane's query i is loaded per register (a byte, non-zero = -inf, or a float) and ADDED to the
// score in fp32.  What differs from vit_attn:
//   * a query may have seen nothing but excluded keys so far: the running max is -inf, and the exponentials are taken against 0
//     instead (every term is exp(-inf) = 0, the accumulator stays 0), never against -inf (exp(-inf - -inf) is NaN);
//   * a key tile in which no query of the wave has an open key (mask -inf or key past the end) skips both products.  The tile
//     would have left the max and the sum as they are and added 0 * v to the accumulator, so for finite v the result is the
//     same whether it is skipped or not -- a float mask of -inf and a bool mask give the same bits;
//   * a query with EVERY key excluded ends with sum 0 and accumulator 0: 0 * (1 / 0) is NaN in all its channels, as the softmax
//     of a row of -inf is in the PyTorch composition.
//
// Exact fp32 products, fp32 accumulation in a fixed order, no float atomics, nothing of size batch * heads * len * len written.
#include "../../include/biattn_hip.h"

#include <math.h>

#include "attn_tile.hpp"
#include "launch_glue.hpp"
#include "msda_common.hpp"

namespace dec_attn {

using namespace attn_tile;            // kTile = 32: streamed rows per LDS tile, queries per workgroup

constexpr int kD = 32;                // head dimension
constexpr int kWaves = 2;             // key ranges of a workgroup, one wave each
constexpr int kThreads = 64 * kWaves;
constexpr int kPitch = kD + 4;        // floats per LDS row: rows 16-byte aligned, 4-bank step between rows
constexpr int kPre = kTileItems<kD, 64>;   // float4 items of a tile per lane: every wave loads its own tiles
constexpr int kMaxLen = 65535;

// ------------------------------------------------------------------------------------------------
// grid (batch * heads * NG), NG = groups of 32 queries.  MASK: BIATTN_MASK_NONE / _BOOL / _F32.
template <int MASK>
__global__ void __launch_bounds__(kThreads)
attn(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int64_t qs, int64_t ks, int64_t vs,
     const void* __restrict__ mask, int heads, int L, int NG, float scale, float* __restrict__ out) {
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
      if (MASK != BIATTN_MASK_NONE && kr < nv) {
        const size_t at = (size_t)ic * (size_t)L + (size_t)(t * kTile + kr);
        if (MASK == BIATTN_MASK_BOOL) a = static_cast<const unsigned char*>(mask)[at] ? -INFINITY : 0.f;
        else a = static_cast<const float*>(mask)[at];
      }
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
    const float inv = 1.f / (l_run * a0 + l1 * a1);                 // every key excluded: 1 / 0, and 0 * inf below is NaN
    // out[i, h D + d]: d in the registers (four consecutive d per register quad), the query on the lane
    float* o = out + ((int64_t)b * L + i) * ((int64_t)heads * kD) + h * kD;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      f32x4 r;
#pragma unroll
      for (int u = 0; u < 4; ++u) r[u] = (acc[0][g4 * 4 + u] * a0 + Part[g4 * 4 + u][lane] * a1) * inv;
      *reinterpret_cast<f32x4*>(o + g4 * 8 + half * 4) = r;
    }
  }
}

}  // namespace dec_attn

extern "C" {

static const char* g_dec_attn_last = "";

const char* biattn_hip_self_last_kernel(void) { return g_dec_attn_last; }

int biattn_hip_self_forward_f32(const float* q, const float* k, const float* v, long long q_stride, long long k_stride,
                                long long v_stride, const void* mask, int mask_kind, int batch, int num_heads, int len, int head_dim,
                                float q_scale, float* out, void* stream) {
  using namespace dec_attn;
  if (batch < 0 || num_heads <= 0 || len <= 0 || head_dim <= 0)
    return msda::set_error(BIATTN_ERR_BAD_DIMS, "dec_attn: bad dimensions");
  if (len > kMaxLen) return msda::set_error(BIATTN_ERR_BAD_DIMS, "dec_attn: len must be at most 65535");
  if (head_dim != kD) return msda::set_error(BIATTN_ERR_UNSUPPORTED, "dec_attn: head_dim must be 32");
  if (mask_kind != BIATTN_MASK_NONE && mask_kind != BIATTN_MASK_BOOL && mask_kind != BIATTN_MASK_F32)
    return msda::set_error(BIATTN_ERR_UNSUPPORTED, "dec_attn: unknown mask kind (none, bool or fp32)");
  const long long E = (long long)num_heads * kD, NG = msda::ceil_div(len, kTile);
  for (long long s : {q_stride, k_stride, v_stride}) {
    if (s < E) return msda::set_error(BIATTN_ERR_BAD_DIMS, "dec_attn: a row stride is smaller than num_heads * head_dim");
    if (s % 4 != 0) return msda::set_error(BIATTN_ERR_UNSUPPORTED, "dec_attn: row strides must be multiples of 4 floats");
    if (s >= (1ll << 31) || (long long)batch * len * s >= (1ll << 42))
      return msda::set_error(BIATTN_ERR_BAD_DIMS, "dec_attn: problem too large");
  }
  if ((long long)batch * num_heads * NG >= (1ll << 31)) return msda::set_error(BIATTN_ERR_BAD_DIMS, "dec_attn: problem too large");
  if (batch == 0) return 0;   // nothing to enqueue, no buffer is looked at
  if (!q || !k || !v || !out || (mask_kind != BIATTN_MASK_NONE && !mask))
    return msda::set_error(BIATTN_ERR_NULL_POINTER, "dec_attn: null pointer argument");
  if (!msda::aligned16({q, k, v, out}))
    return msda::set_error(BIATTN_ERR_UNSUPPORTED, "dec_attn: q, k, v and out must be 16-byte aligned");
  if (mask_kind == BIATTN_MASK_F32 && reinterpret_cast<uintptr_t>(mask) % 4 != 0)
    return msda::set_error(BIATTN_ERR_UNSUPPORTED, "dec_attn: an fp32 mask must be 4-byte aligned");

  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((long long)batch * num_heads * NG)), block(kThreads);
#define DEC_ATTN_LAUNCH(KIND)                                                                                               \
  hipLaunchKernelGGL(attn<KIND>, grid, block, 0, st, q, k, v, (int64_t)q_stride, (int64_t)k_stride, (int64_t)v_stride, mask, \
                     num_heads, len, (int)NG, q_scale, out)
  if (mask_kind == BIATTN_MASK_NONE) DEC_ATTN_LAUNCH(BIATTN_MASK_NONE);
  else if (mask_kind == BIATTN_MASK_BOOL) DEC_ATTN_LAUNCH(BIATTN_MASK_BOOL);
  else DEC_ATTN_LAUNCH(BIATTN_MASK_F32);
#undef DEC_ATTN_LAUNCH
  if (const int e = msda::launch_status()) return e;
  g_dec_attn_last = mask_kind == BIATTN_MASK_NONE ? "dec_attn<none>" : mask_kind == BIATTN_MASK_BOOL ? "dec_attn<bool>" : "dec_attn<f32>";
  return 0;
}

}  // extern "C"
