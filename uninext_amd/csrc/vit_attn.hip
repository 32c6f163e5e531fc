// Fused attention core of the ViTDet-style ViT blocks with decomposed relative positions -- see include/patch_embed_hip.h
// (patch_embed_hip_vit_attn_f32).
//
// The streamed-attention tile scheme (attn_tile.hpp) as self-attention: a wave OWNS 32 queries of one (b, h), and the keys, then
// the values, of the same (b, h) are STREAMED through LDS, one running softmax with rescaling over all of them.  The [S, S]
// scores exist only as one 32 x 32 tile per wave.
//
// Decomposed relative positions: rel_terms writes rel[bh, c, i] = q[i, :] . table row (unscaled q; c < Hq: the height table's row
// ih - c + Hq - 1, c >= Hq: the width table's row iw - (c - Hq) + Wq - 1) to the workspace, query fastest.  In a score tile the
// key (jh, jw) of a register is the same for all queries of a lane half, so the two terms are two coalesced loads per register:
// column jh and column Hq + jw of the lane's query.
//
// Exact fp32 products, fp32 accumulation in a fixed order, no float atomics, one workgroup per 128 queries over ALL keys (no
// split of the key range, nothing to combine).  Key tails are excluded from max and sum (-inf), their value rows are zero.
//
// The tile configuration Cfg<D>, the pad columns' zero-fill, div_w, rel_term and store_row are in vit_attn_launch.hpp, which the
// training route (vit_attn_bwd.hip: the same forward with the row log-sum-exp, and the recomputing backward) shares.
#include "../../include/patch_embed_hip.h"

#include <math.h>

#include "attn_tile.hpp"
#include "launch_glue.hpp"
#include "msda_common.hpp"
#include "vit_attn_launch.hpp"

namespace vit_attn {

constexpr int kMaxSide = 4095;        // q_h, q_w
constexpr int kMaxTokens = 1 << 20;   // q_h * q_w

// ------------------------------------------------------------------------------------------------
// grid (B' * heads * NG), NG = groups of 128 queries.  rel: [B' * heads, Hq + Wq, SP], SP = S rounded up to 32 (see the top).
template <int D, bool REL>
__global__ void __launch_bounds__(kThreads)
attn(const float* __restrict__ qkv, const float* __restrict__ rel, int heads, int S, int Hq, int Wq, unsigned wq_magic, int SP,
     int NG, float scale, float* __restrict__ out) {
  using C = Cfg<D>;
  __shared__ __attribute__((aligned(16))) float Ts[kTile][C::kPitch];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r32 = lane & 31, half = lane >> 5;
  const int bh = blockIdx.x / NG, grp = blockIdx.x - bh * NG, b = bh / heads, h = bh - b * heads;
  const int64_t E = (int64_t)heads * D, E3 = 3 * E;
  const int i_wave = grp * kGroup + wv * kTile;
  const bool active = i_wave < S;                                  // wave-uniform
  const int i = i_wave + r32;

  zero_pad_columns<D>(Ts, tid);   // the second product reads the V tile's columns up to kDP

  // the owned query's row, scaled first (in fp32, as the module does).  Queries past S are zero rows; they are not stored.
  f32x4 own[D / 8];
  {
    const float* row = qkv + ((int64_t)b * S + (i < S ? i : S - 1)) * E3 + h * D;
#pragma unroll
    for (int ss = 0; ss < D / 8; ++ss) own[ss] = own_part(row, i < S, scale, half, ss);
  }

  const float* kbase = qkv + (int64_t)b * S * E3 + E + h * D;
  const float* vbase = kbase + E;
  const float* relp = REL ? rel + (int64_t)bh * (Hq + Wq) * SP + i : nullptr;   // i < SP in every active wave
  const int tiles = (S + kTile - 1) / kTile;
  auto rows_of = [&](int t) { const int n = S - t * kTile; return n < kTile ? n : kTile; };

  float m_run = -INFINITY, l_run = 0.f;
  f32x16 acc[C::kDB];
#pragma unroll
  for (int db = 0; db < C::kDB; ++db)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[db][v] = 0.f;

  f32x4 pre[C::kPre];
  tile_load<D, kThreads>(pre, kbase, E3, rows_of(0), tid);
  tile_store<D, kThreads>(Ts, pre, tid);
  __syncthreads();

  for (int t = 0; t < tiles; ++t) {
    const int nv = rows_of(t);
    tile_load<D, kThreads>(pre, vbase + (int64_t)t * kTile * E3, E3, nv, tid);
    f32x16 X;
#pragma unroll
    for (int v = 0; v < 16; ++v) X[v] = 0.f;
    if (active) {
      float rh[16], rw[16];
      if (REL) {                                                    // tail keys are masked below
#pragma unroll
        for (int v = 0; v < 16; ++v) rel_term(rh[v], rw[v], relp, t * kTile + acc_row(v) + 4 * half, S, Hq, Wq, wq_magic, SP);
      }
#pragma unroll
      for (int ss = 0; ss < D / 8; ++ss) score_step(Ts, own[ss], X, r32, half, ss);
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        float s = X[v];
        if (REL) s = (s + rh[v]) + rw[v];
        X[v] = acc_row(v) + 4 * half < nv ? s : -INFINITY;
      }
      rescale(acc, softmax_step<false, false>(X, m_run, l_run));   // the max is finite: every tile has a valid key
    }
    __syncthreads();
    tile_store<D, kThreads>(Ts, pre, tid);
    __syncthreads();
    if (t + 1 < tiles) tile_load<D, kThreads>(pre, kbase + (int64_t)(t + 1) * kTile * E3, E3, rows_of(t + 1), tid);
    if (active) pv(Ts, X, acc, r32, half);
    __syncthreads();
    if (t + 1 < tiles) tile_store<D, kThreads>(Ts, pre, tid);
    __syncthreads();
  }

  // out[i, h D + d]
  if (active && i < S) store_row<D>(out + ((int64_t)b * S + i) * E + h * D, acc, half, 1.f / l_run);
}

// ------------------------------------------------------------------------------------------------
// grid (B' * heads * NG).  A thread keeps one query's unscaled row in registers and writes every second column of
// rel[bh, :, i] (threads 0..127: even columns, 128..255: odd); each dot product is one fmaf chain in d order.  Queries in
// [S, SP) get zeros.
template <int D>
__global__ void __launch_bounds__(kThreads)
rel_terms(const float* __restrict__ qkv, const float* __restrict__ th, const float* __restrict__ tw, int heads, int S, int Hq, int Wq,
    unsigned wq_magic, int SP, int NG, float* __restrict__ ws) {
  const int tid = threadIdx.x;
  const int bh = blockIdx.x / NG, grp = blockIdx.x - bh * NG, b = bh / heads, h = bh - b * heads;
  const int i = grp * kGroup + (tid & (kGroup - 1));
  if (i >= SP) return;
  const int64_t E3 = 3 * (int64_t)heads * D;
  const int ic = i < S ? i : S - 1;
  const int ih = div_w(ic, Wq, wq_magic), iw = ic - ih * Wq;

  f32x4 q[D / 4];
  {
    const float* row = qkv + ((int64_t)b * S + ic) * E3 + h * D;
#pragma unroll
    for (int c = 0; c < D / 4; ++c) {
      f32x4 z = {0.f, 0.f, 0.f, 0.f};
      q[c] = i < S ? *reinterpret_cast<const f32x4*>(row + c * 4) : z;
    }
  }
  float* dst = ws + (int64_t)bh * (Hq + Wq) * SP + i;
  for (int c = tid / kGroup; c < Hq + Wq; c += kThreads / kGroup) {
    const float* trow = c < Hq ? th + (int64_t)(ih - c + Hq - 1) * D : tw + (int64_t)(iw - (c - Hq) + Wq - 1) * D;
    float s = 0.f;
#pragma unroll
    for (int c4 = 0; c4 < D / 4; ++c4) {
      const f32x4 tv = *reinterpret_cast<const f32x4*>(trow + c4 * 4);
#pragma unroll
      for (int u = 0; u < 4; ++u) s = fmaf(q[c4][u], tv[u], s);
    }
    dst[(int64_t)c * SP] = s;
  }
}

// ---- host side: declared in vit_attn_launch.hpp ------------------------------------------------
int geometry(int batch, int num_heads, int q_h, int q_w, int head_dim) {
  if (batch < 0 || num_heads <= 0 || q_h <= 0 || q_w <= 0 || head_dim <= 0)
    return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "vit_attn: bad dimensions");
  if (head_dim != 64 && head_dim != 80) return msda::set_error(PATCH_EMBED_ERR_UNSUPPORTED, "vit_attn: head_dim must be 64 or 80");
  const long long S = (long long)q_h * q_w, BH = (long long)batch * num_heads;
  if (q_h > kMaxSide || q_w > kMaxSide || S > kMaxTokens) return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "vit_attn: problem too large");
  const long long SP = (S + kTile - 1) / kTile * kTile, NG = (S + kGroup - 1) / kGroup;
  if (BH * NG >= (1ll << 31) || (long long)(q_h + q_w) * SP >= (1ll << 31) || BH * (q_h + q_w) * SP >= (1ll << 40) ||
      BH * S * 3 * head_dim >= (1ll << 42))
    return msda::set_error(PATCH_EMBED_ERR_BAD_DIMS, "vit_attn: problem too large");
  return 0;
}

size_t rel_bytes(int batch, int num_heads, int q_h, int q_w) {
  const long long S = (long long)q_h * q_w, SP = (S + kTile - 1) / kTile * kTile;
  const size_t bytes = (size_t)batch * num_heads * (size_t)(q_h + q_w) * (size_t)SP * sizeof(float);
  return bytes < 256 ? 256 : bytes;
}

unsigned div_magic(int q_w) { return q_w == 1 ? 0u : (unsigned)(((1ull << 32) + (unsigned)q_w - 1) / (unsigned)q_w); }

int launch_rel_terms(int head_dim, hipStream_t stream, const float* qkv, const float* rel_h_table, const float* rel_w_table, int batch,
                     int num_heads, int q_h, int q_w, float* rel) {
  const int S = q_h * q_w, SP = msda::round_up(S, kTile), NG = msda::ceil_div(S, kGroup);
  const dim3 grid((unsigned)((long long)batch * num_heads * NG)), block(kThreads);
  if (head_dim == 64)
    hipLaunchKernelGGL(rel_terms<64>, grid, block, 0, stream, qkv, rel_h_table, rel_w_table, num_heads, S, q_h, q_w, div_magic(q_w), SP, NG, rel);
  else
    hipLaunchKernelGGL(rel_terms<80>, grid, block, 0, stream, qkv, rel_h_table, rel_w_table, num_heads, S, q_h, q_w, div_magic(q_w), SP, NG, rel);
  return msda::launch_status();
}

}  // namespace vit_attn

extern "C" {

static const char* g_vit_attn_last = "";

size_t patch_embed_hip_vit_attn_workspace_bytes(int batch, int num_heads, int q_h, int q_w, int head_dim) {
  if (vit_attn::geometry(batch, num_heads, q_h, q_w, head_dim) != 0) return 0;
  return vit_attn::rel_bytes(batch, num_heads, q_h, q_w);
}

const char* patch_embed_hip_vit_attn_last_kernel(void) { return g_vit_attn_last; }

int patch_embed_hip_vit_attn_f32(const float* qkv, const float* rel_h_table, const float* rel_w_table, int batch, int num_heads,
                                 int q_h, int q_w, int head_dim, float scale, float* out, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  using namespace vit_attn;
  int rc = vit_attn::geometry(batch, num_heads, q_h, q_w, head_dim);
  if (rc) return rc;
  if (batch == 0) return 0;   // nothing to enqueue, no buffer is looked at
  if (!qkv || !out || !workspace) return msda::set_error(PATCH_EMBED_ERR_NULL_POINTER, "vit_attn: null pointer argument");
  if ((rel_h_table == nullptr) != (rel_w_table == nullptr))
    return msda::set_error(PATCH_EMBED_ERR_NULL_POINTER, "vit_attn: rel_h_table and rel_w_table go together (both or neither)");
  if (!msda::aligned16({qkv, rel_h_table, rel_w_table, out, workspace}))
    return msda::set_error(PATCH_EMBED_ERR_UNSUPPORTED, "vit_attn: pointers must be 16-byte aligned");
  if (workspace_bytes < vit_attn::rel_bytes(batch, num_heads, q_h, q_w))
    return msda::set_error(PATCH_EMBED_ERR_WORKSPACE, "vit_attn: workspace smaller than the workspace_bytes query answers");

  hipStream_t st = static_cast<hipStream_t>(stream);
  const int S = q_h * q_w, SP = msda::round_up(S, kTile), NG = msda::ceil_div(S, kGroup);
  const unsigned magic = div_magic(q_w);
  const dim3 grid((unsigned)((long long)batch * num_heads * NG)), block(kThreads);
  float* ws = static_cast<float*>(workspace);
  const bool has_rel = rel_h_table != nullptr;

#define VIT_ATTN_LAUNCH(D)                                                                                                        \
  do {                                                                                                                            \
    if (has_rel) {                                                                                                                \
      if ((rc = launch_rel_terms(D, st, qkv, rel_h_table, rel_w_table, batch, num_heads, q_h, q_w, ws))) return rc;                     \
      hipLaunchKernelGGL((attn<D, true>), grid, block, 0, st, qkv, (const float*)ws, num_heads, S, q_h, q_w, magic, SP, NG, scale, \
                         out);                                                                                                    \
    } else {                                                                                                                      \
      hipLaunchKernelGGL((attn<D, false>), grid, block, 0, st, qkv, (const float*)nullptr, num_heads, S, q_h, q_w, magic, SP, NG, \
                         scale, out);                                                                                             \
    }                                                                                                                             \
  } while (0)
  if (head_dim == 64) VIT_ATTN_LAUNCH(64);
  else VIT_ATTN_LAUNCH(80);
#undef VIT_ATTN_LAUNCH
  if ((rc = msda::launch_status())) return rc;
  g_vit_attn_last = has_rel ? (head_dim == 64 ? "vit_rel<64>+vit_attn<64,rel>" : "vit_rel<80>+vit_attn<80,rel>")
                            : (head_dim == 64 ? "vit_attn<64>" : "vit_attn<80>");
  return 0;
}

}  // extern "C"
