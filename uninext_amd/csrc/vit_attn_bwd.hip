// Training route of the ViT attention core -- see include/patch_embed_hip.h (patch_embed_hip_vit_attn_train_f32,
// patch_embed_hip_vit_attn_backward_f32).  vit_attn.hip's scheme (attn_tile.hpp) with a recomputing backward: no [S, S] tensor is
// ever written, a wave holds one 32 x 32 tile of scores, probabilities and score gradients at a time.
//
//   attn_lse     the forward of vit_attn.hip, text for text, that also stores lse[bh, i] = running max + log(running sum).  (One
//                text for both, one body <D, REL, LSE> behind two thin kernels as dec_attn_launch.hpp has it, moved
//                vit_attn::attn<80, true> from 186 VGPRs to 187, one over its pinned bound, so the inference kernels keep theirs;
//                so did a body that returns the running max and sum through out-parameters and leaves the lse store to the thin
//                kernel, which also moved attn_lse<*> up by 2 - 3; the two share vit_attn_launch.hpp's pieces: Cfg<D>, the pad columns, the relative-position terms, the row store.)
//   (rel_terms)  vit_attn.hip's kernel, launched through vit_attn_launch.hpp, as are its geometry limits.
//   bwd_q        a wave OWNS 32 queries (scaled q and g in registers), K and V tiles are STREAMED.  p = exp(s - lse), dp = g . v,
//                ds = p (dp - delta); dq^T += K^T ds is attn_tile's second product.  The relative-position bins: the height bin of
//                a query is complete when the streamed keys leave a key row, so it is one running register, stored once; the width
//                bins live in a per-wave LDS column block [Wq][32].  Both go to drel[bh, Hq + Wq, SP] (query fastest, like rel), and
//                the table part of dq is added in the epilogue, bins in column order.
//   bwd_kv       a wave OWNS 32 keys (k and v rows in registers), scaled-q and g tiles are STREAMED with lse, delta and the
//                relative-position terms of their queries.  dv^T += G^T p^T, dk^T += (scale Q)^T ds^T.
//   dtables      dTh / dTw: one workgroup per (table row, chunk of bh) sums drel[bh, c, i] q[i, :] in float64 in a fixed order;
//                dtables_reduce adds the chunks in order and rounds once.
//
// Exact fp32 products, every sum in one fixed order, no float atomics, each output element written by exactly one thread.
#include "../../include/patch_embed_hip.h"

#include <math.h>

#include <atomic>

#include "attn_bwd_tile.hpp"
#include "launch_glue.hpp"
#include "msda_common.hpp"
#include "vit_attn_launch.hpp"

namespace vit_attn_bwd {

using namespace vit_attn;             // kTile, kThreads, kGroup, Cfg<D> and the pieces of vit_attn_launch.hpp
using namespace attn_bwd_tile;

constexpr int kMaxTrainW = 256;       // q_w: the width bins of a workgroup, 4 x [q_w][32] floats, stay inside the LDS
constexpr int kChunks = 16;           // float64 partial sums per table entry

// acc[d, lane's token] += r * trow[d] for the lane's d (accumulator layout of attn_tile's second product)
template <int D>
__device__ __forceinline__ void add_table_row(f32x16 (&acc)[Cfg<D>::kDB], float r, const float* __restrict__ trow, int half) {
#pragma unroll
  for (int db = 0; db < Cfg<D>::kDB; ++db)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int d = db * 32 + g4 * 8 + half * 4;
      if (d < D) {
        const f32x4 tv = *reinterpret_cast<const f32x4*>(trow + d);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[db][g4 * 4 + u] = fmaf(r, tv[u], acc[db][g4 * 4 + u]);
      }
    }
}

// ------------------------------------------------------------------------------------------------
// vit_attn::attn with the row log-sum-exp.  grid (B' * heads * NG), NG = groups of 128 queries.  lse: [B' * heads, SP]; the
// entries of queries in [S, SP) (zero rows) are finite.
template <int D, bool REL>
__global__ void __launch_bounds__(kThreads)
attn_lse(const float* __restrict__ qkv, const float* __restrict__ rel, int heads, int S, int Hq, int Wq, unsigned wq_magic, int SP,
         int NG, float scale, float* __restrict__ out, float* __restrict__ lse) {
  using C = Cfg<D>;
  __shared__ __attribute__((aligned(16))) float Ts[kTile][C::kPitch];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r32 = lane & 31, half = lane >> 5;
  const int bh = blockIdx.x / NG, grp = blockIdx.x - bh * NG, b = bh / heads, h = bh - b * heads;
  const int64_t E = (int64_t)heads * D, E3 = 3 * E;
  const int i_wave = grp * kGroup + wv * kTile;
  const bool active = i_wave < S;                                  // wave-uniform
  const int i = i_wave + r32;

  zero_pad_columns<D>(Ts, tid);

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

  if (active && i < S) store_row<D>(out + ((int64_t)b * S + i) * E + h * D, acc, half, 1.f / l_run);
  if (active && half == 0) lse[(int64_t)bh * SP + i] = m_run + logf(l_run);
}

// ------------------------------------------------------------------------------------------------
// The query pass.  grid (B' * heads * NG); dynamic LDS (REL): 4 waves x [Wq][32] floats.  Writes dq (the first third of
// grad_qkv's rows), delta[bh, i] = g_i . o_i for i < SP, and (REL) drel[bh, :, i] for i < SP.
template <int D, bool REL>
__global__ void __launch_bounds__(kThreads)
bwd_q(const float* __restrict__ qkv, const float* __restrict__ rel, const float* __restrict__ th, const float* __restrict__ tw,
      const float* __restrict__ out, const float* __restrict__ lse, const float* __restrict__ gout, int heads, int S, int Hq, int Wq,
      unsigned wq_magic, int SP, int NG, float scale, float* __restrict__ gqkv, float* drel, float* __restrict__ delta) {
  using C = Cfg<D>;
  __shared__ __attribute__((aligned(16))) float Ks[kTile][C::kPitch];
  __shared__ __attribute__((aligned(16))) float Vs[kTile][C::kPitch];
  extern __shared__ float wbins[];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r32 = lane & 31, half = lane >> 5;
  const int bh = blockIdx.x / NG, grp = blockIdx.x - bh * NG, b = bh / heads, h = bh - b * heads;
  const int64_t E = (int64_t)heads * D, E3 = 3 * E;
  const int i_wave = grp * kGroup + wv * kTile;
  const bool active = i_wave < S;                                  // wave-uniform
  const int i = i_wave + r32, ic = i < S ? i : S - 1;

  zero_pad_columns<D>(Ks, tid);   // the second product reads the K tile's columns up to kDP; the V tile's only up to D

  // owned rows: the scaled q as the forward rounds it, g, and delta = g . o (each lane half its floats, then one exchange)
  f32x4 ownq[D / 8], owng[D / 8];
  const int64_t row = (int64_t)b * S + ic;
  const float dl = own_rows<D>(ownq, owng, qkv + row * E3 + h * D, gout + row * E + h * D, out + row * E + h * D, i < S, scale, half);
  float lse_i = 0.f;
  float* wb = REL ? wbins + (wv * Wq) * kTile + r32 : nullptr;     // the wave's width bins of the lane's query: wb[c * 32]
  float* drel_i = REL ? drel + (int64_t)bh * (Hq + Wq) * SP + i : nullptr;
  if (active) {                                                     // i < SP
    lse_i = lse[(int64_t)bh * SP + i];
    if (half == 0) delta[(int64_t)bh * SP + i] = dl;
    if (REL)
      for (int c = half; c < Wq; c += 2) wb[c * kTile] = 0.f;
  }

  const float* kbase = qkv + (int64_t)b * S * E3 + E + h * D;
  const float* vbase = kbase + E;
  const float* relp = REL ? rel + (int64_t)bh * (Hq + Wq) * SP + i : nullptr;
  const int tiles = (S + kTile - 1) / kTile;
  auto rows_of = [&](int t) { const int n = S - t * kTile; return n < kTile ? n : kTile; };

  f32x16 acc[C::kDB];
  zero_acc(acc);
  int cur_h = 0;          // the key row whose height bin is running
  float hacc = 0.f;

  for (int t = 0; t < tiles; ++t) {
    const int nv = rows_of(t);
    __syncthreads();                                                // the tiles of step t - 1 have been read
    {
      f32x4 pre[C::kPre];
      tile_load<D, kThreads>(pre, kbase + (int64_t)t * kTile * E3, E3, nv, tid);
      tile_store<D, kThreads>(Ks, pre, tid);
      tile_load<D, kThreads>(pre, vbase + (int64_t)t * kTile * E3, E3, nv, tid);
      tile_store<D, kThreads>(Vs, pre, tid);
    }
    __syncthreads();
    if (active) {
      f32x16 X, DP;
      zero_acc(X);
      zero_acc(DP);
      float rh[16], rw[16];
      if (REL) {                                                    // tail keys are masked below
#pragma unroll
        for (int v = 0; v < 16; ++v) rel_term(rh[v], rw[v], relp, t * kTile + acc_row(v) + 4 * half, S, Hq, Wq, wq_magic, SP);
      }
      scores<D>(Ks, ownq, X, r32, half);
      scores<D>(Vs, owng, DP, r32, half);
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        float s = X[v];
        if (REL) s = (s + rh[v]) + rw[v];
        const float p = acc_row(v) + 4 * half < nv ? expf(s - lse_i) : 0.f;
        X[v] = p * (DP[v] - dl);                                    // ds
      }
      pv(Ks, X, acc, r32, half);
      if (REL) {
        // both lane halves get the query's 32 values in key order: lo[v] is tile row 8 (v / 4) + v % 4, hi[v] the row 4 below
        float lo[16], hi[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const float o = __shfl_xor(X[v], 32);
          lo[v] = half == 0 ? X[v] : o;
          hi[v] = half == 0 ? o : X[v];
        }
#pragma unroll
        for (int kk = 0; kk < kTile; ++kk) {
          const float val = (kk & 4) ? hi[4 * (kk / 8) + (kk & 3)] : lo[4 * (kk / 8) + (kk & 3)];
          int key = t * kTile + kk;                                 // wave-uniform
          key = key < S ? key : S - 1;                              // tail keys add zeros to the last bins
          const int jh = div_w(key, Wq, wq_magic), jw = key - jh * Wq;
          if (jh != cur_h) {                                        // the keys have left row cur_h: its bin is complete
            if (half == 0) drel_i[(int64_t)cur_h * SP] = hacc;
            hacc = 0.f;
            cur_h = jh;
          }
          hacc += val;
          if (half == 1) wb[jw * kTile] += val;
        }
      }
    }
  }
  if (REL && active && half == 0) drel_i[(int64_t)cur_h * SP] = hacc;   // cur_h == Hq - 1
  __syncthreads();   // the height bins in drel are visible to the other lane half

  if (active) {
#pragma unroll
    for (int db = 0; db < C::kDB; ++db)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[db][v] *= scale;
    if (REL) {
      for (int c = half; c < Wq; c += 2) drel_i[(int64_t)(Hq + c) * SP] = wb[c * kTile];
      const int ih = div_w(ic, Wq, wq_magic), iw = ic - ih * Wq;
      for (int c = 0; c < Hq; ++c) add_table_row<D>(acc, drel_i[(int64_t)c * SP], th + (int64_t)(ih - c + Hq - 1) * D, half);
      for (int c = 0; c < Wq; ++c) add_table_row<D>(acc, wb[c * kTile], tw + (int64_t)(iw - c + Wq - 1) * D, half);
    }
    if (i < S) store_row<D>(gqkv + ((int64_t)b * S + i) * E3 + h * D, acc, half);
  }
}

// ------------------------------------------------------------------------------------------------
// The key pass.  grid (B' * heads * NG).  Writes dk and dv (the second and third third of grad_qkv's rows).  Reads delta, which
// the query pass wrote: the two run in stream order.
template <int D, bool REL>
__global__ void __launch_bounds__(kThreads)
bwd_kv(const float* __restrict__ qkv, const float* __restrict__ rel, const float* __restrict__ lse, const float* __restrict__ delta,
       const float* __restrict__ gout, int heads, int S, int Hq, int Wq, unsigned wq_magic, int SP, int NG, float scale,
       float* __restrict__ gqkv) {
  using C = Cfg<D>;
  __shared__ __attribute__((aligned(16))) float Qs[kTile][C::kPitch];
  __shared__ __attribute__((aligned(16))) float Gs[kTile][C::kPitch];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r32 = lane & 31, half = lane >> 5;
  const int bh = blockIdx.x / NG, grp = blockIdx.x - bh * NG, b = bh / heads, h = bh - b * heads;
  const int64_t E = (int64_t)heads * D, E3 = 3 * E;
  const int j_wave = grp * kGroup + wv * kTile;
  const bool active = j_wave < S;                                  // wave-uniform
  const int j = j_wave + r32, jc = j < S ? j : S - 1;

  zero_pad_columns<D>(Qs, tid);
  zero_pad_columns<D>(Gs, tid);

  f32x4 ownk[D / 8], ownv[D / 8];
  {
    const float* krow = qkv + ((int64_t)b * S + jc) * E3 + E + h * D;
    own_load<D>(ownk, krow, j < S, 1.f, half);
    own_load<D>(ownv, krow + E, j < S, 1.f, half);
  }
  const int jh = div_w(jc, Wq, wq_magic), jw = jc - jh * Wq;
  const float* relh = REL ? rel + ((int64_t)bh * (Hq + Wq) + jh) * SP : nullptr;   // the lane's key's two columns, by query
  const float* relw = REL ? rel + ((int64_t)bh * (Hq + Wq) + Hq + jw) * SP : nullptr;
  const float* lsep = lse + (int64_t)bh * SP;
  const float* delp = delta + (int64_t)bh * SP;

  const float* qbase = qkv + (int64_t)b * S * E3 + h * D;
  const float* gbase = gout + (int64_t)b * S * E + h * D;
  const int tiles = (S + kTile - 1) / kTile;
  auto rows_of = [&](int t) { const int n = S - t * kTile; return n < kTile ? n : kTile; };

  f32x16 acck[C::kDB], accv[C::kDB];
  zero_acc(acck);
  zero_acc(accv);

  for (int t = 0; t < tiles; ++t) {
    const int nv = rows_of(t);
    __syncthreads();                                                // the tiles of step t - 1 have been read
    {
      f32x4 pre[C::kPre];
      stage_scaled<D, kThreads>(Qs, pre, qbase + (int64_t)t * kTile * E3, E3, nv, scale, tid);
      tile_load<D, kThreads>(pre, gbase + (int64_t)t * kTile * E, E, nv, tid);
      tile_store<D, kThreads>(Gs, pre, tid);
    }
    __syncthreads();
    if (active) {
      f32x16 X, DP;
      zero_acc(X);
      zero_acc(DP);
      scores<D>(Qs, ownk, X, r32, half);                            // s^T: the streamed query in the register, the key on the lane
      scores<D>(Gs, ownv, DP, r32, half);
      float dlt[16];
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int row = acc_row(v) + 4 * half, i = t * kTile + row;   // i < SP
        float s = X[v];
        if (REL) s = (s + relh[i]) + relw[i];
        X[v] = (row < nv && j < S) ? expf(s - lsep[i]) : 0.f;       // p^T; queries past S contribute exactly zero
        dlt[v] = delp[i];
      }
      pv(Gs, X, accv, r32, half);
      ds_t(X, DP, dlt);
      pv(Qs, X, acck, r32, half);
    }
  }

  if (active && j < S) {
    float* row = gqkv + ((int64_t)b * S + j) * E3 + E + h * D;
    store_row<D>(row, acck, half);
    store_row<D>(row + E, accv, half);
  }
}

// ------------------------------------------------------------------------------------------------
// dTh[r] = sum_{bh} sum_{(ih, c): ih - c + Hq - 1 = r} sum_iw drel[bh, c, (ih, iw)] q[(ih, iw), :] (unscaled q); dTw likewise with
// the roles of the two axes exchanged.  grid (2 Hq - 1 + 2 Wq - 1, NC): workgroup (r, chunk) sums the bh = chunk, chunk + NC, ..
// in float64: slot s of the workgroup takes the items s, s + kSlots, .. of every bh in order, the slots are added in order.
template <int D>
__global__ void __launch_bounds__(kThreads)
dtables(const float* __restrict__ qkv, const float* __restrict__ drel, int BH, int heads, int S, int Hq, int Wq, int SP, int NC,
        double* __restrict__ part) {
  constexpr int kD4 = D / 4, kSlots = kThreads / kD4;   // float4 columns of a row, and the items a workgroup takes at once
  __shared__ double red[kSlots][D];
  const int tid = threadIdx.x, d4 = tid % kD4, slot = tid / kD4;
  const int R = 2 * Hq - 1 + 2 * Wq - 1, r = blockIdx.x, chunk = blockIdx.y;
  const bool is_h = r < 2 * Hq - 1;
  const int n1 = is_h ? Hq : Wq, n2 = is_h ? Wq : Hq;             // the table's axis, the other axis
  const int off = (is_h ? r : r - (2 * Hq - 1)) - (n1 - 1);       // query coordinate - key coordinate
  const int a0 = off > 0 ? off : 0, na = n1 - (off > 0 ? off : -off), items = na * n2;
  const int64_t E3 = 3 * (int64_t)heads * D;

  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (slot < kSlots) {
    for (int bh = chunk; bh < BH; bh += NC) {
      const int b = bh / heads, h = bh - b * heads;
      const float* dr = drel + (int64_t)bh * (Hq + Wq) * SP;
      const float* qb = qkv + (int64_t)b * S * E3 + h * D + d4 * 4;
      for (int n = slot; n < items; n += kSlots) {
        const int p = n / n2, o = n - p * n2, a = a0 + p, c = a - off;
        const int i = is_h ? a * Wq + o : o * Wq + a;
        const float w = dr[(int64_t)(is_h ? c : Hq + c) * SP + i];
        const f32x4 q4 = *reinterpret_cast<const f32x4*>(qb + (int64_t)i * E3);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = fma((double)w, (double)q4[u], acc[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) red[slot][d4 * 4 + u] = acc[u];
  }
  __syncthreads();
  if (tid < D) {
    double s = 0.0;
    for (int k = 0; k < kSlots; ++k) s += red[k][tid];
    part[((int64_t)chunk * R + r) * D + tid] = s;
  }
}

// grad_th[r, d], grad_tw[r, d] = the chunks' partial sums added in order, rounded once
__global__ void __launch_bounds__(kThreads)
dtables_reduce(const double* __restrict__ part, int RD, int split, int NC, float* __restrict__ grad_th, float* __restrict__ grad_tw) {
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx >= RD) return;
  double s = 0.0;
  for (int c = 0; c < NC; ++c) s += part[(int64_t)c * RD + idx];
  if (idx < split) grad_th[idx] = (float)s;
  else grad_tw[idx - split] = (float)s;
}

// ---- host side ----------------------------------------------------------------------------------
// 0, or a negative PATCH_EMBED_ERR_* (message set): the forward's limits, and q_w inside the width bins' LDS
static int train_geometry(int batch, int num_heads, int q_h, int q_w, int head_dim) {
  const int rc = geometry(batch, num_heads, q_h, q_w, head_dim);
  if (rc) return rc;
  if (q_w > kMaxTrainW) return msda::set_error(PATCH_EMBED_ERR_UNSUPPORTED, "vit_attn_bwd: q_w above 256");
  return 0;
}

struct Layout {   // the backward's workspace: rel | drel | delta | the table partial sums
  size_t rel, drel, delta, part, total;
  int NC;
};

static Layout layout(int batch, int num_heads, int q_h, int q_w, int head_dim) {
  const size_t S = (size_t)q_h * q_w, SP = (S + kTile - 1) / kTile * kTile, BH = (size_t)batch * num_heads;
  const size_t rel = msda::align256(BH * (size_t)(q_h + q_w) * SP * sizeof(float));
  Layout L;
  L.NC = BH < (size_t)kChunks ? (BH ? (int)BH : 1) : kChunks;
  L.rel = 0;
  L.drel = rel;
  L.delta = 2 * rel;
  L.part = L.delta + msda::align256(BH * SP * sizeof(float));
  L.total = L.part + msda::align256((size_t)L.NC * (size_t)(2 * q_h - 1 + 2 * q_w - 1) * head_dim * sizeof(double));
  if (L.total < 256) L.total = 256;
  return L;
}

// the query pass with tables: its width bins may need the opt-in for more than 64 KiB of LDS
template <int D>
static int launch_bwd_q_rel(dim3 grid, hipStream_t st, const float* qkv, const float* rel, const float* th, const float* tw,
                            const float* out, const float* lse, const float* gout, int heads, int S, int Hq, int Wq, unsigned magic,
                            int SP, int NG, float scale, float* gqkv, float* drel, float* delta) {
  static std::atomic<uint64_t> done{0};
  const int bins = 4 * Wq * kTile * (int)sizeof(float);
  if (bins + 2 * kTile * Cfg<D>::kPitch * (int)sizeof(float) > 64 * 1024) {
    const int rc = msda::ensure_dynamic_lds(reinterpret_cast<const void*>(&bwd_q<D, true>), 4 * kMaxTrainW * kTile * (int)sizeof(float), done);
    if (rc) return msda::launch_status(rc);
  }
  hipLaunchKernelGGL((bwd_q<D, true>), grid, dim3(kThreads), bins, st, qkv, rel, th, tw, out, lse, gout, heads, S, Hq, Wq, magic, SP,
                     NG, scale, gqkv, drel, delta);
  return msda::launch_status();
}

}  // namespace vit_attn_bwd

extern "C" {

static const char* g_vit_attn_bwd_last = "";

size_t patch_embed_hip_vit_attn_backward_workspace_bytes(int batch, int num_heads, int q_h, int q_w, int head_dim) {
  if (vit_attn_bwd::train_geometry(batch, num_heads, q_h, q_w, head_dim) != 0) return 0;
  return vit_attn_bwd::layout(batch, num_heads, q_h, q_w, head_dim).total;
}

const char* patch_embed_hip_vit_attn_backward_last_kernel(void) { return g_vit_attn_bwd_last; }

int patch_embed_hip_vit_attn_train_f32(const float* qkv, const float* rel_h_table, const float* rel_w_table, int batch, int num_heads,
                                       int q_h, int q_w, int head_dim, float scale, float* out, float* lse, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  using namespace vit_attn_bwd;
  int rc = train_geometry(batch, num_heads, q_h, q_w, head_dim);
  if (rc) return rc;
  if (batch == 0) return 0;   // nothing to enqueue, no buffer is looked at
  if (!qkv || !out || !lse || !workspace) return msda::set_error(PATCH_EMBED_ERR_NULL_POINTER, "vit_attn_train: null pointer argument");
  if ((rel_h_table == nullptr) != (rel_w_table == nullptr))
    return msda::set_error(PATCH_EMBED_ERR_NULL_POINTER, "vit_attn_train: rel_h_table and rel_w_table go together (both or neither)");
  if (!msda::aligned16({qkv, rel_h_table, rel_w_table, out, lse, workspace}))
    return msda::set_error(PATCH_EMBED_ERR_UNSUPPORTED, "vit_attn_train: pointers must be 16-byte aligned");
  if (workspace_bytes < rel_bytes(batch, num_heads, q_h, q_w))
    return msda::set_error(PATCH_EMBED_ERR_WORKSPACE, "vit_attn_train: workspace smaller than the vit_attn workspace_bytes query answers");

  hipStream_t st = static_cast<hipStream_t>(stream);
  const int S = q_h * q_w, SP = msda::round_up(S, kTile), NG = msda::ceil_div(S, kGroup);
  const unsigned magic = div_magic(q_w);
  const dim3 grid((unsigned)((long long)batch * num_heads * NG)), block(kThreads);
  float* ws = static_cast<float*>(workspace);

#define VIT_TRAIN_LAUNCH(D)                                                                                                       \
  do {                                                                                                                            \
    if (rel_h_table) {                                                                                                            \
      if ((rc = launch_rel_terms(D, st, qkv, rel_h_table, rel_w_table, batch, num_heads, q_h, q_w, ws))) return rc;     \
      hipLaunchKernelGGL((attn_lse<D, true>), grid, block, 0, st, qkv, (const float*)ws, num_heads, S, q_h, q_w, magic, SP, NG,   \
                         scale, out, lse);                                                                                        \
    } else {                                                                                                                      \
      hipLaunchKernelGGL((attn_lse<D, false>), grid, block, 0, st, qkv, (const float*)nullptr, num_heads, S, q_h, q_w, magic, SP, \
                         NG, scale, out, lse);                                                                                    \
    }                                                                                                                             \
  } while (0)
  if (head_dim == 64) VIT_TRAIN_LAUNCH(64);
  else VIT_TRAIN_LAUNCH(80);
#undef VIT_TRAIN_LAUNCH
  return msda::launch_status();
}

int patch_embed_hip_vit_attn_backward_f32(const float* qkv, const float* rel_h_table, const float* rel_w_table, const float* out,
                                          const float* lse, const float* grad_out, int batch, int num_heads, int q_h, int q_w,
                                          int head_dim, float scale, float* grad_qkv, float* grad_rel_h_table, float* grad_rel_w_table,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  using namespace vit_attn_bwd;
  int rc = train_geometry(batch, num_heads, q_h, q_w, head_dim);
  if (rc) return rc;
  if (batch == 0) return 0;   // nothing to enqueue, no buffer is looked at
  const bool has_rel = rel_h_table != nullptr;
  if (!qkv || !out || !lse || !grad_out || !grad_qkv || !workspace)
    return msda::set_error(PATCH_EMBED_ERR_NULL_POINTER, "vit_attn_backward: null pointer argument");
  if ((rel_h_table == nullptr) != (rel_w_table == nullptr))
    return msda::set_error(PATCH_EMBED_ERR_NULL_POINTER, "vit_attn_backward: rel_h_table and rel_w_table go together (both or neither)");
  if (has_rel && (!grad_rel_h_table || !grad_rel_w_table))
    return msda::set_error(PATCH_EMBED_ERR_NULL_POINTER, "vit_attn_backward: tables need grad_rel_h_table and grad_rel_w_table");
  if (!msda::aligned16({qkv, rel_h_table, rel_w_table, out, lse, grad_out, grad_qkv, grad_rel_h_table, grad_rel_w_table, workspace}))
    return msda::set_error(PATCH_EMBED_ERR_UNSUPPORTED, "vit_attn_backward: pointers must be 16-byte aligned");
  const Layout L = layout(batch, num_heads, q_h, q_w, head_dim);
  if (workspace_bytes < L.total)
    return msda::set_error(PATCH_EMBED_ERR_WORKSPACE, "vit_attn_backward: workspace smaller than the workspace_bytes query answers");

  hipStream_t st = static_cast<hipStream_t>(stream);
  const int S = q_h * q_w, SP = msda::round_up(S, kTile), NG = msda::ceil_div(S, kGroup), BH = batch * num_heads;
  const unsigned magic = div_magic(q_w);
  const dim3 grid((unsigned)((long long)BH * NG)), block(kThreads);
  char* base = static_cast<char*>(workspace);
  float* rel = reinterpret_cast<float*>(base + L.rel);
  float* drel = reinterpret_cast<float*>(base + L.drel);
  float* delta = reinterpret_cast<float*>(base + L.delta);
  double* part = reinterpret_cast<double*>(base + L.part);
  const int R = 2 * q_h - 1 + 2 * q_w - 1;

#define VIT_BWD_LAUNCH(D)                                                                                                         \
  do {                                                                                                                            \
    if (has_rel) {                                                                                                                \
      if ((rc = launch_rel_terms(D, st, qkv, rel_h_table, rel_w_table, batch, num_heads, q_h, q_w, rel))) return rc;    \
      if ((rc = launch_bwd_q_rel<D>(grid, st, qkv, rel, rel_h_table, rel_w_table, out, lse, grad_out, num_heads, S, q_h, q_w, magic,    \
                                    SP, NG, scale, grad_qkv, drel, delta)))                                                       \
        return rc;                                                                                                                \
      hipLaunchKernelGGL((bwd_kv<D, true>), grid, block, 0, st, qkv, (const float*)rel, lse, (const float*)delta, grad_out, num_heads,  \
                         S, q_h, q_w, magic, SP, NG, scale, grad_qkv);                                                            \
      if ((rc = msda::launch_status())) return rc;                                                                                \
      hipLaunchKernelGGL(dtables<D>, dim3(R, L.NC), block, 0, st, qkv, (const float*)drel, BH, num_heads, S, q_h, q_w, SP, L.NC, part); \
      if ((rc = msda::launch_status())) return rc;                                                                                \
      hipLaunchKernelGGL(dtables_reduce, dim3(msda::ceil_div(R * D, kThreads)), block, 0, st, (const double*)part, R * D,         \
                         (2 * q_h - 1) * D, L.NC, grad_rel_h_table, grad_rel_w_table);                                            \
    } else {                                                                                                                      \
      hipLaunchKernelGGL((bwd_q<D, false>), grid, block, 0, st, qkv, (const float*)nullptr, (const float*)nullptr,                \
                         (const float*)nullptr, out, lse, grad_out, num_heads, S, q_h, q_w, magic, SP, NG, scale, grad_qkv,       \
                         (float*)nullptr, delta);                                                                                 \
      if ((rc = msda::launch_status())) return rc;                                                                                \
      hipLaunchKernelGGL((bwd_kv<D, false>), grid, block, 0, st, qkv, (const float*)nullptr, lse, (const float*)delta, grad_out,  \
                         num_heads, S, q_h, q_w, magic, SP, NG, scale, grad_qkv);                                                 \
    }                                                                                                                             \
  } while (0)
  if (head_dim == 64) VIT_BWD_LAUNCH(64);
  else VIT_BWD_LAUNCH(80);
#undef VIT_BWD_LAUNCH
  if ((rc = msda::launch_status())) return rc;
  g_vit_attn_bwd_last = has_rel ? (head_dim == 64 ? "vit_rel<64>+vit_bwd_q<64,rel>+vit_bwd_kv<64,rel>+vit_bwd_tables<64>"
                                                  : "vit_rel<80>+vit_bwd_q<80,rel>+vit_bwd_kv<80,rel>+vit_bwd_tables<80>")
                                : (head_dim == 64 ? "vit_bwd_q<64>+vit_bwd_kv<64>" : "vit_bwd_q<80>+vit_bwd_kv<80>");
  return 0;
}

}  // extern "C"
