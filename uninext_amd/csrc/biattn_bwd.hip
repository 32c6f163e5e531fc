// Training route of the bi-directional attention core of the early vision-language fusion layer -- see include/biattn_hip.h
// (biattn_hip_train_f32, biattn_hip_backward_f32).  biattn.hip's scheme (attn_tile.hpp, head dimension 256, both clamps, the
// [B, T] text mask) with a recomputing backward after dec_attn_bwd.hip: nothing of size B * H * S * T is ever written, the
// probabilities of both directions are recomputed from the scores and two numbers per row (the maximum and the log of the sum).
//
//   image_train    a thin kernel around biattn_common.hpp's image_fwd, the ONE text of the image side, with the row statistics on;
//                  biattn_image is the other, so out_v has the same bits.  The text side of the training forward is
//                  biattn.hip's own (biattn::enqueue_text_side), and
//   text_stats     reads M[j] and log L[j] off its workspace through the range combine that biattn_combine uses.
//   row_dots       delta_v[i] = g_v[i] . out_v[i] and delta_l[j] = g_l[j] . out_l[j], a wave per row.
//   bwd_image<VV>  biattn_image's grid: a wave OWNS 32 image tokens, qs in its registers, and takes the text tokens tile by tile in
//                  a runtime loop.  With the row's two numbers kept by the forward a tile of r needs no other tile, so nothing
//                  is held for all T and one kernel serves every T.  Per tile of 32 text tokens:
//                    VV = false   r from the K tile; dr = [-50000 <= r <= 50000] (p_v (g_v . vl - delta_v) + p_l (g_l . vv - delta_l))
//                                 from a V_l and a G_l tile; dq += dr K, scaled by q_scale at the end
//                    VV = true    r from the K tile; p_l; dvv += p_l^T G_l
//                  The products with dr or p_l as the A operand are the forward's second half (rows_times_tile).  dq
//                  and dvv are two kernels because each accumulator is 128 of the 256 AGPRs and r, dp tiles need the rest.
//   bwd_text<M>    biattn_text's grid and ranges: a wave OWNS 32 text tokens (k in its registers), Q (scaled) and one more tile
//                  are STREAMED.
//                    M = 0   stream Q, G_v                       dvl^T += G_v^T p_v
//                    M = 1   stream Q, G_v, the vl row read      dk^T  += Q^T [gate] ds_v
//                    M = 2   stream Q, V_v, the g_l row read     dk^T  += Q^T [gate] ds_l
//                  dk is two sums because each needs its own second row of the owned token.  Each range's partial goes to the
//                  workspace and
//   bwd_combine    adds the ranges in range order: dvl, and dk = (sum of M = 1) + (sum of M = 2).
//
// At D = 256 an owned row is 128 VGPRs and two of them fill the VGPR half of the register file, so only ONE row of a token is
// owned: the second one a pass needs (g_v and vv in bwd_image<false>, vl or g_l in bwd_text<1 | 2>) is read from memory step by
// step (scores_of_row).  The streamed tiles are loaded, stored to LDS and synchronised before the products start; there is no
// register prefetch of the next tile as in biattn.hip.  NOT MEASURED against a prefetching version.
//
// p_v = exp((a - max) - logsum) and p_l = exp(max(s - M, -50000) - log L) are ONE expression each, used by the image-owner and
// the text-owner kernels alike; r is the same sum in the same order on both sides (the products commute), so both use the same
// gate.  A text-side entry with s - M < -50000 has p_l = exp(-50000 - log L) = 0 in fp32 and adds nothing; the gradient that
// autograd routes through torch.max to the argmax is the sum of ds_l over the row's column, which is analytically zero, so it
// is not imitated.  The mask gets no gradient; an all-masked row of `a` is uniform over T and its ds_v is NOT zero.
//
// Exact fp32 products, every sum in one fixed order, no float atomics, each output element written by exactly one thread.
//
// Attention dropout (biattn_hip_train_dropout_f32, biattn_hip_backward_dropout_f32): a DROP template parameter on the same
// texts -- image_fwd, biattn.hip's text_fwd, and image_pass / text_pass here, which bwd_image<VV> / bwd_text<M> and their
// *_dropout twins wrap as thin kernels, so the kernels without dropout keep their names and registers.  The keep decisions
// are philox.hpp's, a pure function of (seed, offset, side, b * heads + h, i, j) that the forward and every backward pass
// recompute; a tile's 16 decisions of a lane are drawn as 16 bits before its scores.  dropout_keep writes them out for tests.
//
// Resources (hipcc -O3 --offload-arch=gfx950, tools/kernel_resources.py): scratch 0 in all; the figures are pinned in
// tests/test_biattn_bwd_resources_cpu.py and tests/test_vlfuse_dropout_cpu.py and listed in DESIGN.md.
#include "attn_bwd_tile.hpp"
#include "biattn_common.hpp"
#include "wave_ops.hpp"

namespace biattn_bwd {

using namespace biattn;
using attn_bwd_tile::ds_t;

// The two probabilities, as every kernel of this file takes them.
__device__ __forceinline__ float prob_v(float r, float add, float mx, float logsum) { return expf((clamp_score(r) + add - mx) - logsum); }
__device__ __forceinline__ float prob_l(float r, float M, float logL) { return expf(fmaxf(clamp_score(r) - M, -kClamp) - logL); }
// torch.clamp passes the gradient at both ends
__device__ __forceinline__ bool gate(float r) { return r >= -kClamp && r <= kClamp; }

// ------------------------------------------------------------------------------------------------
// The image side of the training forward: image_fwd (biattn_common.hpp) with the row statistics.  grid (tiles of 128 image
// tokens, B * H).  stat_v: [B * H, 2, SP].
template <int NJ>
__global__ void __launch_bounds__(kThreads)
image_train(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ vl, const void* __restrict__ mask,
            int mask_kind, int H, int S, int T, int SP, float q_scale, float* __restrict__ out_v, float* __restrict__ stat_v) {
  image_fwd<NJ, true>(q, k, vl, mask, mask_kind, H, S, T, SP, q_scale, out_v, stat_v);
}

// ... and with dropout on p_v (biattn_hip_train_dropout_f32): the same text, the statistics bitwise the same.
template <int NJ>
__global__ void __launch_bounds__(kThreads)
image_train_dropout(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ vl,
                    const void* __restrict__ mask, int mask_kind, int H, int S, int T, int SP, float q_scale,
                    float* __restrict__ out_v, float* __restrict__ stat_v, philox::Dropout drop) {
  image_fwd<NJ, true, true>(q, k, vl, mask, mask_kind, H, S, T, SP, q_scale, out_v, stat_v, drop);
}

// stat_l[bh, 0, j] = M[j], stat_l[bh, 1, j] = log L[j] from the forward's workspace, by biattn_combine's range combine; 0 for the
// columns past T.  One thread per (bh, j < TP).
__global__ void __launch_bounds__(kThreads)
text_stats(const float* __restrict__ ws, int T, int NC, int TP, int64_t total, float* __restrict__ stat_l) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const int j = (int)(idx % TP);
  const int64_t bh = idx / TP;
  float M = 0.f, logL = 0.f;
  if (j < T) {
    const RangeStats s = combine_ranges(ws + bh * NC * (int64_t)(kD + 2) * TP + j, NC, (int64_t)(kD + 2) * TP, TP, [](int, float) {});
    M = s.M;
    logL = logf(s.L);
  }
  stat_l[bh * 2 * TP + j] = M;
  stat_l[(bh * 2 + 1) * TP + j] = logL;
}

// out[bh, n] = g[b, n, h, :] . o[b, n, h, :] for n < N, 0 for N <= n < NP.  A wave per row: each lane its four floats, then a
// butterfly.
__global__ void __launch_bounds__(kThreads)
row_dots(const float* __restrict__ g, const float* __restrict__ o, int H, int N, int NP, int64_t rows, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;                                          // wave-uniform
  const int n = (int)(row % NP);
  const int64_t bh = row / NP, b = bh / H, h = bh - b * H;
  float dl = 0.f;
  if (n < N) {
    const int64_t off = ((b * N + n) * H + h) * kD + lane * 4;
    const f32x4 x = *reinterpret_cast<const f32x4*>(g + off), y = *reinterpret_cast<const f32x4*>(o + off);
#pragma unroll
    for (int u = 0; u < 4; ++u) dl = fmaf(x[u], y[u], dl);
    dl = wave_ops::wave_sum(dl);
  }
  if (lane == 0) out[row] = dl;
}

// attn_tile's scores with the owned row NOT kept: X[streamed row, owned token] += Ts[streamed row, :] . row[:], the lane's share
// of each reduction step read from memory as it is needed.  The row is 1 KB of a tensor that the cache holds, and a step is
// four MFMAs of 64 cycles: where two owned rows and an accumulator do not fit the register file, this one is not owned.
__device__ __forceinline__ void scores_of_row(const float (*Ts)[kPitch], const float* __restrict__ row, bool valid, f32x16& X, int r32,
                                              int half) {
#pragma unroll
  for (int ss = 0; ss < kD / 8; ++ss) {
    if (ss % 8 == 0) __builtin_amdgcn_sched_barrier(0);             // eight steps' operands in flight, not all thirty-two
    score_step(Ts, own_part(row, valid, 1.f, half, ss), X, r32, half, ss);
  }
  __builtin_amdgcn_sched_barrier(0);
}

// ------------------------------------------------------------------------------------------------
// The image-owner passes.  grid (tiles of 128 image tokens, B * H), biattn_image's.  A wave OWNS 32 image tokens (qs in its
// registers) and takes the text tokens tile by tile: with the row's two numbers kept by the forward, a tile of r needs no other
// tile, so -- unlike biattn_image -- nothing is held for all T and one kernel serves every T.  Per tile of 32 text tokens:
//   VV = false   r from the K tile;  dr = [gate] (p_v (g_v . vl - delta_v) + p_l (g_l . vv - delta_l)) from a V_l and a G_l tile
//                (the g_v and vv rows of the token are not owned: scores_of_row);  dq += dr K, scaled by q_scale at the end
//   VV = true    r from the K tile;  p_l;  dvv += p_l^T G_l
// The products with dr or p_l as the A operand are the forward's second half (rows_times_tile): the channel on the lanes.
// DROP (biattn_hip_backward_dropout_f32): g_v . vl and g_l . vv are multiplied by c m_v and c m_l before delta is taken off, and
// p_l by c m_l in dvv; a tile's keep bits (philox.hpp, four calls a side) are drawn before its scores.  Without it `drop` is
// not looked at.
template <bool VV, bool DROP>
__device__ __forceinline__ void
image_pass(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ vv, const float* __restrict__ vl,
          const void* __restrict__ mask, int mask_kind, const float* __restrict__ stat_v, const float* __restrict__ stat_l,
          const float* __restrict__ gv, const float* __restrict__ gl, const float* __restrict__ delta_v,
           const float* __restrict__ delta_l, int H, int S, int T, int SP, int TP, float q_scale, float* __restrict__ dst,
           const philox::Dropout& drop = philox::Dropout()) {
  __shared__ __attribute__((aligned(16))) float Ks[kTile][kPitch];
  __shared__ __attribute__((aligned(16))) float Gs[kTile][kPitch];
  __shared__ __attribute__((aligned(16))) float Vs[VV ? 1 : kTile][kPitch];
  __shared__ float addv[kMaxT], Ml[kMaxT], Ll[kMaxT], Dl[kMaxT];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r32 = lane & 31, half = lane >> 5;
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const int64_t E = (int64_t)H * kD;
  const int i_wave = blockIdx.x * (4 * kTile) + wv * kTile;

  {   // per text token: what the mask adds (-inf past T), M, log L and delta_l
    const int j = tid;
    float a = -INFINITY, m = 0.f, l = 0.f, d = 0.f;
    if (j < T) {
      a = mask_term(mask, mask_kind, b, T, j);
      m = stat_l[(int64_t)bh * 2 * TP + j];
      l = stat_l[((int64_t)bh * 2 + 1) * TP + j];
      d = delta_l[(int64_t)bh * TP + j];
    }
    addv[j] = a;
    Ml[j] = m;
    Ll[j] = l;
    Dl[j] = d;
  }

  // the lane's image token; rows past S repeat the last one and are not stored
  const int ic = i_wave + r32 < S ? i_wave + r32 : S - 1;
  const int64_t row = ((int64_t)b * S + ic) * E + h * kD;
  const float mx = stat_v[(int64_t)bh * 2 * SP + ic], logsum = stat_v[((int64_t)bh * 2 + 1) * SP + ic];
  const float dlv = delta_v[(int64_t)bh * SP + ic];

  const float* kbase = k + (int64_t)b * T * E + h * kD;
  const float* vlbase = vl + (int64_t)b * T * E + h * kD;
  const float* glbase = gl + (int64_t)b * T * E + h * kD;

  f32x4 own[kD / 8];
  own_load<kD>(own, q + row, true, q_scale, half);
  f32x16 acc[kD / 32];
  zero_acc(acc);

  for (int jt = 0; jt * kTile < T; ++jt) {
    const int nv = T - jt * kTile < kTile ? T - jt * kTile : kTile;
    __syncthreads();                                                // the tiles of step jt - 1 have been read (and addv .. Dl written)
    {
      f32x4 pre[kPre];
      tile_load(pre, kbase + (int64_t)jt * kTile * E, E, nv, tid);
      tile_store(Ks, pre, 1.f, tid);
      tile_load(pre, glbase + (int64_t)jt * kTile * E, E, nv, tid);
      tile_store(Gs, pre, 1.f, tid);
      if constexpr (!VV) {
        tile_load(pre, vlbase + (int64_t)jt * kTile * E, E, nv, tid);
        tile_store(Vs, pre, 1.f, tid);
      }
    }
    __syncthreads();

    [[maybe_unused]] uint32_t keep_v = 0, keep_l = 0;
    if constexpr (DROP) {
      const philox::Stream ps = philox::stream_of(drop);
      if constexpr (!VV) keep_v = philox::keep_bits_image_owner(ps, drop.threshold, philox::kSideV, bh, ic, jt * kTile, half);
      keep_l = philox::keep_bits_image_owner(ps, drop.threshold, philox::kSideL, bh, ic, jt * kTile, half);
    }
    f32x16 R;
    zero_acc(R);
    scores<kD>(Ks, own, R, r32, half);
    if constexpr (VV) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int j = jt * kTile + acc_row(v) + 4 * half;
        R[v] = j < T ? prob_l(R[v], Ml[j], Ll[j]) : 0.f;
        if constexpr (DROP) R[v] *= philox::keep_factor(keep_l, v, drop.scale);
      }
      rows_times_tile(Gs, R, acc, r32, half);
    } else {
      f32x16 DPV, DPL;
      zero_acc(DPV);
      zero_acc(DPL);
      // the pointers are opaque in every step, or the compiler hoists both rows out of the loop (256 more registers)
      const float *grow = gv + row, *vrow = vv + row;
      asm volatile("" : "+v"(grow), "+v"(vrow));
      scores_of_row(Vs, grow, true, DPV, r32, half);
      scores_of_row(Gs, vrow, true, DPL, r32, half);
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int j = jt * kTile + acc_row(v) + 4 * half;           // j < 256; past T: p_v = exp(-inf) = 0 and p_l is set to 0
        const float r = R[v];
        if constexpr (DROP) {
          DPV[v] *= philox::keep_factor(keep_v, v, drop.scale);
          DPL[v] *= philox::keep_factor(keep_l, v, drop.scale);
        }
        const float dsv = prob_v(r, addv[j], mx, logsum) * (DPV[v] - dlv);
        const float dsl = (j < T ? prob_l(r, Ml[j], Ll[j]) : 0.f) * (DPL[v] - Dl[j]);
        R[v] = gate(r) ? dsv + dsl : 0.f;
      }
      rows_times_tile(Ks, R, acc, r32, half);
    }
  }
  store_rows(dst, acc, b, h, E, S, i_wave, VV ? 1.f : q_scale, r32, half);
}

#define BIATTN_IMAGE_PASS_PARAMS                                                                                                    \
  const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ vv, const float *__restrict__ vl,            \
      const void *__restrict__ mask, int mask_kind, const float *__restrict__ stat_v, const float *__restrict__ stat_l,            \
      const float *__restrict__ gv, const float *__restrict__ gl, const float *__restrict__ delta_v,                               \
      const float *__restrict__ delta_l, int H, int S, int T, int SP, int TP, float q_scale, float *__restrict__ dst
#define BIATTN_IMAGE_PASS_ARGS q, k, vv, vl, mask, mask_kind, stat_v, stat_l, gv, gl, delta_v, delta_l, H, S, T, SP, TP, q_scale, dst

// The thin kernels around image_pass: without dropout (biattn_hip_backward_f32) and with it.
template <bool VV>
__global__ void __launch_bounds__(kThreads) bwd_image(BIATTN_IMAGE_PASS_PARAMS) {
  image_pass<VV, false>(BIATTN_IMAGE_PASS_ARGS);
}

template <bool VV>
__global__ void __launch_bounds__(kThreads) bwd_image_dropout(BIATTN_IMAGE_PASS_PARAMS, philox::Dropout drop) {
  image_pass<VV, true>(BIATTN_IMAGE_PASS_ARGS, drop);
}

// ------------------------------------------------------------------------------------------------
// The text-owner passes.  grid (NC ranges of S, NG groups of 128 text tokens, B * H), biattn_text's.
//   MODE 0   own2 unused   xs = g_v   dlt = delta_v [B * H, SP]    slab 0: dvl^T
//   MODE 1   own2 = vl     xs = g_v   dlt = delta_v                slab 1: dk^T, the image side's share
//   MODE 2   own2 = g_l    xs = vv    dlt = delta_l [B * H, TP]    slab 2: dk^T, the text side's share
// ws: per (MODE, bh, range) a [kD][TP] slab, the owned text token fastest.
// DROP: MODE 0 multiplies p_v by c m_v, MODE 1 g_v . vl by c m_v and MODE 2 g_l . vv by c m_l before delta is taken off.  The tile
// lies the other way round than the keep decisions are grouped (philox.hpp): sixteen calls a tile, drawn before its scores.
template <int MODE, bool DROP>
__device__ __forceinline__ void
text_pass(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ own2, const float* __restrict__ xs,
         const void* __restrict__ mask, int mask_kind, const float* __restrict__ stat_v, const float* __restrict__ stat_l,
          const float* __restrict__ dlt, int H, int S, int T, int SP, int TP, float q_scale, int NC, float* __restrict__ ws,
          const philox::Dropout& drop = philox::Dropout()) {
  __shared__ __attribute__((aligned(16))) float Qs[kTile][kPitch];
  __shared__ __attribute__((aligned(16))) float Xs[kTile][kPitch];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r32 = lane & 31, half = lane >> 5;
  const int c = blockIdx.x, bh = blockIdx.z, b = bh / H, h = bh - b * H;
  const int64_t E = (int64_t)H * kD;
  const int j0 = (blockIdx.y * 4 + wv) * kTile;
  const bool active = j0 < T;                                       // wave-uniform
  const int j = j0 + r32;
  const bool jv = j < T;
  const int64_t jrow = ((int64_t)b * T + (jv ? j : 0)) * E + h * kD;

  f32x4 ownk[kD / 8];
  own_load<kD>(ownk, k + jrow, jv, 1.f, half);

  // the lane's text token: what the mask adds, or M, log L and delta_l
  float addj = -INFINITY, Mj = 0.f, Lj = 0.f, dlj = 0.f;
  if (jv) {
    if constexpr (MODE == 2) {
      Mj = stat_l[(int64_t)bh * 2 * TP + j];
      Lj = stat_l[((int64_t)bh * 2 + 1) * TP + j];
      dlj = dlt[(int64_t)bh * TP + j];
    } else {
      addj = mask_term(mask, mask_kind, b, T, j);
    }
  }

  const int tiles = (S + kTile - 1) / kTile;
  const int tb = (int)((long long)tiles * c / NC), te = (int)((long long)tiles * (c + 1) / NC);
  const float* qbase = q + (int64_t)b * S * E + h * kD;
  const float* xbase = xs + (int64_t)b * S * E + h * kD;
  const float* mxp = stat_v + (int64_t)bh * 2 * SP;                 // the streamed image tokens' max, log sum and delta_v
  const float* lsp = mxp + SP;
  const float* dvp = dlt + (int64_t)bh * SP;                        // MODE 0, 1 only
  auto rows_of = [&](int t) { const int n = S - t * kTile; return n < kTile ? n : kTile; };

  f32x16 acc[kD / 32];
  zero_acc(acc);

  for (int t = tb; t < te; ++t) {
    const int nv = rows_of(t);
    __syncthreads();                                                // the tiles of step t - 1 have been read
    {
      f32x4 pre[kPre];
      tile_load(pre, qbase + (int64_t)t * kTile * E, E, nv, tid);
      tile_store(Qs, pre, q_scale, tid);
      tile_load(pre, xbase + (int64_t)t * kTile * E, E, nv, tid);
      tile_store(Xs, pre, 1.f, tid);
    }
    __syncthreads();
    if (active) {
      [[maybe_unused]] uint32_t keep = 0;
      if constexpr (DROP)
        keep = philox::keep_bits_text_owner(philox::stream_of(drop), drop.threshold, MODE == 2 ? philox::kSideL : philox::kSideV, bh,
                                            j, t * kTile, half);
      f32x16 X;
      zero_acc(X);
      scores<kD>(Qs, ownk, X, r32, half);                           // r^T: the streamed image token in the register
      if constexpr (MODE == 0) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int row = acc_row(v) + 4 * half, i = t * kTile + row;                 // i < SP
          X[v] = row < nv ? prob_v(X[v], addj, mxp[i], lsp[i]) : 0.f;
          if constexpr (DROP) X[v] *= philox::keep_factor(keep, v, drop.scale);
        }
        pv(Xs, X, acc, r32, half);
      } else {
        f32x16 DP;
        zero_acc(DP);
        scores_of_row(Xs, own2 + jrow, jv, DP, r32, half);
        float dl[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int row = acc_row(v) + 4 * half, i = t * kTile + row;                 // i < SP
          const float r = X[v];
          float p;
          if constexpr (MODE == 1) {
            p = prob_v(r, addj, mxp[i], lsp[i]);
            dl[v] = dvp[i];
          } else {
            p = jv ? prob_l(r, Mj, Lj) : 0.f;
            dl[v] = dlj;
          }
          X[v] = row < nv && gate(r) ? p : 0.f;
          if constexpr (DROP) DP[v] *= philox::keep_factor(keep, v, drop.scale);
        }
        ds_t(X, DP, dl);
        pv(Qs, X, acc, r32, half);
      }
    }
  }

  if (active) {   // biattn_text's slab store, written out in both: as one shared function it cost these kernels 2 - 4 % (profiles/r37)
    float* slab = ws + (((int64_t)MODE * gridDim.z + bh) * NC + c) * kD * TP + j;
#pragma unroll
    for (int db = 0; db < kD / 32; ++db)
#pragma unroll
      for (int v = 0; v < 16; ++v) slab[(int64_t)(db * 32 + acc_row(v) + 4 * half) * TP] = acc[db][v];
  }
}

#define BIATTN_TEXT_PASS_PARAMS                                                                                                     \
  const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ own2, const float *__restrict__ xs,          \
      const void *__restrict__ mask, int mask_kind, const float *__restrict__ stat_v, const float *__restrict__ stat_l,            \
      const float *__restrict__ dlt, int H, int S, int T, int SP, int TP, float q_scale, int NC, float *__restrict__ ws
#define BIATTN_TEXT_PASS_ARGS q, k, own2, xs, mask, mask_kind, stat_v, stat_l, dlt, H, S, T, SP, TP, q_scale, NC, ws

// The thin kernels around text_pass: without dropout (biattn_hip_backward_f32) and with it.
template <int MODE>
__global__ void __launch_bounds__(kThreads) bwd_text(BIATTN_TEXT_PASS_PARAMS) {
  text_pass<MODE, false>(BIATTN_TEXT_PASS_ARGS);
}

template <int MODE>
__global__ void __launch_bounds__(kThreads) bwd_text_dropout(BIATTN_TEXT_PASS_PARAMS, philox::Dropout drop) {
  text_pass<MODE, true>(BIATTN_TEXT_PASS_ARGS, drop);
}

// dvl and dk [b, j, h * 256 + d] from the NC partials of (b, h), in range order.  One thread per (bh, d, j), j fastest.
__global__ void __launch_bounds__(kThreads)
bwd_combine(const float* __restrict__ ws, int H, int T, int NC, int TP, int64_t total, int64_t mode_step, float* __restrict__ dk,
            float* __restrict__ dvl) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const int j = (int)(idx % T);
  const int d = (int)((idx / T) % kD);
  const int64_t bh = idx / ((int64_t)T * kD);
  const int64_t b = bh / H, h = bh - b * H;
  const float* slab = ws + (bh * NC * (int64_t)kD + d) * TP + j;
  const int64_t step = (int64_t)kD * TP;
  float sv = 0.f, s1 = 0.f, s2 = 0.f;
  for (int c = 0; c < NC; ++c) sv += slab[c * step];
  for (int c = 0; c < NC; ++c) s1 += slab[mode_step + c * step];
  for (int c = 0; c < NC; ++c) s2 += slab[2 * mode_step + c * step];
  const int64_t o = (b * T + j) * ((int64_t)H * kD) + h * kD + d;
  dvl[o] = sv;
  dk[o] = s1 + s2;
}

// keep_v[bh, i, j] and keep_l[bh, j, i] as bytes (1 = kept), by the kernels' own decision (philox.hpp): for tests and tools, the
// only place where a mask of size B * H * S * T exists.  One thread per (bh, i, group of four text tokens).
__global__ void __launch_bounds__(kThreads)
dropout_keep(philox::Dropout drop, int S, int T, int64_t total, unsigned char* __restrict__ keep_v, unsigned char* __restrict__ keep_l) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const int NG4 = (T + 3) / 4;
  const int g = (int)(idx % NG4);
  const int i = (int)((idx / NG4) % S);
  const int bh = (int)(idx / ((int64_t)NG4 * S));
  const philox::Stream ps = philox::stream_of(drop);
  const philox::Words wv = philox::entry_words(ps, philox::kSideV, bh, i, g), wl = philox::entry_words(ps, philox::kSideL, bh, i, g);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = 4 * g + t;
    if (j < T) {
      keep_v[((int64_t)bh * S + i) * T + j] = wv.w[t] >= drop.threshold;
      keep_l[((int64_t)bh * T + j) * S + i] = wl.w[t] >= drop.threshold;
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------
struct Layout {                       // the backward's workspace: delta_v | delta_l | the three slab sets, 256 bytes apart
  Plan p;
  int SP;
  size_t delta_v, delta_l, slabs, mode_floats, bytes;
};

static Layout layout(long long BH, int S, int T) {
  Layout w;
  w.p = plan(BH, S, T);
  w.SP = msda::round_up(S, kTile);
  w.delta_v = 0;
  w.delta_l = msda::align256((size_t)BH * w.SP * sizeof(float));
  w.slabs = w.delta_l + msda::align256((size_t)BH * w.p.TP * sizeof(float));
  w.mode_floats = (size_t)BH * w.p.NC * kD * w.p.TP;
  w.bytes = w.slabs + 3 * w.mode_floats * sizeof(float);
  if (w.bytes < 256) w.bytes = 256;
  return w;
}

}  // namespace biattn_bwd

extern "C" {

static const char* g_biattn_bwd_last = "";

size_t biattn_hip_backward_workspace_bytes(int batch, int num_heads, int image_len, int text_len, int head_dim) {
  if (biattn_hip_workspace_bytes(batch, num_heads, image_len, text_len, head_dim) == 0) return 0;
  return biattn_bwd::layout((long long)batch * num_heads, image_len, text_len).bytes;
}

const char* biattn_hip_backward_last_kernel(void) { return g_biattn_bwd_last; }

// Both training forwards: `drop` is null (biattn_hip_train_f32) or the checked dropout arguments.
static int biattn_train(const float* q, const float* k, const float* vv, const float* vl, const void* mask, int mask_kind, int batch,
                        int num_heads, int image_len, int text_len, int head_dim, float q_scale, float* out_v, float* out_l,
                        float* stat_v, float* stat_l, void* workspace, size_t workspace_bytes, void* stream,
                        const philox::Dropout* drop) {
  using namespace biattn_bwd;
  Plan p;
  int rc = forward_args(batch, num_heads, image_len, text_len, head_dim, mask_kind, mask,
                        {q, k, vv, vl, out_v, out_l, stat_v, stat_l, workspace}, workspace_bytes, p);
  const long long BH = (long long)batch * num_heads;
  if (rc || BH == 0) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int S = image_len, T = text_len, H = num_heads, SP = msda::round_up(S, kTile);

  with_nj(p.TP, [&](auto nj) {
    if (drop)
      hipLaunchKernelGGL(image_train_dropout<decltype(nj)::value>, image_grid(S, BH), dim3(kThreads), 0, st, q, k, vl, mask, mask_kind,
                         H, S, T, SP, q_scale, out_v, stat_v, *drop);
    else
      hipLaunchKernelGGL(image_train<decltype(nj)::value>, image_grid(S, BH), dim3(kThreads), 0, st, q, k, vl, mask, mask_kind, H, S,
                         T, SP, q_scale, out_v, stat_v);
  });
  if ((rc = msda::launch_status())) return rc;

  float* ws = static_cast<float*>(workspace);
  if ((rc = enqueue_text_side(q, k, vv, H, S, T, q_scale, p, BH, ws, out_l, st, drop))) return rc;
  const int64_t total = (int64_t)BH * p.TP;
  hipLaunchKernelGGL(text_stats, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, (const float*)ws, T,
                     p.NC, p.TP, total, stat_l);
  return msda::launch_status();
}

int biattn_hip_train_f32(const float* q, const float* k, const float* vv, const float* vl, const void* mask, int mask_kind,
                         int batch, int num_heads, int image_len, int text_len, int head_dim, float q_scale, float* out_v,
                         float* out_l, float* stat_v, float* stat_l, void* workspace, size_t workspace_bytes, void* stream) {
  return biattn_train(q, k, vv, vl, mask, mask_kind, batch, num_heads, image_len, text_len, head_dim, q_scale, out_v, out_l, stat_v,
                      stat_l, workspace, workspace_bytes, stream, nullptr);
}

int biattn_hip_train_dropout_f32(const float* q, const float* k, const float* vv, const float* vl, const void* mask, int mask_kind,
                                 int batch, int num_heads, int image_len, int text_len, int head_dim, float q_scale, float* out_v,
                                 float* out_l, float* stat_v, float* stat_l, void* workspace, size_t workspace_bytes, float dropout_p,
                                 const unsigned long long* seed, void* stream) {
  philox::Dropout drop;
  const int rc = biattn::dropout_args(dropout_p, seed, drop);
  if (rc) return rc;
  return biattn_train(q, k, vv, vl, mask, mask_kind, batch, num_heads, image_len, text_len, head_dim, q_scale, out_v, out_l, stat_v,
                      stat_l, workspace, workspace_bytes, stream, &drop);
}

// Both backwards: `drop` is null (biattn_hip_backward_f32) or the checked dropout arguments.
static int biattn_backward(const float* q, const float* k, const float* vv, const float* vl, const void* mask, int mask_kind,
                           const float* out_v, const float* out_l, const float* stat_v, const float* stat_l,
                           const float* grad_out_v, const float* grad_out_l, int batch, int num_heads, int image_len, int text_len,
                           int head_dim, float q_scale, float* dq, float* dk, float* dvv, float* dvl, void* workspace,
                           size_t workspace_bytes, void* stream, const philox::Dropout* drop) {
  using namespace biattn_bwd;
  int rc = check_args(batch, num_heads, image_len, text_len, head_dim, mask_kind, mask,
                      {q, k, vv, vl, out_v, out_l, stat_v, stat_l, grad_out_v, grad_out_l, dq, dk, dvv, dvl, workspace});
  if (rc) return rc;
  if (!msda::aligned16({q, k, vv, vl, out_v, out_l, stat_v, stat_l, grad_out_v, grad_out_l, dq, dk, dvv, dvl, workspace}))
    return msda::set_error(BIATTN_ERR_UNSUPPORTED, "biattn: every pointer but the mask must be 16-byte aligned");
  const long long BH = (long long)batch * num_heads;
  const Layout w = layout(BH, image_len, text_len);
  if (workspace_bytes < w.bytes)
    return msda::set_error(BIATTN_ERR_WORKSPACE, "biattn: workspace smaller than biattn_hip_backward_workspace_bytes");
  if (BH == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int S = image_len, T = text_len, H = num_heads, SP = w.SP, TP = w.p.TP, NC = w.p.NC;
  char* base = static_cast<char*>(workspace);
  float* delta_v = reinterpret_cast<float*>(base + w.delta_v);
  float* delta_l = reinterpret_cast<float*>(base + w.delta_l);
  float* slabs = reinterpret_cast<float*>(base + w.slabs);

  const int64_t rows_v = (int64_t)BH * SP, rows_l = (int64_t)BH * TP;
  hipLaunchKernelGGL(row_dots, dim3((unsigned)((rows_v + 3) / 4)), dim3(kThreads), 0, st, grad_out_v, out_v, H, S, SP, rows_v, delta_v);
  hipLaunchKernelGGL(row_dots, dim3((unsigned)((rows_l + 3) / 4)), dim3(kThreads), 0, st, grad_out_l, out_l, H, T, TP, rows_l, delta_l);
  if ((rc = msda::launch_status())) return rc;

  const dim3 gi = image_grid(S, BH);
  const dim3 gt((unsigned)NC, (unsigned)w.p.NG, (unsigned)BH);
  const float *dv = delta_v, *dl = delta_l, *none = nullptr;
  if (drop) {
    hipLaunchKernelGGL(bwd_image_dropout<false>, gi, dim3(kThreads), 0, st, q, k, vv, vl, mask, mask_kind, stat_v, stat_l, grad_out_v,
                       grad_out_l, dv, dl, H, S, T, SP, TP, q_scale, dq, *drop);
    hipLaunchKernelGGL(bwd_image_dropout<true>, gi, dim3(kThreads), 0, st, q, k, vv, vl, mask, mask_kind, stat_v, stat_l, grad_out_v,
                       grad_out_l, dv, dl, H, S, T, SP, TP, q_scale, dvv, *drop);
    if ((rc = msda::launch_status())) return rc;
    hipLaunchKernelGGL(bwd_text_dropout<0>, gt, dim3(kThreads), 0, st, q, k, none, grad_out_v, mask, mask_kind, stat_v, stat_l, dv, H,
                       S, T, SP, TP, q_scale, NC, slabs, *drop);
    hipLaunchKernelGGL(bwd_text_dropout<1>, gt, dim3(kThreads), 0, st, q, k, vl, grad_out_v, mask, mask_kind, stat_v, stat_l, dv, H,
                       S, T, SP, TP, q_scale, NC, slabs, *drop);
    hipLaunchKernelGGL(bwd_text_dropout<2>, gt, dim3(kThreads), 0, st, q, k, grad_out_l, vv, mask, mask_kind, stat_v, stat_l, dl, H,
                       S, T, SP, TP, q_scale, NC, slabs, *drop);
  } else {
    hipLaunchKernelGGL(bwd_image<false>, gi, dim3(kThreads), 0, st, q, k, vv, vl, mask, mask_kind, stat_v, stat_l, grad_out_v,
                       grad_out_l, dv, dl, H, S, T, SP, TP, q_scale, dq);
    hipLaunchKernelGGL(bwd_image<true>, gi, dim3(kThreads), 0, st, q, k, vv, vl, mask, mask_kind, stat_v, stat_l, grad_out_v,
                       grad_out_l, dv, dl, H, S, T, SP, TP, q_scale, dvv);
    if ((rc = msda::launch_status())) return rc;
    hipLaunchKernelGGL(bwd_text<0>, gt, dim3(kThreads), 0, st, q, k, none, grad_out_v, mask, mask_kind, stat_v, stat_l, dv, H, S, T, SP,
                       TP, q_scale, NC, slabs);
    hipLaunchKernelGGL(bwd_text<1>, gt, dim3(kThreads), 0, st, q, k, vl, grad_out_v, mask, mask_kind, stat_v, stat_l, dv, H, S, T, SP,
                       TP, q_scale, NC, slabs);
    hipLaunchKernelGGL(bwd_text<2>, gt, dim3(kThreads), 0, st, q, k, grad_out_l, vv, mask, mask_kind, stat_v, stat_l, dl, H, S, T, SP,
                       TP, q_scale, NC, slabs);
  }
  if ((rc = msda::launch_status())) return rc;
  const int64_t total = (int64_t)BH * kD * T;
  hipLaunchKernelGGL(bwd_combine, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, (const float*)slabs, H,
                     T, NC, TP, total, (int64_t)w.mode_floats, dk, dvl);
  if ((rc = msda::launch_status())) return rc;
  g_biattn_bwd_last = drop ? "biattn_row_dots+biattn_bwd_image_dropout<dq>+biattn_bwd_image_dropout<dvv>+biattn_bwd_text_dropout<0,1,2>"
                             "+biattn_bwd_combine"
                           : "biattn_row_dots+biattn_bwd_image<dq>+biattn_bwd_image<dvv>+biattn_bwd_text<0,1,2>+biattn_bwd_combine";
  return 0;
}

int biattn_hip_backward_f32(const float* q, const float* k, const float* vv, const float* vl, const void* mask, int mask_kind,
                            const float* out_v, const float* out_l, const float* stat_v, const float* stat_l,
                            const float* grad_out_v, const float* grad_out_l, int batch, int num_heads, int image_len,
                            int text_len, int head_dim, float q_scale, float* dq, float* dk, float* dvv, float* dvl,
                            void* workspace, size_t workspace_bytes, void* stream) {
  return biattn_backward(q, k, vv, vl, mask, mask_kind, out_v, out_l, stat_v, stat_l, grad_out_v, grad_out_l, batch, num_heads,
                         image_len, text_len, head_dim, q_scale, dq, dk, dvv, dvl, workspace, workspace_bytes, stream, nullptr);
}

int biattn_hip_backward_dropout_f32(const float* q, const float* k, const float* vv, const float* vl, const void* mask, int mask_kind,
                                    const float* out_v, const float* out_l, const float* stat_v, const float* stat_l,
                                    const float* grad_out_v, const float* grad_out_l, int batch, int num_heads, int image_len,
                                    int text_len, int head_dim, float q_scale, float* dq, float* dk, float* dvv, float* dvl,
                                    void* workspace, size_t workspace_bytes, float dropout_p,
                                    const unsigned long long* seed, void* stream) {
  philox::Dropout drop;
  const int rc = biattn::dropout_args(dropout_p, seed, drop);
  if (rc) return rc;
  return biattn_backward(q, k, vv, vl, mask, mask_kind, out_v, out_l, stat_v, stat_l, grad_out_v, grad_out_l, batch, num_heads,
                         image_len, text_len, head_dim, q_scale, dq, dk, dvv, dvl, workspace, workspace_bytes, stream, &drop);
}

int biattn_hip_dropout_keep_u8(const unsigned long long* seed, float dropout_p, int batch, int num_heads, int image_len, int text_len,
                               unsigned char* keep_v, unsigned char* keep_l, void* stream) {
  using namespace biattn_bwd;
  int rc = geometry(batch, num_heads, image_len, text_len, kD);
  if (rc) return rc;
  if (!keep_v || !keep_l) return msda::set_error(BIATTN_ERR_NULL_POINTER, "biattn: null pointer argument");
  philox::Dropout drop;
  if ((rc = dropout_args(dropout_p, seed, drop))) return rc;
  const int64_t total = (int64_t)batch * num_heads * image_len * ((text_len + 3) / 4);
  if (total == 0) return 0;
  if (total > (int64_t)0x7fffffff * kThreads) return msda::set_error(BIATTN_ERR_BAD_DIMS, "biattn: problem too large");
  hipLaunchKernelGGL(dropout_keep, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), drop, image_len, text_len, total, keep_v, keep_l);
  return msda::launch_status();
}

}  // extern "C"
