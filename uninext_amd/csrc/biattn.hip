// Fused bi-directional attention core of the early vision-language fusion layer -- see include/biattn_hip.h.
//
// Both directions share the score tile s[i, j] = (q[i, :] * q_scale) . k[j, :] and both kernels follow the streamed-attention
// tile scheme (attn_tile.hpp): a wave OWNS 32 tokens of one side, whose operand rows (256 floats each) stay in its registers, and
// the tokens of the other side are STREAMED through LDS in tiles of 32 full rows.
//
//   * biattn_image: a workgroup owns 128 image tokens (32 per wave) of one (b, h) and streams K, then V_l.  All T scores of a
//     token are kept (NJ accumulator tiles), clamped, masked, normalised, and multiplied as the A operand with V_l tiles:
//     out_v[i, d] comes out with d on the lanes, so rows are stored in 128-byte runs.  Its text is biattn_common.hpp's
//     image_fwd, which the training forward (biattn_bwd::image_train) runs as well; the kernel here is a thin one around it.
//   * biattn_text: a wave owns 32 text tokens, a workgroup four such blocks, and streams the image tokens of one range of S:
//     Q tile -> scores -> running max / sum with rescaling -> V_v tile -> out_l^T[d, j] += V_v^T . P (P as the B operand, so
//     the rescale factor of a column is the lane's own).  The partial (max, sum, accumulator) of each range goes to the
//     workspace and biattn_combine adds the ranges in range order.  The number of ranges depends on the shapes only.
//
// Exact fp32 products, fp32 accumulation in a fixed order, no float atomics.  The streamed tile is single-buffered in LDS
// (33 KB); the next tile is fetched into registers while the current one is multiplied.
#include "biattn_common.hpp"

namespace biattn {

// The image side: image_fwd (biattn_common.hpp) without the row statistics.  grid (tiles of 128 image tokens, B * H).
template <int NJ>
__global__ void __launch_bounds__(kThreads)
biattn_image(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ vl, const void* __restrict__ mask,
             int mask_kind, int H, int S, int T, float q_scale, float* __restrict__ out_v) {
  image_fwd<NJ, false>(q, k, vl, mask, mask_kind, H, S, T, 0, q_scale, out_v, nullptr);
}

// ------------------------------------------------------------------------------------------------
// The ONE text of the text side, for a grid of (NC ranges of S, NG groups of 128 text tokens, B * H).  ws: per (bh, range) a
// [kD + 2][TP] slab: rows d < 256 the accumulator out_l^T[d, j], row 256 the running max, row 257 the running sum.
// DROP: the probabilities are multiplied by c m_l (philox.hpp) on their way into the product, a tile's keep bits drawn after
// its V_v tile is staged; the running max and sum are those of the undropped softmax.  Without it `drop` is not looked at.
template <bool DROP>
__device__ __forceinline__ void text_fwd(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ vv, int H,
                                         int S, int T, float q_scale, int NC, int TP, float* __restrict__ ws,
                                         const philox::Dropout& drop = philox::Dropout()) {
  __shared__ __attribute__((aligned(16))) float Ts[kTile][kPitch];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r32 = lane & 31, half = lane >> 5;
  const int c = blockIdx.x, bh = blockIdx.z, b = bh / H, h = bh - b * H;
  const int64_t E = (int64_t)H * kD;
  const int j0 = (blockIdx.y * 4 + wv) * kTile;
  const bool active = j0 < T;                                    // wave-uniform

  f32x4 own[kD / 8];
  {
    const int j = j0 + r32;
    own_load<kD>(own, k + ((int64_t)b * T + (j < T ? j : 0)) * E + h * kD, j < T, 1.f, half);
  }

  const int tiles = (S + kTile - 1) / kTile;
  const int tb = (int)((long long)tiles * c / NC), te = (int)((long long)tiles * (c + 1) / NC);
  const float* qbase = q + (int64_t)b * S * E + h * kD;
  const float* vbase = vv + (int64_t)b * S * E + h * kD;
  auto rows_of = [&](int t) { const int n = S - t * kTile; return n < kTile ? n : kTile; };

  float m_run = -INFINITY, l_run = 0.f;
  f32x16 acc[kD / 32];
#pragma unroll
  for (int db = 0; db < kD / 32; ++db)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[db][v] = 0.f;

  f32x4 pre[kPre];
  if (tb < te) {
    tile_load(pre, qbase + (int64_t)tb * kTile * E, E, rows_of(tb), tid);
    tile_store(Ts, pre, q_scale, tid);
  }
  __syncthreads();

  for (int t = tb; t < te; ++t) {
    const int nv = rows_of(t);
    tile_load(pre, vbase + (int64_t)t * kTile * E, E, nv, tid);
    f32x16 X;
#pragma unroll
    for (int v = 0; v < 16; ++v) X[v] = 0.f;
    if (active) {
      scores<kD>(Ts, own, X, r32, half);
#pragma unroll
      for (int v = 0; v < 16; ++v) X[v] = acc_row(v) + 4 * half < nv ? clamp_score(X[v]) : -INFINITY;
      // the max is finite: every tile has a valid row and scores are clamped
      rescale(acc, softmax_step<false, true>(X, m_run, l_run, kClamp));
    }
    __syncthreads();
    tile_store(Ts, pre, 1.f, tid);
    __syncthreads();
    if constexpr (DROP) {   // here, where neither a staged tile nor the scores' operands are live: the kernel fills the register file
      if (active) {
        const uint32_t keep =
            philox::keep_bits_text_owner(philox::stream_of(drop), drop.threshold, philox::kSideL, bh, j0 + r32, t * kTile, half);
#pragma unroll
        for (int v = 0; v < 16; ++v) X[v] *= philox::keep_factor(keep, v, drop.scale);
      }
    }
    if (t + 1 < te) tile_load(pre, qbase + (int64_t)(t + 1) * kTile * E, E, rows_of(t + 1), tid);
    if (active) pv(Ts, X, acc, r32, half);
    __syncthreads();
    if (t + 1 < te) tile_store(Ts, pre, q_scale, tid);
    __syncthreads();
  }

  if (active) {
    float* slab = ws + ((int64_t)bh * NC + c) * (kD + 2) * TP + j0 + r32;
#pragma unroll
    for (int db = 0; db < kD / 32; ++db)
#pragma unroll
      for (int v = 0; v < 16; ++v) slab[(int64_t)(db * 32 + acc_row(v) + 4 * half) * TP] = acc[db][v];
    if (half == 0) {
      slab[(int64_t)kD * TP] = m_run;
      slab[(int64_t)(kD + 1) * TP] = l_run;
    }
  }
}

// The text side: text_fwd without and with dropout.
__global__ void __launch_bounds__(kThreads)
biattn_text(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ vv, int H, int S, int T,
            float q_scale, int NC, int TP, float* __restrict__ ws) {
  text_fwd<false>(q, k, vv, H, S, T, q_scale, NC, TP, ws);
}

__global__ void __launch_bounds__(kThreads)
biattn_text_dropout(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ vv, int H, int S, int T,
                    float q_scale, int NC, int TP, float* __restrict__ ws, philox::Dropout drop) {
  text_fwd<true>(q, k, vv, H, S, T, q_scale, NC, TP, ws, drop);
}

// out_l[b, j, h * 256 + d] from the NC partials of (b, h), in range order.  One thread per (bh, d, j), j fastest.
__global__ void __launch_bounds__(kThreads)
biattn_combine(const float* __restrict__ ws, int H, int T, int NC, int TP, int64_t total, float* __restrict__ out_l) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const int j = (int)(idx % T);
  const int d = (int)((idx / T) % kD);
  const int64_t bh = idx / ((int64_t)T * kD);
  const int64_t b = bh / H, h = bh - b * H;
  const float* slab = ws + bh * NC * (int64_t)(kD + 2) * TP + j;
  const int64_t step = (int64_t)(kD + 2) * TP;
  float o = 0.f;
  const RangeStats s = combine_ranges(slab, NC, step, TP, [&](int c, float w) { o += slab[c * step + (int64_t)d * TP] * w; });
  out_l[(b * T + j) * ((int64_t)H * kD) + h * kD + d] = o / s.L;
}

int enqueue_text_side(const float* q, const float* k, const float* vv, int H, int S, int T, float q_scale, const Plan& p,
                      long long BH, float* ws, float* out_l, hipStream_t st, const philox::Dropout* drop) {
  const dim3 grid((unsigned)p.NC, (unsigned)p.NG, (unsigned)BH);
  if (drop) hipLaunchKernelGGL(biattn_text_dropout, grid, dim3(kThreads), 0, st, q, k, vv, H, S, T, q_scale, p.NC, p.TP, ws, *drop);
  else hipLaunchKernelGGL(biattn_text, grid, dim3(kThreads), 0, st, q, k, vv, H, S, T, q_scale, p.NC, p.TP, ws);
  int rc = msda::launch_status();
  if (rc) return rc;
  const int64_t total = (int64_t)BH * kD * T;
  hipLaunchKernelGGL(biattn_combine, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, ws, H, T, p.NC,
                     p.TP, total, out_l);
  return msda::launch_status();
}

}  // namespace biattn

extern "C" {

static const char* g_biattn_last = "";

size_t biattn_hip_workspace_bytes(int batch, int num_heads, int image_len, int text_len, int head_dim) {
  if (batch < 0 || num_heads <= 0 || image_len <= 0 || text_len <= 0 || head_dim != biattn::kD || text_len > biattn::kMaxT) return 0;
  if (biattn::geometry(batch, num_heads, image_len, text_len, head_dim) != 0) return 0;
  return biattn::plan((long long)batch * num_heads, image_len, text_len).bytes;
}

const char* biattn_hip_last_kernel(void) { return g_biattn_last; }

int biattn_hip_forward_f32(const float* q, const float* k, const float* vv, const float* vl, const void* mask, int mask_kind,
                           int batch, int num_heads, int image_len, int text_len, int head_dim, float q_scale,
                           float* out_v, float* out_l, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace biattn;
  Plan p;
  int rc = forward_args(batch, num_heads, image_len, text_len, head_dim, mask_kind, mask, {q, k, vv, vl, out_v, out_l, workspace},
                        workspace_bytes, p);
  const long long BH = (long long)batch * num_heads;
  if (rc || BH == 0) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int S = image_len, T = text_len, H = num_heads;

  with_nj(p.TP, [&](auto nj) {
    hipLaunchKernelGGL(biattn_image<decltype(nj)::value>, image_grid(S, BH), dim3(kThreads), 0, st, q, k, vl, mask, mask_kind, H, S, T,
                       q_scale, out_v);
  });
  if ((rc = msda::launch_status())) return rc;

  if ((rc = enqueue_text_side(q, k, vv, H, S, T, q_scale, p, BH, static_cast<float*>(workspace), out_l, st))) return rc;
  g_biattn_last = "biattn_image+biattn_text+biattn_combine";
  return 0;
}

}  // extern "C"
