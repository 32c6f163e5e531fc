// Training route of the decoder layers' self-attention core -- see include/biattn_hip.h (biattn_hip_self_train_f32,
// biattn_hip_self_backward_f32).  dec_attn.hip's scheme (attn_tile.hpp, head dimension 32, the [Lq, Lq] mask) with a recomputing
// backward after vit_attn_bwd.hip, without its relative-position parts: no [Lq, Lq] tensor is ever written, a wave holds one
// 32 x 32 tile of scores, probabilities and score gradients at a time.
//
//   attn_lse   the forward of dec_attn.hip -- the SAME text, dec_attn_launch.hpp's fwd<MASK, LSE> -- whose wave 0 also stores
//              lse[bh, i] = max + log(sum) of the combined key ranges (-inf for a query with every key excluded, 0 for the rows
//              past len).  One text costs dec_attn::attn nothing: both kernels compile to the registers they had as two.
//   bwd_q      a workgroup OWNS 32 queries (scaled q and g in registers), K and V tiles are STREAMED.  p = exp(s + m - lse),
//              dp = g . v, ds = p (dp - delta); dq^T += K^T ds is attn_tile's second product, scaled by q_scale at the end.
//              delta[bh, i] = g_i . o_i is taken in the preamble from the owned rows (no kernel of its own: the rows are in
//              the registers anyway) and stored for the key pass, which runs behind it in stream order.
//   bwd_kv     a workgroup OWNS 32 keys (k and v rows in registers), scaled-q and g tiles are STREAMED with lse, delta and the
//              mask's elements of their queries.  dv^T += G^T p^T, dk^T += (q_scale Q)^T ds^T.
// The owned rows of the query pass, the scaled tile and the ds^T step of the key pass are attn_bwd_tile.hpp's, shared with
// vit_attn_bwd.hip; the constants, mask_add and the argument checks are dec_attn_launch.hpp's, shared with dec_attn.hip.
//
// The grid is dec_attn.hip's in all three: batch * heads is 16 at the workload, so a workgroup takes only 32 owned tokens and its
// TWO waves own the SAME tokens and split the streamed tiles, wave 0 the first ceil(tiles / 2), wave 1 the rest, each through
// LDS tiles of its own; wave 1 hands its accumulators over through LDS and wave 0 adds the two in that order and stores.  Lq =
// 1100: 16 * 35 workgroups = 1120 waves over 18 or 17 tiles each, instead of 560 waves over 35.  NOT MEASURED for the backward:
// the choice is carried over from the forward, where one wave per 32 queries left half the card's 1024 SIMDs idle; nobody has
// timed the backward with one wave per workgroup (or four over 128 tokens) against this.
//
// The mask is the forward's: element [i, j] (a byte, non-zero = -inf, or a float) is ADDED to the score; a streamed tile in
// which no owned token has an open partner (the forward's test, !(a == -inf), keys and queries past len being -inf) is skipped
// in all three kernels -- its probabilities would all have been exp(-inf) = 0 -- and is not even loaded in the two backward
// passes.  A bool mask and its -inf float form therefore give the same bits.  The mask gets no gradient.
//
// A query with every key excluded has lse = -inf (and out = NaN).  Both passes read such an lse as 0 and its delta as 0, so
// every p of that query is exp(-inf - 0) = 0 and every ds is 0 * (dp - 0) = 0: for a finite grad_out row it adds exactly nothing
// to dk and dv, and exp(-inf - -inf) never reaches a sum.  (Its g row is still streamed by the key pass: a NaN or infinity in it
// meets p = 0 as 0 * NaN and makes dk and dv of that (batch, head) NaN for every key workgroup that does not skip its tile.)  Its dq row is stored as NaN in all channels.
//
// Exact fp32 products, every sum in one fixed order, no float atomics, each output element written by exactly one thread.
//
// Resources (hipcc -O3 --offload-arch=gfx950, tools/kernel_resources.py; LDS per workgroup of 128 threads; scratch 0 in all):
//   attn_lse<none | f32 | bool>   VGPRs 123 | 130 | 130 (dec_attn::attn's own figures), AGPRs 32, LDS 13 824 B, 3 waves per SIMD
//   bwd_q<none | f32 | bool>      VGPRs 122 | 140 | 140, AGPRs 44 | 32 | 32, LDS 22 528 B, 3 | 2 | 2 waves per SIMD
//   bwd_kv<none | f32 | bool>     VGPRs 160 | 162 | 164, AGPRs 48, LDS 26 624 B, 2 waves per SIMD
#include "attn_bwd_tile.hpp"
#include "dec_attn_launch.hpp"

namespace dec_attn_bwd {

using namespace dec_attn;             // the constants, mask_add, the forward's text and the argument checks
using namespace attn_bwd_tile;

// dst[d] = (a[d, lane's token] + Part[.][lane]) * scale for the lane's d, or NaN: wave 0's accumulator and wave 1's, in that order
__device__ __forceinline__ void store_sum(float* __restrict__ dst, const f32x16& a, const float (*part)[64], int lane, int half,
                                          float scale, bool nan) {
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    f32x4 r;
#pragma unroll
    for (int u = 0; u < 4; ++u) r[u] = nan ? __builtin_nanf("") : (a[g4 * 4 + u] + part[g4 * 4 + u][lane]) * scale;
    *reinterpret_cast<f32x4*>(dst + g4 * 8 + half * 4) = r;
  }
}

// ------------------------------------------------------------------------------------------------
// dec_attn::attn with the row log-sum-exp.  grid (batch * heads * NG), NG = groups of 32 queries.  lse: [batch * heads, SP].
template <int MASK>
__global__ void __launch_bounds__(kThreads)
attn_lse(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int64_t qs, int64_t ks, int64_t vs,
         const void* __restrict__ mask, int heads, int L, int SP, int NG, float scale, float* __restrict__ out,
         float* __restrict__ lse) {
  fwd<MASK, true>(q, k, v, qs, ks, vs, mask, heads, L, SP, NG, scale, out, lse);
}

// ------------------------------------------------------------------------------------------------
// The query pass.  grid (batch * heads * NG).  Writes dq, and delta[bh, i] for i < SP.
template <int MASK>
__global__ void __launch_bounds__(kThreads)
bwd_q(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int64_t qs, int64_t ks, int64_t vs,
      const void* __restrict__ mask, const float* __restrict__ out, const float* __restrict__ lse, const float* __restrict__ gout,
      int heads, int L, int SP, int NG, float scale, float* __restrict__ dq, int64_t dqs, float* __restrict__ delta) {
  __shared__ __attribute__((aligned(16))) float Ks[kWaves][kTile][kPitch];
  __shared__ __attribute__((aligned(16))) float Vs[kWaves][kTile][kPitch];
  __shared__ float Part[16][64];      // wave 1's accumulator registers, by lane

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r32 = lane & 31, half = lane >> 5;
  const int bh = blockIdx.x / NG, grp = blockIdx.x - bh * NG, b = bh / heads, h = bh - b * heads;
  const int64_t E = (int64_t)heads * kD;
  const int i = grp * kTile + r32;                                  // i < SP
  const int ic = i < L ? i : L - 1;

  // owned rows: the scaled q as the forward rounds it, g, and delta = g . o (each lane half its floats, then one exchange)
  f32x4 ownq[kD / 8], owng[kD / 8];
  const int64_t row = (int64_t)b * L + ic;
  float dl = own_rows<kD>(ownq, owng, q + row * qs + h * kD, gout + row * E + h * kD, out + row * E + h * kD, i < L, scale, half);
  const float lse_raw = lse[(int64_t)bh * SP + i];
  const bool dead = lse_raw == -INFINITY;                           // every key excluded: out and g . o are NaN
  const float lse_i = dead ? 0.f : lse_raw;
  dl = dead ? 0.f : dl;
  if (wv == 0 && half == 0) delta[(int64_t)bh * SP + i] = dl;

  const float* kbase = k + (int64_t)b * L * ks + h * kD;
  const float* vbase = v + (int64_t)b * L * vs + h * kD;
  const int tiles = (L + kTile - 1) / kTile;
  const int per_wave = (tiles + kWaves - 1) / kWaves;               // the same trip count in both waves: the barriers meet
  const int t0 = wv * per_wave;
  auto rows_of = [&](int t) { const int n = L - t * kTile; return n < kTile ? n : kTile; };   // <= 0 past the last tile
  float (*Kt)[kPitch] = Ks[wv];
  float (*Vt)[kPitch] = Vs[wv];

  f32x16 acc[1];
  zero_acc(acc);

  for (int it = 0; it < per_wave; ++it) {
    const int t = t0 + it;
    const int nv = rows_of(t);                                      // wave-uniform; <= 0: this wave has no tile left

    // what is added to the scores of the lane's query: the mask's element, -inf for keys past the end
    float add[16];
    bool open = false;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int kr = acc_row(u) + 4 * half;
      float a = -INFINITY;
      if (kr < nv) a = mask_add<MASK>(mask, (size_t)ic * (size_t)L + (size_t)(t * kTile + kr));
      add[u] = a;
      open = open || !(a == -INFINITY);
    }
    const bool live = __any(open) != 0;                             // wave-uniform, the forward's test

    __syncthreads();                                                // the tiles of step it - 1 have been read
    if (live) {
      f32x4 pre[kPre];
      tile_load<kD, 64>(pre, kbase + (int64_t)t * kTile * ks, ks, nv, lane);
      tile_store<kD, 64>(Kt, pre, lane);
      tile_load<kD, 64>(pre, vbase + (int64_t)t * kTile * vs, vs, nv, lane);
      tile_store<kD, 64>(Vt, pre, lane);
    }
    __syncthreads();
    if (live) {
      f32x16 X, DP;
      zero_acc(X);
      zero_acc(DP);
      scores<kD>(Kt, ownq, X, r32, half);
      scores<kD>(Vt, owng, DP, r32, half);
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const float p = expf((X[u] + add[u]) - lse_i);              // an excluded key: exp(-inf) = 0
        X[u] = p * (DP[u] - dl);                                    // ds
      }
      pv(Kt, X, acc, r32, half);
    }
  }

  // the two key ranges, added in range order by wave 0
  if (wv == 1) {
#pragma unroll
    for (int u = 0; u < 16; ++u) Part[u][lane] = acc[0][u];
  }
  __syncthreads();
  if (wv == 0 && i < L) store_sum(dq + ((int64_t)b * L + i) * dqs + h * kD, acc[0], Part, lane, half, scale, dead);
}

// ------------------------------------------------------------------------------------------------
// The key pass.  grid (batch * heads * NG).  Writes dk and dv.  Reads lse, and delta, which the query pass wrote: the two run
// in stream order.
template <int MASK>
__global__ void __launch_bounds__(kThreads)
bwd_kv(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int64_t qs, int64_t ks, int64_t vs,
       const void* __restrict__ mask, const float* __restrict__ lse, const float* __restrict__ delta,
       const float* __restrict__ gout, int heads, int L, int SP, int NG, float scale, float* __restrict__ dk, float* __restrict__ dv,
       int64_t dks, int64_t dvs) {
  __shared__ __attribute__((aligned(16))) float Qs[kWaves][kTile][kPitch];
  __shared__ __attribute__((aligned(16))) float Gs[kWaves][kTile][kPitch];
  __shared__ float Part[32][64];      // wave 1's accumulator registers (dk, then dv), by lane

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r32 = lane & 31, half = lane >> 5;
  const int bh = blockIdx.x / NG, grp = blockIdx.x - bh * NG, b = bh / heads, h = bh - b * heads;
  const int64_t E = (int64_t)heads * kD;
  const int j = grp * kTile + r32;
  const int jc = j < L ? j : L - 1;

  f32x4 ownk[kD / 8], ownv[kD / 8];
  own_load<kD>(ownk, k + ((int64_t)b * L + jc) * ks + h * kD, j < L, 1.f, half);
  own_load<kD>(ownv, v + ((int64_t)b * L + jc) * vs + h * kD, j < L, 1.f, half);

  const float* lsep = lse + (int64_t)bh * SP;
  const float* delp = delta + (int64_t)bh * SP;
  const float* qbase = q + (int64_t)b * L * qs + h * kD;
  const float* gbase = gout + (int64_t)b * L * E + h * kD;
  const int tiles = (L + kTile - 1) / kTile;
  const int per_wave = (tiles + kWaves - 1) / kWaves;               // the same trip count in both waves: the barriers meet
  const int t0 = wv * per_wave;
  auto rows_of = [&](int t) { const int n = L - t * kTile; return n < kTile ? n : kTile; };   // <= 0 past the last tile
  float (*Qt)[kPitch] = Qs[wv];
  float (*Gt)[kPitch] = Gs[wv];

  f32x16 acck[1], accv[1];
  zero_acc(acck);
  zero_acc(accv);

  for (int it = 0; it < per_wave; ++it) {
    const int t = t0 + it;
    const int nv = rows_of(t);                                      // wave-uniform; <= 0: this wave has no tile left

    // what is added to the scores of the lane's key: the mask's element of every streamed query, -inf past either end
    float add[16];
    bool open = false;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int row = acc_row(u) + 4 * half;
      float a = -INFINITY;
      if (row < nv && j < L) a = mask_add<MASK>(mask, (size_t)(t * kTile + row) * (size_t)L + (size_t)j);
      add[u] = a;
      open = open || !(a == -INFINITY);
    }
    const bool live = __any(open) != 0;                             // wave-uniform, the forward's test

    __syncthreads();                                                // the tiles of step it - 1 have been read
    if (live) {
      f32x4 pre[kPre];
      stage_scaled<kD, 64>(Qt, pre, qbase + (int64_t)t * kTile * qs, qs, nv, scale, lane);
      tile_load<kD, 64>(pre, gbase + (int64_t)t * kTile * E, E, nv, lane);
      tile_store<kD, 64>(Gt, pre, lane);
    }
    __syncthreads();
    if (live) {                                                     // nv >= 1: the tile's 32 queries are below SP
      f32x16 X, DP;
      zero_acc(X);
      zero_acc(DP);
      scores<kD>(Qt, ownk, X, r32, half);                           // s^T: the streamed query in the register, the key on the lane
      scores<kD>(Gt, ownv, DP, r32, half);
      float dlt[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int i = t * kTile + acc_row(u) + 4 * half;
        const float l = lsep[i];
        X[u] = expf((X[u] + add[u]) - (l == -INFINITY ? 0.f : l));  // p^T; excluded, or a query with no open key: exp(-inf) = 0
        dlt[u] = delp[i];
      }
      pv(Gt, X, accv, r32, half);
      ds_t(X, DP, dlt);
      pv(Qt, X, acck, r32, half);
    }
  }

  // the two query ranges, added in range order by wave 0
  if (wv == 1) {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      Part[u][lane] = acck[0][u];
      Part[16 + u][lane] = accv[0][u];
    }
  }
  __syncthreads();
  if (wv == 0 && j < L) {
    store_sum(dk + ((int64_t)b * L + j) * dks + h * kD, acck[0], Part, lane, half, 1.f, false);
    store_sum(dv + ((int64_t)b * L + j) * dvs + h * kD, accv[0], Part + 16, lane, half, 1.f, false);
  }
}

// ---- host side: the argument checks are dec_attn_launch.hpp's ----------------------------------
constexpr const char* kWho = "dec_attn_bwd";   // the prefix of this file's refusals

static size_t delta_bytes(int batch, int num_heads, int len) {
  const size_t n = msda::align256((size_t)batch * num_heads * msda::round_up(len, kTile) * sizeof(float));
  return n < 256 ? 256 : n;
}

}  // namespace dec_attn_bwd

extern "C" {

static const char* g_dec_attn_bwd_last = "";

size_t biattn_hip_self_backward_workspace_bytes(int batch, int num_heads, int len, int head_dim) {
  if (dec_attn::geometry(dec_attn_bwd::kWho, batch, num_heads, len, head_dim, BIATTN_MASK_NONE, {}) != 0) return 0;
  return dec_attn_bwd::delta_bytes(batch, num_heads, len);
}

const char* biattn_hip_self_backward_last_kernel(void) { return g_dec_attn_bwd_last; }

int biattn_hip_self_train_f32(const float* q, const float* k, const float* v, long long q_stride, long long k_stride,
                              long long v_stride, const void* mask, int mask_kind, int batch, int num_heads, int len, int head_dim,
                              float q_scale, float* out, float* lse, void* stream) {
  using namespace dec_attn_bwd;
  int rc = geometry(kWho, batch, num_heads, len, head_dim, mask_kind, {q_stride, k_stride, v_stride});
  if (rc) return rc;
  if (batch == 0) return 0;   // nothing to enqueue, no buffer is looked at
  if (!q || !k || !v || !out || !lse) return refuse(kWho, BIATTN_ERR_NULL_POINTER, "null pointer argument");
  if ((rc = mask_pointer(kWho, mask, mask_kind))) return rc;
  if (!msda::aligned16({q, k, v, out, lse}))
    return refuse(kWho, BIATTN_ERR_UNSUPPORTED, "q, k, v, out and lse must be 16-byte aligned");

  hipStream_t st = static_cast<hipStream_t>(stream);
  const int NG = msda::ceil_div(len, kTile), SP = NG * kTile;
  const dim3 grid((unsigned)((long long)batch * num_heads * NG)), block(kThreads);
#define DEC_TRAIN_LAUNCH(KIND)                                                                                                   \
  hipLaunchKernelGGL(attn_lse<KIND>, grid, block, 0, st, q, k, v, (int64_t)q_stride, (int64_t)k_stride, (int64_t)v_stride, mask, \
                     num_heads, len, SP, NG, q_scale, out, lse)
  if (mask_kind == BIATTN_MASK_NONE) DEC_TRAIN_LAUNCH(BIATTN_MASK_NONE);
  else if (mask_kind == BIATTN_MASK_BOOL) DEC_TRAIN_LAUNCH(BIATTN_MASK_BOOL);
  else DEC_TRAIN_LAUNCH(BIATTN_MASK_F32);
#undef DEC_TRAIN_LAUNCH
  return msda::launch_status();
}

int biattn_hip_self_backward_f32(const float* q, const float* k, const float* v, long long q_stride, long long k_stride,
                                 long long v_stride, const void* mask, int mask_kind, const float* out, const float* lse,
                                 const float* grad_out, int batch, int num_heads, int len, int head_dim, float q_scale, float* dq,
                                 float* dk, float* dv, long long dq_stride, long long dk_stride, long long dv_stride, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  using namespace dec_attn_bwd;
  int rc = geometry(kWho, batch, num_heads, len, head_dim, mask_kind, {q_stride, k_stride, v_stride, dq_stride, dk_stride, dv_stride});
  if (rc) return rc;
  if (batch == 0) return 0;   // nothing to enqueue, no buffer is looked at
  if (!q || !k || !v || !out || !lse || !grad_out || !dq || !dk || !dv || !workspace)
    return refuse(kWho, BIATTN_ERR_NULL_POINTER, "null pointer argument");
  if ((rc = mask_pointer(kWho, mask, mask_kind))) return rc;
  if (!msda::aligned16({q, k, v, out, lse, grad_out, dq, dk, dv, workspace}))
    return refuse(kWho, BIATTN_ERR_UNSUPPORTED, "every pointer but the mask must be 16-byte aligned");
  if (workspace_bytes < delta_bytes(batch, num_heads, len))
    return refuse(kWho, BIATTN_ERR_WORKSPACE, "workspace smaller than the workspace_bytes query answers");

  hipStream_t st = static_cast<hipStream_t>(stream);
  const int NG = msda::ceil_div(len, kTile), SP = NG * kTile;
  const dim3 grid((unsigned)((long long)batch * num_heads * NG)), block(kThreads);
  float* delta = static_cast<float*>(workspace);
#define DEC_BWD_LAUNCH(KIND)                                                                                                      \
  do {                                                                                                                            \
    hipLaunchKernelGGL(bwd_q<KIND>, grid, block, 0, st, q, k, v, (int64_t)q_stride, (int64_t)k_stride, (int64_t)v_stride, mask,   \
                       out, lse, grad_out, num_heads, len, SP, NG, q_scale, dq, (int64_t)dq_stride, delta);                       \
    if ((rc = msda::launch_status())) return rc;                                                                                  \
    hipLaunchKernelGGL(bwd_kv<KIND>, grid, block, 0, st, q, k, v, (int64_t)q_stride, (int64_t)k_stride, (int64_t)v_stride, mask,  \
                       lse, (const float*)delta, grad_out, num_heads, len, SP, NG, q_scale, dk, dv, (int64_t)dk_stride,           \
                       (int64_t)dv_stride);                                                                                       \
  } while (0)
  if (mask_kind == BIATTN_MASK_NONE) DEC_BWD_LAUNCH(BIATTN_MASK_NONE);
  else if (mask_kind == BIATTN_MASK_BOOL) DEC_BWD_LAUNCH(BIATTN_MASK_BOOL);
  else DEC_BWD_LAUNCH(BIATTN_MASK_F32);
#undef DEC_BWD_LAUNCH
  if ((rc = msda::launch_status())) return rc;
  g_dec_attn_bwd_last = mask_kind == BIATTN_MASK_NONE   ? "dec_bwd_q<none>+dec_bwd_kv<none>"
                        : mask_kind == BIATTN_MASK_BOOL ? "dec_bwd_q<bool>+dec_bwd_kv<bool>"
                                                        : "dec_bwd_q<f32>+dec_bwd_kv<f32>";
  return 0;
}

}  // extern "C"
