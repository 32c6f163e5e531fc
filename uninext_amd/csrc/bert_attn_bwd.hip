// Training route of the text encoder's self-attention core -- see include/dynmask_hip.h (bert_hip_self_attention_train_f32,
// bert_hip_self_attention_backward_f32, bert_hip_dropout_keep_u8).  bert.hip's scheme (attn_tile.hpp, head dimension 64, a KEEP
// mask per key or per (query, key)) with a recomputing backward after dec_attn_bwd.hip and the in-kernel attention dropout of
// biattn_bwd.hip (philox.hpp): no [T, T] tensor is ever written, a wave holds one 32 x 32 tile of scores, probabilities and score
// gradients at a time, and the keep decisions are recomputed, never stored.
//
//   attn_train  the forward of bert.hip -- the SAME text, bert_attn_common.hpp's fwd<MASK, LSE, DROP> -- whose wave 0 also stores
//               lse[bh, i] = max + log(sum) of the combined key ranges (-inf for a query that keeps no key, 0 for the rows past
//               len) and which, with DROP, multiplies the tile of probabilities by c m before the second product.
//   bwd_q       a workgroup OWNS 32 queries (scaled q and g in registers), K and V tiles are STREAMED.  p = exp(s - lse) on the
//               kept keys, dp = c m (g . v), ds = p (dp - delta); dq^T += K^T ds is attn_tile's second product, scaled by q_scale
//               at the end.  delta[bh, i] = g_i . o_i is taken in the preamble from the owned rows and stored for the key pass,
//               which runs behind it in stream order.
//   bwd_kv      a workgroup OWNS 32 keys (k and v rows in registers), scaled-q and g tiles are STREAMED with lse and delta of
//               their queries.  dv^T += G^T (c m p)^T, dk^T += (q_scale Q)^T ds^T.
// The owned rows of the query pass, the scaled tile and the ds^T step of the key pass are attn_bwd_tile.hpp's.
//
// The grid is bert.hip's in all three: a workgroup takes 32 owned tokens and its TWO waves own the SAME tokens and split the
// streamed tiles, wave 0 the first ceil(tiles / 2), wave 1 the rest, each through LDS tiles of its own; wave 1 hands its
// accumulators over through LDS and wave 0 adds the two in that order and stores.  NOT MEASURED against other splits.
//
// Skipping.  A streamed tile in which no owned token has a kept partner is neither loaded nor multiplied (its probabilities
// would all have been exactly 0).  For the [B, T] mask kinds the test is wave-uniform from a ballot: of the streamed keys' flags
// in the query pass (the forward's tile_keep), of the owned keys' flags in the key pass.  A key-pass workgroup whose 32 owned
// keys a [B, T] mask all excludes stores zeros and streams nothing: at 20 valid tokens of 256 that is 7 of 8 workgroups.
//
// A query that keeps no key has lse = -inf and out = 0.  Both passes read such an lse as 0 and its delta as 0; every p of that
// query is exp(-inf) = 0 and every ds is 0 * (dp - 0) = 0, so for a finite grad_out row it adds exactly nothing to dk and dv, and
// its dq row is stored as zeros.
//
// Dropout.  The decision for (query i, key j) is philox::entry_words(stream, side 0, bh, i, j / 4), word j % 4: the query pass
// and the forward own queries and draw four calls a tile (keep_bits_row_owner), the key pass owns keys and draws sixteen
// (keep_bits_col_owner), dropout_keep writes the same decisions out.  dropout_p == 0 runs the kernels without DROP.
//
// Exact fp32 products, every sum in one fixed order, no float atomics, each output element written by exactly one thread.
//
// Resources (hipcc -O3 --offload-arch=gfx950, tools/kernel_resources.py; workgroups of 128 threads, one wave per SIMD; scratch 0
// and no spill in all; VGPRs by mask kind none | key_i64 | key_u8 | full_u8, accumulation registers included):
//   attn_train<*, no drop>   223 | 226 | 226 | 223 (bert::attn's own figures), LDS 26 112 B
//   attn_train<*, drop>      237 | 240 | 240 | 237
//   bwd_q<*, no drop>        208 | 212 | 212 | 210, LDS 43 008 B
//   bwd_q<*, drop>           222 | 226 | 226 | 194
//   bwd_kv<*, no drop>       248 | 252 | 252 | 252, LDS 51 200 B
//   bwd_kv<*, drop>          247 | 251 | 251 | 250
//   dropout_keep             16
#include "attn_bwd_tile.hpp"
#include "bert_attn_common.hpp"

namespace bert_attn_bwd {

using namespace bert;                 // the constants, tile_keep, the forward's text and the argument checks
using namespace attn_bwd_tile;

// The key pass's form of tile_keep: what the mask adds to the scores of the lane's key j (own_keep: it exists and a [B, T] mask
// keeps it) against the queries of tile t, which are the registers' rows.  Returns whether any key of the wave has a kept query
// in the tile: wave-uniform.
template <int MASK>
__device__ __forceinline__ bool tile_keep_t(float (&add)[16], const void* __restrict__ mask, int b, int jc, bool own_keep, int T, int t,
                                            int nv, int half) {
  const unsigned char* col = static_cast<const unsigned char*>(mask) + ((size_t)b * T + (size_t)t * kTile) * (size_t)T + jc;
  bool open = false;
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int row = acc_row(u) + 4 * half;
    bool keep = own_keep && row < nv;
    if (MASK == BERT_MASK_FULL_U8 && keep) keep = col[(size_t)row * T] != 0;
    add[u] = keep ? 0.f : -INFINITY;
    open = open || keep;
  }
  return __any(open) != 0;
}

// dst[d] = (a[d, lane's token] + part[.][lane]) * scale for the lane's 32 d of one block, or zeros: wave 0's accumulator and
// wave 1's, in that order
__device__ __forceinline__ void store_sum(float* __restrict__ dst, const f32x16& a, const float (*part)[64], int lane, int half,
                                          float scale, bool zero) {
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    f32x4 r;
#pragma unroll
    for (int u = 0; u < 4; ++u) r[u] = zero ? 0.f : (a[g4 * 4 + u] + part[g4 * 4 + u][lane]) * scale;
    *reinterpret_cast<f32x4*>(dst + g4 * 8 + half * 4) = r;
  }
}

// ------------------------------------------------------------------------------------------------
// bert::attn with the row log-sum-exp and, with DROP, the dropout.  grid (batch * heads * NG).  lse: [batch * heads, SP].
template <int MASK, bool DROP>
__global__ void __launch_bounds__(kThreads)
attn_train(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int64_t qs, int64_t ks, int64_t vs,
           const void* __restrict__ mask, int heads, int T, int SP, int NG, float scale, float* __restrict__ out,
           float* __restrict__ lse, philox::Dropout drop) {
  fwd<MASK, true, DROP>(q, k, v, qs, ks, vs, mask, heads, T, SP, NG, scale, out, lse, drop);
}

// ------------------------------------------------------------------------------------------------
// The query pass.  grid (batch * heads * NG).  Writes dq, and delta[bh, i] for i < SP.
template <int MASK, bool DROP>
__global__ void __launch_bounds__(kThreads)
bwd_q(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int64_t qs, int64_t ks, int64_t vs,
      const void* __restrict__ mask, const float* __restrict__ out, const float* __restrict__ lse, const float* __restrict__ gout,
      int heads, int T, int SP, int NG, float scale, float* __restrict__ dq, int64_t dqs, float* __restrict__ delta,
      philox::Dropout drop) {
  __shared__ __attribute__((aligned(16))) float Ks[kWaves][kTile][kPitch];
  __shared__ __attribute__((aligned(16))) float Vs[kWaves][kTile][kPitch];
  __shared__ float Part[16 * kDB][64];   // wave 1's accumulator registers, by lane

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r32 = lane & 31, half = lane >> 5;
  const int bh = blockIdx.x / NG, grp = blockIdx.x - bh * NG, b = bh / heads, h = bh - b * heads;
  const int64_t E = (int64_t)heads * kD;
  const int i = grp * kTile + r32;                                  // i < SP
  const int ic = i < T ? i : T - 1;

  // owned rows: the scaled q as the forward rounds it, g, and delta = g . o (each lane half its floats, then one exchange)
  f32x4 ownq[kD / 8], owng[kD / 8];
  const int64_t row = (int64_t)b * T + ic;
  float dl = own_rows<kD>(ownq, owng, q + row * qs + h * kD, gout + row * E + h * kD, out + row * E + h * kD, i < T, scale, half);
  const float lse_raw = lse[(int64_t)bh * SP + i];
  const bool dead = lse_raw == -INFINITY;                           // no key kept: out is zeros, every p below is 0
  const float lse_i = dead ? 0.f : lse_raw;
  dl = dead ? 0.f : dl;
  if (wv == 0 && half == 0) delta[(int64_t)bh * SP + i] = dl;

  const float* kbase = k + (int64_t)b * T * ks + h * kD;
  const float* vbase = v + (int64_t)b * T * vs + h * kD;
  const int tiles = (T + kTile - 1) / kTile;
  const int per_wave = (tiles + kWaves - 1) / kWaves;               // the same trip count in both waves: the barriers meet
  const int t0 = wv * per_wave;
  auto rows_of = [&](int t) { const int n = T - t * kTile; return n < kTile ? n : kTile; };   // <= 0 past the last tile
  float (*Kt)[kPitch] = Ks[wv];
  float (*Vt)[kPitch] = Vs[wv];

  f32x16 acc[kDB];
  zero_acc(acc);

  for (int it = 0; it < per_wave; ++it) {
    const int t = t0 + it;
    const int nv = rows_of(t);                                      // wave-uniform; <= 0: this wave has no tile left
    float add[16];
    const bool live = tile_keep<MASK>(add, mask, b, ic, T, t, nv, r32, half);   // wave-uniform, the forward's test

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
      uint32_t keep = 0;                                            // drawn before the score fragments are live
      if (DROP) keep = philox::keep_bits_row_owner(philox::stream_of(drop), drop.threshold, bh, ic, t * kTile, half);
      f32x16 X, DP;
      zero_acc(X);
      zero_acc(DP);
      scores<kD>(Kt, ownq, X, r32, half);
      scores<kD>(Vt, owng, DP, r32, half);
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const float p = expf((X[u] + add[u]) - lse_i);              // an excluded key: exp(-inf) = 0
        const float dp = DROP ? DP[u] * philox::keep_factor(keep, u, drop.scale) : DP[u];
        X[u] = p * (dp - dl);                                       // ds
      }
      pv(Kt, X, acc, r32, half);
    }
  }

  // the two key ranges, added in range order by wave 0
  if (wv == 1) {
#pragma unroll
    for (int db = 0; db < kDB; ++db)
#pragma unroll
      for (int u = 0; u < 16; ++u) Part[db * 16 + u][lane] = acc[db][u];
  }
  __syncthreads();
  if (wv == 0 && i < T) {
    float* o = dq + ((int64_t)b * T + i) * dqs + h * kD;
#pragma unroll
    for (int db = 0; db < kDB; ++db) store_sum(o + db * 32, acc[db], Part + db * 16, lane, half, scale, dead);
  }
}

// ------------------------------------------------------------------------------------------------
// The key pass.  grid (batch * heads * NG).  Writes dk and dv.  Reads lse, and delta, which the query pass wrote: the two run
// in stream order.
template <int MASK, bool DROP>
__global__ void __launch_bounds__(kThreads)
bwd_kv(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int64_t qs, int64_t ks, int64_t vs,
       const void* __restrict__ mask, const float* __restrict__ lse, const float* __restrict__ delta,
       const float* __restrict__ gout, int heads, int T, int SP, int NG, float scale, float* __restrict__ dk, float* __restrict__ dv,
       int64_t dks, int64_t dvs, philox::Dropout drop) {
  __shared__ __attribute__((aligned(16))) float Qs[kWaves][kTile][kPitch];
  __shared__ __attribute__((aligned(16))) float Gs[kWaves][kTile][kPitch];
  __shared__ float Part[32 * kDB][64];   // wave 1's accumulator registers (dk, then dv), by lane

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r32 = lane & 31, half = lane >> 5;
  const int bh = blockIdx.x / NG, grp = blockIdx.x - bh * NG, b = bh / heads, h = bh - b * heads;
  const int64_t E = (int64_t)heads * kD;
  const int j = grp * kTile + r32;
  const int jc = j < T ? j : T - 1;
  float* dkrow = dk + ((int64_t)b * T + jc) * dks + h * kD;
  float* dvrow = dv + ((int64_t)b * T + jc) * dvs + h * kD;

  // the owned keys' flags of a [B, T] mask: the same in both waves, so the whole workgroup leaves together
  bool own_keep = j < T;
  if (own_keep && MASK == BERT_MASK_KEY_I64) own_keep = static_cast<const long long*>(mask)[(size_t)b * T + j] != 0;
  if (own_keep && MASK == BERT_MASK_KEY_U8) own_keep = static_cast<const unsigned char*>(mask)[(size_t)b * T + j] != 0;
  if ((MASK == BERT_MASK_KEY_I64 || MASK == BERT_MASK_KEY_U8) && !__any(own_keep)) {   // nothing but padding: zeros, nothing streamed
    if (wv == 0 && j < T) {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < kD / 8; ++c) {
        *reinterpret_cast<f32x4*>(dkrow + c * 8 + half * 4) = z;
        *reinterpret_cast<f32x4*>(dvrow + c * 8 + half * 4) = z;
      }
    }
    return;
  }

  f32x4 ownk[kD / 8], ownv[kD / 8];
  own_load<kD>(ownk, k + ((int64_t)b * T + jc) * ks + h * kD, j < T, 1.f, half);
  own_load<kD>(ownv, v + ((int64_t)b * T + jc) * vs + h * kD, j < T, 1.f, half);

  const float* lsep = lse + (int64_t)bh * SP;
  const float* delp = delta + (int64_t)bh * SP;
  const float* qbase = q + (int64_t)b * T * qs + h * kD;
  const float* gbase = gout + (int64_t)b * T * E + h * kD;
  const int tiles = (T + kTile - 1) / kTile;
  const int per_wave = (tiles + kWaves - 1) / kWaves;               // the same trip count in both waves: the barriers meet
  const int t0 = wv * per_wave;
  auto rows_of = [&](int t) { const int n = T - t * kTile; return n < kTile ? n : kTile; };   // <= 0 past the last tile
  float (*Qt)[kPitch] = Qs[wv];
  float (*Gt)[kPitch] = Gs[wv];

  f32x16 acck[kDB], accv[kDB];
  zero_acc(acck);
  zero_acc(accv);

  for (int it = 0; it < per_wave; ++it) {
    const int t = t0 + it;
    const int nv = rows_of(t);                                      // wave-uniform; <= 0: this wave has no tile left
    float add[16];
    const bool live = tile_keep_t<MASK>(add, mask, b, jc, own_keep, T, t, nv, half);   // wave-uniform

    __syncthreads();                                                // the tiles of step it - 1 have been read
    if (live) {
      f32x4 pre[kPre];
      stage_scaled<kD, 64>(Qt, pre, qbase + (int64_t)t * kTile * qs, qs, nv, scale, lane);
      tile_load<kD, 64>(pre, gbase + (int64_t)t * kTile * E, E, nv, lane);
      tile_store<kD, 64>(Gt, pre, lane);
    }
    __syncthreads();
    if (live) {                                                     // nv >= 1: the tile's 32 queries are below SP
      uint32_t keep = 0;                                            // drawn before the score fragments are live
      if (DROP) keep = philox::keep_bits_col_owner(philox::stream_of(drop), drop.threshold, bh, jc, t * kTile, half);
      f32x16 X, DP;
      zero_acc(X);
      zero_acc(DP);
      scores<kD>(Qt, ownk, X, r32, half);                           // s^T: the streamed query in the register, the key on the lane
      scores<kD>(Gt, ownv, DP, r32, half);
      float dlt[16];
      f32x16 PD;                                                    // c m p^T: the dropped probabilities
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int i = t * kTile + acc_row(u) + 4 * half;
        const float l = lsep[i];
        X[u] = expf((X[u] + add[u]) - (l == -INFINITY ? 0.f : l));  // p^T; excluded, or a query that keeps no key: exp(-inf) = 0
        dlt[u] = delp[i];
        PD[u] = X[u];
        if (DROP) {
          const float f = philox::keep_factor(keep, u, drop.scale);
          PD[u] *= f;
          DP[u] *= f;
        }
      }
      pv(Gt, PD, accv, r32, half);
      ds_t(X, DP, dlt);
      pv(Qt, X, acck, r32, half);
    }
  }

  // the two query ranges, added in range order by wave 0
  if (wv == 1) {
#pragma unroll
    for (int db = 0; db < kDB; ++db)
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        Part[db * 16 + u][lane] = acck[db][u];
        Part[16 * kDB + db * 16 + u][lane] = accv[db][u];
      }
  }
  __syncthreads();
  if (wv == 0 && j < T) {
#pragma unroll
    for (int db = 0; db < kDB; ++db) {
      store_sum(dkrow + db * 32, acck[db], Part + db * 16, lane, half, 1.f, false);
      store_sum(dvrow + db * 32, accv[db], Part + 16 * kDB + db * 16, lane, half, 1.f, false);
    }
  }
}

// keep[bh, i, j] as bytes (1 = kept), by the kernels' own decision (philox.hpp): for tests and tools, the only place where a
// mask of size B * H * T * T exists.  One thread per (bh, query, group of four keys).
__global__ void __launch_bounds__(kThreads)
dropout_keep(philox::Dropout drop, int T, int64_t total, unsigned char* __restrict__ keep) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const int NG4 = (T + 3) / 4;
  const int g = (int)(idx % NG4);
  const int i = (int)((idx / NG4) % T);
  const int bh = (int)(idx / ((int64_t)NG4 * T));
  const philox::Words w = philox::entry_words(philox::stream_of(drop), philox::kSideV, bh, i, g);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = 4 * g + t;
    if (j < T) keep[((int64_t)bh * T + i) * T + j] = w.w[t] >= drop.threshold;
  }
}

// ---- host side: the argument checks are bert_attn_common.hpp's ---------------------------------
static size_t delta_bytes(int batch, int num_heads, int len) {
  const size_t n = msda::align256((size_t)batch * num_heads * msda::round_up(len, kTile) * sizeof(float));
  return n < 256 ? 256 : n;
}

// The dropout arguments of the C ABI, before the device is touched: 0, or a negative BERT_ERR_* (message set).  `d` is filled
// with the threshold (uint32) llrint(p 2^32) and the scale 1.0f / (1.0f - p); `on` says whether the DROP kernels run.  The seed
// pointer is looked at with the other pointers (dropout_seed), after the empty batch has returned.
static int dropout_args(const char* who, float dropout_p, const unsigned long long* seed, long long bh, philox::Dropout& d, bool& on) {
  if (!(dropout_p >= 0.f && dropout_p < 1.f)) return refuse(who, BERT_ERR_BAD_DIMS, "dropout_p must be in [0, 1)");
  on = dropout_p > 0.f;
  if (on && bh > 65535) return refuse(who, BERT_ERR_UNSUPPORTED, "batch * num_heads must be at most 65535 with dropout");
  d.seed = seed;
  d.threshold = (uint32_t)llrint((double)dropout_p * 4294967296.0);
  d.scale = 1.0f / (1.0f - dropout_p);
  return 0;
}

static int dropout_seed(const char* who, const philox::Dropout& d, bool on) {
  if (on && !d.seed) return refuse(who, BERT_ERR_NULL_POINTER, "null seed with dropout_p > 0");
  if (on && reinterpret_cast<uintptr_t>(d.seed) % 8 != 0) return refuse(who, BERT_ERR_UNSUPPORTED, "the seed must be 8-byte aligned");
  return 0;
}

// F<MASK, DROP>::run(args...) for the mask kind and the dropout switch of the call
template <template <int, bool> class F, typename... A>
static void dispatch(int mask_kind, bool drop, A... a) {
#define BERT_KIND(KIND)                 \
  if (mask_kind == KIND) {              \
    if (drop) F<KIND, true>::run(a...); \
    else F<KIND, false>::run(a...);     \
    return;                             \
  }
  BERT_KIND(BERT_MASK_NONE);
  BERT_KIND(BERT_MASK_KEY_I64);
  BERT_KIND(BERT_MASK_KEY_U8);
  BERT_KIND(BERT_MASK_FULL_U8);
#undef BERT_KIND
}

struct Call {                         // what the three launches take
  const float *q, *k, *v;
  int64_t qs, ks, vs;
  const void* mask;
  int heads, T, SP, NG;
  float scale;
  philox::Dropout drop;
  dim3 grid;
  hipStream_t st;
};

template <int MASK, bool DROP>
struct Train {
  static void run(const Call& c, float* out, float* lse) {
    hipLaunchKernelGGL((attn_train<MASK, DROP>), c.grid, dim3(kThreads), 0, c.st, c.q, c.k, c.v, c.qs, c.ks, c.vs, c.mask, c.heads, c.T,
                       c.SP, c.NG, c.scale, out, lse, c.drop);
  }
};

template <int MASK, bool DROP>
struct QueryPass {
  static void run(const Call& c, const float* out, const float* lse, const float* g, float* dq, int64_t dqs, float* delta) {
    hipLaunchKernelGGL((bwd_q<MASK, DROP>), c.grid, dim3(kThreads), 0, c.st, c.q, c.k, c.v, c.qs, c.ks, c.vs, c.mask, out, lse, g,
                       c.heads, c.T, c.SP, c.NG, c.scale, dq, dqs, delta, c.drop);
  }
};

template <int MASK, bool DROP>
struct KeyPass {
  static void run(const Call& c, const float* lse, const float* delta, const float* g, float* dk, float* dv, int64_t dks, int64_t dvs) {
    hipLaunchKernelGGL((bwd_kv<MASK, DROP>), c.grid, dim3(kThreads), 0, c.st, c.q, c.k, c.v, c.qs, c.ks, c.vs, c.mask, lse, delta, g,
                       c.heads, c.T, c.SP, c.NG, c.scale, dk, dv, dks, dvs, c.drop);
  }
};

static Call call_of(const float* q, const float* k, const float* v, long long qs, long long ks, long long vs, const void* mask,
                    int batch, int heads, int len, float scale, const philox::Dropout& drop, void* stream) {
  const int NG = msda::ceil_div(len, kTile);
  return {q, k, v, (int64_t)qs, (int64_t)ks, (int64_t)vs, mask, heads, len, NG * kTile, NG, scale, drop,
          dim3((unsigned)((long long)batch * heads * NG)), static_cast<hipStream_t>(stream)};
}

// the names the last_kernel queries return, by mask kind and dropout switch
static const char* const kTrainNames[4][2] = {
    {"bert_attn_train<none>", "bert_attn_train<none,drop>"},
    {"bert_attn_train<key_i64>", "bert_attn_train<key_i64,drop>"},
    {"bert_attn_train<key_u8>", "bert_attn_train<key_u8,drop>"},
    {"bert_attn_train<full_u8>", "bert_attn_train<full_u8,drop>"}};
static const char* const kBackwardNames[4][2] = {
    {"bert_bwd_q<none>+bert_bwd_kv<none>", "bert_bwd_q<none,drop>+bert_bwd_kv<none,drop>"},
    {"bert_bwd_q<key_i64>+bert_bwd_kv<key_i64>", "bert_bwd_q<key_i64,drop>+bert_bwd_kv<key_i64,drop>"},
    {"bert_bwd_q<key_u8>+bert_bwd_kv<key_u8>", "bert_bwd_q<key_u8,drop>+bert_bwd_kv<key_u8,drop>"},
    {"bert_bwd_q<full_u8>+bert_bwd_kv<full_u8>", "bert_bwd_q<full_u8,drop>+bert_bwd_kv<full_u8,drop>"}};

}  // namespace bert_attn_bwd

extern "C" {

static const char* g_bert_train_last = "";
static const char* g_bert_bwd_last = "";

const char* bert_hip_attention_train_last_kernel(void) { return g_bert_train_last; }
const char* bert_hip_attention_backward_last_kernel(void) { return g_bert_bwd_last; }

size_t bert_hip_self_attention_backward_workspace_bytes(int batch, int num_heads, int len, int head_dim) {
  if (bert::geometry("bert_attn_bwd", batch, num_heads, len, head_dim, BERT_MASK_NONE, {}) != 0) return 0;
  return bert_attn_bwd::delta_bytes(batch, num_heads, len);
}

int bert_hip_self_attention_train_f32(const float* q, const float* k, const float* v, long long q_stride, long long k_stride,
                                      long long v_stride, const void* mask, int mask_kind, int batch, int num_heads, int len,
                                      int head_dim, float q_scale, float* out, float* lse, float dropout_p,
                                      const unsigned long long* seed, void* stream) {
  using namespace bert_attn_bwd;
  static const char* const kWho = "bert_attn_train";
  int rc = geometry(kWho, batch, num_heads, len, head_dim, mask_kind, {q_stride, k_stride, v_stride});
  if (rc) return rc;
  philox::Dropout drop;
  bool on = false;
  if ((rc = dropout_args(kWho, dropout_p, seed, (long long)batch * num_heads, drop, on))) return rc;
  if (batch == 0) return 0;   // nothing to enqueue, no buffer is looked at
  if (!q || !k || !v || !out || !lse) return refuse(kWho, BERT_ERR_NULL_POINTER, "null pointer argument");
  if ((rc = mask_pointer(kWho, mask, mask_kind))) return rc;
  if ((rc = dropout_seed(kWho, drop, on))) return rc;
  if (!msda::aligned16({q, k, v, out, lse})) return refuse(kWho, BERT_ERR_UNSUPPORTED, "q, k, v, out and lse must be 16-byte aligned");

  const Call c = call_of(q, k, v, q_stride, k_stride, v_stride, mask, batch, num_heads, len, q_scale, drop, stream);
  dispatch<Train>(mask_kind, on, c, out, lse);
  if ((rc = msda::launch_status())) return rc;
  g_bert_train_last = kTrainNames[mask_kind][on];
  return 0;
}

int bert_hip_self_attention_backward_f32(const float* q, const float* k, const float* v, long long q_stride, long long k_stride,
                                         long long v_stride, const void* mask, int mask_kind, const float* out, const float* lse,
                                         const float* grad_out, int batch, int num_heads, int len, int head_dim, float q_scale,
                                         float* dq, float* dk, float* dv, long long dq_stride, long long dk_stride,
                                         long long dv_stride, void* workspace, size_t workspace_bytes, float dropout_p,
                                         const unsigned long long* seed, void* stream) {
  using namespace bert_attn_bwd;
  static const char* const kWho = "bert_attn_bwd";
  int rc = geometry(kWho, batch, num_heads, len, head_dim, mask_kind, {q_stride, k_stride, v_stride, dq_stride, dk_stride, dv_stride});
  if (rc) return rc;
  philox::Dropout drop;
  bool on = false;
  if ((rc = dropout_args(kWho, dropout_p, seed, (long long)batch * num_heads, drop, on))) return rc;
  if (batch == 0) return 0;   // nothing to enqueue, no buffer is looked at
  if (!q || !k || !v || !out || !lse || !grad_out || !dq || !dk || !dv || !workspace)
    return refuse(kWho, BERT_ERR_NULL_POINTER, "null pointer argument");
  if ((rc = mask_pointer(kWho, mask, mask_kind))) return rc;
  if ((rc = dropout_seed(kWho, drop, on))) return rc;
  if (!msda::aligned16({q, k, v, out, lse, grad_out, dq, dk, dv, workspace}))
    return refuse(kWho, BERT_ERR_UNSUPPORTED, "every pointer but the mask and the seed must be 16-byte aligned");
  if (workspace_bytes < delta_bytes(batch, num_heads, len))
    return refuse(kWho, BERT_ERR_WORKSPACE, "workspace smaller than the workspace_bytes query answers");

  const Call c = call_of(q, k, v, q_stride, k_stride, v_stride, mask, batch, num_heads, len, q_scale, drop, stream);
  float* delta = static_cast<float*>(workspace);
  dispatch<QueryPass>(mask_kind, on, c, out, lse, grad_out, dq, (int64_t)dq_stride, delta);
  if ((rc = msda::launch_status())) return rc;
  dispatch<KeyPass>(mask_kind, on, c, lse, (const float*)delta, grad_out, dk, dv, (int64_t)dk_stride, (int64_t)dv_stride);
  if ((rc = msda::launch_status())) return rc;
  g_bert_bwd_last = kBackwardNames[mask_kind][on];
  return 0;
}

int bert_hip_dropout_keep_u8(const unsigned long long* seed, float dropout_p, int batch, int num_heads, int len,
                             unsigned char* keep, void* stream) {
  using namespace bert_attn_bwd;
  static const char* const kWho = "bert_dropout_keep";
  int rc = geometry(kWho, batch, num_heads, len, kD, BERT_MASK_NONE, {});
  if (rc) return rc;
  philox::Dropout drop;
  bool on = false;
  if ((rc = dropout_args(kWho, dropout_p, seed, (long long)batch * num_heads, drop, on))) return rc;
  if ((long long)batch * num_heads > 65535) return refuse(kWho, BERT_ERR_UNSUPPORTED, "batch * num_heads must be at most 65535 with dropout");
  if (batch == 0) return 0;
  if (!seed || !keep) return refuse(kWho, BERT_ERR_NULL_POINTER, "null pointer argument");
  if (reinterpret_cast<uintptr_t>(seed) % 8 != 0) return refuse(kWho, BERT_ERR_UNSUPPORTED, "the seed must be 8-byte aligned");
  const int64_t total = (int64_t)batch * num_heads * len * ((len + 3) / 4);   // < 2^16 * 2^9 * 2^7
  hipLaunchKernelGGL(dropout_keep, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), drop, len, total, keep);
  return msda::launch_status();
}

}  // extern "C"
