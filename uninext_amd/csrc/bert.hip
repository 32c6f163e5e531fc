// The text encoder's two kernels (BERT of bert-base geometry) -- see include/dynmask_hip.h (bert_hip_self_attention_f32,
// bert_hip_embed_layernorm_f32).
//
// attn: the streamed-attention tile scheme (attn_tile.hpp) as self-attention for head dimension 64 with a KEEP flag per key.  As
// in dec_attn, batch * heads is small (24 at bs 2), so a workgroup takes 32 queries and its TWO waves own the SAME 32 queries
// and split the key tiles between them, each through an LDS tile of its own; wave 1 hands (max, sum, accumulator) over through
// LDS and wave 0 combines the two in range order and stores.  bs 2 x 12 heads x 256 tokens: 192 workgroups of 4 tiles a wave.
//
// The mask.  A key-mask kind ([B, T]) is one flag per streamed row, the same for every query: lane l loads the flag of row
// l % 32 and a ballot turns the tile's 32 flags into a wave-uniform word.  The full kind ([B, T, T]) is a byte per (query, key),
// loaded per register as dec_attn loads its mask.  An excluded key is -inf in the score tile, so it enters neither the max nor
// the sum and its probability is exactly 0.  What differs from dec_attn:
//   * a tile in which no query of the wave keeps a key is not even LOADED (its liveness is known one tile ahead): at 256-token
//     padding most tiles of a short prompt are empty.  Such a tile would have left max, sum and accumulator as they are;
//   * a query that keeps no key ends with sum 0 and accumulator 0 and is stored as ZEROS, not NaN.
//
// embed: BertEmbeddings + LayerNorm, one wave per token, layernorm.hip's register layout and sum order.
#include "../../include/dynmask_hip.h"

#include <stdio.h>

#include "attn_tile.hpp"
#include "launch_glue.hpp"
#include "msda_common.hpp"

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

// grid (batch * heads * NG), NG = groups of 32 queries
template <int MASK>
__global__ void __launch_bounds__(kThreads)
attn(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int64_t qs, int64_t ks, int64_t vs,
     const void* __restrict__ mask, int heads, int T, int NG, float scale, float* __restrict__ out) {
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

    f32x16 X;
#pragma unroll
    for (int u = 0; u < 16; ++u) X[u] = 0.f;
    if (live) {
      scores<kD>(Tw, own, X, r32, half);
#pragma unroll
      for (int u = 0; u < 16; ++u) X[u] += add[u];
      rescale(acc, softmax_step<true, false>(X, m_run, l_run));     // guarded: this query may have kept nothing yet
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
  }
}

// ---- embeddings ---------------------------------------------------------------------------------
using wave_ops::wave_sum;
constexpr int kEmbedThreads = 256, kMaxChunks = 16;   // 16 float4 per lane = 4096 features

template <int CHUNKS>   // float4 chunks per lane: hidden <= CHUNKS * 256
__global__ void __launch_bounds__(kEmbedThreads)
embed(const long long* __restrict__ ids, const long long* __restrict__ tts, const float* __restrict__ word,
      const float* __restrict__ position, const float* __restrict__ type, const float* __restrict__ gamma,
      const float* __restrict__ beta, float eps, long long rows, int T, int hidden, int vocab, int type_vocab,
      float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (kEmbedThreads / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nvec = hidden / 4;
  const int t = (int)(row % T);                                     // < max_positions: checked by the host
  const long long id = ids[row], tt = tts ? tts[row] : 0;           // wave-uniform
  f32x4* orow = reinterpret_cast<f32x4*>(out + row * hidden);
  if (id < 0 || id >= vocab || tt < 0 || tt >= type_vocab) {        // no table row to read: the row is NaN
    const float nan = __builtin_nanf("");
    for (int i = lane; i < nvec; i += 64) orow[i] = f32x4{nan, nan, nan, nan};
    return;
  }
  const f32x4* wr = reinterpret_cast<const f32x4*>(word + id * hidden);
  const f32x4* tr = reinterpret_cast<const f32x4*>(type + tt * hidden);
  const f32x4* pr = reinterpret_cast<const f32x4*>(position + (long long)t * hidden);
  f32x4 v[CHUNKS];
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    const int i = c * 64 + lane;
    v[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (i < nvec) {
      v[c] = (wr[i] + tr[i]) + pr[i];
      sum += (v[c][0] + v[c][1]) + (v[c][2] + v[c][3]);
    }
  }
  const float mean = wave_sum(sum) / (float)hidden;
  float sq = 0.f;
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    const int i = c * 64 + lane;
    if (i < nvec) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float dlt = v[c][e] - mean;
        sq += dlt * dlt;
      }
    }
  }
  const float rstd = rsqrtf(wave_sum(sq) / (float)hidden + eps);
  const f32x4* gv = reinterpret_cast<const f32x4*>(gamma);
  const f32x4* bv = reinterpret_cast<const f32x4*>(beta);
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    const int i = c * 64 + lane;
    if (i < nvec) {
      f32x4 r;
      const f32x4 g = gv[i], bb = bv[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = (v[c][e] - mean) * rstd * g[e] + bb[e];
      orow[i] = r;
    }
  }
}

// sets "<who>: <what>" as the thread's last error (msda::set_error copies the text) and returns `code`
static int refuse(const char* who, int code, const char* what) {
  char text[160];
  snprintf(text, sizeof(text), "%s: %s", who, what);
  return msda::set_error(code, text);
}

}  // namespace bert

extern "C" {

static const char* g_bert_attn_last = "";
static const char* g_bert_embed_last = "";

const char* bert_hip_attention_last_kernel(void) { return g_bert_attn_last; }
const char* bert_hip_embed_last_kernel(void) { return g_bert_embed_last; }

int bert_hip_self_attention_f32(const float* q, const float* k, const float* v, long long q_stride, long long k_stride,
                                long long v_stride, const void* mask, int mask_kind, int batch, int num_heads, int len, int head_dim,
                                float q_scale, float* out, void* stream) {
  using namespace bert;
  static const char* const kWho = "bert_attn";
  if (batch < 0 || num_heads <= 0 || len <= 0 || head_dim <= 0) return refuse(kWho, BERT_ERR_BAD_DIMS, "bad dimensions");
  if (head_dim != kD) return refuse(kWho, BERT_ERR_UNSUPPORTED, "head_dim must be 64");
  if (len > kMaxLen) return refuse(kWho, BERT_ERR_UNSUPPORTED, "len must be at most 512");
  if (mask_kind != BERT_MASK_NONE && mask_kind != BERT_MASK_KEY_I64 && mask_kind != BERT_MASK_KEY_U8 && mask_kind != BERT_MASK_FULL_U8)
    return refuse(kWho, BERT_ERR_UNSUPPORTED, "unknown mask kind (none, key int64, key u8 or full u8)");
  const long long E = (long long)num_heads * kD, NG = msda::ceil_div(len, kTile);
  for (long long s : {q_stride, k_stride, v_stride}) {
    if (s < E) return refuse(kWho, BERT_ERR_BAD_DIMS, "a row stride is smaller than num_heads * head_dim");
    if (s % 4 != 0) return refuse(kWho, BERT_ERR_UNSUPPORTED, "row strides must be multiples of 4 floats");
    if (s >= (1ll << 31) || (long long)batch * len * s >= (1ll << 42)) return refuse(kWho, BERT_ERR_BAD_DIMS, "problem too large");
  }
  if ((long long)batch * num_heads * NG >= (1ll << 31)) return refuse(kWho, BERT_ERR_BAD_DIMS, "problem too large");
  if (batch == 0) return 0;   // nothing to enqueue, no buffer is looked at
  if (!q || !k || !v || !out || (mask_kind != BERT_MASK_NONE && !mask)) return refuse(kWho, BERT_ERR_NULL_POINTER, "null pointer argument");
  if (!msda::aligned16({q, k, v, out})) return refuse(kWho, BERT_ERR_UNSUPPORTED, "q, k, v and out must be 16-byte aligned");
  if (mask_kind == BERT_MASK_KEY_I64 && reinterpret_cast<uintptr_t>(mask) % 8 != 0)
    return refuse(kWho, BERT_ERR_UNSUPPORTED, "an int64 mask must be 8-byte aligned");

  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((long long)batch * num_heads * NG)), block(kThreads);
#define BERT_ATTN_LAUNCH(KIND)                                                                                                 \
  hipLaunchKernelGGL(attn<KIND>, grid, block, 0, st, q, k, v, (int64_t)q_stride, (int64_t)k_stride, (int64_t)v_stride, mask, \
                     num_heads, len, (int)NG, q_scale, out)
  if (mask_kind == BERT_MASK_NONE) BERT_ATTN_LAUNCH(BERT_MASK_NONE);
  else if (mask_kind == BERT_MASK_KEY_I64) BERT_ATTN_LAUNCH(BERT_MASK_KEY_I64);
  else if (mask_kind == BERT_MASK_KEY_U8) BERT_ATTN_LAUNCH(BERT_MASK_KEY_U8);
  else BERT_ATTN_LAUNCH(BERT_MASK_FULL_U8);
#undef BERT_ATTN_LAUNCH
  if (const int e = msda::launch_status()) return e;
  g_bert_attn_last = mask_kind == BERT_MASK_NONE      ? "bert_attn<none>"
                     : mask_kind == BERT_MASK_KEY_I64 ? "bert_attn<key_i64>"
                     : mask_kind == BERT_MASK_KEY_U8  ? "bert_attn<key_u8>"
                                                      : "bert_attn<full_u8>";
  return 0;
}

int bert_hip_embed_layernorm_f32(const long long* ids, const long long* token_type_ids, const float* word, const float* position,
                                 const float* type, const float* gamma, const float* beta, float eps, int batch, int len, int hidden,
                                 int vocab, int max_positions, int type_vocab, float* out, void* stream) {
  using namespace bert;
  static const char* const kWho = "bert_embed";
  if (batch < 0 || len <= 0 || hidden <= 0 || vocab <= 0 || max_positions <= 0 || type_vocab <= 0)
    return refuse(kWho, BERT_ERR_BAD_DIMS, "bad dimensions");
  if (hidden % 4 != 0 || hidden > kMaxChunks * 256) return refuse(kWho, BERT_ERR_UNSUPPORTED, "hidden must be a multiple of 4 and <= 4096");
  if (len > max_positions) return refuse(kWho, BERT_ERR_BAD_DIMS, "len exceeds the position table");
  const long long rows = (long long)batch * len, blocks = msda::ceil_div(rows, (long long)(kEmbedThreads / 64));
  if (blocks >= (1ll << 31)) return refuse(kWho, BERT_ERR_BAD_DIMS, "problem too large");
  if (batch == 0) return 0;
  if (!ids || !word || !position || !type || !gamma || !beta || !out) return refuse(kWho, BERT_ERR_NULL_POINTER, "null pointer argument");
  if (!msda::aligned16({word, position, type, gamma, beta, out})) return refuse(kWho, BERT_ERR_UNSUPPORTED, "tables, gamma, beta and out must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(ids) % 8 != 0 || reinterpret_cast<uintptr_t>(token_type_ids) % 8 != 0)
    return refuse(kWho, BERT_ERR_UNSUPPORTED, "ids must be 8-byte aligned");

  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)blocks), block(kEmbedThreads);
  const int chunks = (hidden / 4 + 63) / 64;
#define BERT_EMBED_LAUNCH(C)                                                                                                  \
  hipLaunchKernelGGL((embed<C>), grid, block, 0, st, ids, token_type_ids, word, position, type, gamma, beta, eps, rows, len, \
                     hidden, vocab, type_vocab, out)
  if (chunks <= 1) BERT_EMBED_LAUNCH(1);
  else if (chunks <= 2) BERT_EMBED_LAUNCH(2);
  else if (chunks <= 4) BERT_EMBED_LAUNCH(4);
  else if (chunks <= 8) BERT_EMBED_LAUNCH(8);
  else BERT_EMBED_LAUNCH(16);
#undef BERT_EMBED_LAUNCH
  if (const int e = msda::launch_status()) return e;
  g_bert_embed_last = token_type_ids ? "bert_embed<types>" : "bert_embed";
  return 0;
}

}  // extern "C"
