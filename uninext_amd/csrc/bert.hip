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
#include "bert_attn_common.hpp"

namespace bert {

// grid (batch * heads * NG), NG = groups of 32 queries.  The text is bert_attn_common.hpp's fwd, shared with the training route.
template <int MASK>
__global__ void __launch_bounds__(kThreads)
attn(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int64_t qs, int64_t ks, int64_t vs,
     const void* __restrict__ mask, int heads, int T, int NG, float scale, float* __restrict__ out) {
  fwd<MASK, false, false>(q, k, v, qs, ks, vs, mask, heads, T, 0, NG, scale, out, nullptr);
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
  if (const int rc = geometry(kWho, batch, num_heads, len, head_dim, mask_kind, {q_stride, k_stride, v_stride})) return rc;
  const int NG = msda::ceil_div(len, kTile);
  if (batch == 0) return 0;   // nothing to enqueue, no buffer is looked at
  if (!q || !k || !v || !out || (mask_kind != BERT_MASK_NONE && !mask)) return refuse(kWho, BERT_ERR_NULL_POINTER, "null pointer argument");
  if (!msda::aligned16({q, k, v, out})) return refuse(kWho, BERT_ERR_UNSUPPORTED, "q, k, v and out must be 16-byte aligned");
  if (mask_kind == BERT_MASK_KEY_I64 && reinterpret_cast<uintptr_t>(mask) % 8 != 0)
    return refuse(kWho, BERT_ERR_UNSUPPORTED, "an int64 mask must be 8-byte aligned");

  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((long long)batch * num_heads * NG)), block(kThreads);
#define BERT_ATTN_LAUNCH(KIND)                                                                                                 \
  hipLaunchKernelGGL(attn<KIND>, grid, block, 0, st, q, k, v, (int64_t)q_stride, (int64_t)k_stride, (int64_t)v_stride, mask, \
                     num_heads, len, NG, q_scale, out)
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
