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
//
// The kernel's text, the constants and the argument checks are in dec_attn_launch.hpp: the training route (dec_attn_bwd.hip) runs
// the same forward with the row log-sum-exp stored, and checks its arguments by the same rules.
#include "dec_attn_launch.hpp"

namespace dec_attn {

// grid (batch * heads * NG), NG = groups of 32 queries.  MASK: BIATTN_MASK_NONE / _BOOL / _F32.  The body is fwd<MASK, false>
// of dec_attn_launch.hpp.
template <int MASK>
__global__ void __launch_bounds__(kThreads)
attn(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int64_t qs, int64_t ks, int64_t vs,
     const void* __restrict__ mask, int heads, int L, int NG, float scale, float* __restrict__ out) {
  fwd<MASK, false>(q, k, v, qs, ks, vs, mask, heads, L, 0, NG, scale, out, nullptr);
}

}  // namespace dec_attn

extern "C" {

static const char* g_dec_attn_last = "";

const char* biattn_hip_self_last_kernel(void) { return g_dec_attn_last; }

int biattn_hip_self_forward_f32(const float* q, const float* k, const float* v, long long q_stride, long long k_stride,
                                long long v_stride, const void* mask, int mask_kind, int batch, int num_heads, int len, int head_dim,
                                float q_scale, float* out, void* stream) {
  using namespace dec_attn;
  static const char* const kWho = "dec_attn";
  int rc = geometry(kWho, batch, num_heads, len, head_dim, mask_kind, {q_stride, k_stride, v_stride});
  if (rc) return rc;
  if (batch == 0) return 0;   // nothing to enqueue, no buffer is looked at
  if (!q || !k || !v || !out || (mask_kind != BIATTN_MASK_NONE && !mask))
    return refuse(kWho, BIATTN_ERR_NULL_POINTER, "null pointer argument");
  if (!msda::aligned16({q, k, v, out})) return refuse(kWho, BIATTN_ERR_UNSUPPORTED, "q, k, v and out must be 16-byte aligned");
  if ((rc = mask_pointer(kWho, mask, mask_kind))) return rc;   // the mask is there: its alignment

  hipStream_t st = static_cast<hipStream_t>(stream);
  const int NG = msda::ceil_div(len, kTile);
  const dim3 grid((unsigned)((long long)batch * num_heads * NG)), block(kThreads);
#define DEC_ATTN_LAUNCH(KIND)                                                                                               \
  hipLaunchKernelGGL(attn<KIND>, grid, block, 0, st, q, k, v, (int64_t)q_stride, (int64_t)k_stride, (int64_t)v_stride, mask, \
                     num_heads, len, NG, q_scale, out)
  if (mask_kind == BIATTN_MASK_NONE) DEC_ATTN_LAUNCH(BIATTN_MASK_NONE);
  else if (mask_kind == BIATTN_MASK_BOOL) DEC_ATTN_LAUNCH(BIATTN_MASK_BOOL);
  else DEC_ATTN_LAUNCH(BIATTN_MASK_F32);
#undef DEC_ATTN_LAUNCH
  if (const int e = msda::launch_status()) return e;
  g_dec_attn_last = mask_kind == BIATTN_MASK_NONE ? "dec_attn<none>" : mask_kind == BIATTN_MASK_BOOL ? "dec_attn<bool>" : "dec_attn<f32>";
  return 0;
}

}  // extern "C"
