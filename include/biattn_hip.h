/*
 * include/biattn_hip.h -- C ABI of the fused bi-directional attention core of UNINEXT's early vision-language fusion layer
 * on MI355X (gfx950), part of libmsda_hip.so.  SURVEY.md 2b.
 *
 * The core of BiMultiHeadAttention.forward (projects/UNINEXT/uninext/models/deformable_detr/fuse_helper.py:52-139) between
 * the four input projections and the two output projections, at inference (dropout is the identity), with both clamps on and
 * STABLE_SOFTMAX_2D off (the shipped config).  For every batch b and head h, with D = head dimension, image tokens i < S and
 * text tokens j < T:
 *     s[i, j]   = min(max(sum_d (q[i, d] * q_scale) * k[j, d], -50000), 50000)        (q is scaled first, in fp32)
 *     p_l[j, i] = softmax_i(max(s[i, j] - max_i s[i, j], -50000))                     out_l[j, :] = sum_i p_l[j, i] * vv[i, :]
 *     p_v[i, j] = softmax_j(s[i, j] + m[b, j])                                        out_v[i, :] = sum_j p_v[i, j] * vl[j, :]
 * where m[b, j] is what the reference's `masked_fill(mask == 0, -9e15)` leaves of the text mask: -9e15f where the mask is 0 and
 * the mask's own value (1 for a tokenizer mask) elsewhere, ADDED in fp32 -- so a masked score is exactly -9e15f and a row whose
 * tokens are all masked is uniform over all T tokens.  The text mask is not applied on the text side and padded image tokens
 * take part, as in the reference.
 *
 * Exact fp32 products with fp32 accumulation on v_mfma_f32_32x32x2_f32, no float atomics.  Nothing of size B*H*S*T is written
 * to memory: one kernel keeps the scores of 128 image tokens x T text tokens in registers and finishes the image side there;
 * a second kernel recomputes the scores for the text side over a number of ranges of S that depends on the shapes only, keeps
 * a running max / sum / accumulator per range and writes them to the workspace; a third combines the ranges in range order.
 * Results are bitwise repeatable across runs and streams.
 *
 * All pointers are device pointers, contiguous; `stream` is a hipStream_t as void*; the kernels are only enqueued.  Returns
 * 0, a negative BIATTN_ERR_*, or a positive hipError_t; the message is available from msda_hip_last_error().  Every check
 * runs before the device is touched.
 */
#ifndef BIATTN_HIP_H_
#define BIATTN_HIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BIATTN_ERR_NULL_POINTER (-1)
#define BIATTN_ERR_BAD_DIMS (-2)
#define BIATTN_ERR_UNSUPPORTED (-5)   /* a head_dim, text_len, stride or alignment without a kernel, or an unknown mask kind */
#define BIATTN_ERR_WORKSPACE (-6)     /* workspace_bytes below biattn_hip_workspace_bytes */

#define BIATTN_MASK_NONE 0            /* mask is ignored (may be NULL): nothing is added */
#define BIATTN_MASK_INT64 1           /* mask [batch, text_len] int64 */
#define BIATTN_MASK_F32 2             /* mask [batch, text_len] fp32 (biattn_hip_self_forward_f32: [len, len] fp32, added) */
#define BIATTN_MASK_BOOL 3            /* biattn_hip_self_forward_f32 only: mask [len, len], one byte each, non-zero = excluded */

/* Bytes of scratch the text side needs (a function of the shapes only); 0 for bad or unsupported dimensions. */
size_t biattn_hip_workspace_bytes(int batch, int num_heads, int image_len, int text_len, int head_dim);

/*
 * q, vv   [batch, image_len, num_heads * head_dim]      v_proj(v) (NOT scaled) and values_v_proj(v)
 * k, vl   [batch, text_len,  num_heads * head_dim]      l_proj(l) and values_l_proj(l)
 * mask    [batch, text_len] of mask_kind, or NULL with BIATTN_MASK_NONE
 * out_v   [batch, image_len, num_heads * head_dim]      token-major: the input of out_v_proj
 * out_l   [batch, text_len,  num_heads * head_dim]      token-major: the input of out_l_proj
 * workspace: at least biattn_hip_workspace_bytes(...) bytes, owned by the caller, in use until the enqueued work is done.
 * Supported: head_dim == 256, 1 <= text_len <= 256, image_len >= 1, any batch and num_heads (an empty batch enqueues nothing).
 */
int biattn_hip_forward_f32(const float* q, const float* k, const float* vv, const float* vl, const void* mask, int mask_kind,
                           int batch, int num_heads, int image_len, int text_len, int head_dim, float q_scale,
                           float* out_v, float* out_l, void* workspace, size_t workspace_bytes, void* stream);

/* Names of the kernels the latest biattn_hip_forward_f32 call of this process enqueued ("" before the first call). */
const char* biattn_hip_last_kernel(void);

/*
 * The same core under autograd (opt-in from Python: BiMultiHeadAttention.own_training): a forward that also keeps two numbers
 * per row of each softmax, and a backward that recomputes both probabilities from them tile by tile.  Dropout is inactive.
 *
 * biattn_hip_train_f32: biattn_hip_forward_f32's arguments, limits and refusals; out_v and out_l are bitwise its results.  Plus
 *     stat_v [batch * num_heads, 2, roundup(image_len, 32)]: row 0 max_j a[i, j] with a = s + m, row 1 log sum_j exp(a - max)
 *     stat_l [batch * num_heads, 2, roundup(text_len, 32)]:  row 0 M[j] = max_i s[i, j], row 1 log L[j] with
 *            L[j] = sum_i exp(max(s[i, j] - M[j], -50000)), the ranges of S combined in range order as for out_l
 *     Columns past image_len / text_len hold 0.  TWO numbers, not one log-sum-exp: scores reach 5e4 here, where one fp32
 *     max + log sum would cost 4e-3 on every recomputed probability (see the decoder core below); p = exp((x - max) - logsum).
 *
 * biattn_hip_backward_f32: with r[i, j] = qs[i] . k[j] (qs = fp32(q * q_scale)), s = clamp(r), g_v = grad_out_v, g_l = grad_out_l,
 *     delta_v[i] = g_v[i] . out_v[i]                     delta_l[j] = g_l[j] . out_l[j]
 *     ds_v[i, j] = p_v[i, j] (g_v[i] . vl[j] - delta_v[i])
 *     ds_l[i, j] = p_l[j, i] (g_l[j] . vv[i] - delta_l[j])
 *     dr[i, j]   = (ds_v + ds_l)[i, j] * [-50000 <= r[i, j] <= 50000]     (torch.clamp: both ends pass the gradient)
 *     dq[i]  = q_scale * sum_j dr[i, j] k[j]             dk[j]  = sum_i dr[i, j] qs[i]
 *     dvl[j] = sum_i p_v[i, j] g_v[i]                    dvv[i] = sum_j p_l[j, i] g_l[j]
 *   The inner clamp and the max: a text-side entry with s - M < -50000 has p_l = exp(-50000 - log L) = 0 in fp32, so it adds
 *   nothing, and what autograd sends through torch.max to the argmax is sum_i ds_l[i, j], which is analytically zero: ds_l above
 *   is exact and the argmax routing is not imitated.  The mask gets no gradient.  A row of `a` that is all -9e15f is uniform
 *   over text_len and its ds_v is NOT zero: the gradient passes through the add, as in autograd.
 *   q .. q_scale as given to biattn_hip_train_f32; out_v, out_l, stat_v, stat_l its results; grad_out_v [batch, image_len, E] and
 *   grad_out_l [batch, text_len, E]; dq, dvv [batch, image_len, E] and dk, dvl [batch, text_len, E] (E = num_heads * head_dim).
 *   All tensors contiguous, token-major fp32 and, the mask apart, 16-byte aligned (BIATTN_ERR_UNSUPPORTED otherwise).
 *   workspace: at least biattn_hip_backward_workspace_bytes(...) bytes (BIATTN_ERR_WORKSPACE), 16-byte aligned: delta_v, delta_l
 *   and, per range of S, the partial dvl and the two partial halves of dk -- O(batch * heads * (S + T * ranges) * head_dim), a
 *   function of the shapes only, with the forward's number of ranges.
 * Every check runs before the device is touched; an empty batch enqueues nothing and returns 0.  Exact fp32 products on
 * v_mfma_f32_32x32x2_f32, every sum in one fixed order (ranges in range order, then dk = image-side half + text-side half), no
 * float atomics, every output element written by exactly one thread, nothing of size B * H * S * T written.  Bitwise repeatable
 * across runs and streams.
 */
size_t biattn_hip_backward_workspace_bytes(int batch, int num_heads, int image_len, int text_len, int head_dim);   /* 0: bad dimensions */

int biattn_hip_train_f32(const float* q, const float* k, const float* vv, const float* vl, const void* mask, int mask_kind,
                         int batch, int num_heads, int image_len, int text_len, int head_dim, float q_scale, float* out_v,
                         float* out_l, float* stat_v, float* stat_l, void* workspace, size_t workspace_bytes, void* stream);

int biattn_hip_backward_f32(const float* q, const float* k, const float* vv, const float* vl, const void* mask, int mask_kind,
                            const float* out_v, const float* out_l, const float* stat_v, const float* stat_l,
                            const float* grad_out_v, const float* grad_out_l, int batch, int num_heads, int image_len,
                            int text_len, int head_dim, float q_scale, float* dq, float* dk, float* dvv, float* dvl,
                            void* workspace, size_t workspace_bytes, void* stream);

/* Names of the kernels the latest biattn_hip_backward_f32 or biattn_hip_backward_dropout_f32 call of this process enqueued (""
 * before the first call); the second's carry "_dropout". */
const char* biattn_hip_backward_last_kernel(void);

/*
 * The training route with ACTIVE DROPOUT on both attention probabilities, as fuse_helper.py has it after each softmax
 * (p_v = dropout(softmax_v), p_l = dropout(softmax_l)), opt-in from Python: BiMultiHeadAttention.own_dropout.  The keep
 * decisions come from a counter-based generator inside the kernels (Philox4x32-10, uninext_amd/csrc/philox.hpp): no keep mask
 * and nothing of size B * H * S * T is written in the forward or in the backward, and the backward reproduces the forward's
 * mask by recomputation.
 *
 * The decision for entry (i, j) is a pure function of (seed, offset, side, b * num_heads + h, image token i, text token j):
 * independent of tile, range, wave, launch geometry and of which kernel asks.  With seed[0] the seed and seed[1] the offset:
 *     key     = (seed & 0xffffffff, seed >> 32)
 *     counter = (offset & 0xffffffff, offset >> 32, i, side << 31 | (b * num_heads + h) << 8 | j / 4)
 *     word j % 4 of Philox4x32-10(counter, key) decides:  keep <=> word >= (uint32) llrint(dropout_p * 2^32)
 * side 0 is the image side (m_v[i, j] on p_v[i, j]), side 1 the text side (m_l[j, i] on p_l[j, i]): two independent masks.  One
 * call decides four consecutive text tokens of one image token on BOTH sides.  dropout_p = 0 keeps everything.  Kept
 * probabilities are multiplied by c = 1.0f / (1.0f - dropout_p), computed on the host in fp32.
 *
 * `seed` is a DEVICE pointer to two unsigned long long values (seed, offset) that the kernels read: no host copy and no
 * synchronisation.  It has to hold the same values for the forward and its backward.
 *
 * With m_v, m_l the keep indicators and p_v, p_l the UNDROPPED probabilities from the kept statistics:
 *     out_v[i] = sum_j c m_v[i, j] p_v[i, j] vl[j]       out_l[j] = sum_i c m_l[j, i] p_l[j, i] vv[i]
 *     stat_v, stat_l: unchanged, bitwise biattn_hip_train_f32's (the softmax sums run over ALL entries; dropout comes after
 *                     the normalisation)
 *     delta_v[i] = g_v[i] . out_v[i]                     delta_l[j] = g_l[j] . out_l[j]
 *                  (unchanged in form: sum_j p (c m (g . vl)) is g . out of the dropped output)
 *     ds_v[i, j] = p_v[i, j] (c m_v[i, j] (g_v[i] . vl[j]) - delta_v[i])
 *     ds_l[i, j] = p_l[j, i] (c m_l[j, i] (g_l[j] . vv[i]) - delta_l[j])
 *     dvl[j] = sum_i c m_v[i, j] p_v[i, j] g_v[i]        dvv[i] = sum_j c m_l[j, i] p_l[j, i] g_l[j]
 *     dr, dq, dk: as in biattn_hip_backward_f32
 * The clamp gate, the inner clamp, the mask and the all-masked row behave as there.
 *
 * biattn_hip_train_dropout_f32 / biattn_hip_backward_dropout_f32: the arguments, limits, workspace sizes and refusals of
 * biattn_hip_train_f32 / biattn_hip_backward_f32, plus dropout_p and seed, which are checked FIRST: a null seed is
 * BIATTN_ERR_NULL_POINTER, a dropout_p outside [0, 1) or NaN is BIATTN_ERR_BAD_DIMS.  Every check runs before the device is
 * touched.  With dropout_p = 0 every result is bitwise that of the entry point without dropout (a multiply by 1.0f and an
 * all-keep mask change no bit).  Bitwise repeatable across runs and streams for one (seed, offset).
 */
int biattn_hip_train_dropout_f32(const float* q, const float* k, const float* vv, const float* vl, const void* mask, int mask_kind,
                                 int batch, int num_heads, int image_len, int text_len, int head_dim, float q_scale, float* out_v,
                                 float* out_l, float* stat_v, float* stat_l, void* workspace, size_t workspace_bytes, float dropout_p,
                                 const unsigned long long* seed, void* stream);

int biattn_hip_backward_dropout_f32(const float* q, const float* k, const float* vv, const float* vl, const void* mask, int mask_kind,
                                    const float* out_v, const float* out_l, const float* stat_v, const float* stat_l,
                                    const float* grad_out_v, const float* grad_out_l, int batch, int num_heads, int image_len,
                                    int text_len, int head_dim, float q_scale, float* dq, float* dk, float* dvv, float* dvl,
                                    void* workspace, size_t workspace_bytes, float dropout_p,
                                    const unsigned long long* seed, void* stream);

/*
 * FOR TESTS AND TOOLS: the keep decisions of the two entry points above written out as bytes (1 = kept), by the kernels' own
 * device function -- the only place where a mask of full size exists.  keep_v [batch * num_heads, image_len, text_len] and
 * keep_l [batch * num_heads, text_len, image_len], device pointers.  The geometry limits of the core (text_len <= 256), the
 * refusals of seed and dropout_p above, BIATTN_ERR_NULL_POINTER for a null output; an empty batch enqueues nothing and returns 0.
 */
int biattn_hip_dropout_keep_u8(const unsigned long long* seed, float dropout_p, int batch, int num_heads, int image_len, int text_len,
                               unsigned char* keep_v, unsigned char* keep_l, void* stream);

/*
 * Self-attention core of the decoder layers: nn.MultiheadAttention among the queries (DeformableTransformerDecoderLayer,
 * deformable_transformer_dino.py:385, :411-412) between its input projections and out_proj, at inference, with the 2-D
 * attn_mask of the denoising queries.  For every batch b, head h and query i, with D = head_dim:
 *     s[i, j]   = sum_d (q[i, d] * q_scale) * k[j, d] + m[i, j]                       (q is scaled first, in fp32)
 *     out[i, :] = sum_j softmax_j(s[i, :])[j] * v[j, :]
 * m[i, j] is 0 without a mask, the fp32 mask's element (it may be -inf), or -inf where the bool mask's byte is non-zero; the
 * same [len, len] mask serves every batch and head.  A query whose keys are ALL excluded gets NaN in all its channels, which is
 * what softmax over a row of -inf gives in the PyTorch composition; any query with one open key is finite, however many whole
 * stretches of keys are excluded before or after it.
 *
 * q, k, v   [batch, len, num_heads * head_dim] each, rows q_stride / k_stride / v_stride floats apart (batches len rows apart):
 *           q and k may be the two halves of one [batch, len, 2 * E] projection output, read in place
 * mask      [len, len] of mask_kind (row = query, column = key), or NULL with BIATTN_MASK_NONE
 * out       [batch, len, num_heads * head_dim], contiguous, token-major: the input of out_proj
 * Supported: head_dim == 32, 1 <= len <= 65535, any batch and num_heads (an empty batch enqueues nothing and returns 0);
 * q, k, v, out 16-byte aligned, strides multiples of 4 and at least num_heads * head_dim.  v is to be finite.
 *
 * Exact fp32 products with fp32 accumulation on v_mfma_f32_32x32x2_f32 in a fixed order, no float atomics, no workspace, and
 * nothing of size batch * heads * len * len is written: a workgroup keeps 32 queries, its two waves take one half of the keys
 * each and are combined in that order.  Bitwise repeatable across runs and streams.
 */
int biattn_hip_self_forward_f32(const float* q, const float* k, const float* v, long long q_stride, long long k_stride,
                                long long v_stride, const void* mask, int mask_kind, int batch, int num_heads, int len,
                                int head_dim, float q_scale, float* out, void* stream);

/* Name of the kernel the latest biattn_hip_self_forward_f32 call of this process enqueued ("" before the first call);
 * biattn_hip_last_kernel does not see these calls. */
const char* biattn_hip_self_last_kernel(void);

/*
 * The same core under autograd (opt-in from Python: DeformableTransformerDecoderLayer.own_training): a forward that also
 * keeps the row log-sum-exp, and a backward that recomputes the probabilities from it tile by tile.
 *
 * biattn_hip_self_train_f32: biattn_hip_self_forward_f32's arguments, limits and result (`out` is bitwise the same), plus
 *     lse [batch * num_heads, roundup(len, 32)], 16-byte aligned:  lse[b * num_heads + h, i] = log sum_j exp(s[i, j]) for
 *     i < len, -inf for a query whose keys are all excluded, 0 for the rows past len.
 *
 * biattn_hip_self_backward_f32: with g = grad_out, p[i, j] = exp(s[i, j] - lse[i]) and delta[i] = sum_d g[i, d] * out[i, d],
 *     dp[i, j] = sum_d g[i, d] * v[j, d]                 ds[i, j] = p[i, j] * (dp[i, j] - delta[i])
 *     dq[i, :] = q_scale * sum_j ds[i, j] * k[j, :]      dk[j, :] = sum_i ds[i, j] * (q[i, :] * q_scale)
 *     dv[j, :] = sum_i p[i, j] * g[i, :]
 * (s as above, from the scaled q rounded in fp32 and the same mask; the mask gets no gradient.)
 *   q, k, v, strides, mask, mask_kind, q_scale    as given to biattn_hip_self_train_f32
 *   out, lse                                      its results;  grad_out [batch, len, num_heads * head_dim], contiguous
 *   dq, dk, dv   [batch, len, num_heads * head_dim] each, rows dq_stride / dk_stride / dv_stride floats apart (batches len rows
 *                apart): dq and dk may be the two halves of one [batch, len, 2 * E] buffer, as q and k are.  Every element is
 *                written by exactly one thread.
 *   workspace    at least biattn_hip_self_backward_workspace_bytes(...) bytes (delta), owned by the caller, 16-byte aligned,
 *                in use until the enqueued work is done.
 * Supported: what the forward supports, the same limits on the three gradient strides, all pointers but the mask 16-byte
 * aligned; failures are the same BIATTN_ERR_* codes (BIATTN_ERR_WORKSPACE for a workspace that is too small), every check runs
 * before the device is touched, and an empty batch enqueues nothing and returns 0.
 *
 * A query with EVERY key excluded (out already NaN): its dq row is NaN in all channels, and FOR A FINITE grad_out ROW it
 * contributes exactly nothing to dk and dv, which stay finite: the bits are those of the call with that grad_out row zeroed.
 * This DEVIATES from the PyTorch composition, where the NaN probabilities of that row turn all of dk and dv of its
 * (batch, head) into NaN; the loss is NaN either way.  A NaN or infinity in that query's grad_out row is multiplied by its zero
 * probabilities in the key pass and can make dk and dv of that (batch, head) NaN, as in the composition: for every key whose
 * workgroup streams the query's tile (a tile that is skipped is not loaded, and those keys stay finite); no other
 * (batch, head) is touched, and neither is dq.
 *
 * lse is ONE fp32 number per query.  Where |lse| is large its rounding (up to 2^-11 at |lse| = 1e4) becomes, through
 * exp(s - lse), a common relative error of that query's recomputed probabilities and so of its share of dq, dk and dv: at
 * scores of +-1e4 the gradients are good to about 5e-4 of their size, not to the 1e-4 held elsewhere.
 *
 * Two kernels, a query pass (dq, delta) and a key pass (dk, dv), on the forward's grid and its split of the streamed tiles
 * between a workgroup's two waves; a streamed tile in which no owned token has an open partner is skipped, by the forward's
 * test, so a bool mask and its -inf fp32 form give the same bits.  Exact fp32 products, every sum in one fixed order, no float
 * atomics, nothing of size batch * heads * len * len is written.  Bitwise repeatable across runs and streams.
 */
size_t biattn_hip_self_backward_workspace_bytes(int batch, int num_heads, int len, int head_dim);   /* 0: bad dimensions */

int biattn_hip_self_train_f32(const float* q, const float* k, const float* v, long long q_stride, long long k_stride,
                              long long v_stride, const void* mask, int mask_kind, int batch, int num_heads, int len,
                              int head_dim, float q_scale, float* out, float* lse, void* stream);

int biattn_hip_self_backward_f32(const float* q, const float* k, const float* v, long long q_stride, long long k_stride,
                                 long long v_stride, const void* mask, int mask_kind, const float* out, const float* lse,
                                 const float* grad_out, int batch, int num_heads, int len, int head_dim, float q_scale, float* dq,
                                 float* dk, float* dv, long long dq_stride, long long dk_stride, long long dv_stride,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* Names of the kernels the latest biattn_hip_self_backward_f32 call of this process enqueued ("" before the first call); they
 * tell the mask kind: "dec_bwd_q<none>+dec_bwd_kv<none>", "...<bool>...", "...<f32>...". */
const char* biattn_hip_self_backward_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif /* BIATTN_HIP_H_ */
