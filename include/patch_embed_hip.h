/*
 * include/patch_embed_hip.h -- C ABI of the backbone's kernels of UNINEXT on MI355X (gfx950), part of libmsda_hip.so: the
 * patch-embedding convolutions and, further down, the ConvNeXt block's fused depthwise 7x7 + LayerNorm,
 * its layer-scale + residual tail and the channels-first LayerNorm, and at the end the ViT blocks' fused attention core
 * with decomposed relative positions.
 *
 * A convolution whose kernel size equals its stride, without padding, is a GEMM over non-overlapping patches:
 *     out[b, py, px, e] = bias[e] + sum_{c, ky, kx} x[b, c, py*k + ky, px*k + kx] * weight[e, c, ky, kx]
 * with M = B * (H / k) * (W / k) rows, N = E columns, K = C * k * k.  Replaces
 *   - ViT   PatchEmbed.proj + permute   projects/UNINEXT/uninext/backbone/utils.py:177-186   (k = 16, 3 -> 768/1280,
 *                                       constructed at uninext/backbone/vit.py:291)         channels_last = 1
 *   - ConvNeXt stem conv                projects/UNINEXT/uninext/backbone/convnext.py:80     (k = 4, 3 -> 96/192/...)
 *   - ConvNeXt downsample convs         projects/UNINEXT/uninext/backbone/convnext.py:87     (k = 2, C -> 2C)
 * by one implicit-GEMM kernel: the patches are never materialised (no im2col buffer); 128 x 128 x 16 tiles are staged
 * through double-buffered LDS and multiplied with v_mfma_f32_32x32x2_f32 -- exact fp32 (an fmaf chain in k order), so
 * results match nn.Conv2d to fp32 round-off; there is no TF32-like mode on gfx950.
 *
 * Rows/columns that do not fill a tile are masked; H and W need not be multiples of k (the remainder is ignored, as
 * nn.Conv2d does).  All pointers are device pointers, contiguous fp32; `bias` may be NULL; `stream` is a hipStream_t
 * as void*; the kernel is only enqueued.  Returns 0, a negative PATCH_EMBED_ERR_*, or a positive hipError_t; the
 * message is available from msda_hip_last_error().
 */
#ifndef PATCH_EMBED_HIP_H_
#define PATCH_EMBED_HIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PATCH_EMBED_ERR_NULL_POINTER (-1)
#define PATCH_EMBED_ERR_BAD_DIMS (-2)
#define PATCH_EMBED_ERR_UNSUPPORTED (-5)   /* patch not in {2, 4, 8, 16} or C * patch^2 not a multiple of 16 */
#define PATCH_EMBED_ERR_WORKSPACE (-6)     /* backward: workspace_bytes below patch_embed_hip_backward_workspace_bytes */

/*
 * x       [batch, in_chans, height, width]
 * weight  [embed_dim, in_chans, patch, patch]        (nn.Conv2d layout)
 * bias    [embed_dim] or NULL
 * out     channels_last != 0: [batch, height / patch, width / patch, embed_dim]   (PatchEmbed.forward, after its permute)
 *         channels_last == 0: [batch, embed_dim, height / patch, width / patch]   (nn.Conv2d)
 */
int patch_embed_hip_f32(const float* x, const float* weight, const float* bias, int batch, int in_chans, int height,
                        int width, int embed_dim, int patch, int channels_last, float* out, void* stream);

/*
 * Fast path for inference with fixed weights: split-bf16 products.  Every fp32 operand is split into two bf16 halves
 * (x = hi + lo, 16 mantissa bits kept) and a product is hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 with fp32
 * accumulation: ~2e-5 of the output scale (inside the 1e-4 parity bound of this path) at 3/16 of the matrix-pipe time
 * of the exact kernel.  The weights are split and re-ordered ONCE by patch_embed_hip_pack_weight_f32 into a
 * caller-owned device buffer of patch_embed_hip_packed_weight_bytes(...) bytes (0 = unsupported geometry: patch not
 * in {2, 4, 8, 16} or in_chans * patch^2 not a multiple of 48); patch_embed_hip_packed_f32 then takes that buffer in
 * place of `weight`.  Same argument meaning and layouts as patch_embed_hip_f32.
 */
size_t patch_embed_hip_packed_weight_bytes(int embed_dim, int in_chans, int patch);
int patch_embed_hip_pack_weight_f32(const float* weight, int embed_dim, int in_chans, int patch, void* packed, void* stream);
int patch_embed_hip_packed_f32(const float* x, const void* packed, const float* bias, int batch, int in_chans, int height,
                               int width, int embed_dim, int patch, int channels_last, float* out, void* stream);

/*
 * BACKWARD of patch_embed_hip_f32, for training.  With G = grad_out as the [M, E] matrix of the forward's output:
 *     grad_weight[e, c, ky, kx]                = sum_m G[m, e] * x[b, c, py*patch + ky, px*patch + kx]
 *     grad_bias[e]                             = sum_m G[m, e]
 *     grad_x[b, c, py*patch + ky, px*patch + kx] = sum_e G[m, e] * weight[e, c, ky, kx]
 * and grad_x = 0 in the rows / columns past (height / patch) * patch and (width / patch) * patch, which no patch covers (only those
 * pixels are zeroed).  grad_out has the forward's output layout: [batch, height / patch, width / patch, embed_dim] when
 * channels_last != 0, else [batch, embed_dim, height / patch, width / patch]; both are read in place.  Exact fp32 products,
 * fp32 accumulation in a fixed order on v_mfma_f32_32x32x2_f32, no float atomics: bitwise repeatable across runs, streams and
 * processes.  The reduction of grad_weight over the patches is split into a number of ranges that depends on the shape only;
 * the partial sums go to the workspace and are added in split order, grad_bias likewise.
 *
 * Each of grad_x [batch, in_chans, height, width], grad_weight [embed_dim, in_chans, patch, patch] and grad_bias [embed_dim] may
 * be NULL and its part is skipped; x may be NULL when grad_weight is, weight when grad_x is.  workspace: a device buffer of at
 * least patch_embed_hip_backward_workspace_bytes(...) bytes (a function of the shape only; 0 for bad dimensions or an unsupported
 * geometry), owned by the caller and in use until the enqueued work has finished; needed only for grad_weight / grad_bias.  An
 * empty batch (or an image smaller than one patch) writes zeros into grad_weight and grad_bias.  Every check runs before the
 * device is touched; a short workspace returns PATCH_EMBED_ERR_WORKSPACE.
 */
size_t patch_embed_hip_backward_workspace_bytes(int batch, int in_chans, int height, int width, int embed_dim, int patch);
int patch_embed_hip_backward_f32(const float* x, const float* weight, const float* grad_out, int batch, int in_chans,
                                 int height, int width, int embed_dim, int patch, int channels_last,
                                 float* grad_x, float* grad_weight, float* grad_bias,
                                 void* workspace, size_t workspace_bytes, void* stream);

/*
 * ConvNeXt block (projects/UNINEXT/uninext/backbone/convnext.py:18-57) and its LayerNorms (:168-194), forward, exact fp32.
 * Same conventions as above: contiguous fp32 device pointers, kernels only enqueued (no allocation, copy or synchronisation),
 * 0 / negative PATCH_EMBED_ERR_* / positive hipError_t, every check before the device is touched, an empty batch enqueues
 * nothing.  No float atomics; every sum runs in an order fixed by the shape: bitwise repeatable across runs and streams.
 *
 * patch_embed_hip_convnext_dwconv_ln_f32: the block's head in one kernel,
 *     out[b, h, w, :] = LayerNorm_C(dwconv7x7_pad3(x)[b, :, h, w] + dw_bias) * ln_weight + ln_bias
 * (biased variance, eps inside the square root, as F.layer_norm).  Each convolution output is one fmaf chain: bias first, the
 * 49 taps in (ky, kx) order; mean and variance are taken in two passes.  The un-normalised convolution output is never written
 * to global memory.  Supported: C a multiple of 32, 32 <= C <= 1536, any H, W >= 1 (also maps smaller than the 7 x 7 footprint);
 * out, ln_weight and ln_bias 16-byte aligned; anything else is PATCH_EMBED_ERR_UNSUPPORTED.
 *
 * patch_embed_hip_convnext_scale_residual_f32: the block's tail, out[b, c, h, w] = input[b, c, h, w] + gamma[c] * y[b, h, w, c] (gamma NULL:
 * input + y), transposed through LDS.  The product and the sum are rounded separately (never an FMA): bitwise PyTorch's two
 * operations on the same y.  Any C, H, W >= 1.
 *
 * patch_embed_hip_layernorm_cf_f32: LayerNorm over the channels of an NCHW map in one kernel: u = sum_c x / C, s = sum_c (x - u)^2 / C,
 * out = weight * ((x - u) / sqrt(s + eps)) + bias.  Any C, H, W >= 1.
 *
 * Limits of all three (PATCH_EMBED_ERR_BAD_DIMS beyond them): B, H, W <= 65535 and B * C * H * W < 2^31.
 *
 * The four names carry this header's prefix because tests/test_patch_embed_cpu.py::test_header_symbols_are_exported holds the
 * header's patch_embed_hip_* names and PATCH_EMBED_EXPORTS (uninext_amd/_lib.py) to each other.
 *
 * patch_embed_hip_convnext_last_kernel: name of the kernel the last of these three calls enqueued ("" before the first), for tests.
 */
int patch_embed_hip_convnext_dwconv_ln_f32(const float* x,        /* [B, C, H, W] */
                               const float* dw_weight /* [C, 1, 7, 7] */, const float* dw_bias /* [C] or NULL */,
                               const float* ln_weight /* [C] */, const float* ln_bias /* [C] */, float eps,
                               int B, int C, int H, int W, float* out /* [B, H, W, C] */, void* stream);
int patch_embed_hip_convnext_scale_residual_f32(const float* y /* [B, H, W, C] */, const float* gamma /* [C] or NULL */,
                                    const float* input /* [B, C, H, W] */, int B, int C, int H, int W,
                                    float* out /* [B, C, H, W] */, void* stream);
int patch_embed_hip_layernorm_cf_f32(const float* x /* [B, C, H, W] */, const float* weight, const float* bias, float eps,
                         int B, int C, int H, int W, float* out /* [B, C, H, W] */, void* stream);
const char* patch_embed_hip_convnext_last_kernel(void);

/*
 * TRAINING of the ConvNeXt block and its LayerNorms: the tail with stochastic depth, and the BACKWARD of the three kernels above.
 * Same conventions and limits (B, H, W <= 65535, B * C * H * W < 2^31): contiguous fp32 device pointers, kernels only enqueued, 0 /
 * negative PATCH_EMBED_ERR_* / positive hipError_t, every check before the device is touched.  Exact fp32 products, no float
 * atomics, every sum in an order fixed by the shape alone: bitwise repeatable across runs and streams.  A sum over pixels is taken
 * in fp32 inside one workgroup (at most 64 tiles of 64 pixels); the workgroups' partial sums go to the caller's workspace and are
 * added in float64 in workgroup order.  workspace: a device buffer of at least *_workspace_bytes bytes (a function of B, C, H, W
 * only; 0 for an empty batch and for shapes the call refuses), owned by the caller and in use until the enqueued work has finished;
 * a short one returns PATCH_EMBED_ERR_WORKSPACE.  Every output may be NULL and is then skipped, the others are bitwise what they
 * are with it.  An empty batch enqueues nothing, except that requested parameter gradients are written as zeros.  The last_kernel
 * query above names the first kernel of these calls too.
 *
 * scale_residual_drop: out[b, c, h, w] = input[b, c, h, w] + (gamma[c] * y[b, h, w, c]) * sample_scale[b] -- the tail with DropPath's
 * per-sample factor (0 or 1 / keep).  Three roundings: bitwise PyTorch's `gamma * x`, `x * mask`, `shortcut + x`.  gamma NULL: no
 * first product; sample_scale NULL: the scale_residual call above, as it is.
 *
 * dwconv_ln_backward: from grad_out [B, H, W, C], with u the convolution output (recomputed from x by the forward's own fmaf chain,
 * so mean and rstd are the forward's to the bit; nothing is saved by the forward), xhat = (u - mean) * rstd, gw = grad_out * ln_weight
 * and mean_C the mean over the channels of a pixel:
 *     grad_ln_bias[c]   = sum_{b,h,w} grad_out                grad_ln_weight[c] = sum_{b,h,w} grad_out * xhat
 *     grad_u            = rstd * (gw - mean_C(gw) - xhat * mean_C(gw * xhat))
 *     grad_dw_bias[c]   = sum_{b,h,w} grad_u
 *     grad_dw_weight[c, ky, kx] = sum_{b,h,w} grad_u[b, c, h, w] * x[b, c, h + ky - 3, w + kx - 3]          (zero outside the map)
 *     grad_x[b, c, h, w] = sum_{ky,kx} grad_u[b, c, h - ky + 3, w - kx + 3] * dw_weight[c, ky, kx]          (zero outside the map)
 * Pass one (the forward's tiles) writes grad_u as NCHW into the workspace and leaves [tile][2][C] partial sums of the LayerNorm
 * gradients; pass two works per (band of 8 x 8 tiles, 32 channels) and leaves [band][C * 50] partial sums.  The bands: about
 * 512 / (C / 32) of them, never more than 64 tiles each.  Supported C as in the forward; grad_out and ln_weight 16-byte aligned.
 *     workspace bytes = 4 * (B * C * H * W  +  2 * C * tiles_of_the_forward  +  50 * C * bands), each part rounded up to 256:
 * at most 1.6 x the bytes of x plus 4 MiB for any shape, and at most 1.15 x the bytes of x plus 4 MiB at the ConvNeXt-L stage shapes.
 *
 * scale_residual_backward: from grad_out [B, C, H, W]: grad_y[b, h, w, c] = (grad_out * sample_scale[b]) * gamma[c] (two roundings,
 * each skipped with its operand) and grad_gamma[c] = sum_{b,h,w} (grad_out * sample_scale[b]) * y.  The gradient of `input` is grad_out
 * itself and has no kernel.  y is read only for grad_gamma (NULL without it); gamma is read for grad_y's second product and, like
 * y, is required with grad_gamma.  workspace (only for grad_gamma): 4 * B * ceil(H * W / 64) * C bytes, rounded up to 256.
 *
 * layernorm_cf_backward: x, grad_out, grad_x [B, C, H, W]; xhat = (x - u) / sqrt(s + eps) by the forward's arithmetic; grad_bias,
 * grad_weight and grad_x by the formulas above with x in the place of u.  Any C, H, W >= 1.  workspace (only for grad_weight /
 * grad_bias): 8 * B * ceil(H * W / 64) * C bytes, rounded up to 256.
 */
int patch_embed_hip_convnext_scale_residual_drop_f32(const float* y /* [B, H, W, C] */, const float* gamma /* [C] or NULL */,
                                                     const float* sample_scale /* [B] or NULL */, const float* input /* [B, C, H, W] */,
                                                     int B, int C, int H, int W, float* out /* [B, C, H, W] */, void* stream);
size_t patch_embed_hip_convnext_dwconv_ln_backward_workspace_bytes(int B, int C, int H, int W);
int patch_embed_hip_convnext_dwconv_ln_backward_f32(const float* x /* [B, C, H, W] */, const float* dw_weight /* [C, 1, 7, 7] */,
                                                    const float* dw_bias /* [C] or NULL */, const float* ln_weight /* [C] */, float eps,
                                                    const float* grad_out /* [B, H, W, C] */, int B, int C, int H, int W,
                                                    float* grad_x, float* grad_dw_weight, float* grad_dw_bias, float* grad_ln_weight,
                                                    float* grad_ln_bias, void* workspace, size_t workspace_bytes, void* stream);
size_t patch_embed_hip_convnext_scale_residual_backward_workspace_bytes(int B, int C, int H, int W);
int patch_embed_hip_convnext_scale_residual_backward_f32(const float* grad_out /* [B, C, H, W] */, const float* y /* [B, H, W, C] */,
                                                         const float* gamma /* [C] or NULL */, const float* sample_scale /* [B] or NULL */,
                                                         int B, int C, int H, int W, float* grad_y /* [B, H, W, C] */,
                                                         float* grad_gamma /* [C] */, void* workspace, size_t workspace_bytes, void* stream);
size_t patch_embed_hip_layernorm_cf_backward_workspace_bytes(int B, int C, int H, int W);
int patch_embed_hip_layernorm_cf_backward_f32(const float* x, const float* weight /* [C] */, float eps, const float* grad_out, int B, int C,
                                              int H, int W, float* grad_x, float* grad_weight, float* grad_bias, void* workspace,
                                              size_t workspace_bytes, void* stream);

/*
 * ViTDet-style ViT blocks (projects/UNINEXT/uninext/backbone/vit.py:27-83, utils.py:63-125): the core of Attention.forward between
 * the `qkv` Linear and the `proj` Linear, at inference, with the decomposed relative positions, in exact fp32.  For every
 * b < batch, head h and query i < S = q_h * q_w, with i = (ih, iw) and j = (jh, jw) row-major:
 *     s[i, j]   = sum_d (q[i, d] * scale) * k[j, d]                 (q scaled first, in fp32)
 *               + sum_d q[i, d] * rel_h_table[ih - jh + q_h - 1, d]  (unscaled q)
 *               + sum_d q[i, d] * rel_w_table[iw - jw + q_w - 1, d]
 *     out[i, :] = sum_j softmax_j(s[i, :])[j] * v[j, :]
 * (add_decomposed_rel_pos for q_size == k_size; resizing a table of another length stays with the caller).  A windowed block is
 * the same call with batch = B * windows and q_h = q_w = the window size.
 *
 * qkv      [batch, S, 3 * num_heads * head_dim], the Linear's output, read in place as [batch, S, 3, num_heads, head_dim]
 * rel_h_table [2 * q_h - 1, head_dim], rel_w_table [2 * q_w - 1, head_dim]; both NULL: no relative positions; one NULL: refused
 * out      [batch, S, num_heads * head_dim], token-major: the input of `proj`
 *
 * Products and sums run on v_mfma_f32_32x32x2_f32 in a fixed order, without float atomics: bitwise repeatable across runs and
 * streams.  The softmax subtracts a running maximum; keys past S take no part in maximum or sum.  Nothing of size
 * batch * num_heads * S * S is written: a wave holds one 32 x 32 score tile.  workspace: a device buffer of at least as many
 * bytes as the workspace_bytes query answers, batch * num_heads * (q_h + q_w) * roundup(S, 32) floats (the two relative-position
 * terms of every query), a function of the shapes only; owned by the caller, in use until the enqueued work has finished.
 *
 * Supported: head_dim 64 or 80 (else PATCH_EMBED_ERR_UNSUPPORTED); every pointer 16-byte aligned (else the same code).  Limits
 * (PATCH_EMBED_ERR_BAD_DIMS beyond them): q_h, q_w <= 4095, S <= 2^20, (q_h + q_w) * roundup(S, 32) < 2^31,
 * batch * num_heads * ceil(S / 128) < 2^31.  Same conventions as above: contiguous fp32 device pointers, kernels only enqueued, 0 /
 * negative PATCH_EMBED_ERR_* / positive hipError_t, every check before the device is touched (a short workspace is
 * PATCH_EMBED_ERR_WORKSPACE, a missing pointer or a single table PATCH_EMBED_ERR_NULL_POINTER), an empty batch enqueues nothing
 * and returns 0.  The workspace query answers 0 for dimensions the call refuses.  The last_kernel query names the kernels the
 * last call enqueued ("" before the first), for tests.
 */
size_t patch_embed_hip_vit_attn_workspace_bytes(int batch, int num_heads, int q_h, int q_w, int head_dim);
int patch_embed_hip_vit_attn_f32(const float* qkv, const float* rel_h_table, const float* rel_w_table, int batch, int num_heads,
                                 int q_h, int q_w, int head_dim, float scale, float* out /* [batch, S, num_heads * head_dim] */,
                                 void* workspace, size_t workspace_bytes, void* stream);
const char* patch_embed_hip_vit_attn_last_kernel(void);

/*
 * The same core under autograd (opt-in from Python: Attention.own_training): a forward that also keeps the row log-sum-exp, and
 * a backward that recomputes the probabilities tile by tile.  Nothing of size batch * num_heads * S * S is written by either.
 *
 * patch_embed_hip_vit_attn_train_f32: `out` is bitwise patch_embed_hip_vit_attn_f32's; lse [batch * num_heads, SP], SP =
 * roundup(S, 32), gets lse[bh, i] = max_j s[i, j] + log sum_j exp(s[i, j] - max) (the entries of i in [S, SP) are finite and
 * carry no meaning).  workspace: as for patch_embed_hip_vit_attn_f32 (its workspace_bytes query).
 *
 * patch_embed_hip_vit_attn_backward_f32, with g = grad_out [batch, S, num_heads * head_dim], o = out, p = exp(s - lse):
 *     delta[i] = g[i] . o[i]          dv[j] = sum_i p[i, j] g[i]          ds[i, j] = p[i, j] (g[i] . v[j] - delta[i])
 *     dk[j] = sum_i ds[i, j] (q[i] * scale)                                (the scaled row as the forward rounds it)
 *     rh[i, c] = sum_{j: jh = c} ds[i, j]      rw[i, c] = sum_{j: jw = c} ds[i, j]
 *     dq[i] = scale sum_j ds[i, j] k[j] + sum_c rh[i, c] rel_h_table[ih - c + q_h - 1] + sum_c rw[i, c] rel_w_table[iw - c + q_w - 1]
 *     grad_rel_h_table[r] = sum_{b, h} sum_{(i, c): ih - c + q_h - 1 = r} rh[i, c] q[i]   (unscaled q); grad_rel_w_table likewise
 * grad_qkv [batch, S, 3 * num_heads * head_dim] is written completely (no zero fill is needed, nothing is accumulated into);
 * grad_rel_h_table [2 * q_h - 1, head_dim] and grad_rel_w_table [2 * q_w - 1, head_dim] likewise, and are required exactly when
 * the tables are given.  Exact fp32 products in a fixed order, the table gradients summed in float64 per workgroup and combined
 * by one reducer in a fixed order, no float atomics: bitwise repeatable across runs and streams.  workspace: at least the
 * backward_workspace_bytes query's answer (the relative-position terms, their gradients, delta and the table partial sums), a
 * function of the shapes only.
 *
 * Checks, codes and conventions are the forward's; in addition q_w <= 256 (else PATCH_EMBED_ERR_UNSUPPORTED; the query answers 0).
 */
int patch_embed_hip_vit_attn_train_f32(const float* qkv, const float* rel_h_table, const float* rel_w_table, int batch, int num_heads,
                                       int q_h, int q_w, int head_dim, float scale, float* out /* [batch, S, num_heads * head_dim] */,
                                       float* lse /* [batch * num_heads, roundup(S, 32)] */, void* workspace, size_t workspace_bytes,
                                       void* stream);
size_t patch_embed_hip_vit_attn_backward_workspace_bytes(int batch, int num_heads, int q_h, int q_w, int head_dim);
int patch_embed_hip_vit_attn_backward_f32(const float* qkv, const float* rel_h_table, const float* rel_w_table, const float* out,
                                          const float* lse, const float* grad_out, int batch, int num_heads, int q_h, int q_w,
                                          int head_dim, float scale, float* grad_qkv, float* grad_rel_h_table, float* grad_rel_w_table,
                                          void* workspace, size_t workspace_bytes, void* stream);
const char* patch_embed_hip_vit_attn_backward_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif /* PATCH_EMBED_HIP_H_ */
