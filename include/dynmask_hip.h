/*
 * include/dynmask_hip.h -- C ABI of the CondInst-style dynamic mask head of UNINEXT on MI355X (gfx950), part of
 * libmsda_hip.so.  SURVEY.md 8(f) rank 2: the step after the decoder on the inference path.
 *
 * Replaces, for inference, the body of DDETRSegmUniDN.dynamic_mask_with_coords
 * (projects/UNINEXT/uninext/models/ddetrs_dn.py:755-844) between "build mask_head_inputs" and "upsample":
 *   - compute_locations + relative coordinates (ddetrs_dn.py:765-784, 1199-1212),
 *   - the repeat/cat that materialises [1, n_inst*(C+2), H, W] (ddetrs_dn.py:786-808; 1.2 GB at 1800 instances),
 *   - parse_dynamic_params (ddetrs_dn.py:1148-1171) and the three grouped 1x1 convolutions of
 *     mask_heads_forward (ddetrs_dn.py:734-752): (C+2) -> 8 -> 8 -> 1 with ReLU between,
 * by one kernel that keeps the C mask-feature channels of a pixel in registers and walks the instances of the
 * image with their 169 parameters staged in LDS; and aligned_bilinear (ddetrs_dn.py:1174-1196) by a second one.
 *
 * All pointers are device pointers except `num_insts` (host), contiguous fp32 unless noted; `stream` is a
 * hipStream_t as void*.  Kernels are only enqueued.  Returns 0, a negative DYNMASK_ERR_*, or a positive hipError_t;
 * the message is available from msda_hip_last_error().
 */
#ifndef DYNMASK_HIP_H_
#define DYNMASK_HIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DYNMASK_ERR_NULL_POINTER (-1)
#define DYNMASK_ERR_BAD_DIMS (-2)
#define DYNMASK_ERR_UNSUPPORTED (-5)   /* feature channels != 8: use the PyTorch composition */

/*
 * mask_feats   [batch, 8, H, W]            output of the mask-feature branch (hidden_dim / 32 = 8 channels)
 * inst_xy      [n_inst_all, 2]             instance reference points (x, y) in input-image pixels
 * params       [n_inst_all, 169]           controller output: w0 (8 x 10) w1 (8 x 8) w2 (1 x 8) b0 (8) b1 (8) b2 (1);
 *                                          with rel_coord == 0: w0 is 8 x 8 and a row has 153 values
 * num_insts    [batch] (HOST ints)         instances per image, in order; n_inst_all = sum
 * out_logits   [n_inst_all, H, W]          mask logits at the feature stride
 * stride       mask_feat_stride (8): pixel (y, x) sits at (x * stride + stride / 2, y * stride + stride / 2)
 */
int dynmask_hip_forward_f32(const float* mask_feats, const float* inst_xy, const float* params,
                            const int* num_insts, int batch, int channels, int H, int W, int stride,
                            int rel_coord, float* out_logits, void* stream);

/*
 * Kernel behind dynmask_hip_forward_f32: 0 = auto (the faster one measured on MI355X), 1 = packed-FMA VALU kernel,
 * 2 / 3 = MFMA kernel (v_mfma_f32_4x4x1_16b_f32; 2 / 4 pixels per lane).  The environment variable
 * DYNMASK_HIP_VARIANT seeds the choice.  Returns 0 or DYNMASK_ERR_BAD_DIMS.  dynmask_hip_last_kernel names the
 * kernel the last forward call enqueued ("dynmask_fwd_pkfma", "dynmask_fwd_mfma_q2", "dynmask_fwd_mfma_q4").
 */
int dynmask_hip_set_variant(int variant);
const char* dynmask_hip_last_kernel(void);

/*
 * aligned_bilinear (ddetrs_dn.py:1174-1196): in [n, h, w] -> out [n, factor*h, factor*w]; factor >= 1.
 */
int aligned_bilinear_hip_f32(const float* in, int n, int h, int w, int factor, float* out, void* stream);

/*
 * Backward of dynmask_hip_forward_f32 (training: BASELINE configs[4] trains the CondInst head, ddetrs_dn.py:493-560 calls
 * dynamic_mask_with_coords under autograd).  Same inputs as the forward plus
 *   grad_logits  [n_inst_all, H, W]     gradient of the loss with respect to out_logits
 * and the gradients, every element written (no accumulation, no float atomics: results are bitwise repeatable):
 *   grad_feats   [batch, 8, H, W] or NULL       sum over the image's instances (zeros for an image without instances)
 *   grad_params  [n_inst_all, 169|153] or NULL  sum over the pixels, in the layout of `params`
 *   grad_xy      [n_inst_all, 2] or NULL        gradient with respect to inst_xy (zeros with rel_coord == 0); needs grad_params
 * A NULL gradient is not computed: grad_feats == NULL skips the pixel-major kernels, grad_params == NULL (with grad_xy == NULL)
 * the instance-major ones and the workspace (frozen mask features / detached parameters; round 6).
 * workspace: device memory of at least dynmask_hip_backward_workspace_bytes(n_inst_all, H, W) bytes (partial sums of the
 * pixel slices, dynmask_hip_backward_parts of them per instance), contents undefined before and after; borrowed for the call
 * in stream order.  At most DYNMASK_HIP_BWD_MAX_BATCH images per call (DYNMASK_ERR_UNSUPPORTED beyond).
 * The activations are recomputed per (instance, pixel) from the inputs: nothing of the forward has to be kept.
 */
#define DYNMASK_HIP_BWD_MAX_BATCH 64
size_t dynmask_hip_backward_workspace_bytes(int n_inst_all, int H, int W);
int dynmask_hip_backward_parts(int n_inst_all, int H, int W);
int dynmask_hip_backward_f32(const float* mask_feats, const float* inst_xy, const float* params, const int* num_insts,
                             int batch, int channels, int H, int W, int stride, int rel_coord, const float* grad_logits,
                             float* grad_feats, float* grad_params, float* grad_xy, void* workspace, size_t workspace_bytes,
                             void* stream);

/*
 * Backward of aligned_bilinear_hip_f32: grad_out [n, factor*h, factor*w] -> grad_in [n, h, w], every element written; a
 * gather (each input pixel sums the output pixels that read it, in a fixed order): bitwise repeatable.
 */
int aligned_bilinear_hip_backward_f32(const float* grad_out, int n, int h, int w, int factor, float* grad_in, void* stream);

/*
 * Two-stage query selection (qsel_*), the step between the encoder's memory and the decoder's queries that precedes this head
 * on the inference path (deformable_transformer_dino.py:132-162 and :216-224).  The entry points live in this header because
 * the set of headers is fixed and every other header's exported names are pinned to its own prefix; error codes are the
 * DYNMASK_ERR_* above (d_model != 256: DYNMASK_ERR_UNSUPPORTED).  Every token s of image b has a proposal from its level lvl, its
 * (y, x) in the level and valid_wh[b, lvl] = (valid_W, valid_H): cx = (x + 0.5) / valid_W, cy = (y + 0.5) / valid_H (IEEE
 * fp32 divisions), w = h = 0.05 * 2^lvl; it is valid iff all four lie strictly inside (0.01, 0.99) in fp32.  The row of a padded
 * token (padding_mask != 0) or of an invalid proposal counts as zeros, and its proposal logit log(p / (1 - p)) as +inf.
 *
 *     out_mem[b, s, :] = LayerNorm(row @ enc_weight^T + enc_bias) * ln_weight + ln_bias
 *
 * qsel_scores_hip_f32, over all batch * S rows:
 *     logits[b, s] = dot(out_mem[b, s, :], class_vec[b]) / scale[0] + class_bias[b], clamped to +-clamp when clamp > 0;
 *     class_vec + b * class_vec_stride and class_bias + b * class_bias_stride (strides in floats; 0: one head for every image);
 *     scale is a DEVICE pointer to one float, or NULL for 1; output_memory [batch, S, 256] is written when it is not NULL.
 * qsel_boxes_hip_f32, over the rows idx[b, k] (int64, [batch, K]; an index outside [0, S) counts as a padded row):
 *     coords_unact[b, k, :] = w3 relu(w2 relu(w1 out_mem + b1) + b2) + b3 + proposal logit;  reference_points = sigmoid of it
 *     (+inf gives exactly 1).  w1, w2 [256, 256], w3 [4, 256], row-major [out, in] as nn.Linear keeps them.
 * Both: fp32, d_model must be 256, spatial_shapes [n_levels, 2] int64 (H, W) on the device, memory [batch, S, 256] contiguous;
 * exact fp32 products in a fixed order (bitwise repeatable; a row's result does not depend on its neighbours).
 * qsel_hip_last_kernel names the kernel the last successful qsel_* call enqueued ("" before the first).
 */
int qsel_scores_hip_f32(const float* memory, const unsigned char* padding_mask, const long long* spatial_shapes, int n_levels,
                        const float* valid_wh, const float* enc_weight, const float* enc_bias, const float* ln_weight,
                        const float* ln_bias, float eps, const float* class_vec, long long class_vec_stride,
                        const float* class_bias, long long class_bias_stride, const float* scale, float clamp, int batch,
                        long long S, int d_model, float* logits, float* output_memory, void* stream);
int qsel_boxes_hip_f32(const float* memory, const unsigned char* padding_mask, const long long* spatial_shapes, int n_levels,
                       const float* valid_wh, const float* enc_weight, const float* enc_bias, const float* ln_weight,
                       const float* ln_bias, float eps, const long long* idx, long long K, const float* w1, const float* b1,
                       const float* w2, const float* b2, const float* w3, const float* b3, int batch, long long S, int d_model,
                       float* coords_unact, float* reference_points, void* stream);
const char* qsel_hip_last_kernel(void);

/*
 * Decoder prediction heads (pred_heads_*), the step from one decoder level's hidden states to its predictions
 * (ddetrs_dn.py:413-435 and :468-469; per level :190-222): class_embed[lvl], bbox_embed[lvl], iou_head[lvl] and the controller
 * on the same rows, one launch.  In this header for the same reason as qsel_*; error codes are the DYNMASK_ERR_* above.
 *
 *     hs [batch, Q, 256]; tokens [batch, T, 256] and token_bias [batch, T] the text side of VL_Align (its projected tokens and
 *     token biases), image b's at tokens + b * tokens_stride and token_bias + b * token_bias_stride (strides in floats; 0: one
 *     text for every image -- a Still_Classifier passes its weight and bias as one token, T = 1, strides 0, scale NULL);
 *     scale a DEVICE pointer to one float, or NULL for 1; reference [batch, Q, ref_dim] in sigmoid space, ref_dim 2 or 4.
 *     logits[b, q, t] = dot(hs[b, q], tokens[b, t]) / scale[0] + token_bias[b, t], clamped to +-clamp when clamp > 0
 *     boxes[b, q, :]  = sigmoid(w3 relu(w2 relu(w1 hs + b1) + b2) + b3 + inverse_sigmoid(reference[b, q])), the last term on
 *                       the first ref_dim columns; inverse_sigmoid(x) = log(max(x', 1e-5) / max(1 - x', 1e-5)), x' = x clamped
 *                       to [0, 1]
 *     iou[b, q]       = dot(hs[b, q], iou_weight) + iou_bias[0]                 (iou == NULL: not computed, weights not read)
 *     params[b, q, :] = c3 relu(c2 relu(c1 hs + cb1) + cb2) + cb3, c3 [P, 256]  (params == NULL: likewise)
 * Weights row-major [out, in] as nn.Linear keeps them: box_w1, box_w2, ctrl_w1, ctrl_w2 [256, 256], box_w3 [4, 256].
 * d_model != 256, T > PRED_HEADS_HIP_MAX_TOKENS, P > PRED_HEADS_HIP_MAX_PARAMS: DYNMASK_ERR_UNSUPPORTED; T < 1, P < 1, another
 * ref_dim: DYNMASK_ERR_BAD_DIMS.  A refused call enqueues nothing.  Exact fp32 products in a fixed order, no atomics: bitwise
 * repeatable, and a row's result does not depend on its neighbours.
 * pred_heads_hip_set_variant picks the grid: 0 = auto (the faster one measured on MI355X), 1 = "split" (the branch class /
 * box + IoU / controller is a grid dimension), 2 = "tile" (one workgroup runs all branches of its 32 rows); the results are
 * bitwise equal.  pred_heads_hip_last_kernel names the kernel of the last successful call ("pred_heads<split>",
 * "pred_heads<tile>"; "" before the first).
 */
#define PRED_HEADS_HIP_MAX_TOKENS 256
#define PRED_HEADS_HIP_MAX_PARAMS 256
int pred_heads_hip_f32(const float* hs, const float* tokens, long long tokens_stride, const float* token_bias,
                       long long token_bias_stride, const float* scale, float clamp, const float* reference, int ref_dim,
                       const float* box_w1, const float* box_b1, const float* box_w2, const float* box_b2, const float* box_w3,
                       const float* box_b3, const float* iou_weight, const float* iou_bias, const float* ctrl_w1,
                       const float* ctrl_b1, const float* ctrl_w2, const float* ctrl_b2, const float* ctrl_w3, const float* ctrl_b3,
                       int P, int batch, long long Q, int T, int d_model, float* logits, float* boxes, float* iou, float* params,
                       void* stream);
int pred_heads_hip_set_variant(int variant);
const char* pred_heads_hip_last_kernel(void);

/*
 * Detection post-processing (detpost_*), the step after the decoder that turns its token logits, boxes and IoU logits into
 * scored, labelled boxes (uninext_img.py:367-485 with convert_grounding_to_od_logits, :598-613).  In this header for the same
 * reason as qsel_*; error codes are the DYNMASK_ERR_* above.  Exact fp32 in fixed orders, no atomics: bitwise repeatable.
 *
 * detpost_scores_hip_f32, over all batch * Q rows:
 *     logits [batch, Q, T]; iou_logits [batch, Q] or NULL; the positive map as CSR: class c (the reference's label - 1) owns the
 *     tokens tok_idx[cls_ptr[c] .. cls_ptr[c + 1]), both int32 on the device, nnz = the length of tok_idx.
 *     mean = (sum of the row's logits at the class's tokens, in list order) / their number, 0.0 for a class without tokens;
 *     p = sigmoid(mean), or sqrt(sigmoid(mean) * sigmoid(iou)) with IoU logits.  With score_thres > 0 an entry that is not above
 *     it becomes -1.0.
 *     prob [batch, Q, C]; row_max [batch, Q] and row_arg [batch, Q] (int32) the row's maximum and its FIRST index;
 *     row_valid [batch, Q] (int32) the row's number of entries above score_thres (0 without a threshold).
 *     C > DETPOST_HIP_MAX_CLASSES or T > DETPOST_HIP_MAX_TOKENS: DYNMASK_ERR_UNSUPPORTED.  A token index outside [0, T) counts
 *     as a logit of 0.0 and offsets outside [0, nnz] are clamped: nothing outside the arrays is read.
 * detpost_nms_hip_f32, one workgroup per image:
 *     boxes [batch, Q, 4] as (cx, cy, w, h), 16-byte aligned; row_max / row_arg as above are the score and the class of a query.
 *     xyxy = (cx - 0.5 w, cy - 0.5 h, cx + 0.5 w, cy + 0.5 h).  per_class == 0: float(class) * (max_coord + 1) is added to the
 *     four coordinates, max_coord the image's maximum over all xyxy coordinates, and IoU alone decides; per_class == 1: boxes
 *     stay as they are and only a pair of one class suppresses.  Queries are visited by decreasing score, equal scores by
 *     increasing index (a NaN score counts as +inf); a visited query that is not suppressed is kept and suppresses every later
 *     one with inter / (area_i + area_j - inter) > iou_threshold, widths and heights of the intersection clamped at 0 (0 / 0 is
 *     NaN and does not suppress).  Every operation rounds as one IEEE fp32 operation (no FMA contraction).
 *     keep [batch, Q] (int32) the kept queries in visiting order, padded with -1; n_keep [batch] (int32);
 *     kept_mask [batch, Q] (uint8).  Q > DETPOST_HIP_MAX_QUERIES: DYNMASK_ERR_UNSUPPORTED.
 * detpost_hip_last_kernel names the kernel the last successful detpost_* call enqueued ("" before the first).
 */
#define DETPOST_HIP_MAX_CLASSES 4096
#define DETPOST_HIP_MAX_TOKENS 256
#define DETPOST_HIP_MAX_QUERIES 1024
int detpost_scores_hip_f32(const float* logits, const float* iou_logits, const int* cls_ptr, const int* tok_idx, int nnz,
                           float score_thres, int batch, int Q, int C, int T, float* prob, float* row_max, int* row_arg,
                           int* row_valid, void* stream);
int detpost_nms_hip_f32(const float* boxes, const float* row_max, const int* row_arg, float iou_threshold, int per_class,
                        int batch, int Q, int* keep, int* n_keep, unsigned char* kept_mask, void* stream);
const char* detpost_hip_last_kernel(void);

/*
 * Mask post-processing (maskpost_*), the mask lines that follow detection post-processing on every inference route
 * (uninext_img.py:474-480, segmentation.py:60-65, uninext_vid.py:1263-1267) and the tracker's mask NMS (tracker.py:17-46).
 * In this header for the same reason as detpost_*; error codes are the DYNMASK_ERR_* above.  No atomics, fixed orders: bitwise
 * repeatable.  Non-finite logits are outside the contract (nothing outside the arrays is read or written for them, but the
 * bytes they give are unspecified).
 *
 * maskpost_binarize_hip_f32: logits [Q, h, w]; rows [n] (int64, the instances' rows of Q, in any order, repeats allowed; a row
 *     outside [0, Q) gives a mask of zeros); out [n, out_h, out_w] bytes holding 0 or 1, any alignment.  Byte (i, oy, ox) is
 *         sigmoid(B(Y, X)) > thres,   Y = near(oy, crop_h, out_h),  X = near(ox, crop_w, out_w)
 *     where B is the bilinear upsampling (align_corners = False) of plane rows[i] to (h * stride, w * stride): no plane of that
 *     size is ever formed, only the pixels the nearest step picks.  With (out_h, out_w) == (crop_h, crop_w) near is the
 *     identity and the bytes are the reference's inference() masks.  Pinned conventions:
 *         bilinear source coordinate  s = max(0, (dst + 0.5) / stride - 0.5), lower neighbour floor(s), upper neighbour
 *                                     min(floor(s) + 1, size - 1), weight s - floor(s) on the upper one;
 *                                     value = (1 - lx) * r[x0] + lx * r[x1] with r[x] = (1 - ly) * p[y0][x] + ly * p[y1][x];
 *         nearest source index        near(dst, in, out) = min(floor(dst * scale), in - 1), scale = (float)in / (float)out,
 *                                     the product taken in fp32 (F.interpolate(mode='nearest') does; a float64 product picks
 *                                     other pixels, e.g. at 34 positions of 1344 -> 1920);
 *         sigmoid                     1 / (1 + expf(-v)) in fp32, compared with thres by >.
 *     Accepted: stride 1, 2, 4 or 8 and 0 < thres < 1 and w <= MASKPOST_HIP_MAX_WIDTH (else DYNMASK_ERR_UNSUPPORTED);
 *     1 <= crop_h <= h * stride, 1 <= crop_w <= w * stride, out_h, out_w >= 1, Q * h * w and n * out_h * out_w below 2^31, every
 *     extent at most 2^24 (else DYNMASK_ERR_BAD_DIMS).  n == 0 returns 0 without a launch.
 * maskpost_pack_hip_f32: bits [n, words] (uint32), words = ceil(h * w / 32): bit k % 32 of word k / 32 is
 *     sigmoid(plane rows[i], pixel k) > 0.5 at the low resolution, as mask_nms binarises (tracker.py:31); the bits past h * w
 *     are zero.  area [n] (int32) the number of set bits.  One workgroup per instance.
 * maskpost_nms_hip_u32: inter [n, n] (int32), inter[i, j] = popcount(bits_i & bits_j), every entry written (the diagonal is the
 *     area); keep [n] bytes.  The greedy scan runs in the GIVEN order (the reference uses its scores for their number only): a
 *     kept i suppresses every later j with (float(inter) + 1e-6f) / (float(area_i + area_j - inter) + 1e-6f) > nms_thr, every
 *     operation one IEEE fp32 operation.  Two empty masks have IoU 1: the later one goes, as in the reference.
 *     n > MASKPOST_HIP_MAX_MASKS: DYNMASK_ERR_UNSUPPORTED.
 * maskpost_hip_last_kernel names the kernel the last successful maskpost_* call enqueued ("" before the first).
 */
#define MASKPOST_HIP_MAX_WIDTH 8192
#define MASKPOST_HIP_MAX_MASKS 1024
int maskpost_binarize_hip_f32(const float* logits, const long long* rows, int Q, int h, int w, int n, int stride, int crop_h,
                              int crop_w, int out_h, int out_w, float thres, unsigned char* out, void* stream);
int maskpost_pack_hip_f32(const float* logits, const long long* rows, int Q, int h, int w, int n, unsigned* bits, int* area,
                          void* stream);
int maskpost_nms_hip_u32(const unsigned* bits, const int* area, int n, int words, float nms_thr, int* inter, unsigned char* keep,
                     void* stream);
const char* maskpost_hip_last_kernel(void);

/*
 * The online IDOL tracker (track_hip_*): the association and the memory bank of IDOL_Tracker.match / update_memo / memo
 * (tracker.py:98-298, match_metric 'bisoftmax'), in uninext_amd/csrc/tracker.hip.  In this header for the same reason as
 * detpost_*; error codes are the DYNMASK_ERR_* above.  Exact fp32, every operation of a pinned expression one IEEE operation, no
 * atomics, reductions in fixed orders: bitwise repeatable.  Non-finite embeddings or scores are outside the contract.
 *
 * The memory bank is ONE device buffer of track_hip_state_offset(TRACK_HIP_STATE_FIELDS, capacity, D, memory_len) bytes whose
 * fields start at track_hip_state_offset(field, ...) (16-byte aligned; 0 for bad arguments), in this order:
 *     0 meta [2] int64 (live slots `count`, `num_tracklets`)   1 id [C] int64        2 label [C] int64     3 bbox [C, 5] f32
 *     4 velocity [C, 5] f32      5 last_frame [C] int32        6 acc_frame [C] int32  7 exist_frame [C] int32
 *     8 long_len [C] int32       9 long_score [C, L] f32      10 embed [C, D] f32    11 long_embed [C, L, D] f32
 * Slots 0 .. count - 1 are live, in the insertion order of the reference's dict (tracker.py:132, :176): that order is what
 * torch.max's lowest-index tie rule sees (:254-258) and what `memo` returns.  Entry k of a slot's ring is its k-th oldest.
 * A call reads `state` and writes `next_state`, another buffer of the same geometry; M is the caller's copy of `count`.
 *
 * track_hip_scores_f32: embeds [n, D]; keep [n] bytes, the pre-NMS' flags (maskpost_nms_hip_u32): rows with 0 take no part
 *     (tracker.py:212-218) and their scores are not written.  The matching embedding of slot m is `embed`, or with long_match
 *     (:179-186) sum_k long_embed[k] * w[k] / sum_k w[k], oldest to newest, w = long_score, plus temporal[length * L + k] when
 *     `temporal` (a [L + 1, L] table of the reference's torch.range(0, 1, 1 / length)[1:]) is given; memo_embed [M, D] is the
 *     workspace they are formed in.  scores [n, M] = (softmax over the row + softmax over the column) / 2 of embeds . memo^T
 *     (:232-235), both with the maximum subtracted; row_stats [2 n] is a workspace.  n == 0 or M == 0: no launch.
 * track_hip_associate_f32: one workgroup walks the kept rows in order (:245-264): the row maximum conf and its lowest index
 *     memo_ind over the scores with the columns taken so far read as 0; with frame_weight, when more than one of these scores is
 *     above 0.5, the hits are scaled by their slots' exist_frame and every other column by the mean of the hits' exist_frame
 *     before the maximum (:247-254).  conf > match_score_thr gives the row the slot's id and takes the column.  Rows still -2
 *     with bboxes[i, 4] > new_score_thr (the caller passes addnew_score_thr, or init_score_thr for an empty memory, :265, :282)
 *     get num_tracklets, num_tracklets + 1, ... in order; a row still -2 becomes -1 when (float(inter) + 1e-6f) /
 *     (float(area_i + area_j - inter) + 1e-6f) < nms_thr_post for every earlier kept row j (:273-277), with inter [n, n] and
 *     area [n] as maskpost_nms_hip_u32 and maskpost_pack_hip_f32 wrote them.  result [3 n + 2] int64 = keep flags, ids (-3 for
 *     a row the pre-NMS dropped), the next count, the next num_tracklets (the caller's one host copy), then the kept rows'
 *     indices in order, zeros after them (for the caller's gathers on the device).  plan [2 capacity + n]
 *     int32 is the update's plan (which row feeds a slot, where a slot lands after the stable compaction of the slots with
 *     frame_id - last_frame >= memo_tracklet_frames, :152-161, where a new tracklet lands); next_state's meta is written.
 *     M + n <= capacity is required (DYNMASK_ERR_BAD_DIMS): the caller falls back before the bank can overflow.
 * track_hip_update_f32: writes next_state from state, plan and result (:111-141): a matched slot gets velocity = (bbox - old
 *     bbox) / (frame_id - last_frame) averaged over acc_frame, embed = keep_weight * embed + momentum * new (the caller rounds
 *     1 - momentum as the reference's Python does), its ring appended, the oldest entry leaving beyond memory_len; an unmatched
 *     slot moves unchanged; new tracklets are appended in detection order with the reference's initial values.
 *     labels [n] int64.
 * Limits (DYNMASK_ERR_UNSUPPORTED beyond): n <= MASKPOST_HIP_MAX_MASKS, capacity <= TRACK_HIP_MAX_CAPACITY,
 * D <= TRACK_HIP_MAX_DIM, memory_len <= TRACK_HIP_MAX_MEMORY_LEN.  track_hip_last_kernel names the last call's kernels.
 */
#define TRACK_HIP_MAX_CAPACITY 4096
#define TRACK_HIP_MAX_DIM 256
#define TRACK_HIP_MAX_MEMORY_LEN 64
#define TRACK_HIP_STATE_FIELDS 12
size_t track_hip_state_offset(int field, int capacity, int D, int memory_len);
int track_hip_scores_f32(const float* embeds, const unsigned char* keep, const void* state, const float* temporal, int long_match,
                         int n, int M, int capacity, int D, int memory_len, float* memo_embed, float* row_stats, float* scores,
                         void* stream);
int track_hip_associate_f32(const float* scores, const unsigned char* keep, const float* bboxes, const int* inter, const int* area,
                            const void* state, void* next_state, int n, int M, int capacity, int D, int memory_len, int frame_weight,
                            float match_score_thr, float new_score_thr, float nms_thr_post, int frame_id, int memo_tracklet_frames,
                            int* plan, long long* result, void* stream);
int track_hip_update_f32(const float* embeds, const float* bboxes, const long long* labels, const int* plan, const long long* result,
                         const void* state, void* next_state, int n, int M, int capacity, int D, int memory_len, float keep_weight,
                         float momentum, int frame_id, void* stream);
const char* track_hip_last_kernel(void);

/*
 * The QuasiDense embedding tracker (qdtrack_hip_*): the box pre-NMS, the association and the memory bank of
 * QuasiDenseEmbedTracker.match / update_memo / memo (tracker.py:304-503, match_metric 'bisoftmax', the bdd_track route) with
 * mmcv's bbox_overlaps (util/mmcv_utils.py:146-191, mode 'iou', not aligned, eps 1e-6), in uninext_amd/csrc/qdtrack.hip.  In this
 * header for the same reason as detpost_*; error codes are the DYNMASK_ERR_* above.  Exact fp32, every operation of a pinned
 * expression one IEEE operation, no atomics, reductions in fixed orders: bitwise repeatable.  Non-finite boxes, embeddings or
 * scores are outside the contract (nothing outside the arrays is read or written for them).
 *
 * The memory bank is ONE device buffer of qdtrack_hip_state_offset(QDTRACK_HIP_STATE_FIELDS, capacity, D, backdrop_capacity,
 * backdrop_frames) bytes whose fields start at qdtrack_hip_state_offset(field, ...) (16-byte aligned; 0 for bad arguments), with
 * C = capacity, B = backdrop_capacity and K = max(backdrop_frames, 1), in this order:
 *     0 meta [2 + QDTRACK_HIP_MAX_BACKDROP_FRAMES] int64 (live slots `count`, `num_tracklets`, the rows of backdrop frame 0, 1, ..)
 *     1 id [C] int64             2 label [C] int64             3 bbox [C, 5] f32       4 velocity [C, 5] f32
 *     5 last_frame [C] int32     6 acc_frame [C] int32         7 embed [C, D] f32
 *     8 backdrop_label [K, B] int64     9 backdrop_bbox [K, B, 5] f32     10 backdrop_embed [K, B, D] f32
 * Slots 0 .. count - 1 are live, in the insertion order of the reference's dict.  Backdrop frame 0 is the newest (the reference
 * inserts at the front, :381); a frame's rows keep their stored order.  The memory's COLUMNS are the live slots, then the rows of
 * frame 0, frame 1, ... (`memo`, :406-428): that order is what torch.max's lowest-index tie rule sees.  A call reads `state` and
 * writes `next_state`, another buffer of the same geometry; M and b0 .. b3 are the caller's copies of `count` and of the frames'
 * rows (b_k is ignored for k >= backdrop_frames; a value outside [0, B] is DYNMASK_ERR_BAD_DIMS).
 *
 * qdtrack_hip_prepare_f32: bboxes [n, 5] (x1, y1, x2, y2, score).  order [n] int32: order[r] is the detection of rank r by
 *     descending score, found by counting; equal scores (-0.0 equals 0.0) rank by lower index.  The reference's sort (:434) is not
 *     stable, so what it does with equal scores is outside the contract.  iou [n, n] is the box IoU of the rows IN SORTED ORDER,
 *     every entry written:  area = (x2 - x1) * (y2 - y1) of each box;  w = max(min(x2_i, x2_j) - max(x1_i, x1_j), 0), h likewise;
 *     overlap = w * h;  union = max((area_i + area_j) - overlap, 1e-6f);  iou = overlap / union.  valid [n] bytes: sorted row i
 *     is dropped (0) when ANY earlier sorted row j < i, dropped or not, has iou[i, j] > thr_i, thr_i = nms_backdrop_iou_thr when
 *     the row's score < obj_score_thr, else nms_class_iou_thr (:440-446).  Not a greedy NMS: rows are independent.
 * qdtrack_hip_scores_f32: embeds [n, D], labels [n] int64 (in detection order; the kernels go through `order`).  scores
 *     [n, Mt], Mt = M + b0 + .. : row r is sorted row r; rows with valid 0 take no part and are not written.  scores = (softmax
 *     over the row + softmax over the column over the valid rows) / 2 of embeds . memo^T, both with the maximum subtracted
 *     (:463-466), times (label == the column's label ? 1 : 0) when with_cats (:477-479).  row_stats [2 n] is a workspace.  n == 0
 *     or Mt == 0: no launch.
 * qdtrack_hip_associate_f32: one workgroup walks the valid rows in sorted order (:481-492), only when M > 0 (`self.empty`, :458,
 *     looks at the tracklets alone): the row maximum conf and its lowest index over the scores with the tracklet columns taken
 *     so far read as 0.  When conf > match_score_thr and the column is a tracklet: score > obj_score_thr gives the row the
 *     tracklet's id and takes the column, else conf > nms_conf_thr makes the id -2.  A best column that is a backdrop changes
 *     nothing.  Rows still -1 with score > init_score_thr get num_tracklets, num_tracklets + 1, ... in order (:493-499).  The new
 *     backdrop frame is the rows with id -1 after that, but for those with iou[i, j] > nms_backdrop_iou_thr for an earlier VALID
 *     row j (:374-379); with backdrop_frames == 0 it is not kept and counts 0 rows.  result [4 n + 4] int64 = the valid rows'
 *     detections in sorted order (zeros after them), their ids (-3 after them), their sorted rows (zeros after them; the
 *     reference picks `indices` by these, :448), the number of valid rows, the next count, the next num_tracklets, the rows of
 *     the new backdrop frame (to here the caller's one host copy), then the ids by sorted row (-3 for a dropped row), which the
 *     update reads.  plan [2 capacity + 2 n] int32 is the update's plan: the detection that feeds a slot,
 *     where a slot lands after the stable compaction of the slots with frame_id - last_frame >= memo_tracklet_frames (:389-394),
 *     where a sorted row's new tracklet lands, and its row of the new backdrop frame.  next_state's meta is written.  n == 0 is a
 *     call like any other (expiry runs, an empty backdrop frame is pushed).  M + n <= capacity and n <= backdrop_capacity are
 *     required (DYNMASK_ERR_BAD_DIMS): the caller falls back before the bank can overflow.
 * qdtrack_hip_update_f32: writes next_state from state, plan and result (:346-397): a matched slot gets velocity = (bbox - old
 *     bbox) / (frame_id - last_frame) averaged over acc_frame, embed = keep_weight * embed + momentum * new (the caller rounds
 *     1 - momentum as the reference's Python does), the detection's label, last_frame = frame_id and acc_frame + 1; an unmatched
 *     slot moves unchanged; new tracklets are appended in row order with zero velocity and acc_frame 0; the new backdrop frame
 *     becomes frame 0 and frame k moves to k + 1, the one past backdrop_frames leaving.  frame_id must be above every
 *     last_frame.
 * Limits (DYNMASK_ERR_UNSUPPORTED beyond): n <= MASKPOST_HIP_MAX_MASKS, capacity <= TRACK_HIP_MAX_CAPACITY, D <= TRACK_HIP_MAX_DIM,
 * backdrop_capacity <= QDTRACK_HIP_MAX_BACKDROPS, backdrop_frames <= QDTRACK_HIP_MAX_BACKDROP_FRAMES.  qdtrack_hip_last_kernel
 * names the last successful call's kernels ("" before the first).
 */
#define QDTRACK_HIP_MAX_BACKDROPS 1024
#define QDTRACK_HIP_MAX_BACKDROP_FRAMES 4
#define QDTRACK_HIP_STATE_FIELDS 11
size_t qdtrack_hip_state_offset(int field, int capacity, int D, int backdrop_capacity, int backdrop_frames);
int qdtrack_hip_prepare_f32(const float* bboxes, int n, float obj_score_thr, float nms_backdrop_iou_thr, float nms_class_iou_thr,
                            int* order, float* iou, unsigned char* valid, void* stream);
int qdtrack_hip_scores_f32(const float* embeds, const long long* labels, const int* order, const unsigned char* valid, const void* state,
                           int n, int M, int b0, int b1, int b2, int b3, int capacity, int D, int backdrop_capacity,
                           int backdrop_frames, int with_cats, float* row_stats, float* scores, void* stream);
int qdtrack_hip_associate_f32(const float* scores, const unsigned char* valid, const int* order, const float* bboxes, const float* iou,
                              const void* state, void* next_state, int n, int M, int b0, int b1, int b2, int b3, int capacity, int D,
                              int backdrop_capacity, int backdrop_frames, float match_score_thr, float obj_score_thr, float nms_conf_thr,
                              float init_score_thr, float nms_backdrop_iou_thr, int frame_id, int memo_tracklet_frames, int* plan,
                              long long* result, void* stream);
int qdtrack_hip_update_f32(const float* embeds, const float* bboxes, const long long* labels, const int* order, const int* plan,
                           const long long* result, const void* state, void* next_state, int n, int M, int b0, int b1, int b2, int b3,
                           int capacity, int D, int backdrop_capacity, int backdrop_frames, float keep_weight, float momentum,
                           int frame_id, void* stream);
const char* qdtrack_hip_last_kernel(void);

/*
 * The training criterion (criterion_hip_*) that consumes the matcher's indices (SetCriterion / DINOCriterion, deformable_detr.py:290-784, the loss functions
 * of segmentation.py:74-166) has its two streaming losses in uninext_amd/csrc/criterion.hip.  In this header because the set of headers under include/ is pinned (tests/test_binding_signatures_cpu.py) and every
 * export declared by matcher_cost_hip.h has to be named matcher_cost_hip_* (tests/test_lsap_cpu.py), which these are not; error codes are the DYNMASK_ERR_* above plus CRITERION_ERR_WORKSPACE.  Exact fp32 inputs and
 * outputs, no float atomics: every sum is formed as per-workgroup partial sums (float64) in the workspace the caller lends, and
 * one small kernel adds them in a fixed order, so a result is the same bits on every call.
 *
 *   term(x, t) = alpha_t * ce * (1 - p_t)^2,  p = sigmoid(x),  ce = max(x, 0) - x t + log(1 + exp(-|x|)),
 *                p_t = p t + (1 - p)(1 - t),  alpha_t = alpha t + (1 - alpha)(1 - t)          (segmentation.py:155-162, gamma = 2)
 *
 * criterion_hip_token_focal_forward_f32: loss[0] = the sum of term over the counted tokens of logits [batch, Q, T] (T <= 256, more is
 *   DYNMASK_ERR_UNSUPPORTED).  text_mask [batch, T] is int64 (CRITERION_MASK_INT64), bytes (CRITERION_MASK_BOOL) or absent
 *   (CRITERION_MASK_NONE, NULL); a token counts when its mask is > 0.  row_target int32 [batch, Q]: the row of positive_map_all
 *   [G, T] fp32 (targets in [0, 1], not only 0 / 1) the query is matched to; any value outside [0, G) is "unmatched", target 0.
 * criterion_hip_token_focal_backward_f32: grad_logits [batch, Q, T] = scale[0] * d loss / d logits, recomputed from the logits, exactly
 *   0.0 at tokens that do not count; every element is written.  scale is a DEVICE scalar.
 * criterion_hip_mask_losses_forward_f32: src [n, F, h, w] fp32 logits; gt [R, H_im, W_im] bytes (the padded boolean masks); the target of
 *   pixel (f, y, x) of instance i is gt[gt_row[i] + f, start + stride y, start + stride x] != 0 with start = stride / 2 (rows outside
 *   [0, R) read as 0).  sums [n, 4] = per instance (sum of term at alpha 0.25, sum sigmoid(x) t, sum sigmoid(x), sum t);
 *   losses[0] = sum_i sums[i, 0] / (F h w) / num_boxes (loss_mask), losses[1] = sum_i (1 - (2 I_i + 1) / (S_i + T_i + 1)) / num_boxes
 *   (loss_dice).
 * criterion_hip_mask_losses_backward_f32: grad_src [n, F, h, w] = grad_mask[0] * d loss_mask / d src + grad_dice[0] * d loss_dice / d src
 *   from src, gt and the forward's sums; grad_mask and grad_dice are DEVICE scalars; every element is written.
 * criterion_hip_workspace_bytes(which, count, per): CRITERION_TOKEN_FOCAL: (batch * Q, T); CRITERION_MASK_LOSSES: (n, F h w).  The
 *   workspace is 16-byte aligned.  Empty problems (batch * Q == 0, n == 0) return 0 and write zeros to loss / losses.
 * criterion_hip_last_kernel(): the kernel the last successful call enqueued, e.g. "token_focal_fwd<vec4>" (16-byte loads: T or w a
 *   multiple of 4 and aligned bases) or "mask_losses_bwd<scalar>".
 */
#define CRITERION_ERR_WORKSPACE (-6)     /* workspace_bytes below criterion_hip_workspace_bytes, or not 16-byte aligned */
#define CRITERION_HIP_MAX_TOKENS 256
#define CRITERION_MASK_NONE 0
#define CRITERION_MASK_INT64 1
#define CRITERION_MASK_BOOL 2
#define CRITERION_TOKEN_FOCAL 0
#define CRITERION_MASK_LOSSES 1
#define CRITERION_BOXINST 2
#define CRITERION_BOXINST_MAX_DILATION 8
#define CRITERION_IMAGE_U8 0
#define CRITERION_IMAGE_F32 1

size_t criterion_hip_workspace_bytes(int which, long long count, long long per);
const char* criterion_hip_last_kernel(void);
int criterion_hip_token_focal_forward_f32(const float* logits, const void* text_mask, int mask_kind, const int32_t* row_target,
                                      const float* positive_map_all, int G, float alpha, int batch, int Q, int T, float* loss,
                                      void* workspace, size_t workspace_bytes, void* stream);
int criterion_hip_token_focal_backward_f32(const float* logits, const void* text_mask, int mask_kind, const int32_t* row_target,
                                       const float* positive_map_all, int G, float alpha, const float* scale, int batch, int Q,
                                       int T, float* grad_logits, void* stream);
int criterion_hip_mask_losses_forward_f32(const float* src, const unsigned char* gt, const int32_t* gt_row, int n, int F, int h, int w,
                                      int R, int H_im, int W_im, int stride, float num_boxes, float* sums, float* losses,
                                      void* workspace, size_t workspace_bytes, void* stream);
int criterion_hip_mask_losses_backward_f32(const float* src, const unsigned char* gt, const int32_t* gt_row, const float* sums,
                                       const float* grad_mask, const float* grad_dice, int n, int F, int h, int w, int R, int H_im,
                                       int W_im, int stride, float num_boxes, float* grad_src, void* stream);

/*
 * BoxInst training (uninext_amd/csrc/boxinst.hip): the box-supervised mask losses of SetCriterion.loss_masks_boxinst
 * (deformable_detr.py:457-527, :787-851) and the two target tensors of add_bitmasks_from_boxes (uninext_img.py:563-659).  The same
 * rules as above: exact fp32 in and out, float64 partial sums combined in a fixed order, no float atomics, bitwise repeatable,
 * kernels reported by criterion_hip_last_kernel().  Empty problems return 0 and write zeros.
 *
 * criterion_hip_box_bitmasks: boxes [G, 4] fp32 xyxy in pixels (>= 0) -> out [G, H, W] bytes (0 / 1): pixel (y, x) is set where
 *   int(y1) <= y < int(y2 + 1) and int(x1) <= x < int(x2 + 1), truncation toward zero, y2 + 1 one fp32 addition, the far ends clamped
 *   to H and W as a slice clamps them.  No coordinate is copied to the host.  "box_bitmasks<vec4>": W a multiple of 16 and an aligned
 *   `out`, 16 bytes a store.
 * criterion_hip_color_similarity_f32: images [bs, 3, H, W] BGR, bytes (CRITERION_IMAGE_U8) or fp32 holding integers
 *   (CRITERION_IMAGE_F32); mask [bs, H, W] bytes; table [256] float64, the sRGB linearisation of byte / 255, on the device.  With
 *   h = H / stride, w = W / stride: every channel is averaged over stride x stride pixels in fp32 and truncated to a byte, the pixel
 *   converted to CIE Lab (D65, 2 degrees; skimage.color.rgb2lab) in float64 and rounded to fp32; out [bs, 8, h, w]:
 *   out[b, k, y, x] = exp(-0.5 ||lab(y, x) - lab(y + dy_k, x + dx_k)||_2) (fp32) * (mask[b, start + stride (y + dy_k),
 *   start + stride (x + dx_k)] != 0), 0 where the neighbour is outside the image; (dy_k, dx_k) = dilation * the 3 x 3 window's offsets
 *   in row-major order without the centre (F.unfold's order).  lab [bs, 3, h, w] is written too unless NULL.  1 <= dilation <= 8.
 * criterion_hip_boxinst_forward_f32: src [N_all, F, h, w] fp32 logits, F == 1 (more: DYNMASK_ERR_UNSUPPORTED); inst int32 [n]: the row
 *   of src kept instance i reads (distinct rows; outside [0, N_all): logits 0); gt / gt_row / stride as in
 *   criterion_hip_mask_losses_forward_f32; sim [B, 8, h, w] as above and img int32 [n], the image of instance i (outside [0, B): no
 *   weight); warmup a DEVICE scalar.  With lf = logsigmoid(x), lb = logsigmoid(-x), both 0 at a neighbour outside the image:
 *     l(i, p, k) = -logsumexp(lf_p + lf_p', lb_p + lb_p'),  p' = p + (dy_k, dx_k),   w(i, p, k) = (sim[img_i, k, p] >= thresh) t_p
 *     losses[1] = warmup[0] * sum w l / max(sum w, 1)                                                        (loss_pairwise)
 *     losses[0] = mean_i (dice(sigmoid(colmax_i), colmax t_i) + dice(sigmoid(rowmax_i), rowmax t_i)),
 *                 dice(a, b) = 1 - 2 <a, b> / (|a|^2 + |b|^2 + 1e-5)                                           (loss_prj)
 *   The maxima are taken of the LOGITS, the lowest index among equals (torch takes them of the fp32 sigmoids: they differ only
 *   where two logits of a row or column collide in sigmoid space).  Saved for the backward: pos int32 [n, h + w] (per row the
 *   column of its maximum, then per column the row), tmax bytes [n, h + w] (the targets' maxima), sums float64 [n, 4] = (I_row, U_row,
 *   I_col, U_col) with the 1e-5 inside U, totals float64 [2] = (sum w l, sum w).  Rows wider than the LDS tile allows
 *   ((8 + 2 dilation) * 9 * w bytes > 63 KiB): DYNMASK_ERR_UNSUPPORTED.
 * criterion_hip_boxinst_backward_f32: grad_src [N_all, F, h, w] = grad_prj[0] * d losses[0] / d src + grad_pairwise[0] * d losses[1] /
 *   d src, every element written, exactly 0.0 in the rows no instance reads; grad_prj and grad_pairwise are DEVICE scalars.
 * criterion_hip_workspace_bytes(CRITERION_BOXINST, n, F h w): the forward's workspace.
 */
int criterion_hip_box_bitmasks(const float* boxes, int G, int H, int W, unsigned char* out, void* stream);
int criterion_hip_color_similarity_f32(const void* images, int image_kind, const unsigned char* mask, const double* table, int bs,
                                       int H, int W, int stride, int dilation, float* out, float* lab, void* stream);
int criterion_hip_boxinst_forward_f32(const float* src, const int32_t* inst, const unsigned char* gt, const int32_t* gt_row,
                                      const float* sim, const int32_t* img, const float* warmup, int n, int N_all, int F, int h, int w,
                                      int R, int H_im, int W_im, int stride, int B, float thresh, int dilation, int32_t* pos,
                                      unsigned char* tmax, double* sums, double* totals, float* losses, void* workspace,
                                      size_t workspace_bytes, void* stream);
int criterion_hip_boxinst_backward_f32(const float* src, const int32_t* inst, const unsigned char* gt, const int32_t* gt_row,
                                       const float* sim, const int32_t* img, const float* warmup, const int32_t* pos,
                                       const unsigned char* tmax, const double* sums, const double* totals, const float* grad_prj,
                                       const float* grad_pairwise, int n, int N_all, int F, int h, int w, int R, int H_im, int W_im,
                                       int stride, int B, float thresh, int dilation, float* grad_src, void* stream);

/*
 * Encoder input preparation (encprep_hip_*): the step between the backbone's features and the first encoder layer, in
 * uninext_amd/csrc/enc_prep.hip -- the loop over `features` of coco_forward (ddetrs_dn.py:117-143) with PositionEmbeddingSine
 * (position_encoding.py:36-56, normalize = True), the GroupNorm(32, 256) of input_proj, the flatten statements of
 * deformable_transformer_dino.py:181-201 and get_reference_points (:289-301).  In this header for the same reason as detpost_*;
 * error codes are the DYNMASK_ERR_* above.  No atomics, every sum in a fixed order: bitwise repeatable.
 *
 * `levels` is a HOST array [n_levels, 3] of ints (H, W, source): the level's padding mask is resized from the image mask
 * (source -1) or from the mask of an earlier level whose own source is the image, by PyTorch's legacy `nearest` rule
 * (maskpost_binarize_hip_f32 pins it), applied twice in the second case.  S = sum H W tokens an image, level after level;
 * T = sum (W + H).  More than ENCPREP_HIP_MAX_LEVELS levels: DYNMASK_ERR_UNSUPPORTED.  batch == 0 or n_levels == 0 returns 0
 * before any runtime call.  x / weight / bias are HOST arrays of n_levels device pointers, eps a HOST array of n_levels floats.
 *
 * encprep_hip_masks_u8: image_mask [batch, Hi, Wi] bytes (non-zero: padded).  mask_flatten [batch, S] bytes (0 / 1);
 *     yx_embed [batch, S, 2] = (y_embed, x_embed), the cumulative counts of unpadded pixels down the token's column and along its
 *     row, itself included (exact integers); totals [batch, T]: per level its W column totals, then its H row totals;
 *     valid_ratios [batch, n_levels, 2] = (first row's count / W, first column's count / H).
 * encprep_hip_pos_f32: lvl_pos_embed [batch, S, 256]: channel c < 128 belongs to y, c >= 128 to x; with j = c mod 128
 *     arg = (((count - 0.5) / (total + eps)) * scale) / dim_t[j], every step one IEEE fp32 operation; sinf(arg) for even j and
 *     cosf(arg) for odd j, plus level_embed[level, c].  dim_t [128] and level_embed [n_levels, 256] on the device.
 *     reference_points [batch, S, n_levels, 2]: ((x + 0.5) / (valid_ratios[b, l, 0] * W), (y + 0.5) / (valid_ratios[b, l, 1] * H))
 *     of the token's own level l, times valid_ratios[b, l', :].  channels must be 256.
 * encprep_hip_gn_stats_f32: x[l] [batch, 256, H_l, W_l], 16-byte aligned.  partials: encprep_hip_workspace_bytes(batch, levels,
 *     n_levels) bytes, 16-byte aligned: float64 sums of x and x * x of the slices of every (image, level, group).
 * encprep_hip_gn_apply_f32: adds a group's slices first to last, mean = sum / n, rstd = 1 / sqrt(max(sumsq / n - mean^2, 0) +
 *     eps[l]) in float64, and writes src_flatten[b, start_l + p, c] = (x - mean) * rstd * weight[l][c] + bias[l][c], rounded to
 *     fp32 once; x[l] needs no alignment here.  mean, rstd [batch, n_levels, 32] (fp32) are written too.
 *     channels != 256 or groups != 32: DYNMASK_ERR_UNSUPPORTED.
 * encprep_hip_last_kernel names the kernel the last successful call enqueued ("" before the first).
 */
#define ENCPREP_HIP_MAX_LEVELS 8
#define ENCPREP_HIP_CHANNELS 256
#define ENCPREP_HIP_GROUPS 32
#define ENCPREP_HIP_PIXEL_TILE 32
size_t encprep_hip_workspace_bytes(int batch, const int* levels, int n_levels);
int encprep_hip_masks_u8(const unsigned char* image_mask, int batch, int Hi, int Wi, const int* levels, int n_levels,
                         unsigned char* mask_flatten, float* valid_ratios, float* yx_embed, float* totals, void* stream);
int encprep_hip_pos_f32(const float* yx_embed, const float* totals, const float* valid_ratios, const float* level_embed,
                        const float* dim_t, int batch, const int* levels, int n_levels, int channels, float scale, float eps,
                        float* lvl_pos_embed, float* reference_points, void* stream);
int encprep_hip_gn_stats_f32(const float* const* x, int batch, const int* levels, int n_levels, int channels, int groups,
                             double* partials, size_t partial_bytes, void* stream);
int encprep_hip_gn_apply_f32(const float* const* x, const float* const* weight, const float* const* bias, const float* eps,
                             const double* partials, size_t partial_bytes, int batch, const int* levels, int n_levels, int channels,
                             int groups, float* src_flatten, float* mean, float* rstd, void* stream);
const char* encprep_hip_last_kernel(void);

/*
 * The text encoder (uninext_amd/csrc/bert.hip): the two kernels of a BERT prompt encoder of bert-base geometry, the
 * reference's BertEncoder (projects/UNINEXT/uninext/models/deformable_detr/bert_model.py) around transformers' BertModel.
 * Declared in this header like the other stages around the mask head; the names carry their own prefix.
 * Returns 0, a negative BERT_ERR_*, or a positive hipError_t; the message is available from msda_hip_last_error().  Every check
 * runs before the device is touched; an empty batch enqueues nothing and returns 0.
 */
#define BERT_ERR_NULL_POINTER (-1)
#define BERT_ERR_BAD_DIMS (-2)
#define BERT_ERR_UNSUPPORTED (-5)     /* a head_dim, len, hidden size, stride or alignment without a kernel, or an unknown mask kind */

#define BERT_MASK_NONE 0              /* mask is ignored (may be NULL): every key is kept */
#define BERT_MASK_KEY_I64 1           /* mask [batch, len] int64, non-zero = the key is kept (the tokenizer's attention_mask) */
#define BERT_MASK_KEY_U8 2            /* mask [batch, len], one byte each, non-zero = kept */
#define BERT_MASK_FULL_U8 3           /* mask [batch, len, len] indexed [b, query, key], one byte each, non-zero = kept (PARALLEL_DET) */

/*
 * Self-attention core of BertSelfAttention between the q / k / v projections and attention.output.dense, at inference.  For
 * every batch b, head h and query i, with D = head_dim = 64 and K(b, i) the keys the mask keeps:
 *     s[i, j]   = sum_d (q[i, d] * q_scale) * k[j, d]                                  (q is scaled first, in fp32)
 *     out[i, :] = sum_{j in K} softmax_{j in K}(s[i, :])[j] * v[j, :]
 * An excluded key has probability exactly 0.  For every query that keeps at least one key that is what transformers 4.x's
 * additive `(1 - mask) * finfo.min` gives in fp32.  A query that keeps NO key is outside the reference's reach (the tokenizer
 * always emits [CLS]); its row of `out` is written as zeros (the composition would give the uniform average of all values).
 *
 * q, k, v   [batch, len, num_heads * 64] each, rows q_stride / k_stride / v_stride floats apart (batches len rows apart): the
 *           three may be views of one [batch, len, 3 * hidden] projection output, read in place
 * mask      of mask_kind, or NULL with BERT_MASK_NONE
 * out       [batch, len, num_heads * 64], contiguous, token-major: the input of attention.output.dense
 * Supported: head_dim == 64 and 1 <= len <= 512 (BERT_ERR_UNSUPPORTED otherwise), any batch and num_heads; q, k, v, out 16-byte
 * aligned, strides multiples of 4 and at least num_heads * 64.  v is to be finite.
 *
 * Exact fp32 products with fp32 accumulation on v_mfma_f32_32x32x2_f32 in a fixed order, no float atomics, no workspace, and
 * nothing of size batch * heads * len * len is written: a workgroup keeps 32 queries, its two waves take one half of the key
 * tiles each and are combined in that order; a tile of 32 keys none of which is kept (by any of the wave's queries) is neither
 * loaded nor multiplied.  Bitwise repeatable across runs and streams, and the same bits whatever the strides.
 */
int bert_hip_self_attention_f32(const float* q, const float* k, const float* v, long long q_stride, long long k_stride,
                                long long v_stride, const void* mask, int mask_kind, int batch, int num_heads, int len,
                                int head_dim, float q_scale, float* out, void* stream);

/*
 * BertEmbeddings at inference in one launch:
 *     out[b, t, :] = LayerNorm(word[ids[b, t]] + type[tt[b, t]] + position[t]) * gamma + beta
 * summed in that order (transformers'), biased variance, eps inside the square root, a row's sums in add_layernorm_hip_f32's
 * order.  ids [batch, len] int64; token_type_ids [batch, len] int64 or NULL (type 0); word [vocab, hidden], position
 * [max_positions, hidden], type [type_vocab, hidden], gamma, beta [hidden], out [batch, len, hidden], all contiguous fp32 and
 * 16-byte aligned.  hidden % 4 == 0 and hidden <= 4096, len <= max_positions (BERT_ERR_UNSUPPORTED / BERT_ERR_BAD_DIMS).
 * No table is read outside its rows: a row whose id or type id is out of range is written as NaN, its neighbours are not
 * affected.
 */
int bert_hip_embed_layernorm_f32(const long long* ids, const long long* token_type_ids, const float* word, const float* position,
                                 const float* type, const float* gamma, const float* beta, float eps, int batch, int len,
                                 int hidden, int vocab, int max_positions, int type_vocab, float* out, void* stream);

/* Name of the kernel the latest call of each of the two entry points above enqueued ("" before the first call). */
const char* bert_hip_attention_last_kernel(void);
const char* bert_hip_embed_last_kernel(void);

/*
 * The training route of the self-attention core (uninext_amd/csrc/bert_attn_bwd.hip): the forward that keeps the row
 * log-sum-exp, a recomputing backward, and the attention dropout (attention_probs_dropout_prob) decided inside the kernels.
 * Same error codes and conventions as above, plus BERT_ERR_WORKSPACE.
 *
 * DROPOUT.  Entry (query i, key j) of (batch b, head h) is kept when word j % 4 of
 *     Philox4x32-10(key = seed, counter = (offset low, offset high, i, (b * num_heads + h) << 8 | j / 4))
 * is >= (uint32) llrint(dropout_p * 2^32); a kept probability is multiplied by c = 1.0f / (1.0f - dropout_p), formed on the
 * host in fp32 (uninext_amd/csrc/philox.hpp, side 0: the scheme of biattn_hip_train_dropout_f32).  `seed` is a DEVICE pointer
 * to two 64-bit words (seed, offset); it may be NULL only when dropout_p == 0.  The decision is a pure function of those
 * arguments: the forward, both backward passes and bert_hip_dropout_keep_u8 call the same device function, and no mask is
 * stored.  The masks are NOT the stream of torch's F.dropout.  dropout_p outside [0, 1) or NaN: BERT_ERR_BAD_DIMS; a NULL seed
 * with dropout_p > 0: BERT_ERR_NULL_POINTER; batch * num_heads > 65535 with dropout_p > 0: BERT_ERR_UNSUPPORTED (the counter's
 * 16 bits).  With dropout_p == 0 every result is bitwise that of the call without dropout, whatever `seed` is.
 */
#define BERT_ERR_WORKSPACE (-6)       /* workspace_bytes below bert_hip_self_attention_backward_workspace_bytes */

/*
 * bert_hip_self_attention_f32 for training: the same arguments and limits, and
 *     lse [batch * num_heads, roundup(len, 32)]: log sum_{j in K(b, i)} exp(s[i, j]) of the scaled scores over the keys the
 *         mask keeps; -inf for a query that keeps no key; 0 for the rows past len
 *     out[i, :] = sum_{j in K} c m[i, j] softmax_{j in K}(s[i, :])[j] * v[j, :]
 * The softmax statistics run over all keys the mask keeps; dropout comes after the normalisation.  With dropout_p == 0 `out` is
 * bitwise bert_hip_self_attention_f32's.  A query that keeps no key: a row of zeros, as there.  lse 16-byte aligned.
 */
int bert_hip_self_attention_train_f32(const float* q, const float* k, const float* v, long long q_stride, long long k_stride,
                                      long long v_stride, const void* mask, int mask_kind, int batch, int num_heads, int len,
                                      int head_dim, float q_scale, float* out, float* lse, float dropout_p,
                                      const unsigned long long* seed, void* stream);

/*
 * The backward of bert_hip_self_attention_train_f32.  With g = grad_out [batch, len, num_heads * 64] (contiguous), m the keep
 * indicator of the dropout, c as above and p[i, j] = exp(s[i, j] - lse[i]) on the keys the mask keeps (0 elsewhere):
 *     delta[i] = g[i] . out[i]
 *     dp[i, j] = c m[i, j] (g[i] . v[j])
 *     ds[i, j] = p[i, j] (dp[i, j] - delta[i])
 *     dq[i]    = q_scale * sum_j ds[i, j] k[j]
 *     dk[j]    = sum_i ds[i, j] (q[i] * q_scale)
 *     dv[j]    = sum_i c m[i, j] p[i, j] g[i]
 * q, k, v, mask, q_scale, dropout_p and seed as given to the forward; out and lse as it wrote them.  dq, dk, dv have row strides
 * of their own (the limits of q_stride): the three may be views of one [batch, len, 3 * hidden] buffer, as q, k, v may.  Every
 * output element is written by exactly one thread.  An excluded key gets dk = dv = 0.  A query that keeps NO key (its `out` row
 * is zeros, see above) gets a dq row of ZEROS and contributes exactly nothing to dk and dv for a finite grad_out row: the
 * composition's uniform average would give it a gradient, and give the values one through it.  The mask gets no gradient.
 *
 * workspace: at least bert_hip_self_attention_backward_workspace_bytes(...) bytes (0 for dimensions the entry point refuses),
 * 16-byte aligned: delta.  A smaller one is BERT_ERR_WORKSPACE.
 *
 * Two kernels on the forward's grid and wave split: a query pass (dq, delta) and a key pass (dk, dv) behind it in stream order.
 * A streamed tile in which no owned token has a kept partner is neither loaded nor multiplied; a key-pass workgroup whose 32
 * keys a [batch, len] mask all excludes stores zeros and streams nothing.  Exact fp32 products on v_mfma_f32_32x32x2_f32, every
 * sum in one fixed order, no float atomics, nothing of size batch * heads * len * len is written; bitwise repeatable across
 * runs and streams, and the same bits whatever the strides.
 */
size_t bert_hip_self_attention_backward_workspace_bytes(int batch, int num_heads, int len, int head_dim);
int bert_hip_self_attention_backward_f32(const float* q, const float* k, const float* v, long long q_stride, long long k_stride,
                                         long long v_stride, const void* mask, int mask_kind, const float* out, const float* lse,
                                         const float* grad_out, int batch, int num_heads, int len, int head_dim, float q_scale,
                                         float* dq, float* dk, float* dv, long long dq_stride, long long dk_stride,
                                         long long dv_stride, void* workspace, size_t workspace_bytes, float dropout_p,
                                         const unsigned long long* seed, void* stream);

/*
 * FOR TESTS AND TOOLS: the keep decisions of the dropout above written out, keep [batch * num_heads, len, len] indexed
 * [b * num_heads + h, query, key], one byte each, 1 = kept -- by the device function the kernels call, and the only place where
 * a mask of that size exists.  The limits of the training entry points (1 <= len <= 512, batch * num_heads <= 65535).
 */
int bert_hip_dropout_keep_u8(const unsigned long long* seed, float dropout_p, int batch, int num_heads, int len,
                             unsigned char* keep, void* stream);

/* Names of the kernels the latest training forward / backward enqueued ("" before the first call): they tell the mask kind and
 * whether dropout was on, e.g. "bert_attn_train<key_i64,drop>", "bert_bwd_q<none>+bert_bwd_kv<none>". */
const char* bert_hip_attention_train_last_kernel(void);
const char* bert_hip_attention_backward_last_kernel(void);

/*
 * THE TRAINING ROUTE of the add + LayerNorm and FFN blocks of a transformer layer (uninext_amd/csrc/layer_train.hip; the inference
 * kernel is include/layernorm_hip.h's add_layernorm_hip_f32, whose LAYERNORM_ERR_* codes these entry points return), with dropout
 * decided inside the kernels and nothing but one activation kept per block.  fp32, device pointers, contiguous rows.
 *
 *   THE KEEP DECISION of entry (row, column) of a [rows, features] tensor is a pure function of (seed, offset, row, column)
 *   (uninext_amd/csrc/philox.hpp: row_words): Philox4x32-10 with key = the two 32-bit halves of the seed (low, high) and
 *   counter = (offset low, offset high, row, column / 4); word t of the call decides column 4 (column / 4) + t;
 *   keep <=> word >= threshold, threshold = (uint32) llrint(p * 2^32); kept entries are scaled by c = 1 / (1 - p) (fp32).  Both
 *   are computed on the host.  rows < 2^32, features % 4 == 0.  `seed` is two 64-bit integers ON THE DEVICE (seed, offset); it
 *   may be NULL only when p == 0.  The forward, the backward and the export call the same function: no mask is ever stored.
 *
 *   dropout_add_layernorm_hip_train_f32      z = residual + keep c x;   out = LayerNorm(z) gamma + beta.
 *       One wave per row, features <= 4096.  residual, gamma, beta may be NULL (0, 1, 0).  z [rows, features] is the one tensor
 *       the backward needs; no statistics and no mask are written.  At p == 0 out is bitwise add_layernorm_hip_f32's.
 *   dropout_add_layernorm_hip_backward_f32   mean and rstd are recomputed from z with the forward's text; with
 *       g = grad_out gamma, xh = (z - mean) rstd:
 *           grad_z = rstd (g - mean(g) - xh mean(g xh));  grad_residual = grad_z;  grad_x = keep c grad_z (mask recomputed);
 *           grad_gamma = sum_rows grad_out xh;  grad_beta = sum_rows grad_out.
 *       The parameter gradients are summed in float64: a workgroup owns 32 consecutive rows (a function of `rows` alone, not
 *       of the device), writes one row of float64 partials into the workspace, and a second kernel adds the rows of partials
 *       in index order.  No atomics: the bits are the same on every run and every machine.  Each of the four output pointers
 *       may be NULL ("not needed"); with grad_gamma and grad_beta both NULL the workspace is not touched and the second
 *       launch is skipped.  At p == 0 grad_x is bitwise grad_residual, so a caller that needs both may pass grad_x = NULL and
 *       use grad_residual twice.  The workspace holds dropout_add_layernorm_hip_backward_workspace_bytes(rows, features)
 *       bytes (0 for dimensions the call refuses).
 *   relu_dropout_hip_f32                     out = keep c max(h, 0).  Flat 16-byte streaming, features <= 65536.
 *   relu_dropout_hip_backward_f32            grad_h = grad_out (out > 0 ? c : 0): it reads `out` alone, takes no seed and
 *       recomputes nothing.  `out > 0` is exact: out is positive exactly where h was positive AND kept, because a positive fp32
 *       number (subnormals included, which the kernels do not flush) times c >= 1 is at least itself and cannot round to 0, and
 *       every other entry is written as 0.
 *   row_dropout_hip_keep_u8                  FOR TESTS: the decisions as bytes, keep [rows, features], 1 = kept.
 *       features <= 65536.
 *
 *   Refused: features % 4 != 0 or over the limit (UNSUPPORTED); negative rows, rows >= 2^32, p outside [0, 1) (BAD_DIMS); a NULL
 *   required pointer, seed == NULL with p > 0 (NULL_POINTER); a workspace below the query (WORKSPACE).  A refused call writes
 *   nothing.  rows == 0 returns 0 and launches nothing.
 *
 * The C ABI is sized for the follow-ups: the decoder layer's three norms and, with another activation, BertSelfOutput / BertOutput.
 */
int dropout_add_layernorm_hip_train_f32(const float* x, const float* residual, const float* gamma, const float* beta, float eps,
                                        long long rows, int features, float p, const unsigned long long* seed, float* z, float* out,
                                        void* stream);
size_t dropout_add_layernorm_hip_backward_workspace_bytes(long long rows, int features);
int dropout_add_layernorm_hip_backward_f32(const float* grad_out, const float* z, const float* gamma, float eps, long long rows,
                                           int features, float p, const unsigned long long* seed, float* grad_x,
                                           float* grad_residual, float* grad_gamma, float* grad_beta, void* workspace,
                                           size_t workspace_bytes, void* stream);
int relu_dropout_hip_f32(const float* h, long long rows, int features, float p, const unsigned long long* seed, float* out,
                         void* stream);
int relu_dropout_hip_backward_f32(const float* grad_out, const float* out, long long rows, int features, float p, float* grad_h,
                                  void* stream);
int row_dropout_hip_keep_u8(const unsigned long long* seed, float p, long long rows, int features, unsigned char* keep,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DYNMASK_HIP_H_ */
