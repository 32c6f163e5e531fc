/*
 * include/layernorm_hip.h -- residual add + LayerNorm of the transformer layers around the MSDeformAttn operator on
 * MI355X (gfx950), part of libmsda_hip.so.
 *
 *     out[r, :] = LayerNorm(x[r, :] + residual[r, :]) * gamma + beta          (biased variance, eps inside the sqrt)
 *
 * replaces `src = src + dropout(src2); src = self.normN(src)` of DeformableTransformerEncoderLayer
 * (projects/UNINEXT/uninext/models/deformable_detr/deformable_transformer_dino.py:356-357, 364-365) at inference
 * (dropout is the identity): one pass over the three tensors instead of two kernels and an intermediate.
 * fp32; `features` must be a multiple of 4 and at most 4096; `residual` may be NULL (plain LayerNorm).  Device
 * pointers, contiguous rows; `stream` is a hipStream_t as void*; the kernel is only enqueued.  Returns 0, a negative
 * LAYERNORM_ERR_*, or a positive hipError_t; the message is available from msda_hip_last_error().
 *
 * THE TRAINING ROUTE of the same blocks (dropout + add + LayerNorm with a recomputing backward, ReLU + dropout, the dropout
 * decided inside the kernels; uninext_amd/csrc/layer_train.hip) is declared in include/dynmask_hip.h, which states its contracts:
 * the prototypes of this header are the add_layernorm family alone.  It returns the LAYERNORM_ERR_* codes below.
 */
#ifndef LAYERNORM_HIP_H_
#define LAYERNORM_HIP_H_

#ifdef __cplusplus
extern "C" {
#endif

#define LAYERNORM_ERR_NULL_POINTER (-1)
#define LAYERNORM_ERR_BAD_DIMS (-2)
#define LAYERNORM_ERR_UNSUPPORTED (-5)
#define LAYERNORM_ERR_WORKSPACE (-6)   /* the training route's backward: a workspace below its workspace_bytes query */

int add_layernorm_hip_f32(const float* x, const float* residual, const float* gamma, const float* beta, float eps,
                          long long rows, int features, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LAYERNORM_HIP_H_ */
