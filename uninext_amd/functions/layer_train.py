"""The element-wise blocks of a transformer layer under autograd on the HIP training kernels (include/dynmask_hip.h,
uninext_amd/csrc/layer_train.hip): `LayerNorm(residual + dropout(x))` and `dropout(relu(h))`.  Dropout is decided inside the
kernels from (seed, row, column); no mask and no statistics are stored, the backward recomputes them.  Exact fp32, bitwise
repeatable.  DeformableTransformerEncoderLayer.own_training routes through them (opt-in)."""
import torch

from .. import ext as MSDA


class DropoutAddLayerNormFunction(torch.autograd.Function):
    """(x, residual, weight, bias, eps, p, seed) -> LayerNorm(residual + dropout_p(x)) * weight + bias over the last dimension.
    residual, weight and bias may be None; `seed` is ext.bi_attention_seed's two int64 on the device (None at p == 0).  Saves
    z = residual + dropout(x), the weight and the seed: one activation, against the composition's mask, dropped copy, sum and
    statistics.  needs_input_grad decides which gradients the kernel writes."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, eps, p, seed):
        out, z = MSDA.dropout_add_layernorm_train(x, residual, weight, bias, eps, p, seed)
        ctx.save_for_backward(z, *((weight,) if weight is not None else ()), *((seed,) if seed is not None else ()))
        ctx.has_weight, ctx.has_seed, ctx.eps, ctx.p = weight is not None, seed is not None, eps, p
        ctx.has_residual, ctx.has_bias = residual is not None, bias is not None
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        saved = list(ctx.saved_tensors)                            # read once: under checkpoint a second read is an error
        z = saved.pop(0)
        weight = saved.pop(0) if ctx.has_weight else None
        seed = saved.pop(0) if ctx.has_seed else None
        need = ctx.needs_input_grad
        grad_x, grad_res, grad_w, grad_b = MSDA.dropout_add_layernorm_backward(
            grad_out, z, weight, ctx.eps, ctx.p, seed, need_x=need[0], need_residual=ctx.has_residual and need[1],
            need_weight=ctx.has_weight and need[2], need_bias=ctx.has_bias and need[3])
        return grad_x, grad_res, grad_w, grad_b, None, None, None


class ReluDropoutFunction(torch.autograd.Function):
    """(h, p, seed) -> dropout_p(relu(h)).  Saves its own result alone: it is positive exactly where h was positive and kept,
    which is all the backward needs (no seed, no mask, no copy of h or of relu(h))."""

    @staticmethod
    def forward(ctx, h, p, seed):
        out = MSDA.relu_dropout(h, p, seed)
        ctx.save_for_backward(out)
        ctx.p = p
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        out, = ctx.saved_tensors
        return MSDA.relu_dropout_backward(grad_out, out, ctx.p), None, None
