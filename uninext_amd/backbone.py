"""Backbone patch-embedding layers with the reference's names and state-dict layout, running on
include/patch_embed_hip.h at inference.

  PatchEmbed        projects/UNINEXT/uninext/backbone/utils.py:160-186 (ViT; constructed at backbone/vit.py:291)
  patch_conv2d      the same convolution with nn.Conv2d's NCHW output: ConvNeXt stem and downsample convolutions
                    (backbone/convnext.py:80,87)

By default, with autograd recording (training) the layers run the PyTorch-ROCm convolution, which is the same
arithmetic in fp32 and has a backward.  Opt-in (PatchEmbed.own_exact_training, patch_conv2d(..., own_training=True)):
PatchEmbedFunction, the exact forward kernel and its own exact backward (patch_embed_hip_backward_f32: grad-weight,
grad-bias and grad-input on the matrix cores, fixed order, bitwise repeatable).
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ext
from ._cache import CachedModuleMixin, packed_weight


def _use_hip(x, conv):
    needs_grad = torch.is_grad_enabled() and (x.requires_grad or conv.weight.requires_grad)
    return (not needs_grad and conv.groups == 1 and tuple(conv.dilation) == (1, 1) and x.is_contiguous()
            and ext.patch_embed_supported(x, conv.weight, conv.stride, conv.padding))


def _needs_grad(x, conv):
    return torch.is_grad_enabled() and (x.requires_grad or any(p is not None and p.requires_grad for p in (conv.weight, conv.bias)))


def _use_hip_training(x, conv):
    """The training route: autograd records (the input, the weight or the bias), a geometry patch_embed_supported accepts with
    groups 1 and dilation 1, no autocast (PyTorch would run the convolution in a lower precision), parameters fp32 on x's device."""
    return (_needs_grad(x, conv) and conv.groups == 1 and tuple(conv.dilation) == (1, 1) and not torch.is_autocast_enabled()
            and conv.weight.device == x.device and ext.patch_embed_supported(x, conv.weight, conv.stride, conv.padding)
            and (conv.bias is None or (conv.bias.dtype == torch.float32 and conv.bias.device == x.device)))


class PatchEmbedFunction(torch.autograd.Function):
    """`apply(x, weight, bias, channels_last)` -> the patch-embedding convolution of x with `weight` [E, C, k, k] (kernel ==
    stride, no padding) and `bias` [E] or None: [B, H // k, W // k, E] if channels_last, else [B, E, H // k, W // k].  Forward:
    patch_embed_hip_f32, always exact fp32 (never the split-bf16 path); backward: patch_embed_hip_backward_f32 (exact fp32, fixed
    order, bitwise repeatable), only the gradients autograd asks for.  Saved for backward: x and the weight (a parameter: no copy)."""

    @staticmethod
    def forward(ctx, x, weight, bias, channels_last):
        x = x.contiguous()
        w = weight.detach().contiguous()
        out = ext.patch_embed_forward(x, w, bias.detach() if bias is not None else None, channels_last=channels_last)
        ctx.channels_last = bool(channels_last)
        ctx.save_for_backward(x, w)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, w = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        g_x, g_w, g_b = ext.patch_embed_backward(x, w, grad_out.contiguous(), ctx.channels_last, need_input=need_x,
                                                 need_weight=need_w, need_bias=need_b)
        return g_x, g_w, g_b, None


def _packed_weight(conv):
    """Split-bf16 packed copy of conv.weight, cached on the module and rebuilt when the parameter changes."""
    return packed_weight(conv, ext.patch_embed_pack_weight)


def _hip_conv(x, conv, channels_last, exact):
    w = conv.weight
    # short K (ConvNeXt stem, K = 48): the kernel is bound by writing the output and the exact one is faster
    if not exact and w.shape[1] * w.shape[2] * w.shape[3] > 64 and ext.patch_embed_packed_supported(w):
        return ext.patch_embed_packed_forward(x, _packed_weight(conv), w.shape[0], w.shape[2], conv.bias, channels_last)
    return ext.patch_embed_forward(x, w.contiguous(), conv.bias, channels_last=channels_last)


def patch_conv2d(x, conv, exact=True, own_training=False):
    """`conv(x)` for an nn.Conv2d whose kernel equals its stride (no padding): [B, E, H // k, W // k].  Inference on
    the GPU: the exact-fp32 MFMA kernel; exact=False opts into split-bf16 products from cached packed weights (~2e-5 of the output scale).
    own_training=True (opt-in): under autograd the layer runs as PatchEmbedFunction -- the exact forward and its own exact backward;
    what that route does not take (autocast, other dtypes or devices, geometries the kernels lack) stays with PyTorch."""
    if own_training and _use_hip_training(x, conv):
        return PatchEmbedFunction.apply(x, conv.weight, conv.bias, False)
    if _use_hip(x, conv):
        return _hip_conv(x, conv, False, exact)
    return conv(x)


class PatchEmbed(CachedModuleMixin, nn.Module):
    """Image to Patch Embedding (backbone/utils.py:160-186): same constructor, same `proj` parameter names."""

    # True (default): exact-fp32 MFMA kernel (bitwise an fmaf chain, the reference's arithmetic); False -- or env
    # UNINEXT_AMD_SPLIT_BF16=1 -- opts into the split-bf16 path (3 of 4 partial products, ~2e-5 of the output scale, faster)
    exact_fp32 = os.environ.get("UNINEXT_AMD_SPLIT_BF16", "0") != "1"
    # True: under autograd the projection runs as PatchEmbedFunction (exact forward + own exact backward, bitwise repeatable;
    # exact fp32 whatever exact_fp32 says); False (default): PyTorch-ROCm / MIOpen whenever autograd records
    own_exact_training = False

    def __init__(self, kernel_size=(16, 16), stride=(16, 16), padding=(0, 0), in_chans=3, embed_dim=768):
        super().__init__()
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=kernel_size, stride=stride, padding=padding)

    def forward(self, x):
        if self.own_exact_training and _use_hip_training(x, self.proj):
            return PatchEmbedFunction.apply(x, self.proj.weight, self.proj.bias, True)
        if _use_hip(x, self.proj):
            return _hip_conv(x, self.proj, True, self.exact_fp32)
        x = self.proj(x)
        return x.permute(0, 2, 3, 1)   # B C H W -> B H W C (a view, as in the reference)
