"""Backbone layers with the reference's names and state-dict layout, running on include/patch_embed_hip.h at inference
(SURVEY.md 2b).

  PatchEmbed        projects/UNINEXT/uninext/backbone/utils.py:160-186 (ViT; constructed at backbone/vit.py:291)
  patch_conv2d      the same convolution with nn.Conv2d's NCHW output: ConvNeXt stem and downsample convolutions
                    (backbone/convnext.py:80,87)
  LayerNorm, Block, DropPath, ConvNeXt
                    the ConvNeXt backbone (backbone/convnext.py:18-194): at inference on the GPU (Block.fused / LayerNorm.fused, on by default) a block is
                    patch_embed_hip_convnext_dwconv_ln_f32 -> pwconv1 -> GELU -> pwconv2 -> patch_embed_hip_convnext_scale_residual_f32 and a
                    channels-first LayerNorm is patch_embed_hip_layernorm_cf_f32; under autograd, on the CPU and for other dtypes they
                    run the reference's PyTorch operations.

By default, with autograd recording (training) the layers run the PyTorch-ROCm convolution, which is the same
arithmetic in fp32 and has a backward.  Opt-in (PatchEmbed.own_exact_training, patch_conv2d(..., own_training=True)):
PatchEmbedFunction, the exact forward kernel and its own exact backward (patch_embed_hip_backward_f32: grad-weight,
grad-bias and grad-input on the matrix cores, fixed order, bitwise repeatable).  Likewise opt-in (Block.own_training,
LayerNorm.own_training, ConvNeXt.set_own_training): ConvNeXtHeadFunction, ConvNeXtTailFunction (with stochastic depth) and
LayerNormCFFunction, the ConvNeXt kernels and their own exact backward.
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


# ---- ConvNeXt (backbone/convnext.py) --------------------------------------------------------------------------------------
def _records(x, *params):
    """Autograd would record an operation on these."""
    return torch.is_grad_enabled() and (x.requires_grad or any(p is not None and p.requires_grad for p in params))


def _fp32_on(dev, *params):
    return all(p is None or (p.dtype == torch.float32 and p.device == dev) for p in params)


class ConvNeXtHeadFunction(torch.autograd.Function):
    """`apply(x, dw_weight, dw_bias, ln_weight, ln_bias, eps)` -> the block's head [B, H, W, C]: patch_embed_hip_convnext_dwconv_ln_f32
    forward, patch_embed_hip_convnext_dwconv_ln_backward_f32 backward (exact fp32, fixed order, bitwise repeatable), only the gradients
    autograd asks for.  Saved for backward: x and the parameters; the convolution output is recomputed."""

    @staticmethod
    def forward(ctx, x, dw_weight, dw_bias, ln_weight, ln_bias, eps):
        det = lambda t: None if t is None else t.detach().contiguous()
        x, dw_weight, dw_bias, ln_weight = det(x), det(dw_weight), det(dw_bias), det(ln_weight)
        ctx.eps = float(eps)
        ctx.save_for_backward(x, dw_weight, dw_bias, ln_weight)
        return ext.convnext_dwconv_ln(x, dw_weight, dw_bias, ln_weight, det(ln_bias), eps)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, dw_weight, dw_bias, ln_weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        grads = ext.convnext_dwconv_ln_backward(x, dw_weight, dw_bias, ln_weight, ctx.eps, grad_out.contiguous(), need_input=need[0],
                                                need_dw_weight=need[1], need_dw_bias=need[2], need_ln_weight=need[3], need_ln_bias=need[4])
        return grads + (None,)


class ConvNeXtTailFunction(torch.autograd.Function):
    """`apply(y, gamma, sample_scale, input)` -> `input + ((gamma * y) * sample_scale).permute(0, 3, 1, 2)`: y [B, H, W, C], gamma [C]
    or None, sample_scale [B] (stochastic depth's 0 or 1 / keep) or None, input [B, C, H, W].  Saved for backward: y (when gamma's
    gradient is wanted), gamma and sample_scale.  The gradient of `input` is grad_out itself: no kernel, no copy."""

    @staticmethod
    def forward(ctx, y, gamma, sample_scale, input):
        y = y.detach().contiguous()
        gamma = None if gamma is None else gamma.detach().contiguous()
        ctx.save_for_backward(y if (gamma is not None and ctx.needs_input_grad[1]) else None, gamma, sample_scale)
        return ext.convnext_scale_residual_drop(y, gamma, sample_scale, input.detach().contiguous())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        y, gamma, sample_scale = ctx.saved_tensors
        need_y, need_gamma, _, need_input = ctx.needs_input_grad
        g_y, g_gamma = None, None
        if need_y or need_gamma:
            g_y, g_gamma = ext.convnext_scale_residual_backward(grad_out.contiguous(), y, gamma, sample_scale, need_y=need_y,
                                                                need_gamma=need_gamma)
        return g_y, g_gamma, None, (grad_out if need_input else None)


class LayerNormCFFunction(torch.autograd.Function):
    """`apply(x, weight, bias, eps)` -> LayerNorm over the channels of x [B, C, H, W]: patch_embed_hip_layernorm_cf_f32 forward,
    patch_embed_hip_layernorm_cf_backward_f32 backward.  Saved for backward: x and the weight."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        x, weight = x.detach().contiguous(), weight.detach().contiguous()
        ctx.eps = float(eps)
        ctx.save_for_backward(x, weight)
        return ext.layernorm_channels_first(x, weight, bias.detach().contiguous(), eps)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        return ext.layernorm_channels_first_backward(x, weight, ctx.eps, grad_out.contiguous(), need_input=need[0], need_weight=need[1],
                                                     need_bias=need[2]) + (None,)


class DropPath(nn.Module):
    """Stochastic depth: while training, a sample's residual branch is dropped with probability `drop_prob` and the kept ones are
    scaled by 1 / (1 - drop_prob); the identity in eval mode.  (The reference takes this module from timm.)"""

    def __init__(self, drop_prob=0.0):
        super().__init__()
        self.drop_prob = float(drop_prob)

    def forward(self, x):
        if not self.training or self.drop_prob == 0.0:
            return x
        keep = 1.0 - self.drop_prob
        mask = x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(keep)
        if keep > 0.0:
            mask.div_(keep)
        return x * mask

    def extra_repr(self):
        return "drop_prob=%g" % self.drop_prob


class LayerNorm(nn.Module):
    """LayerNorm over the channels of a channels_last [B, H, W, C] (default) or channels_first [B, C, H, W] tensor
    (backbone/convnext.py:168-194): same constructor; `weight` and `bias` are nn.Embedding(1, C) as there, so the state-dict keys
    are `weight.weight` / `bias.weight`.  channels_first at inference on the GPU: one kernel (patch_embed_hip_layernorm_cf_f32)."""

    # True (default): channels_first at inference (fp32, GPU) is the one-kernel route, 2.6-4.3x ahead of the PyTorch expressions at
    # the four ConvNeXt-L stage shapes (profiles/r10_convnext.txt); False: the reference's PyTorch expressions everywhere
    fused = True
    # True (opt-in): channels_first under autograd, and a no-grad forward in training mode (the first pass of a checkpoint), run as
    # LayerNormCFFunction -- the kernel and its own exact backward; False (default): PyTorch whenever autograd records
    own_training = False

    def __init__(self, normalized_shape, eps=1e-6, data_format="channels_last"):
        super().__init__()
        if data_format not in ("channels_last", "channels_first"):
            raise NotImplementedError
        self.weight = nn.Embedding(1, normalized_shape, _weight=torch.ones((1, normalized_shape)))
        self.bias = nn.Embedding(1, normalized_shape, _weight=torch.zeros((1, normalized_shape)))
        self.eps = eps
        self.data_format = data_format
        self.normalized_shape = (normalized_shape,)

    def _use_hip(self, x):
        w, b = self.weight.weight, self.bias.weight
        return (self.fused and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()
                and x.shape[1] == self.normalized_shape[0] and not _records(x, w, b) and _fp32_on(x.device, w, b)
                and not torch.is_autocast_enabled())

    def _use_hip_training(self, x):
        """The training route: own_training, autograd records (or the module is in training mode), a contiguous fp32 GPU x, fp32
        parameters on its device, no autocast."""
        w, b = self.weight.weight, self.bias.weight
        return (self.own_training and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()
                and x.shape[1] == self.normalized_shape[0] and (self.training or _records(x, w, b)) and _fp32_on(x.device, w, b)
                and not torch.is_autocast_enabled())

    def forward(self, x):
        w, b = self.weight.weight[0], self.bias.weight[0]
        if self.data_format == "channels_last":
            return F.layer_norm(x, self.normalized_shape, w, b, self.eps)
        if self._use_hip_training(x):
            return LayerNormCFFunction.apply(x, w, b, self.eps)
        if self._use_hip(x):
            return ext.layernorm_channels_first(x, w, b, self.eps)
        # The reference's arithmetic, step for step, so that fp32 results are bitwise its own: mean, biased variance as the mean of
        # the squared deviations, a division by sqrt(var + eps) (not var_mean / rsqrt, which round differently), then scale and shift.
        mean = x.mean(dim=1, keepdim=True)
        centred = x - mean
        var = (centred * centred).mean(dim=1, keepdim=True)
        normed = centred / torch.sqrt(var + self.eps)
        return w.view(-1, 1, 1) * normed + b.view(-1, 1, 1)


class Block(nn.Module):
    """ConvNeXt block (backbone/convnext.py:18-57): depthwise 7x7 -> LayerNorm -> Linear 4x -> GELU -> Linear -> layer scale ->
    residual; same constructor and parameter names (`gamma` is an nn.Embedding(1, dim) or None).  At inference on the GPU the
    head (dwconv + permute + norm) and the tail (gamma * x, permute, input + x) are one kernel each; the two Linears and the GELU
    stay with PyTorch."""

    # True (default): the fused route below, ahead of the PyTorch operations at all four ConvNeXt-L stage shapes (whole block
    # 1.07-3.3x, profiles/r10_convnext.txt); False: the reference's PyTorch operations everywhere
    fused = True
    # True (opt-in): under autograd, and in a no-grad forward in training mode (the first pass of a checkpoint), head and tail run
    # as ConvNeXtHeadFunction / ConvNeXtTailFunction -- the kernels and their own exact backward, stochastic depth inside the tail;
    # False (default): PyTorch whenever autograd records
    own_training = False

    def __init__(self, dim, drop_path=0., layer_scale_init_value=1e-6):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.norm = LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(4 * dim, dim)
        self.gamma = nn.Embedding(1, dim, _weight=layer_scale_init_value * torch.ones((1, dim))) if layer_scale_init_value > 0 else None
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()

    def _use_hip(self, x):
        """The fused route: autograd records nothing, x is a contiguous fp32 GPU tensor, every parameter is fp32 on its device,
        the depthwise convolution is the constructor's, C is one the kernel takes, and drop_path is the identity."""
        if not (self.fused and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()):
            return False
        conv, gamma = self.dwconv, (self.gamma.weight if self.gamma is not None else None)
        params = (conv.weight, conv.bias, self.norm.weight.weight, self.norm.bias.weight, gamma, self.pwconv1.weight, self.pwconv1.bias,
                  self.pwconv2.weight, self.pwconv2.bias)
        if _records(x, *params) or not _fp32_on(x.device, *params) or torch.is_autocast_enabled():
            return False
        if self.training and not isinstance(self.drop_path, nn.Identity) and getattr(self.drop_path, "drop_prob", 1.0) > 0.0:
            return False
        return self._geometry(x)

    def _geometry(self, x):
        conv = self.dwconv
        return (conv.groups == conv.in_channels == conv.out_channels == x.shape[1] and tuple(conv.kernel_size) == (7, 7)
                and tuple(conv.stride) == (1, 1) and tuple(conv.padding) == (3, 3) and tuple(conv.dilation) == (1, 1)
                and conv.padding_mode == "zeros" and self.norm.data_format == "channels_last"
                and self.pwconv2.out_features == x.shape[1] and ext.convnext_dwconv_ln_supported(x, conv.weight))

    def _use_hip_training(self, x):
        """The training route: own_training, autograd records (or the module is in training mode), x a contiguous fp32 GPU tensor,
        every parameter fp32 on its device, no autocast, the geometry of _use_hip, drop_path an Identity or a DropPath."""
        if not (self.own_training and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()):
            return False
        conv, gamma = self.dwconv, (self.gamma.weight if self.gamma is not None else None)
        params = (conv.weight, conv.bias, self.norm.weight.weight, self.norm.bias.weight, gamma, self.pwconv1.weight, self.pwconv1.bias,
                  self.pwconv2.weight, self.pwconv2.bias)
        if not (self.training or _records(x, *params)) or not _fp32_on(x.device, *params) or torch.is_autocast_enabled():
            return False
        return isinstance(self.drop_path, (nn.Identity, DropPath)) and self._geometry(x)

    def _sample_scale(self, y):
        """Stochastic depth's per-sample factor [B], drawn by the very call DropPath.forward makes (the same random stream); None
        where DropPath is the identity."""
        dp = self.drop_path
        if not isinstance(dp, DropPath) or not dp.training or dp.drop_prob == 0.0:
            return None
        keep = 1.0 - dp.drop_prob
        mask = y.new_empty((y.shape[0], 1, 1, 1)).bernoulli_(keep)
        if keep > 0.0:
            mask.div_(keep)
        return mask.view(-1)

    def forward(self, x):
        if self._use_hip_training(x):
            y = ConvNeXtHeadFunction.apply(x, self.dwconv.weight, self.dwconv.bias, self.norm.weight.weight[0], self.norm.bias.weight[0],
                                           self.norm.eps)
            y = self.pwconv2(self.act(self.pwconv1(y)))
            return ConvNeXtTailFunction.apply(y, self.gamma.weight[0] if self.gamma is not None else None, self._sample_scale(y), x)
        if self._use_hip(x):
            y = ext.convnext_dwconv_ln(x, self.dwconv.weight, self.dwconv.bias, self.norm.weight.weight[0], self.norm.bias.weight[0],
                                       self.norm.eps)
            y = self.pwconv2(self.act(self.pwconv1(y)))
            return ext.convnext_scale_residual(y.contiguous(), self.gamma.weight[0] if self.gamma is not None else None, x)
        shortcut = x
        x = self.dwconv(x).permute(0, 2, 3, 1)     # B C H W -> B H W C
        x = self.pwconv2(self.act(self.pwconv1(self.norm(x))))
        if self.gamma is not None:
            x = self.gamma.weight[0] * x
        x = x.permute(0, 3, 1, 2)                  # B H W C -> B C H W
        return shortcut + self.drop_path(x)


class ConvNeXt(nn.Module):
    """The ConvNeXt backbone (backbone/convnext.py:60-166): a stem (4x4 / 4 convolution + LayerNorm), three downsample layers
    (LayerNorm + 2x2 / 2 convolution), four stages of Blocks, `norm1..3` on the outputs of stages 1..3; forward returns
    {"res2": ..., ...} for the stages in `out_indices`.  Same constructor and state-dict keys.  The four strided convolutions go
    through patch_conv2d.  set_own_training(True) opts the whole backbone into the kernels' training routes."""

    def __init__(self, in_chans=3, depths=(3, 3, 9, 3), dims=(96, 192, 384, 768), drop_path_rate=0., layer_scale_init_value=1e-6,
                 out_indices=(0, 1, 2, 3), use_checkpoint=False):
        super().__init__()
        self.downsample_layers = nn.ModuleList([nn.Sequential(
            nn.Conv2d(in_chans, dims[0], kernel_size=4, stride=4), LayerNorm(dims[0], eps=1e-6, data_format="channels_first"))])
        for i in range(3):
            self.downsample_layers.append(nn.Sequential(
                LayerNorm(dims[i], eps=1e-6, data_format="channels_first"), nn.Conv2d(dims[i], dims[i + 1], kernel_size=2, stride=2)))
        rates = torch.linspace(0, drop_path_rate, sum(depths)).tolist()
        self.stages = nn.ModuleList()
        for i in range(4):
            first = sum(depths[:i])
            self.stages.append(nn.Sequential(*[Block(dim=dims[i], drop_path=rates[first + j], layer_scale_init_value=layer_scale_init_value)
                                               for j in range(depths[i])]))
        self.out_indices = out_indices
        for i in range(1, 4):
            self.add_module("norm%d" % i, LayerNorm(dims[i], eps=1e-6, data_format="channels_first"))
        self.apply(self._init_weights)
        self.use_checkpoint = use_checkpoint
        self.num_features = dims

    # set_own_training: the whole backbone's training step on the project's kernels (opt-in)
    own_training = False

    def set_own_training(self, flag=True):
        """Block.own_training and LayerNorm.own_training on every block and channels-first LayerNorm of this backbone, and
        patch_conv2d(..., own_training=flag) for the four strided convolutions."""
        self.own_training = bool(flag)
        for m in self.modules():
            if isinstance(m, Block) or (isinstance(m, LayerNorm) and m.data_format == "channels_first"):
                m.own_training = bool(flag)
        return self

    @staticmethod
    def _init_weights(m):
        if isinstance(m, (nn.Conv2d, nn.Linear)):
            nn.init.trunc_normal_(m.weight, std=.02)
            nn.init.constant_(m.bias, 0)

    def forward_features(self, x):
        outs = []
        for i in range(4):
            for layer in self.downsample_layers[i]:
                x = patch_conv2d(x, layer, own_training=self.own_training) if isinstance(layer, nn.Conv2d) else layer(x)
            if self.use_checkpoint:
                from torch.utils import checkpoint
                x = checkpoint.checkpoint(self.stages[i], x)
            else:
                x = self.stages[i](x)
            if i in self.out_indices:
                outs.append(x if i == 0 else getattr(self, "norm%d" % i)(x))
        return tuple(outs)

    def forward(self, x):
        return {"res%d" % (k + 2): v for k, v in enumerate(self.forward_features(x))}
