"""Float64 restatement of the ConvNeXt block and its LayerNorms (torch on the CPU), written from the formulas of
include/patch_embed_hip.h: what the kernels and the modules of uninext_amd/backbone.py are compared with.  The depthwise
convolution is a sum of 49 shifted slices of the zero-padded input, not a call of a convolution routine."""
import math

import torch
import torch.nn.functional as F


def f64(t):
    return None if t is None else torch.as_tensor(t).detach().to("cpu", torch.float64)


def dwconv7(x, weight, bias=None):
    """x [B, C, H, W], weight [C, 1, 7, 7], bias [C] or None -> [B, C, H, W]; zero padding 3."""
    x, weight, bias = f64(x), f64(weight), f64(bias)
    B, C, H, W = x.shape
    xp = F.pad(x, (3, 3, 3, 3))
    out = torch.zeros_like(x)
    for ky in range(7):
        for kx in range(7):
            out += xp[:, :, ky:ky + H, kx:kx + W] * weight[:, 0, ky, kx].view(1, C, 1, 1)
    if bias is not None:
        out += bias.view(1, C, 1, 1)
    return out


def norm_over(v, dim, weight, bias, eps):
    """LayerNorm along `dim`: biased variance, eps inside the square root."""
    v, weight, bias = f64(v), f64(weight), f64(bias)
    u = v.mean(dim, keepdim=True)
    s = ((v - u) ** 2).mean(dim, keepdim=True)
    shape = [1] * v.dim()
    shape[dim] = -1
    return (v - u) / torch.sqrt(s + eps) * weight.view(shape) + bias.view(shape)


def channel_variance(v, dim):
    """Biased variance along `dim`: the quantity whose inverse square root amplifies a rounding of the mean."""
    v = f64(v)
    return ((v - v.mean(dim, keepdim=True)) ** 2).mean(dim)


def dwconv_ln(x, dw_weight, dw_bias, ln_weight, ln_bias, eps):
    """The block's head -> [B, H, W, C]."""
    return norm_over(dwconv7(x, dw_weight, dw_bias).permute(0, 2, 3, 1), 3, ln_weight, ln_bias, eps)


def layernorm_cf(x, weight, bias, eps):
    """Channels-first LayerNorm of x [B, C, H, W]."""
    return norm_over(x, 1, weight, bias, eps)


def scale_residual(y, gamma, inp):
    """input [B, C, H, W] + gamma * y [B, H, W, C], transposed."""
    y, gamma, inp = f64(y), f64(gamma), f64(inp)
    return inp + (y if gamma is None else y * gamma).permute(0, 3, 1, 2)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def block(x, state, prefix="", eps=1e-6):
    """One block from a state dict with the reference's key names (`gamma.weight` absent: no layer scale)."""
    g = lambda k: f64(state[prefix + k])
    y = dwconv_ln(x, g("dwconv.weight"), g("dwconv.bias"), g("norm.weight.weight")[0], g("norm.bias.weight")[0], eps)
    y = gelu(y @ g("pwconv1.weight").t() + g("pwconv1.bias")) @ g("pwconv2.weight").t() + g("pwconv2.bias")
    gamma = g("gamma.weight")[0] if prefix + "gamma.weight" in state else None
    return scale_residual(y, gamma, x)


def patch_conv(x, weight, bias):
    """Convolution whose kernel equals its stride, no padding (the stem and the downsample layers)."""
    x, weight, bias = f64(x), f64(weight), f64(bias)
    k = weight.shape[2]
    B, C, H, W = x.shape
    p = x[:, :, :H // k * k, :W // k * k].reshape(B, C, H // k, k, W // k, k)
    return torch.einsum("bcyixj,ecij->beyx", p, weight) + bias.view(1, -1, 1, 1)


def convnext(x, state, depths, out_indices=(0, 1, 2, 3), eps=1e-6):
    """The whole backbone -> {"res2": ..., ...} as the module's forward."""
    g = lambda k: f64(state[k])
    x = f64(x)
    outs = []
    for i in range(4):
        if i == 0:
            x = patch_conv(x, g("downsample_layers.0.0.weight"), g("downsample_layers.0.0.bias"))
            x = layernorm_cf(x, g("downsample_layers.0.1.weight.weight")[0], g("downsample_layers.0.1.bias.weight")[0], eps)
        else:
            x = layernorm_cf(x, g("downsample_layers.%d.0.weight.weight" % i)[0], g("downsample_layers.%d.0.bias.weight" % i)[0], eps)
            x = patch_conv(x, g("downsample_layers.%d.1.weight" % i), g("downsample_layers.%d.1.bias" % i))
        for j in range(depths[i]):
            x = block(x, state, "stages.%d.%d." % (i, j), eps)
        if i in out_indices:
            outs.append(x if i == 0 else layernorm_cf(x, g("norm%d.weight.weight" % i)[0], g("norm%d.bias.weight" % i)[0], eps))
    return {"res%d" % (k + 2): v for k, v in enumerate(outs)}
