"""Shapes, seeds, inputs and bounds of the encoder-input tests (tests/test_encoder_input_cpu.py, tests/test_encoder_input_gpu.py)
and of their golden generator (tests/golden/make_encoder_input_golden.py).  Everything is made on the CPU from seeds."""
import collections
import os

import numpy as np
import torch

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_input")
BS, D_MODEL = 2, 256
IMAGE = (40, 56)                                  # strides 8, 16, 32 give the three backbone levels below
LEVELS = ((5, 7), (3, 4), (2, 2), (1, 1))         # the fourth is input_proj[3]'s 3x3 stride-2 convolution of the third
IN_CHANNELS = (8, 12, 16)
FIXTURES = ("no_padding", "padding", "holes")
FLOAT_KEYS = ("src_flatten", "lvl_pos_embed_flatten", "valid_ratios", "reference_points")
EXACT_KEYS = ("mask_flatten", "spatial_shapes", "level_start_index", "valid_ratios")
ULP = 2.0 ** -23                                  # fp32 spacing in [1, 2)

# stub layers of the DeformableTransformerEncoderVL key test: (vl layer, encoder layer, num_layers, num_vl_layers)
ENCODER_VL_STUB = dict(num_layers=3, num_vl_layers=2)


def image_mask(kind, seed, bs=BS, size=IMAGE):
    """[bs, H, W] bool, True = padding."""
    H, W = size
    g = torch.Generator().manual_seed(seed)
    mask = torch.zeros((bs, H, W), dtype=torch.bool)
    if kind == "none":
        return mask
    if kind in ("padding", "holes"):
        for b in range(bs):       # right / bottom padding that differs per image
            h = H - (b * 7 + 3) % max(H // 2, 1)
            w = W - ((b + 1) * 11) % max(W // 2, 1)
            mask[b, h:, :] = True
            mask[b, :, w:] = True
    if kind == "holes":
        mask |= torch.rand((bs, H, W), generator=g) < 0.3
    if kind == "one_valid":
        mask[:] = True
        for b in range(bs):
            mask[b, (3 * b + 1) % H, (5 * b + 2) % W] = False
    if kind == "all_masked":
        mask[:] = True
    return mask


def make_proj_state(in_channels, n_levels, seed, d_model=D_MODEL):
    """A state dict for build_input_proj(in_channels, d_model, n_levels) with GroupNorm weights and biases away from (1, 0)."""
    g = torch.Generator().manual_seed(seed)
    state = collections.OrderedDict()
    cin = None
    for l in range(n_levels):
        k = 1 if l < len(in_channels) else 3
        cin = in_channels[l] if l < len(in_channels) else (in_channels[-1] if l == len(in_channels) else d_model)
        state["%d.0.weight" % l] = torch.randn((d_model, cin, k, k), generator=g) / (cin * k * k) ** 0.5
        state["%d.0.bias" % l] = torch.randn((d_model,), generator=g) * 0.1
        state["%d.1.weight" % l] = 1.0 + 0.5 * torch.randn((d_model,), generator=g)
        state["%d.1.bias" % l] = 0.3 * torch.randn((d_model,), generator=g)
    return state


def make_case(name):
    kind = {"no_padding": "none", "padding": "padding", "holes": "holes"}[name]
    seed = 100 + FIXTURES.index(name)
    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn((BS, c, h, w), generator=g) for c, (h, w) in zip(IN_CHANNELS, LEVELS)]
    return dict(features=feats, image_mask=image_mask(kind, seed + 50), state=make_proj_state(IN_CHANNELS, len(LEVELS), seed + 60),
                level_embed=torch.randn((len(LEVELS), D_MODEL), generator=g))


def golden(name):
    with np.load(os.path.join(HERE, name + ".npz")) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


def build(case, device="cpu"):
    """(features, image_mask, input_proj, level_embed, position_embedding) of a case on `device`."""
    from uninext_amd.modules import PositionEmbeddingSine, build_input_proj
    proj = build_input_proj(IN_CHANNELS, D_MODEL, len(LEVELS))
    proj.load_state_dict(case["state"], strict=True)
    proj = proj.to(device).eval()
    return ([f.to(device) for f in case["features"]], case["image_mask"].to(device), proj, case["level_embed"].to(device),
            PositionEmbeddingSine(D_MODEL // 2, normalize=True))


def spacing(x):
    """fp32 ulp at |x| (float64 tensor in, float64 tensor out)."""
    return torch.from_numpy(np.spacing(np.abs(x.numpy()).astype(np.float32)).astype(np.float64))


def level_masks(image_mask_, shapes, n_backbone):
    """The levels' masks as the reference makes them: backbone levels from the image mask, further levels from masks[0]."""
    from uninext_amd.modules import interpolate_mask
    masks = []
    for l, hw in enumerate(shapes):
        masks.append(interpolate_mask(image_mask_ if l < n_backbone else masks[0], hw))
    return masks


def pos_expected(masks, level_embed, num_pos_feats=128, temperature=10000, scale=2 * np.pi):
    """float64 sin / cos of the fp32 argument torch forms on the CPU in the reference's order, plus level_embed: [B, S, 256]."""
    out = []
    for lvl, mask in enumerate(masks):
        not_mask = ~mask.cpu()
        y_embed = not_mask.cumsum(1, dtype=torch.float32)
        x_embed = not_mask.cumsum(2, dtype=torch.float32)
        eps = 1e-6
        y_embed = (y_embed - 0.5) / (y_embed[:, -1:, :] + eps) * scale
        x_embed = (x_embed - 0.5) / (x_embed[:, :, -1:] + eps) * scale
        dim_t = torch.arange(num_pos_feats, dtype=torch.float32)
        dim_t = temperature ** (2 * (dim_t // 2) / num_pos_feats)
        pos_x = (x_embed[:, :, :, None] / dim_t).double()
        pos_y = (y_embed[:, :, :, None] / dim_t).double()
        assert (x_embed[:, :, :, None] / dim_t).dtype == torch.float32
        pos_x = torch.stack((pos_x[:, :, :, 0::2].sin(), pos_x[:, :, :, 1::2].cos()), dim=4).flatten(3)
        pos_y = torch.stack((pos_y[:, :, :, 0::2].sin(), pos_y[:, :, :, 1::2].cos()), dim=4).flatten(3)
        pos = torch.cat((pos_y, pos_x), dim=3).flatten(1, 2)
        out.append(pos + level_embed[lvl].cpu().double().view(1, 1, -1))
    return torch.cat(out, 1)


def pos_error_ulp(got, expected):
    """Largest error of the position embedding in fp32 ulp at max(1, |expected|).  The bound is 4: the library's sin / cos error
    and the one rounding of the add, doubled -- derived, not measured."""
    err = (got.cpu().double() - expected).abs() / spacing(expected.abs().clamp(min=1.0))
    return float(err.max())


def refpoint_error_ulp(got, want):
    """Largest error of reference_points in fp32 ulp of the expected value (NaN and inf have to agree in place)."""
    got, want = got.cpu().double(), want.cpu().double()
    finite = torch.isfinite(want)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got[~finite & ~torch.isnan(want)], want[~finite & ~torch.isnan(want)])
    if not bool(finite.any()):
        return 0.0
    return float(((got[finite] - want[finite]).abs() / spacing(want[finite])).max())


def groupnorm64(conv, weight, bias, eps):
    """float64 nn.GroupNorm(32, 256) of a [B, 256, H, W] tensor, flattened to tokens [B, HW, 256]."""
    norm = torch.nn.GroupNorm(32, conv.shape[1], eps=eps).double()
    with torch.no_grad():
        norm.weight.copy_(weight.cpu().double())
        norm.bias.copy_(bias.cpu().double())
        return norm(conv.cpu().double()).flatten(2).transpose(1, 2)


def groupnorm_bound(conv, weight, bias, eps, expected):
    """Twice the error torch's own fp32 GroupNorm on the CPU shows against float64 on the same input, never below 4 fp32 ulp of the
    case's largest |output|.  Returns (bound, torch's error)."""
    with torch.no_grad():
        own = torch.nn.functional.group_norm(conv.cpu().float(), 32, weight.cpu().float(), bias.cpu().float(), eps)
    own_err = float((own.flatten(2).transpose(1, 2).double() - expected).abs().max())
    floor = 4 * float(spacing(expected.abs().max().reshape(1))[0])
    return max(2 * own_err, floor), own_err
