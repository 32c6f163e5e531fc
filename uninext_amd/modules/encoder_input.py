"""What stands between the backbone's features and the first encoder layer: the reference's loop over `features`
(models/ddetrs_dn.py:117-143), PositionEmbeddingSine (models/deformable_detr/position_encoding.py:20-56), input_proj
(models/deformable_detr/deformable_detr.py:215-230, :146-148), the flatten statements of DeformableTransformerVLDINO.forward
(models/deformable_detr/deformable_transformer_dino.py:181-201) with get_valid_ratio (:164-171), and get_reference_points
(:289-301).

`prepare_encoder_inputs` returns the seven tensors the encoder consumes.  With fused = True the convolutions of input_proj stay
torch (they are GEMMs) and everything after them is four launches of include/dynmask_hip.h's encprep_hip_* kernels: the NCHW
GroupNorm outputs, the NCHW position embeddings and the three torch.cat copies never exist, and nothing is copied to the host.
The fused route takes d_model 256, GroupNorm(32, 256), PositionEmbeddingSine(128, normalize=True), fp32 tensors on a GPU and no
autograd; anything else runs the composition, which is the reference's statements."""
import collections
import math

import torch
import torch.nn.functional as F
from torch import nn

from .. import ext as MSDA

# The module default of prepare_encoder_inputs(fused=None).  On: faster than the composition with the p10 .. p90 ranges apart at
# both R50 shapes, with and without the convolutions in the timed region (profiles/r23_encoder_input.txt).
ENCODER_INPUT_FUSED = True

EncoderInputs = collections.namedtuple("EncoderInputs", ["src_flatten", "mask_flatten", "lvl_pos_embed_flatten", "spatial_shapes",
                                                         "level_start_index", "valid_ratios", "reference_points"])


class NestedTensor(object):
    """util/misc.py:338-366, what the position embedding needs of it."""

    def __init__(self, tensors, mask):
        self.tensors = tensors
        self.mask = mask

    def to(self, device):
        mask = self.mask.to(device) if self.mask is not None else None
        return NestedTensor(self.tensors.to(device), mask)

    def decompose(self):
        return self.tensors, self.mask

    def __repr__(self):
        return str(self.tensors)


class PositionEmbeddingSine(nn.Module):
    """position_encoding.py:20-56, statement for statement: the embedding is fp32 whatever the features' dtype."""

    def __init__(self, num_pos_feats=64, temperature=10000, normalize=False, scale=None):
        super().__init__()
        self.num_pos_feats = num_pos_feats
        self.temperature = temperature
        self.normalize = normalize
        if scale is not None and normalize is False:
            raise ValueError("normalize should be True if scale is passed")
        if scale is None:
            scale = 2 * math.pi
        self.scale = scale
        self._dim_t = {}

    def dim_t(self, device):
        """The 128-entry table of the fused route: the reference's statement on the CPU, once per device."""
        device = torch.device(device)
        if device not in self._dim_t:
            dim_t = torch.arange(self.num_pos_feats, dtype=torch.float32)
            dim_t = self.temperature ** (2 * (dim_t // 2) / self.num_pos_feats)
            self._dim_t[device] = dim_t.to(device)
        return self._dim_t[device]

    def forward(self, tensor_list):
        x = tensor_list.tensors
        mask = tensor_list.mask
        assert mask is not None
        not_mask = ~mask
        y_embed = not_mask.cumsum(1, dtype=torch.float32)
        x_embed = not_mask.cumsum(2, dtype=torch.float32)
        if self.normalize:
            eps = 1e-6
            y_embed = (y_embed - 0.5) / (y_embed[:, -1:, :] + eps) * self.scale
            x_embed = (x_embed - 0.5) / (x_embed[:, :, -1:] + eps) * self.scale

        dim_t = torch.arange(self.num_pos_feats, dtype=torch.float32, device=x.device)
        dim_t = self.temperature ** (2 * (dim_t // 2) / self.num_pos_feats)

        pos_x = x_embed[:, :, :, None] / dim_t
        pos_y = y_embed[:, :, :, None] / dim_t
        pos_x = torch.stack((pos_x[:, :, :, 0::2].sin(), pos_x[:, :, :, 1::2].cos()), dim=4).flatten(3)
        pos_y = torch.stack((pos_y[:, :, :, 0::2].sin(), pos_y[:, :, :, 1::2].cos()), dim=4).flatten(3)
        pos = torch.cat((pos_y, pos_x), dim=3).permute(0, 3, 1, 2)
        return pos


def interpolate_mask(mask, size):
    """The padding mask [B, H, W] at another size, as the backbone and coco_forward resize it (backbone.py, ddetrs_dn.py:137)."""
    return F.interpolate(mask[None].float(), size=tuple(size)).to(torch.bool)[0]


def get_valid_ratio(mask):
    """deformable_transformer_dino.py:164-171."""
    _, H, W = mask.shape
    valid_H = torch.sum(~mask[:, :, 0], 1)
    valid_W = torch.sum(~mask[:, 0, :], 1)
    valid_ratio_h = valid_H.float() / H
    valid_ratio_w = valid_W.float() / W
    valid_ratio = torch.stack([valid_ratio_w, valid_ratio_h], -1)
    return valid_ratio


def get_reference_points(spatial_shapes, valid_ratios, device):
    """DeformableTransformerEncoderVL.get_reference_points (deformable_transformer_dino.py:289-301)."""
    reference_points_list = []
    for lvl, (H_, W_) in enumerate(spatial_shapes):
        ref_y, ref_x = torch.meshgrid(torch.linspace(0.5, H_ - 0.5, H_, dtype=torch.float32, device=device),
                                      torch.linspace(0.5, W_ - 0.5, W_, dtype=torch.float32, device=device), indexing="ij")
        ref_y = ref_y.reshape(-1)[None] / (valid_ratios[:, None, lvl, 1] * H_)
        ref_x = ref_x.reshape(-1)[None] / (valid_ratios[:, None, lvl, 0] * W_)
        ref = torch.stack((ref_x, ref_y), -1)
        reference_points_list.append(ref)
    reference_points = torch.cat(reference_points_list, 1)
    reference_points = reference_points[:, :, None] * valid_ratios[:, None]
    return reference_points


def build_input_proj(num_channels, hidden_dim=256, num_feature_levels=4):
    """deformable_detr.py:215-230 and :146-148: a 1x1 convolution per backbone output (`num_channels`, one entry each), a 3x3
    stride-2 convolution per further level, each followed by GroupNorm(32, hidden_dim); xavier weights, zero biases."""
    num_channels = list(num_channels)
    if num_feature_levels > 1:
        input_proj_list = []
        for in_channels in num_channels:
            input_proj_list.append(nn.Sequential(
                nn.Conv2d(in_channels, hidden_dim, kernel_size=1),
                nn.GroupNorm(32, hidden_dim),
            ))
        for _ in range(num_feature_levels - len(num_channels)):
            input_proj_list.append(nn.Sequential(
                nn.Conv2d(in_channels, hidden_dim, kernel_size=3, stride=2, padding=1),
                nn.GroupNorm(32, hidden_dim),
            ))
            in_channels = hidden_dim
        input_proj = nn.ModuleList(input_proj_list)
    else:
        input_proj = nn.ModuleList([
            nn.Sequential(
                nn.Conv2d(num_channels[0], hidden_dim, kernel_size=1),
                nn.GroupNorm(32, hidden_dim),
            )])
    for proj in input_proj:
        nn.init.xavier_uniform_(proj[0].weight, gain=1)
        nn.init.constant_(proj[0].bias, 0)
    return input_proj


def flatten_encoder_inputs(srcs, masks, pos_embeds, level_embed):
    """deformable_transformer_dino.py:181-201 for callers who already hold srcs, masks and pos_embeds.  Returns (src_flatten,
    mask_flatten, lvl_pos_embed_flatten, spatial_shapes, level_start_index, valid_ratios)."""
    src_flatten = []
    mask_flatten = []
    lvl_pos_embed_flatten = []
    spatial_shapes = []
    for lvl, (src, mask, pos_embed) in enumerate(zip(srcs, masks, pos_embeds)):
        bs, c, h, w = src.shape
        spatial_shape = (h, w)
        spatial_shapes.append(spatial_shape)
        src = src.flatten(2).transpose(1, 2)
        mask = mask.flatten(1)
        pos_embed = pos_embed.flatten(2).transpose(1, 2)
        lvl_pos_embed = pos_embed + level_embed[lvl].view(1, 1, -1)
        lvl_pos_embed_flatten.append(lvl_pos_embed)
        src_flatten.append(src)
        mask_flatten.append(mask)
    src_flatten = torch.cat(src_flatten, 1)
    mask_flatten = torch.cat(mask_flatten, 1)
    lvl_pos_embed_flatten = torch.cat(lvl_pos_embed_flatten, 1)
    spatial_shapes = torch.as_tensor(spatial_shapes, dtype=torch.long, device=src_flatten.device)
    level_start_index = torch.cat((spatial_shapes.new_zeros((1, )), spatial_shapes.prod(1).cumsum(0)[:-1]))
    valid_ratios = torch.stack([get_valid_ratio(m) for m in masks], 1)
    return src_flatten, mask_flatten, lvl_pos_embed_flatten, spatial_shapes, level_start_index, valid_ratios


def _compose(features, image_mask, input_proj, level_embed, position_embedding):
    """ddetrs_dn.py:117-143 on plain tensors: a backbone level's mask is the image mask resized to it (backbone.py), a further
    level's mask is resized from masks[0]."""
    srcs, masks, poses = [], [], []
    for l, feat in enumerate(features):
        mask = interpolate_mask(image_mask, feat.shape[-2:])
        srcs.append(input_proj[l](feat))
        masks.append(mask)
        poses.append(position_embedding(NestedTensor(feat, mask)).to(feat.dtype))
    for l in range(len(features), len(input_proj)):
        src = input_proj[l](features[-1] if l == len(features) else srcs[-1])
        mask = interpolate_mask(masks[0], src.shape[-2:])
        srcs.append(src)
        masks.append(mask)
        poses.append(position_embedding(NestedTensor(src, mask)).to(src.dtype))
    flat = flatten_encoder_inputs(srcs, masks, poses, level_embed)
    return EncoderInputs(*flat, get_reference_points(flat[3], flat[5], flat[0].device))


def _fused_ok(features, image_mask, input_proj, level_embed, position_embedding):
    if not (isinstance(position_embedding, PositionEmbeddingSine) and position_embedding.normalize
            and position_embedding.num_pos_feats == 128 and 0 < len(features) <= len(input_proj) <= 8):
        return False
    if torch.is_grad_enabled() and any(t.requires_grad for t in list(features) + [level_embed] + list(input_proj.parameters())):
        return False
    for proj in input_proj:
        if not (isinstance(proj, nn.Sequential) and len(proj) == 2 and isinstance(proj[0], nn.Conv2d)
                and isinstance(proj[1], nn.GroupNorm) and proj[1].num_groups == 32 and proj[1].num_channels == 256
                and proj[1].affine and proj[1].weight.dtype == torch.float32):
            return False
    dev = image_mask.device
    return (image_mask.is_cuda and image_mask.dtype == torch.bool and image_mask.dim() == 3 and image_mask.numel() > 0
            and all(f.is_cuda and f.device == dev and f.dtype == torch.float32 and f.dim() == 4 and f.numel() > 0 for f in features)
            and level_embed.is_cuda and level_embed.device == dev and level_embed.dtype == torch.float32
            and level_embed.dim() == 2 and level_embed.shape[0] >= len(input_proj) and level_embed.shape[1] == 256
            and level_embed.is_contiguous())


_SHAPE_TENSORS = {}


def _shape_tensors(shapes, device):
    """spatial_shapes and level_start_index on the device, made once per geometry (a list -> device tensor copy synchronises);
    every call gets copies of its own, made on the device."""
    key = (shapes, torch.device(device))
    if key not in _SHAPE_TENSORS:
        if len(_SHAPE_TENSORS) >= 64:
            _SHAPE_TENSORS.clear()
        starts, total = [], 0
        for h, w in shapes:
            starts.append(total)
            total += h * w
        _SHAPE_TENSORS[key] = (torch.tensor(shapes, dtype=torch.long, device=device), torch.tensor(starts, dtype=torch.long, device=device))
    return tuple(t.clone() for t in _SHAPE_TENSORS[key])


def _fused(features, image_mask, input_proj, level_embed, position_embedding):
    n = len(features)
    convs, sources = [], []
    for l, proj in enumerate(input_proj):
        if l < n:
            x = features[l]
        elif l == n:
            x = features[-1]
        else:       # the one NCHW GroupNorm output a further level's convolution reads
            norm = input_proj[l - 1][1]
            x = F.group_norm(convs[-1], norm.num_groups, norm.weight, norm.bias, norm.eps)
        convs.append(proj[0](x).contiguous())
        sources.append(-1 if l < n else 0)
    dev = convs[0].device
    src, mask, pos, valid_ratios, reference_points = MSDA.encoder_input_prepare(
        convs, image_mask, sources, [p[1].weight.detach() for p in input_proj], [p[1].bias.detach() for p in input_proj],
        [p[1].eps for p in input_proj], level_embed.detach(), position_embedding.dim_t(dev), position_embedding.scale)
    spatial_shapes, level_start_index = _shape_tensors(tuple((c.shape[2], c.shape[3]) for c in convs), dev)
    return EncoderInputs(src, mask, pos, spatial_shapes, level_start_index, valid_ratios, reference_points)


def prepare_encoder_inputs(features, image_mask, input_proj, level_embed, position_embedding, fused=None):
    """features: the backbone's outputs [B, C_l, H_l, W_l], finest first; image_mask [B, Hi, Wi] bool (True: padding);
    input_proj: build_input_proj's ModuleList, with len(input_proj) - len(features) further levels; level_embed
    [levels, 256]; position_embedding: a PositionEmbeddingSine.  Returns EncoderInputs.  fused = None: ENCODER_INPUT_FUSED;
    the fused route runs when it can (see the module's docstring), the composition otherwise."""
    if fused is None:
        fused = ENCODER_INPUT_FUSED
    features = list(features)
    if fused and _fused_ok(features, image_mask, input_proj, level_embed, position_embedding):
        with torch.no_grad():
            return _fused(features, image_mask, input_proj, level_embed, position_embedding)
    return _compose(features, image_mask, input_proj, level_embed, position_embedding)
