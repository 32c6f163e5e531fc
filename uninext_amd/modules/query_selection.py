"""Two-stage query selection: the step between the encoder's `memory` and the decoder's `reference_points`.

Host-side mirror of `gen_encoder_output_proposals` and the selection lines of `DeformableTransformerVLDINO.forward`
(projects/UNINEXT/uninext/models/deformable_detr/deformable_transformer_dino.py:132-162, :216-224), of `agg_lang_feat` (:28-43)
and of the classifier heads `VL_Align` and `Still_Classifier` (models/deformable_detr/deformable_detr.py:35-76): the same names,
constructor arguments, parameter names and state-dict keys (`dot_product_projection_text.*`, `log_scale`, `bias_lang`, `bias0`;
`body.*`), so reference checkpoints load unchanged.

Every token of the pyramid proposes a box: its pixel centre over the image's valid size, (x + 0.5) / valid_W and
(y + 0.5) / valid_H, and w = h = 0.05 * 2 ** level.  A proposal counts only if all four numbers lie strictly inside
(0.01, 0.99); the comparison is made in fp32 and the LAST BIT decides it (0.5 / 50 rounds to exactly fp32(0.01): with
valid_W = 50, columns 0 and 49 are out).  The proposals are fp32 whatever the type of `memory`, as in the reference.

`TwoStageQuerySelection` composes the selection.  With `fused` set, at inference on contiguous fp32 GPU tensors with d_model 256
and one pooled text token, it is two HIP kernels around `torch.topk` (include/dynmask_hip.h: qsel_scores_hip_f32 scores every
row; qsel_boxes_hip_f32 runs the box MLP on the `topk` rows only); otherwise it is the reference's composition of PyTorch ops,
so training gradients are PyTorch's.
"""
import math
import weakref

import torch
import torch.nn.functional as F
from torch import nn

from .. import ext as MSDA
from .._cache import tensor_version

CLAMP_DOT_PRODUCT = 50000.0


class VL_Align(nn.Module):
    """Vision-language alignment score of every query with every text token:
    x . W(e / 2) / exp(log_scale) + e . bias_lang + bias0, e the L2-normalised token, clamped to +-50000 when the config asks."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        prior = cfg.MODEL.DYHEAD.PRIOR_PROB
        lang_dim, hidden = cfg.MODEL.LANGUAGE_BACKBONE.LANG_DIM, cfg.MODEL.DDETRS.HIDDEN_DIM
        self.dot_product_projection_image = nn.Identity()
        self.dot_product_projection_text = nn.Linear(lang_dim, hidden, bias=True)
        self.log_scale = nn.Parameter(torch.Tensor([cfg.MODEL.DYHEAD.LOG_SCALE]), requires_grad=True)
        self.bias_lang = nn.Parameter(torch.zeros(lang_dim), requires_grad=True)
        self.bias0 = nn.Parameter(torch.Tensor([-math.log((1 - prior) / prior)]), requires_grad=True)   # focal-loss prior

    @property
    def clamp(self):
        return CLAMP_DOT_PRODUCT if self.cfg.MODEL.DYHEAD.FUSE_CONFIG.CLAMP_DOT_PRODUCT else 0.0

    def token_terms(self, embedding):
        """([B, L, hidden] projected tokens, [B, L] token biases) of the text side [B, L, lang_dim]."""
        e = F.normalize(embedding, p=2, dim=-1)
        return self.dot_product_projection_text(e / 2.0), torch.matmul(e, self.bias_lang) + self.bias0

    def forward(self, x, embedding):
        """x [B, Q, hidden], embedding [B, L, lang_dim] -> [B, Q, L]."""
        tokens, bias = self.token_terms(embedding)
        logit = torch.matmul(self.dot_product_projection_image(x), tokens.transpose(-1, -2)) / self.log_scale.exp()
        logit = logit + bias.unsqueeze(1)
        if self.clamp:
            logit = logit.clamp(min=-self.clamp, max=self.clamp)
        return logit


class Still_Classifier(nn.Module):
    """One Linear to a single score; the text side is ignored."""

    def __init__(self, hidden_dim):
        super().__init__()
        self.body = nn.Linear(hidden_dim, 1)

    def forward(self, x, lang_feat=None):
        return self.body(x)


def agg_lang_feat(features, mask, pool_type="average"):
    """[B, L, C] token features, [B, L] bool mask (True = a real token) -> [B, C]: the masked mean or maximum over the tokens."""
    if pool_type == "average":
        kept = features * mask.unsqueeze(-1).float()
        return kept.sum(1) / mask.sum(-1).unsqueeze(-1).float()
    if pool_type == "max":
        return torch.stack([f[m].max(0)[0] for f, m in zip(features, mask)], dim=0)
    raise ValueError("pool_type should be average or max")


_shapes_seen = {}


def _levels(spatial_shapes):
    """[(H, W), ...] as Python ints.  A tensor is copied to the host once per tensor object and version (weak reference)."""
    if not isinstance(spatial_shapes, torch.Tensor):
        return [(int(h), int(w)) for h, w in spatial_shapes]
    e = _shapes_seen.get(id(spatial_shapes))
    if e is not None and e[0]() is spatial_shapes and e[1] == tensor_version(spatial_shapes):
        return e[2]
    levels = [(int(h), int(w)) for h, w in spatial_shapes.tolist()]
    if len(_shapes_seen) > 64:
        _shapes_seen.clear()
    _shapes_seen[id(spatial_shapes)] = (weakref.ref(spatial_shapes), tensor_version(spatial_shapes), levels)
    return levels


def encoder_output_proposals(memory_padding_mask, spatial_shapes):
    """(proposals [B, S, 4] fp32 as (cx, cy, w, h), valid [B, S, 1] bool) of every token, before the logit."""
    B = memory_padding_mask.shape[0]
    dev = memory_padding_mask.device
    per_level, start = [], 0
    for lvl, (H, W) in enumerate(_levels(spatial_shapes)):
        m = memory_padding_mask[:, start:start + H * W].view(B, H, W)
        valid_h = torch.sum(~m[:, :, 0], 1)
        valid_w = torch.sum(~m[:, 0, :], 1)
        ys = torch.arange(H, dtype=torch.float32, device=dev).view(1, H, 1).expand(B, H, W)
        xs = torch.arange(W, dtype=torch.float32, device=dev).view(1, 1, W).expand(B, H, W)
        centre = (torch.stack((xs, ys), -1) + 0.5) / torch.stack((valid_w, valid_h), -1).view(B, 1, 1, 2)
        size = torch.ones_like(centre) * 0.05 * (2.0 ** lvl)
        per_level.append(torch.cat((centre, size), -1).view(B, H * W, 4))
        start += H * W
    proposals = torch.cat(per_level, 1)
    valid = ((proposals > 0.01) & (proposals < 0.99)).all(-1, keepdim=True)
    return proposals, valid


def gen_encoder_output_proposals(memory, memory_padding_mask, spatial_shapes, enc_output, enc_output_norm):
    """(output_memory [B, S, C], output_proposals [B, S, 4]): `enc_output_norm(enc_output(.))` of the memory with its padded
    and invalid rows zeroed, and the logit of every token's proposal, +inf on those rows."""
    proposals, valid = encoder_output_proposals(memory_padding_mask, spatial_shapes)
    dead = memory_padding_mask.unsqueeze(-1) | ~valid
    output_proposals = torch.log(proposals / (1 - proposals)).masked_fill(dead, float("inf"))
    output_memory = enc_output_norm(enc_output(memory.masked_fill(dead, 0.0)))
    return output_memory, output_proposals


_valid_index = {}


def valid_sizes(memory_padding_mask, spatial_shapes):
    """valid_wh [B, n_levels, 2] fp32 = (valid_W, valid_H) of every image and level, counted along the first row and the first
    column of the level as the reference counts them; a handful of device ops, nothing copied to the host."""
    levels = tuple(_levels(spatial_shapes))
    dev = memory_padding_mask.device
    key = (levels, str(dev))
    if key not in _valid_index:
        rows, cols, row_lvl, col_lvl, start = [], [], [], [], 0
        for lvl, (H, W) in enumerate(levels):
            rows.append(start + torch.arange(W))                 # the first row: W tokens
            cols.append(start + torch.arange(H) * W)             # the first column: H tokens
            row_lvl.append(torch.full((W,), lvl))
            col_lvl.append(torch.full((H,), lvl))
            start += H * W
        onehot = lambda l: F.one_hot(torch.cat(l), len(levels)).float().to(dev)
        if len(_valid_index) > 16:
            _valid_index.clear()
        _valid_index[key] = (torch.cat(rows).to(dev), onehot(row_lvl), torch.cat(cols).to(dev), onehot(col_lvl))
    row_idx, row_hot, col_idx, col_hot = _valid_index[key]
    live = (~memory_padding_mask).float()
    # sums of at most max(H, W) ones: exact in fp32
    return torch.stack((live.index_select(1, row_idx) @ row_hot, live.index_select(1, col_idx) @ col_hot), -1).contiguous()


class TwoStageQuerySelection:
    """reference_points, topk_coords_unact, topk_proposals, enc_outputs_class, enc_outputs_coord_unact = select(...)

    memory [B, S, C], mask_flatten [B, S] bool (True = padded), spatial_shapes [n_levels, 2] (tensor or list of (H, W)),
    enc_output nn.Linear, enc_output_norm nn.LayerNorm, class_embed a VL_Align or Still_Classifier, bbox_embed the 3-layer box
    MLP (uninext_amd.modules.MLP), lang_feat_pool [B, lang_dim] the pooled text feature (None for a Still_Classifier), topk the
    number of proposals.  enc_outputs_class is [B, S, 1]; enc_outputs_coord_unact [B, S, 4] is None unless all_coords (only
    the training criterion reads it)."""

    # The HIP route (qsel_scores_hip_f32 + torch.topk + qsel_boxes_hip_f32).  Opt-in until tools/query_selection_bench.py shows
    # it faster than the composition in every row on an MI355X (README "Two-stage query selection").
    fused = False

    def __call__(self, memory, mask_flatten, spatial_shapes, enc_output, enc_output_norm, class_embed, bbox_embed,
                 lang_feat_pool, topk, all_coords=False):
        if self.fused and self._inference(memory, mask_flatten, enc_output, enc_output_norm, class_embed, bbox_embed,
                                          lang_feat_pool):
            return self._select_fused(memory, mask_flatten, spatial_shapes, enc_output, enc_output_norm, class_embed,
                                      bbox_embed, lang_feat_pool, topk, all_coords)
        return self._select_composition(memory, mask_flatten, spatial_shapes, enc_output, enc_output_norm, class_embed,
                                        bbox_embed, lang_feat_pool, topk, all_coords)

    select = __call__

    @staticmethod
    def _inference(memory, mask, enc_output, enc_output_norm, class_embed, bbox_embed, lang_feat_pool):
        modules = (enc_output, enc_output_norm, class_embed, bbox_embed)
        tensors = (memory, mask) + (() if lang_feat_pool is None else (lang_feat_pool,))
        if torch.is_grad_enabled() and (any(t.requires_grad for t in tensors)
                                        or any(p.requires_grad for m in modules for p in m.parameters())):
            return False
        if not all(t.is_cuda and t.is_contiguous() and t.device == memory.device for t in tensors):
            return False
        if memory.dtype != torch.float32 or mask.dtype != torch.bool or memory.dim() != 3 or mask.shape != memory.shape[:2]:
            return False
        d = MSDA._lib.QSEL_D_MODEL
        if memory.shape[-1] != d or any(p.dtype != torch.float32 or p.device != memory.device
                                        for m in modules for p in m.parameters()):
            return False
        if not (isinstance(enc_output, nn.Linear) and tuple(enc_output.weight.shape) == (d, d) and enc_output.bias is not None
                and isinstance(enc_output_norm, nn.LayerNorm) and tuple(enc_output_norm.normalized_shape) == (d,)
                and enc_output_norm.elementwise_affine and enc_output_norm.bias is not None):
            return False
        layers = getattr(bbox_embed, "layers", None)
        if layers is None or [tuple(l.weight.shape) for l in layers] != [(d, d), (d, d), (4, d)] \
                or any(l.bias is None for l in layers):
            return False
        if isinstance(class_embed, VL_Align):     # a text side of one pooled token
            return (lang_feat_pool is not None and lang_feat_pool.dtype == torch.float32 and lang_feat_pool.dim() == 2
                    and lang_feat_pool.shape[0] == memory.shape[0]
                    and tuple(class_embed.dot_product_projection_text.weight.shape) == (d, lang_feat_pool.shape[1]))
        return isinstance(class_embed, Still_Classifier) and tuple(class_embed.body.weight.shape) == (1, d)

    @staticmethod
    def _select_composition(memory, mask, spatial_shapes, enc_output, enc_output_norm, class_embed, bbox_embed, lang_feat_pool,
                            topk, all_coords):
        output_memory, output_proposals = gen_encoder_output_proposals(memory, mask, spatial_shapes, enc_output, enc_output_norm)
        text = None if lang_feat_pool is None else lang_feat_pool.unsqueeze(1)
        enc_outputs_class = class_embed(output_memory, text)
        enc_outputs_coord_unact = bbox_embed(output_memory) + output_proposals
        topk_proposals = torch.topk(enc_outputs_class[..., 0], topk, dim=1)[1]
        topk_coords_unact = torch.gather(enc_outputs_coord_unact, 1, topk_proposals.unsqueeze(-1).repeat(1, 1, 4))
        return (topk_coords_unact.sigmoid(), topk_coords_unact, topk_proposals, enc_outputs_class,
                enc_outputs_coord_unact if all_coords else None)

    @staticmethod
    def class_terms(class_embed, lang_feat_pool):
        """(class_vec [B | 1, d], class_bias [B | 1], scale [1] or None, clamp) of the head for one pooled token, device tensors."""
        if isinstance(class_embed, VL_Align):
            tokens, bias = class_embed.token_terms(lang_feat_pool.unsqueeze(1))           # [B, 1, d], [B, 1]
            return tokens[:, 0].contiguous(), bias[:, 0].contiguous(), class_embed.log_scale.exp(), class_embed.clamp
        return class_embed.body.weight, class_embed.body.bias, None, 0.0

    @classmethod
    def _select_fused(cls, memory, mask, spatial_shapes, enc_output, enc_output_norm, class_embed, bbox_embed, lang_feat_pool,
                      topk, all_coords):
        with torch.no_grad():
            B, S, _ = memory.shape
            levels = _levels(spatial_shapes)
            if isinstance(spatial_shapes, torch.Tensor) and spatial_shapes.device == memory.device \
                    and spatial_shapes.dtype == torch.long and spatial_shapes.is_contiguous():
                shapes = spatial_shapes
            else:
                shapes = torch.as_tensor(levels, dtype=torch.long).to(memory.device)
            if sum(h * w for h, w in levels) != S:
                raise ValueError("spatial_shapes cover %d tokens, memory has %d" % (sum(h * w for h, w in levels), S))
            geometry = (memory, mask, shapes, valid_sizes(mask, levels), enc_output.weight, enc_output.bias,
                        enc_output_norm.weight, enc_output_norm.bias, enc_output_norm.eps)
            class_vec, class_bias, scale, clamp = cls.class_terms(class_embed, lang_feat_pool)
            logits = MSDA.qsel_scores(*geometry, class_vec, class_bias, scale, clamp)
            topk_proposals = torch.topk(logits, topk, dim=1)[1]
            l1, l2, l3 = bbox_embed.layers
            mlp = (l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias)
            if all_coords:
                every = torch.arange(S, device=memory.device).unsqueeze(0).expand(B, S).contiguous()
                enc_outputs_coord_unact, _ = MSDA.qsel_boxes(*geometry, every, *mlp)
                topk_coords_unact = torch.gather(enc_outputs_coord_unact, 1, topk_proposals.unsqueeze(-1).repeat(1, 1, 4))
                return topk_coords_unact.sigmoid(), topk_coords_unact, topk_proposals, logits.unsqueeze(-1), enc_outputs_coord_unact
            topk_coords_unact, reference_points = MSDA.qsel_boxes(*geometry, topk_proposals, *mlp)
            return reference_points, topk_coords_unact, topk_proposals, logits.unsqueeze(-1), None


def select_queries(*args, fused=None, **kwargs):
    """TwoStageQuerySelection()(...) as a function; `fused` overrides the class attribute for this call."""
    sel = TwoStageQuerySelection()
    if fused is not None:
        sel.fused = bool(fused)
    return sel(*args, **kwargs)
