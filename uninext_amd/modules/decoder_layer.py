"""The decoder side of the deformable transformer: `DeformableTransformerDecoderLayer`, the `DeformableTransformerDecoder`
loop around it with iterative box refinement, `DeformableReidHead`, and the helpers they use (`MLP`, `get_sine_pos_embed`,
`inverse_sigmoid`).

Host-side mirror of projects/UNINEXT/uninext/models/deformable_detr/deformable_transformer_dino.py:373-527, :575-646 and
util/misc.py:493-497: same constructor arguments, attribute names and state-dict keys (`cross_attn.*`, `norm1/2/3.*`,
`self_attn.in_proj_weight`, `self_attn.in_proj_bias`, `self_attn.out_proj.*`, `linear1/2.*`, `ref_point_head.layers.N.*`,
`bbox_embed`, `class_embed`; `self_attn` stays an nn.MultiheadAttention, so reference checkpoints load unchanged) and the same
forward.  When autograd records, dropout is active or an input is not a contiguous fp32 GPU tensor, the layer is the
reference's composition of PyTorch ops around `MSDeformAttn` (the `_inference` test of the encoder layer), so gradients are
PyTorch's.  With `own_training` (opt-in; `set_own_training` of the decoder and the re-id head), autograd recording, dropout
inactive and contiguous fp32 GPU inputs, the self-attention of that composition is instead two token-major Linears, the HIP
core under autograd (`DecoderSelfAttentionFunction`: include/biattn_hip.h, biattn_hip_self_train_f32 and
biattn_hip_self_backward_f32, which recompute the probabilities from the row log-sum-exp, so that no [B * heads, Lq, Lq]
tensor is written or kept, the denoising mask is applied inside and wholly excluded key tiles are skipped) and `out_proj`;
`norm2`, `cross_attn`, `norm1` and the FFN stay the composition.  At inference on the GPU:

  * self-attention among the queries: one Linear of `tgt + query_pos` with the first 2 E rows of `in_proj_weight` gives q and
    k, one of `tgt` with the last E rows gives v, both token-major -- no [L, B, E] transposes; with `fused_self_attn` the
    core runs in ONE kernel (include/biattn_hip.h: biattn_hip_self_forward_f32, q and k read in place, the [Lq, Lq] denoising
    mask applied inside, no [B * heads, Lq, Lq] matrix written and none averaged over the heads to be thrown away); then
    `out_proj`, and `norm2(tgt + .)` as one add + LayerNorm kernel (include/layernorm_hip.h);
  * cross-attention: `MSDeformAttn` with `query_pos` folded into its projections and `norm1(tgt + .)` behind `output_proj`;
  * FFN: as in the encoder layer (one kernel with the split-bf16 opt-in, else two Linears and `norm3` behind `linear2`).
"""
import copy
import math

import torch
import torch.nn.functional as F
import torch.utils.checkpoint as checkpoint
from torch import nn

from .. import ext as MSDA
from .._cache import CachedModuleMixin
from .encoder_layer import _get_activation_fn
from .ms_deform_attn import MSDeformAttn


def inverse_sigmoid(x, eps=1e-5):
    x = x.clamp(min=0, max=1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


def get_sine_pos_embed(pos_tensor, num_pos_feats=128, temperature=10000, exchange_xy=True):
    """Sine embedding of every coordinate of pos_tensor [B, L, n] -> [B, L, n * num_pos_feats]: coordinate * 2 pi over
    temperature ** (2 (c // 2) / num_pos_feats), sin on the even channels c and cos on the odd ones; the first two coordinates'
    blocks swap places (y before x) with exchange_xy.  The frequencies are fp32 whatever the input's type, as in the
    reference."""
    c = torch.arange(num_pos_feats, dtype=torch.float32, device=pos_tensor.device)
    dim_t = temperature ** (2 * torch.div(c, 2, rounding_mode="floor") / num_pos_feats)
    blocks = []
    for x in pos_tensor.split(1, dim=-1):
        ang = x * (2 * math.pi) / dim_t
        blocks.append(torch.stack((ang[..., 0::2].sin(), ang[..., 1::2].cos()), dim=-1).flatten(-2))
    if exchange_xy:
        blocks[0], blocks[1] = blocks[1], blocks[0]
    return torch.cat(blocks, dim=-1)


class MLP(nn.Module):
    """Linear -> ReLU -> ... -> Linear (`layers`: num_layers Linears, no activation after the last)."""

    def __init__(self, input_dim, hidden_dim, output_dim, num_layers):
        super().__init__()
        self.num_layers = num_layers
        dims = [input_dim] + [hidden_dim] * (num_layers - 1) + [output_dim]
        self.layers = nn.ModuleList(nn.Linear(i, o) for i, o in zip(dims[:-1], dims[1:]))

    def forward(self, x):
        for n, layer in enumerate(self.layers):
            x = layer(x)
            if n < self.num_layers - 1:
                x = F.relu(x)
        return x


def _get_clones(module, N):
    return nn.ModuleList([copy.deepcopy(module) for _ in range(N)])


class DecoderSelfAttentionFunction(torch.autograd.Function):
    """`apply(qk, v, heads, mask)` -> the self-attention core [B, L, E] of qk [B, L, 2 E] (q | k, q not scaled) and v [B, L, E]
    under the [L, L] bool / fp32 mask (or None): ext.decoder_self_attention_train forward, ext.decoder_self_attention_backward
    backward (exact fp32, fixed order, bitwise repeatable).  Saved for backward: qk, v, the output, the row log-sum-exp and
    the mask; the probabilities are recomputed.  The mask gets no gradient."""

    @staticmethod
    def forward(ctx, qk, v, heads, mask):
        qk, v = qk.detach().contiguous(), v.detach().contiguous()
        E = v.shape[-1]
        out, lse = MSDA.decoder_self_attention_train(qk[..., :E], qk[..., E:], v, heads, mask)
        ctx.heads = int(heads)
        ctx.save_for_backward(qk, v, out, lse, mask)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        qk, v, out, lse, mask = ctx.saved_tensors
        E = v.shape[-1]
        grads = MSDA.decoder_self_attention_backward(qk[..., :E], qk[..., E:], v, out, lse, grad_out, ctx.heads, mask)
        if len(grads) == 3:       # a single row in all: the halves have no row stride to be told by
            grads = (torch.cat(grads[:2], dim=-1), grads[2])
        return grads[0], grads[1], None, None


class DeformableTransformerDecoderLayer(CachedModuleMixin, nn.Module):
    fuse_ffn = True          # inference: the FFN block as one kernel where include/linear_hip.h covers it (split-bf16 opt-in)
    # True: when autograd records and dropout is inactive (contiguous fp32 GPU inputs, a mask and head size the kernels take),
    # the self-attention core is DecoderSelfAttentionFunction -- the fused forward with the row log-sum-exp and its recomputing
    # backward -- between token-major projections; the rest of the layer stays the training composition.  False (default): the
    # reference's composition whenever autograd records.  Opt-in until measured faster than it with and without the denoising
    # mask (tools/decoder_layer_bench.py --train, profiles/r32_decoder_train.txt); set_own_training of the decoder and the
    # re-id head sets it per instance.
    own_training = False
    # inference: the self-attention core in one HIP kernel (biattn_hip_self_forward_f32) instead of baddbmm + softmax + bmm.
    # Opt-in until the self-attention block is measured faster than the composition on an MI355X, with and without the
    # denoising mask (tools/decoder_layer_bench.py; README "Decoder layers").
    fused_self_attn = False

    def __init__(self, d_model=256, d_ffn=1024, dropout=0.1, activation="relu", n_levels=4, n_heads=8, n_points=4):
        super().__init__()
        self.cross_attn = MSDeformAttn(d_model, n_levels, n_heads, n_points)
        self.dropout1 = nn.Dropout(dropout)
        self.norm1 = nn.LayerNorm(d_model)

        self.self_attn = nn.MultiheadAttention(d_model, n_heads, dropout=dropout)
        self.dropout2 = nn.Dropout(dropout)
        self.norm2 = nn.LayerNorm(d_model)

        self.linear1 = nn.Linear(d_model, d_ffn)
        self.activation = _get_activation_fn(activation)
        self._relu = activation == "relu"
        self.dropout3 = nn.Dropout(dropout)
        self.linear2 = nn.Linear(d_ffn, d_model)
        self.dropout4 = nn.Dropout(dropout)
        self.norm3 = nn.LayerNorm(d_model)

    @staticmethod
    def with_pos_embed(tensor, pos):
        return tensor if pos is None else tensor + pos

    _recorded_segment = False      # set for the call of _checkpointed: see there

    def _checkpointed(self, *args):
        """forward as the function of a checkpointed segment with own_training on: the segment's first pass runs without
        autograd, and would otherwise take the inference route, whose kernels round differently from the training route that the
        recomputation takes -- the next layer would be recomputed from other bits than its gradients are taken at.  Here both
        passes take the training route."""
        self._recorded_segment = True
        try:
            return self(*args)
        finally:
            self._recorded_segment = False

    def _inference(self, *tensors):
        if self._recorded_segment:
            return False
        if self.training and (self.self_attn.dropout > 0
                              or any(d.p > 0 for d in (self.dropout1, self.dropout2, self.dropout3, self.dropout4))):
            return False
        if torch.is_grad_enabled() and (any(t is not None and t.requires_grad for t in tensors)
                                        or any(p.requires_grad for p in self.parameters())):
            return False
        return all(t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()) for t in tensors)

    def _add_norm(self, x, residual, norm):
        if MSDA.add_layernorm_supported(x, norm.normalized_shape) and norm.elementwise_affine:
            return MSDA.add_layernorm(x.contiguous(), residual, norm.weight, norm.bias, norm.eps)
        return norm(x + residual)

    def forward_ffn(self, tgt):
        tgt2 = self.linear2(self.dropout3(self.activation(self.linear1(tgt))))
        return self.norm3(tgt + self.dropout4(tgt2))

    def _self_attn_composition(self, tgt, query_pos, attn_masks):
        """tgt2 of the reference: nn.MultiheadAttention on [L, B, E] views, the head-averaged weights dropped."""
        qk = self.with_pos_embed(tgt, query_pos).transpose(0, 1)
        return self.self_attn(qk, qk, tgt.transpose(0, 1), attn_mask=attn_masks)[0].transpose(0, 1)

    def _own_training_route(self, *tensors):
        """own_training may take this call: the flag, autograd records, dropout is inactive, contiguous fp32 GPU inputs."""
        if not self.own_training:
            return False
        if self.training and (self.self_attn.dropout > 0
                              or any(d.p > 0 for d in (self.dropout1, self.dropout2, self.dropout3, self.dropout4))):
            return False
        if not self._recorded_segment and not (torch.is_grad_enabled() and (any(t is not None and t.requires_grad for t in tensors)
                                                                            or any(p.requires_grad for p in self.parameters()))):
            return False
        return all(t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()) for t in tensors)

    def _self_attn_fused(self, tgt, query_pos, attn_masks, train=False):
        """The same tgt2 [B, L, E] from token-major projections and the HIP core, or None where the kernel does not apply (a 3-D
        or non-fp32 float mask, another head size, an nn.MultiheadAttention with separate or bias-free projections).  train: the
        core under autograd, as DecoderSelfAttentionFunction (a mask that requires grad is not taken: it would get none)."""
        mha = self.self_attn
        if (not mha._qkv_same_embed_dim or mha.in_proj_bias is None or mha.bias_k is not None or mha.bias_v is not None
                or mha.add_zero_attn or mha.head_dim != MSDA._lib.DEC_ATTN_HEAD_DIM):
            return None
        if attn_masks is not None and not (attn_masks.dim() == 2 and attn_masks.dtype in (torch.bool, torch.float32)):
            return None
        if train and attn_masks is not None and attn_masks.requires_grad:
            return None
        E = mha.embed_dim
        w, b = mha.in_proj_weight, mha.in_proj_bias
        qk = F.linear(self.with_pos_embed(tgt, query_pos), w[:2 * E], b[:2 * E])       # [B, L, 2 E]: q | k
        v = F.linear(tgt, w[2 * E:], b[2 * E:])
        q, k = qk[..., :E], qk[..., E:]
        mask = attn_masks.contiguous() if attn_masks is not None else None
        if not MSDA.decoder_self_attention_supported(q, k, v, mha.num_heads, mask):
            return None
        if train:
            core = DecoderSelfAttentionFunction.apply(qk, v, mha.num_heads, mask)
        else:
            core = MSDA.decoder_self_attention(q, k, v, mha.num_heads, mask)
        return F.linear(core, mha.out_proj.weight, mha.out_proj.bias)

    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(self, tgt, query_pos, reference_points, src, src_spatial_shapes, level_start_index, src_padding_mask=None,
                attn_masks=None):
        if not self._inference(tgt, query_pos, reference_points, src):
            own = self._own_training_route(tgt, query_pos, reference_points, src)
            tgt2 = self._self_attn_fused(tgt, query_pos, attn_masks, train=True) if own else None
            if tgt2 is None:
                tgt2 = self._self_attn_composition(tgt, query_pos, attn_masks)
            tgt = self.norm2(tgt + self.dropout2(tgt2))
            tgt2 = self.cross_attn(self.with_pos_embed(tgt, query_pos), reference_points, src, src_spatial_shapes,
                                   level_start_index, src_padding_mask)
            tgt = self.norm1(tgt + self.dropout1(tgt2))
            return self.forward_ffn(tgt)
        tgt2 = self._self_attn_fused(tgt, query_pos, attn_masks) if self.fused_self_attn else None
        if tgt2 is None:
            tgt2 = self._self_attn_composition(tgt, query_pos, attn_masks)
        tgt = self._add_norm(tgt2, tgt, self.norm2)
        attn = self.cross_attn
        tgt = attn(tgt, reference_points, src, src_spatial_shapes, level_start_index, src_padding_mask, query_pos=query_pos,
                   residual_norm=(tgt, self.norm1))                       # norm1(tgt + attention) in output_proj's epilogue
        if self._relu and self.fuse_ffn:
            out = attn._ffn_norm(self.linear1, self.linear2, tgt, self.norm3)   # the whole FFN block in one kernel
            if out is not None:
                return out
        hidden = attn._project(self.linear1, tgt, relu=self._relu)
        if not self._relu:
            hidden = self.activation(hidden)
        return attn._project_norm(self.linear2, hidden, tgt, self.norm3)  # norm3(tgt + ffn) in linear2's epilogue


def _layer_reference_points(reference_points, src_valid_ratios):
    """[B, Lq, n_levels, 2 | 4]: the points scaled by every level's valid ratio."""
    if reference_points.shape[-1] == 4:
        return reference_points[:, :, None] * torch.cat([src_valid_ratios, src_valid_ratios], -1)[:, None]
    assert reference_points.shape[-1] == 2
    return reference_points[:, :, None] * src_valid_ratios[:, None]


class DeformableTransformerDecoder(nn.Module):
    """num_layers decoder layers; before each, the query position is `ref_point_head` of the sine embedding of the current
    reference points; after each, `bbox_embed[lid]` (set by the owner, else None) refines the points for the next one."""

    def __init__(self, embed_dim, decoder_layer, num_layers, return_intermediate=False, look_forward_twice=False,
                 use_checkpoint=False):
        super().__init__()
        self.layers = _get_clones(decoder_layer, num_layers)
        self.num_layers = num_layers
        self.return_intermediate = return_intermediate
        self.look_forward_twice = look_forward_twice
        self.use_checkpoint = use_checkpoint
        self.ref_point_head = MLP(2 * embed_dim, embed_dim, embed_dim, 2)
        self.bbox_embed = None
        self.class_embed = None

    def set_own_training(self, flag=True):
        """DeformableTransformerDecoderLayer.own_training on every layer of this decoder; returns self."""
        for layer in self.layers:
            layer.own_training = bool(flag)
        return self

    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(self, tgt, reference_points, src, src_spatial_shapes, src_level_start_index, src_valid_ratios, query_pos=None,
                src_padding_mask=None, attn_masks=None):
        output = tgt
        if reference_points.dim() == 2:
            reference_points = reference_points.unsqueeze(0).repeat(output.shape[0], 1, 1)
        intermediate, intermediate_points = [], []
        for lid, layer in enumerate(self.layers):
            points_input = _layer_reference_points(reference_points, src_valid_ratios)
            query_pos = self.ref_point_head(get_sine_pos_embed(points_input[:, :, 0, :]))
            args = (output, query_pos, points_input, src, src_spatial_shapes, src_level_start_index, src_padding_mask, attn_masks)
            if self.use_checkpoint:
                segment = layer._checkpointed if layer.own_training and torch.is_grad_enabled() else layer
                output = checkpoint.checkpoint(segment, *args, use_reentrant=True)
            else:
                output = layer(*args)

            if self.bbox_embed is not None:
                tmp = self.bbox_embed[lid](output)
                if reference_points.shape[-1] == 4:
                    new_points = (tmp + inverse_sigmoid(reference_points)).sigmoid()
                else:
                    assert reference_points.shape[-1] == 2
                    new_points = tmp
                    new_points[..., :2] = tmp[..., :2] + inverse_sigmoid(reference_points)
                    new_points = new_points.sigmoid()
                reference_points = new_points.detach()

            if self.return_intermediate:
                intermediate.append(output)
                # look_forward_twice hands out the undetached points (it takes a bbox_embed, as in the reference)
                intermediate_points.append(new_points if self.look_forward_twice else reference_points)

        if self.return_intermediate:
            return torch.stack(intermediate), torch.stack(intermediate_points)
        return output, reference_points


class DeformableReidHead(nn.Module):
    """The decoder loop cut down to what the re-identification head needs: no refinement, the last layer's output."""

    def __init__(self, embed_dim, decoder_layer, num_layers):
        super().__init__()
        self.layers = _get_clones(decoder_layer, num_layers)
        self.num_layers = num_layers
        self.ref_point_head = MLP(2 * embed_dim, embed_dim, embed_dim, 2)

    def set_own_training(self, flag=True):
        """DeformableTransformerDecoderLayer.own_training on every layer of this head; returns self."""
        for layer in self.layers:
            layer.own_training = bool(flag)
        return self

    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(self, tgt, reference_points, src, src_spatial_shapes, src_level_start_index, src_valid_ratios, query_pos=None,
                src_padding_mask=None, attn_masks=None):
        if reference_points.shape[-1] != 4:
            raise ValueError("reference_points.shape[-1] should be 4")
        output = tgt
        for layer in self.layers:
            points_input = _layer_reference_points(reference_points, src_valid_ratios)
            query_pos = self.ref_point_head(get_sine_pos_embed(points_input[:, :, 0, :]))
            output = layer(output, query_pos, points_input, src, src_spatial_shapes, src_level_start_index, src_padding_mask,
                           attn_masks)
        return output
