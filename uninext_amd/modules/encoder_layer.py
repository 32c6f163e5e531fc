"""`DeformableTransformerEncoderLayer` -- the caller of the MSDeformAttn path in the encoder.

Host-side mirror of projects/UNINEXT/uninext/models/deformable_detr/deformable_transformer_dino.py:330-370: same
constructor arguments, parameter names (`self_attn`, `norm1`, `linear1`, `linear2`, `norm2`; reference checkpoints load
unchanged) and forward.  When autograd records (training) the layer is the reference's composition of PyTorch ops
around `MSDeformAttn`.  At inference on the GPU (dropout is the identity):

  * `with_pos_embed(src, pos)` is folded into the operand load of the sampling_offsets / attention_weights projections;
  * `src + dropout(src2)` followed by `normN` runs in the epilogue of the Linear that produced src2 (output_proj,
    linear2: `linear_hip_packed_ln_f32`; a stand-alone add + LayerNorm kernel, include/layernorm_hip.h, covers other widths);
  * `linear1` + ReLU + `linear2` + residual + `norm2` run as ONE kernel (`linear_hip_packed_ffn_f32`: the hidden
    activations never leave the CU); `fuse_ffn = False` or other activations / widths take the two Linear kernels.

A third route is opt-in (`own_training`, `DeformableTransformerEncoderVL.set_own_training`): when autograd records, the
activation is ReLU and both norms are affine, `normN(src + dropoutN(src2))` runs as DropoutAddLayerNormFunction and
`dropout2(relu(.))` as ReluDropoutFunction (functions/layer_train.py); `self_attn` and the two Linears stay what the composition
runs.  Each block keeps one activation for its backward instead of the composition's mask, dropped copy, sum and statistics.
ACTIVE dropout (train(), p > 0: the shipped 0.1) keeps the composition unless `own_dropout` is set too
(`set_own_training(True, dropout=True)`): then the kernels drop by themselves, one (seed, offset) pair per site and forward from
`ext.bi_attention_seed`; the masks are not F.dropout's stream, which is why the flag is separate and off.
"""
import torch
import torch.nn.functional as F
from torch import nn

from .. import ext as MSDA
from .._cache import CachedModuleMixin
from ..functions.layer_train import DropoutAddLayerNormFunction, ReluDropoutFunction
from .ms_deform_attn import MSDeformAttn


def _get_activation_fn(activation):
    if activation == "relu":
        return F.relu
    if activation == "gelu":
        return F.gelu
    if activation == "glu":
        return F.glu
    raise RuntimeError(F"activation should be relu/gelu, not {activation}.")


class DeformableTransformerEncoderLayer(CachedModuleMixin, nn.Module):
    fuse_ffn = True   # inference: linear1 + ReLU + linear2 + residual + norm2 as one kernel (include/linear_hip.h)
    # Route of the blocks around self_attn under autograd.  Off: opt-in (DeformableTransformerEncoderVL.set_own_training).
    # Forward + backward of one layer at bs 2, 22 223 tokens per image, d_ffn 2048 in train(): 4.94 against 5.05 ms at dropout 0,
    # 4.96 against 5.40 ms and 1419 against 1625 MiB with dropout 0.1 active, ranges apart
    # (tools/encoder_layer_train_bench.py, profiles/r40_encoder_layer_train.txt).
    own_training = False
    # With own_training: serve ACTIVE dropout (train mode, dropout > 0 -- the shipped 0.1) on that route too, the kernels
    # dropping by themselves.  Off: opt-in (set_own_training(True, dropout=True)) whatever the numbers, because the keep masks
    # are not F.dropout's stream, so a default flip would change existing training runs.
    own_dropout = False

    def __init__(self, d_model=256, d_ffn=1024, dropout=0.1, activation="relu", n_levels=4, n_heads=8, n_points=4):
        super().__init__()
        self.self_attn = MSDeformAttn(d_model, n_levels, n_heads, n_points)
        self.dropout1 = nn.Dropout(dropout)
        self.norm1 = nn.LayerNorm(d_model)
        self.linear1 = nn.Linear(d_model, d_ffn)
        self.activation = _get_activation_fn(activation)
        self._relu = activation == "relu"
        self.dropout2 = nn.Dropout(dropout)
        self.linear2 = nn.Linear(d_ffn, d_model)
        self.dropout3 = nn.Dropout(dropout)
        self.norm2 = nn.LayerNorm(d_model)

    @staticmethod
    def with_pos_embed(tensor, pos):
        return tensor if pos is None else tensor + pos

    def _inference(self, *tensors):
        if self.training and any(d.p > 0 for d in (self.dropout1, self.dropout2, self.dropout3)):
            return False
        if torch.is_grad_enabled() and (any(t is not None and t.requires_grad for t in tensors)
                                        or any(p.requires_grad for p in self.parameters())):
            return False
        return all(t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()) for t in tensors)

    def _own_training_route(self, src, pos):
        """The training kernels may take this call: own_training, ReLU, autograd records, contiguous fp32 GPU inputs, both norms
        affine and of a supported width, and dropout inactive or own_dropout set with every p below 1."""
        if not (self.own_training and self._relu and torch.is_grad_enabled()):
            return False
        if not (any(t is not None and t.requires_grad for t in (src, pos)) or any(p.requires_grad for p in self.parameters())):
            return False
        if not all(t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()) for t in (src, pos)):
            return False
        for norm in (self.norm1, self.norm2):
            if not (norm.elementwise_affine and norm.bias is not None and norm.weight.dtype == torch.float32
                    and norm.weight.device == src.device and MSDA.dropout_add_layernorm_train_supported(src, norm.normalized_shape)):
                return False
        if self.linear1.out_features % 4 != 0 or self.linear1.weight.dtype != torch.float32:
            return False
        ps = [d.p for d in (self.dropout1, self.dropout2, self.dropout3)]
        return not (self.training and any(p > 0 for p in ps)) or (self.own_dropout and all(0 <= p < 1 for p in ps))

    def _site(self, dropout, dev):
        """(p, seed) of one dropout site for this forward: p = 0 and no seed while it is inactive."""
        p = float(dropout.p) if self.training else 0.0
        return p, (MSDA.bi_attention_seed(dev) if p > 0 else None)

    def forward_own_training(self, src, pos, reference_points, spatial_shapes, level_start_index, padding_mask):
        src2 = self.self_attn(self.with_pos_embed(src, pos), reference_points, src, spatial_shapes, level_start_index, padding_mask)
        n1, n2, dev = self.norm1, self.norm2, src.device
        src = DropoutAddLayerNormFunction.apply(src2.contiguous(), src, n1.weight, n1.bias, n1.eps, *self._site(self.dropout1, dev))
        hidden = ReluDropoutFunction.apply(self.linear1(src).contiguous(), *self._site(self.dropout2, dev))
        src2 = self.linear2(hidden)
        return DropoutAddLayerNormFunction.apply(src2.contiguous(), src, n2.weight, n2.bias, n2.eps, *self._site(self.dropout3, dev))

    def _add_norm(self, x, residual, norm):
        if MSDA.add_layernorm_supported(x, norm.normalized_shape) and norm.elementwise_affine:
            return MSDA.add_layernorm(x.contiguous(), residual, norm.weight, norm.bias, norm.eps)
        return norm(x + residual)

    def forward_ffn(self, src):
        src2 = self.linear2(self.dropout2(self.activation(self.linear1(src))))
        src = src + self.dropout3(src2)
        return self.norm2(src)

    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(self, src, pos, reference_points, spatial_shapes, level_start_index, padding_mask=None):
        if self._own_training_route(src, pos):
            return self.forward_own_training(src, pos, reference_points, spatial_shapes, level_start_index, padding_mask)
        if not self._inference(src, pos):
            src2 = self.self_attn(self.with_pos_embed(src, pos), reference_points, src, spatial_shapes,
                                  level_start_index, padding_mask)
            src = self.norm1(src + self.dropout1(src2))
            return self.forward_ffn(src)
        attn = self.self_attn
        src = attn(src, reference_points, src, spatial_shapes, level_start_index, padding_mask, query_pos=pos,
                   residual_norm=(src, self.norm1))                       # norm1(src + attention) in output_proj's epilogue
        if self._relu and self.fuse_ffn:
            out = attn._ffn_norm(self.linear1, self.linear2, src, self.norm2)   # the whole FFN block in one kernel
            if out is not None:
                return out
        hidden = attn._project(self.linear1, src, relu=self._relu)
        if not self._relu:
            hidden = self.activation(hidden)
        return attn._project_norm(self.linear2, hidden, src, self.norm2)  # norm2(src + ffn) in linear2's epilogue
