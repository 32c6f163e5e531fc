"""The text encoder of UNINEXT: `forward_text`, the stage that turns the tokenised prompt into the {"hidden", "masks"} dict that
VLFuse, VL_Align and agg_lang_feat consume.  In the reference it is `BertEncoder`
(projects/UNINEXT/uninext/models/deformable_detr/bert_model.py) around `transformers.BertModel` of bert-base geometry (12
layers, 768 wide, 12 heads of 64, prompts padded to MAX_QUERY_LEN = 256).  This module does not import `transformers`: it restates
BertModel (no pooler) with transformers' state-dict keys and shapes, so a `bert-base-uncased` checkpoint or the
`text_encoder.model.*` slice of a UNINEXT checkpoint loads with strict=True, and it keeps the mask semantics the reference was
written against (transformers 4.x): a [B, T] or a [B, T, T] mask of ones and zeros, `(1 - mask) * finfo.min` ADDED to the scores.

`BertModel.fused` / `BertEncoder.fused` (on by default: measured faster than the composition and than an SDPA core at 20 and at
256 valid tokens with the p10..p90 ranges apart, tools/text_encoder_bench.py, profiles/r38_text_encoder.txt): with it on, fp32 on the GPU, no
gradient required and dropout inactive, a layer is
    F.linear on the concatenated q / k / v weight -> ext.bert_self_attention (one HIP kernel, the [B * heads, T, T] matrix is never
    written, empty key tiles of a padded prompt are skipped) -> F.linear -> ext.add_layernorm -> F.linear, F.gelu, F.linear ->
    ext.add_layernorm
and the embeddings are one kernel (ext.bert_embed_layernorm).  Otherwise -- fused off, the CPU, float64, under autograd -- every
layer runs the reference-era statements: matmul, / sqrt(d), + (1 - mask) * finfo.min, softmax, dropout, matmul.

A third route is opt-in (`BertSelfAttention.own_training`, `BertModel.set_own_training`, `BertEncoder.set_own_training`): when
autograd records, on fp32 GPU tensors with a keep mask that is not a float one, the attention core of a layer is
BertSelfAttentionFunction -- ext.bert_self_attention_train and a recomputing HIP backward that write no [B * heads, T, T]
tensor -- between one F.linear on the concatenated q / k / v weights and the layer's remaining torch statements.  An ACTIVE
attention dropout (train(), attention_probs_dropout_prob > 0: the shipped 0.1) keeps the composition unless `own_dropout` is
set too (`set_own_training(True, dropout=True)`): then the kernels drop the probabilities themselves from one
ext.bi_attention_seed draw per layer and forward; their keep masks are not F.dropout's stream.  UNINEXT trains this encoder
(FREEZE_TEXT_ENCODER False, LANG_LR 1e-5, USE_CHECKPOINT False) with that dropout active.
"""
import math
from collections import namedtuple
from dataclasses import dataclass

import torch
import torch.nn.functional as F
from torch import nn

from . import ext as MSDA
from ._cache import CachedModuleMixin, concatenated_linears


@dataclass
class BertConfig:
    """bert-base-uncased.  hidden_act "gelu" (erf) and position_embedding_type "absolute" are the only ones restated."""
    vocab_size: int = 30522
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    hidden_act: str = "gelu"
    hidden_dropout_prob: float = 0.1
    attention_probs_dropout_prob: float = 0.1
    max_position_embeddings: int = 512
    type_vocab_size: int = 2
    layer_norm_eps: float = 1e-12
    pad_token_id: int = 0
    position_embedding_type: str = "absolute"

    def __post_init__(self):
        if self.hidden_act != "gelu":
            raise NotImplementedError("BertConfig: hidden_act %r (only \"gelu\")" % self.hidden_act)
        if self.position_embedding_type != "absolute":
            raise NotImplementedError("BertConfig: position_embedding_type %r (only \"absolute\")" % self.position_embedding_type)
        if self.hidden_size % self.num_attention_heads != 0:
            raise ValueError("BertConfig: hidden_size %d is not a multiple of num_attention_heads %d"
                             % (self.hidden_size, self.num_attention_heads))


BertOutputs = namedtuple("BertOutputs", ["last_hidden_state", "hidden_states"])


def _kernel_route(module, *tensors):
    """The HIP route may take this call: the flag, fp32 GPU tensors, no gradient to record, dropout inactive."""
    if not getattr(module, "fused", True) or not all(t.is_cuda and t.dtype == torch.float32 for t in tensors):
        return False
    if module.training and any(isinstance(m, nn.Dropout) and m.p > 0 for m in module.modules()):
        return False
    return not (torch.is_grad_enabled() and (any(t.requires_grad for t in tensors) or any(p.requires_grad for p in module.parameters())))


def _add_norm(x, residual, norm):
    if MSDA.add_layernorm_supported(x, norm.normalized_shape):
        return MSDA.add_layernorm(x.contiguous(), residual.contiguous(), norm.weight, norm.bias, norm.eps)
    return norm(x + residual)


def extended_attention_mask(attention_mask, dtype):
    """What transformers 4.x adds to the scores [B, heads, T, T]: (1 - mask) * finfo(dtype).min, a [B, T] mask broadcast over
    heads and queries, a [B, T, T] mask over heads."""
    if attention_mask.dim() == 3:
        ext = attention_mask[:, None, :, :]
    elif attention_mask.dim() == 2:
        ext = attention_mask[:, None, None, :]
    else:
        raise ValueError("attention_mask must be [B, T] or [B, T, T], got %s" % (tuple(attention_mask.shape),))
    return (1.0 - ext.to(dtype)) * torch.finfo(dtype).min


class BertEmbeddings(nn.Module):
    fused = True

    def __init__(self, config):
        super().__init__()
        self.word_embeddings = nn.Embedding(config.vocab_size, config.hidden_size, padding_idx=config.pad_token_id)
        self.position_embeddings = nn.Embedding(config.max_position_embeddings, config.hidden_size)
        self.token_type_embeddings = nn.Embedding(config.type_vocab_size, config.hidden_size)
        self.LayerNorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        for name in ("position_ids", "token_type_ids"):      # buffers of older transformers checkpoints: arange / zeros
            state_dict.pop(prefix + name, None)
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, input_ids, token_type_ids=None):
        B, T = input_ids.shape
        if T > self.position_embeddings.num_embeddings:
            raise ValueError("BertEmbeddings: %d tokens, %d positions" % (T, self.position_embeddings.num_embeddings))
        tables = (self.word_embeddings.weight, self.position_embeddings.weight, self.token_type_embeddings.weight)
        if _kernel_route(self, *tables) and MSDA.bert_embed_layernorm_supported(input_ids, token_type_ids, *tables, self.LayerNorm.weight,
                                                                               self.LayerNorm.bias):
            return MSDA.bert_embed_layernorm(input_ids, token_type_ids, *tables, self.LayerNorm.weight, self.LayerNorm.bias,
                                             self.LayerNorm.eps)
        if token_type_ids is None:
            token_type_ids = torch.zeros_like(input_ids)
        x = self.word_embeddings(input_ids) + self.token_type_embeddings(token_type_ids)
        x = x + self.position_embeddings(torch.arange(T, device=input_ids.device))[None]
        return self.dropout(self.LayerNorm(x))


class BertSelfAttentionFunction(torch.autograd.Function):
    """qkv [B, T, 3 E] (the q | k | v projection output) -> the context [B, T, E] of the HIP core under autograd; the mask, the
    head count, the dropout probability and the seed are not differentiable.  Saves qkv (q, k and v are its thirds, read in
    place), the output, the row log-sum-exp and the seed -- O(B * T * E), nothing of size [T, T]: the backward recomputes the
    probabilities and the keep decisions.  Its gradient is ONE [B, T, 3 E] tensor dq | dk | dv, so the projection's backward is
    one product."""

    @staticmethod
    def forward(ctx, qkv, mask, num_heads, dropout_p, seed):
        E = qkv.shape[-1] // 3
        out, lse = MSDA.bert_self_attention_train(qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:], num_heads, mask,
                                                  dropout_p=dropout_p, seed=seed)
        ctx.save_for_backward(qkv, out, lse, *(() if seed is None else (seed,)))
        ctx.mask, ctx.num_heads, ctx.dropout_p = mask, num_heads, dropout_p
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        saved = ctx.saved_tensors                                  # read once: under checkpoint a second read is an error
        qkv, out, lse = saved[:3]
        seed = saved[3] if len(saved) > 3 else None
        E = qkv.shape[-1] // 3
        grad = MSDA.bert_self_attention_backward(qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:], out, lse, grad_out, ctx.num_heads,
                                                 ctx.mask, dropout_p=ctx.dropout_p, seed=seed)
        if not torch.is_tensor(grad):                              # a single row has no row stride to tell the thirds by
            grad = torch.cat(grad, dim=-1)
        return grad, None, None, None, None


class BertSelfAttention(CachedModuleMixin, nn.Module):
    # Route of the attention core under autograd.  Off: opt-in (BertModel.set_own_training).  Forward + backward of bert-base
    # at bs 2, T 256 in train(): 10.6 against 14.5 ms at 256 valid tokens and 12.0 against 16.7 ms at 20, ranges apart; 87 MiB
    # less peak memory with the attention dropout active, 5 MiB more without (tools/text_encoder_bench.py --train,
    # profiles/r39_text_encoder_train.txt).
    own_training = False
    # With own_training: serve ACTIVE attention dropout (train mode, attention_probs_dropout_prob > 0 -- the shipped 0.1) on that
    # route too, the kernels dropping the probabilities themselves.  Off: opt-in (set_own_training(True, dropout=True)) whatever
    # the numbers, because the keep masks are not F.dropout's stream, so a default flip would change existing training runs.
    own_dropout = False

    def __init__(self, config):
        super().__init__()
        self.num_attention_heads = config.num_attention_heads
        self.attention_head_size = config.hidden_size // config.num_attention_heads
        self.query = nn.Linear(config.hidden_size, config.hidden_size)
        self.key = nn.Linear(config.hidden_size, config.hidden_size)
        self.value = nn.Linear(config.hidden_size, config.hidden_size)
        self.dropout = nn.Dropout(config.attention_probs_dropout_prob)

    def core(self, q, k, v, additive_mask):
        """[B, heads, T, d] each -> context [B, heads, T, d]: the reference-era statements."""
        scores = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(self.attention_head_size)
        if additive_mask is not None:
            scores = scores + additive_mask
        return torch.matmul(self.dropout(torch.softmax(scores, dim=-1)), v)

    def forward(self, hidden_states, additive_mask=None):
        B, T, E = hidden_states.shape
        heads = lambda t: t.view(B, T, self.num_attention_heads, self.attention_head_size).permute(0, 2, 1, 3)
        ctx = self.core(heads(self.query(hidden_states)), heads(self.key(hidden_states)), heads(self.value(hidden_states)), additive_mask)
        return ctx.permute(0, 2, 1, 3).reshape(B, T, E)

    def forward_fused(self, hidden_states, keep_mask):
        """The same context from one product on the concatenated weights and the HIP core, or None where the kernel does not
        apply (another head size, T > 512)."""
        E = hidden_states.shape[-1]
        w, b = concatenated_linears(self, (self.query, self.key, self.value))
        qkv = F.linear(hidden_states, w, b)
        q, k, v = qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]
        if not MSDA.bert_self_attention_supported(q, k, v, self.num_attention_heads, keep_mask):
            return None
        return MSDA.bert_self_attention(q, k, v, self.num_attention_heads, keep_mask)

    def _own_training_route(self, hidden_states, keep_mask):
        """BertSelfAttentionFunction may take this call: own_training, an fp32 GPU input and fp32 parameters, autograd records,
        a keep mask that is absent or not a float one, and the attention dropout inactive or own_dropout set with 0 < p < 1."""
        if not self.own_training or not (hidden_states.is_cuda and hidden_states.dtype == torch.float32):
            return False
        params = list(self.parameters())
        if any(p.dtype != torch.float32 or p.device != hidden_states.device for p in params):
            return False
        if not (torch.is_grad_enabled() and (hidden_states.requires_grad or any(p.requires_grad for p in params))):
            return False
        if keep_mask is not None and keep_mask.is_floating_point():
            return False
        p = self.dropout.p
        return not (self.training and p > 0) or (self.own_dropout and 0 < p < 1)

    def forward_own_training(self, hidden_states, keep_mask):
        """The context under autograd from the HIP training kernels, or None where they do not apply (another head size,
        T > 512, a mask ext._bert_mask does not know).  The projection is one product on a concatenation of the three weights
        that autograd sees, so its backward is one product too and the gradients reach query, key and value separately."""
        proj = (self.query, self.key, self.value)
        qkv = F.linear(hidden_states, torch.cat([m.weight for m in proj]), torch.cat([m.bias for m in proj]))
        E = hidden_states.shape[-1]
        p = self.dropout.p if self.training else 0.0
        if not MSDA.bert_self_attention_train_supported(qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:], self.num_attention_heads,
                                                        keep_mask, p):
            return None
        seed = MSDA.bi_attention_seed(qkv.device) if p > 0 else None    # one draw per layer and forward
        return BertSelfAttentionFunction.apply(qkv, keep_mask, self.num_attention_heads, p, seed)


class BertSelfOutput(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.hidden_size, config.hidden_size)
        self.LayerNorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)

    def forward(self, hidden_states, input_tensor):
        return self.LayerNorm(self.dropout(self.dense(hidden_states)) + input_tensor)


class BertAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.self = BertSelfAttention(config)
        self.output = BertSelfOutput(config)

    def forward(self, hidden_states, additive_mask=None):
        return self.output(self.self(hidden_states, additive_mask), hidden_states)


class BertIntermediate(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.hidden_size, config.intermediate_size)

    def forward(self, hidden_states):
        return F.gelu(self.dense(hidden_states))


class BertOutput(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.intermediate_size, config.hidden_size)
        self.LayerNorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)

    def forward(self, hidden_states, input_tensor):
        return self.LayerNorm(self.dropout(self.dense(hidden_states)) + input_tensor)


class BertLayer(nn.Module):
    fused = True

    def __init__(self, config):
        super().__init__()
        self.attention = BertAttention(config)
        self.intermediate = BertIntermediate(config)
        self.output = BertOutput(config)

    def _forward_fused(self, x, keep_mask):
        ctx = self.attention.self.forward_fused(x, keep_mask)
        if ctx is None:
            return None
        so = self.attention.output
        x = _add_norm(F.linear(ctx, so.dense.weight, so.dense.bias), x, so.LayerNorm)
        y = F.linear(F.gelu(F.linear(x, self.intermediate.dense.weight, self.intermediate.dense.bias)), self.output.dense.weight,
                     self.output.dense.bias)
        return _add_norm(y, x, self.output.LayerNorm)

    def forward(self, hidden_states, attention_mask=None, additive_mask=None, kernel_route=None):
        """attention_mask: the keep mask as given ([B, T] or [B, T, T] of ones and zeros, or None); additive_mask: its extended
        form, if the caller has it already; kernel_route: the caller's answer of _kernel_route for this call, if it asked."""
        if self.attention.self._own_training_route(hidden_states, attention_mask):
            ctx = self.attention.self.forward_own_training(hidden_states, attention_mask)
            if ctx is not None:                                      # the rest of the layer stays torch autograd
                x = self.attention.output(ctx, hidden_states)
                return self.output(self.intermediate(x), x)
        if kernel_route is None:
            kernel_route = _kernel_route(self, hidden_states)
        if kernel_route and (attention_mask is None or not attention_mask.is_floating_point()):
            out = self._forward_fused(hidden_states, attention_mask)
            if out is not None:
                return out
        if additive_mask is None and attention_mask is not None:
            additive_mask = extended_attention_mask(attention_mask, hidden_states.dtype)
        x = self.attention(hidden_states, additive_mask)
        return self.output(self.intermediate(x), x)


class _BertLayers(nn.Module):
    """`encoder` of transformers' BertModel: the holder of `layer`, named so that the state-dict keys are transformers'."""

    def __init__(self, config):
        super().__init__()
        self.layer = nn.ModuleList(BertLayer(config) for _ in range(config.num_hidden_layers))


class BertModel(nn.Module):
    """transformers' BertModel(config, add_pooling_layer=False) at its state-dict keys.  forward returns
    BertOutputs(last_hidden_state, hidden_states): hidden_states[0] the embeddings, hidden_states[n] layer n's output."""

    def __init__(self, config=None, fused=True):
        super().__init__()
        self.config = config if config is not None else BertConfig()
        self.embeddings = BertEmbeddings(self.config)
        self.encoder = _BertLayers(self.config)
        self.fused = fused

    @property
    def fused(self):
        return self._fused

    @fused.setter
    def fused(self, on):
        self._fused = bool(on)
        self.embeddings.fused = self._fused
        for layer in self.encoder.layer:
            layer.fused = self._fused

    def set_own_training(self, flag=True, dropout=False):
        """BertSelfAttention.own_training on every layer: under autograd the attention core runs on the HIP training kernels
        (BertSelfAttentionFunction) where they apply.  dropout=True sets own_dropout as well: an active attention dropout is
        then served by the kernels' own keep decisions, which are not F.dropout's stream.  Returns self."""
        for layer in self.encoder.layer:
            layer.attention.self.own_training = bool(flag)
            layer.attention.self.own_dropout = bool(flag) and bool(dropout)
        return self

    def forward(self, input_ids, attention_mask=None, token_type_ids=None):
        x = self.embeddings(input_ids, token_type_ids)
        if attention_mask is not None and attention_mask.dim() not in (2, 3):
            raise ValueError("attention_mask must be [B, T] or [B, T, T], got %s" % (tuple(attention_mask.shape),))
        keep = attention_mask
        if keep is not None and not keep.is_floating_point():
            keep = keep.contiguous()
        route = self._fused and _kernel_route(self.encoder, x) and not (keep is not None and keep.is_floating_point())
        additive = None if route or attention_mask is None else extended_attention_mask(attention_mask, x.dtype)
        hidden = [x]
        for layer in self.encoder.layer:
            x = layer(x, keep, additive, route)
            hidden.append(x)
        return BertOutputs(x, tuple(hidden))


def parallel_det_mask(mask):
    """The [B, T, T] keep mask of the reference's PARALLEL_DET detection prompts (bert_model.py:36-43), uint8 on the mask's
    device, without its per-image loop and host reads: every row starts as the image's [T] mask, and among the first
    n = mask.sum() tokens the block is the identity -- a valid token sees itself alone, a padding token every valid one."""
    B, T = mask.shape
    n = (mask != 0).sum(1)[:, None, None]
    idx = torch.arange(T, device=mask.device)
    block = (idx[None, :, None] < n) & (idx[None, None, :] < n)
    eye = idx[:, None] == idx[None, :]
    return torch.where(block, eye[None], (mask != 0)[:, None, :].expand(B, T, T)).to(torch.uint8)


class BertEncoder(nn.Module):
    """The reference's BertEncoder around a BertModel of this module: forward(x, task=None) takes x["input_ids"] and
    x["attention_mask"] and returns {"masks": the [B, T] mask as given, "hidden": the last layer}."""

    def __init__(self, model=None, parallel_det=False, fused=None):
        super().__init__()
        self.model = model if model is not None else BertModel()
        self.language_dim = self.model.config.hidden_size
        self.parallel_det = parallel_det
        if fused is not None:
            self.model.fused = fused

    @property
    def fused(self):
        return self.model.fused

    @fused.setter
    def fused(self, on):
        self.model.fused = on

    def set_own_training(self, flag=True, dropout=False):
        """BertModel.set_own_training of the wrapped model; returns self."""
        self.model.set_own_training(flag, dropout)
        return self

    def forward(self, x, task=None):
        input_ids, mask = x["input_ids"], x["attention_mask"]
        attn = parallel_det_mask(mask) if self.parallel_det and task == "detection" else mask
        return {"masks": mask, "hidden": self.model(input_ids, attention_mask=attn).last_hidden_state}
