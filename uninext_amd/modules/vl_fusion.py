"""`VLFuse` -- the early vision-language fusion layer in front of the deformable encoder.

Host-side mirror of projects/UNINEXT/uninext/models/deformable_detr/vlfusion.py:64-120 (`VLFuse`) and fuse_helper.py:7-179
(`BiMultiHeadAttention`, `BiAttentionBlockForCheckpoint`): same constructor arguments, `cfg` fields, parameter names (`b_attn`,
`layer_norm_v`, `layer_norm_l`, `attn`, `gamma_v`, `gamma_l`, `v_proj`, `l_proj`, `values_v_proj`, `values_l_proj`,
`out_v_proj`, `out_l_proj`; reference checkpoints load with strict=True), initialisation, and the same dict in and out.

`BiMultiHeadAttention` has two routes.  When autograd records nothing, dropout is inactive, the tensors are contiguous fp32 GPU
tensors, both clamps are on and STABLE_SOFTMAX_2D is off (the shipped config), the head dimension is 256, there are at most 256
text tokens and the mask is int64, fp32 or absent, everything between the four input projections and the two output projections
runs as the fused HIP core (include/biattn_hip.h): the [B * heads, S, T] attention matrix is never written.  Otherwise
(training, CPU, a bool mask, other configs) the module runs the reference's sequence of PyTorch ops, written out below.  The
projections, LayerNorms and the `gamma` residual are PyTorch on both routes.  `fused_core` switches the fused route off.

A third route is opt-in (`BiMultiHeadAttention.own_training`, `VLFuse.set_own_training`): when autograd records, dropout is
inactive and the fused route's remaining conditions hold, the core runs as `BiAttentionFunction` -- biattn_hip_train_f32, which
keeps two numbers per softmax row, and biattn_hip_backward_f32, which recomputes both probabilities from them -- so that no
[B * heads, S, T] tensor is written in training either.  Active dropout (the shipped 0.1 in train mode) selects the composition
unless `BiMultiHeadAttention.own_dropout` is set as well (`VLFuse.set_own_training(True, dropout=True)`): then the kernels drop
both attention probabilities themselves, from a counter-based generator (biattn_hip_train_dropout_f32 /
biattn_hip_backward_dropout_f32) whose seed is drawn on the device from torch's CUDA generator; no keep mask is written and the
backward recomputes the forward's.  The masks are not those of F.dropout's stream: the same distribution, other bits.
"""
import torch
import torch.nn.functional as F
import torch.utils.checkpoint as checkpoint
from torch import nn

from .. import ext as MSDA

_CLAMP = 50000           # fuse_helper.py:78-81: "data type half has quite limited range"
_MASKED = -9e15          # fuse_helper.py:98


class BiAttentionFunction(torch.autograd.Function):
    """(q, k, vv, vl) -> (out_v, out_l) of the fused core under autograd; the mask, the head count and the scale are not
    differentiable.  Saves the four inputs, the two outputs and the row statistics -- O(B * (S + T) * E), nothing of size
    B * heads * S * T.  Two optional trailing arguments, (dropout_p, seed), switch the in-kernel dropout on: the seed
    (MSDA.bi_attention_seed's two int64 on the device) is saved too, and the backward recomputes the keep decisions from it."""

    @staticmethod
    def forward(ctx, q, k, vv, vl, mask, num_heads, q_scale, *dropout):
        dropout_p, seed = dropout if dropout else (0.0, None)
        out_v, out_l, stat_v, stat_l = MSDA.bi_attention_train(q, k, vv, vl, mask, num_heads, q_scale, dropout_p, seed)
        ctx.save_for_backward(q, k, vv, vl, out_v, out_l, stat_v, stat_l, *(() if seed is None else (seed,)))
        ctx.mask, ctx.num_heads, ctx.q_scale, ctx.dropout_p, ctx.extra = mask, num_heads, q_scale, dropout_p, len(dropout)
        ctx.mark_non_differentiable(stat_v, stat_l)
        return out_v, out_l, stat_v, stat_l

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out_v, grad_out_l, _grad_stat_v, _grad_stat_l):
        saved = ctx.saved_tensors                                  # read once: under checkpoint a second read is an error
        q, k, vv, vl, out_v, out_l, stat_v, stat_l = saved[:8]
        seed = saved[8] if len(saved) > 8 else None
        if grad_out_v is None:
            grad_out_v = torch.zeros_like(out_v)
        if grad_out_l is None:
            grad_out_l = torch.zeros_like(out_l)
        grads = MSDA.bi_attention_backward(q, k, vv, vl, ctx.mask, out_v, out_l, stat_v, stat_l, grad_out_v, grad_out_l,
                                           ctx.num_heads, ctx.q_scale, ctx.dropout_p, seed)
        # the kernels compute all four; needs_input_grad only decides what is handed back
        return tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[:4])) + (None,) * (3 + ctx.extra)


class BiMultiHeadAttention(nn.Module):
    # Route of the attention core at inference.  On: the fused core is faster than the composition at T = 256 (1.95 against
    # 4.38 ms) and at T = 16 (0.68 against 1.51 ms) by more than the spread of the alternating runs (profiles/r08_vlfuse.txt).
    fused_core = True
    # Route of the attention core under autograd.  Off: opt-in (VLFuse.set_own_training).  Forward + backward against the
    # composition: 14.51 against 15.42 ms at T = 256 but 7.97 against 7.28 ms at T = 16, so not faster at both; its reason is
    # the peak memory, 2.38 against 5.52 GB above the inputs at T = 256 (profiles/r36_vlfuse_train.txt).
    own_training = False
    # With own_training: serve ACTIVE dropout (train mode, dropout > 0 -- the shipped 0.1) on that route too, the kernels dropping
    # both probabilities themselves.  Off: opt-in (VLFuse.set_own_training(True, dropout=True)) whatever the numbers, because the
    # keep masks are not F.dropout's, so a default flip would change existing training runs bit for bit.  Forward + backward at
    # dropout 0.1 against the composition: profiles/r37_vlfuse_dropout.txt.
    own_dropout = False

    def __init__(self, v_dim, l_dim, embed_dim, num_heads, dropout=0.1, cfg=None):
        super().__init__()
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.head_dim = embed_dim // num_heads
        self.v_dim = v_dim
        self.l_dim = l_dim
        assert self.head_dim * self.num_heads == self.embed_dim, \
            f"embed_dim must be divisible by num_heads (got `embed_dim`: {self.embed_dim} and `num_heads`: {self.num_heads})."
        self.scale = self.head_dim ** (-0.5)
        self.dropout = dropout

        self.v_proj = nn.Linear(self.v_dim, self.embed_dim)
        self.l_proj = nn.Linear(self.l_dim, self.embed_dim)
        self.values_v_proj = nn.Linear(self.v_dim, self.embed_dim)
        self.values_l_proj = nn.Linear(self.l_dim, self.embed_dim)
        self.out_v_proj = nn.Linear(self.embed_dim, self.v_dim)
        self.out_l_proj = nn.Linear(self.embed_dim, self.l_dim)

        fuse = cfg.MODEL.DYHEAD.FUSE_CONFIG
        self.stable_softmax_2d = fuse.STABLE_SOFTMAX_2D
        self.clamp_min_for_underflow = fuse.CLAMP_MIN_FOR_UNDERFLOW
        self.clamp_max_for_overflow = fuse.CLAMP_MAX_FOR_OVERFLOW
        self._reset_parameters()

    def _reset_parameters(self):
        for proj in (self.v_proj, self.l_proj, self.values_v_proj, self.values_l_proj, self.out_v_proj, self.out_l_proj):
            nn.init.xavier_uniform_(proj.weight)
            proj.bias.data.fill_(0)

    def _shape(self, tensor, seq_len, bsz):
        return tensor.view(bsz, seq_len, self.num_heads, self.head_dim).transpose(1, 2).contiguous()

    def _records(self, v, l):
        return torch.is_grad_enabled() and (v.requires_grad or l.requires_grad or any(p.requires_grad for p in self.parameters()))

    def _inference(self, v, l, attention_mask_l):
        """True when the fused core serves this call."""
        if not self.fused_core:
            return False
        if self.training and self.dropout > 0:
            return False
        if self._records(v, l):
            return False
        return self._fused_conditions(v, l, attention_mask_l)

    def _own_training(self, v, l, attention_mask_l):
        """True when BiAttentionFunction serves this call: opted in, autograd records, dropout is inactive or own_dropout is
        set as well, and the fused core's remaining conditions hold."""
        if not (self.own_training and self.fused_core) or not self._records(v, l):
            return False
        if self._dropout_active() and not (self.own_dropout and 0 < self.dropout < 1):
            return False
        return self._fused_conditions(v, l, attention_mask_l)

    def _dropout_active(self):
        return self.training and self.dropout != 0

    def _fused_conditions(self, v, l, attention_mask_l):
        if not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in (v, l)):
            return False
        if any(p.dtype != torch.float32 for p in self.parameters()):
            return False
        if self.stable_softmax_2d or not (self.clamp_min_for_underflow and self.clamp_max_for_overflow):
            return False
        if self.head_dim != 256 or v.dim() != 3 or l.dim() != 3 or not (1 <= l.shape[1] <= 256) or v.shape[1] < 1:
            return False
        m = attention_mask_l
        if m is not None and not (m.dtype in (torch.int64, torch.float32) and m.is_cuda and m.is_contiguous()
                                  and tuple(m.shape) == (v.shape[0], l.shape[1])):
            return False
        return True

    def _clamp(self, x):
        if self.clamp_min_for_underflow:
            x = torch.clamp(x, min=-_CLAMP)
        if self.clamp_max_for_overflow:
            x = torch.clamp(x, max=_CLAMP)
        return x

    def _core_torch(self, q, k, vv, vl, attention_mask_l):
        """The reference's op sequence on q = v_proj(v) * scale, k, vv, vl (token-major [B, S | T, E]): returns the inputs of
        out_v_proj / out_l_proj."""
        bsz, tgt_len = q.shape[0], q.shape[1]
        heads = lambda t: self._shape(t, -1, bsz).view(bsz * self.num_heads, -1, self.head_dim)
        q, k, vv, vl = heads(q), heads(k), heads(vv), heads(vl)
        src_len = k.size(1)
        w = torch.bmm(q, k.transpose(1, 2))                        # [B * heads, S, T]
        if self.stable_softmax_2d:
            w = w - w.max()
        w = self._clamp(w)
        w_t = w.transpose(1, 2)
        w_l = self._clamp(w_t - torch.max(w_t, dim=-1, keepdim=True)[0]).softmax(dim=-1)
        if attention_mask_l is not None:
            assert attention_mask_l.dim() == 2
            m = attention_mask_l.unsqueeze(1).unsqueeze(1).expand(bsz, 1, tgt_len, src_len)
            m = m.masked_fill(m == 0, _MASKED)                     # in the MASK's dtype: a bool mask becomes all True (+1)
            w = (w.view(bsz, self.num_heads, tgt_len, src_len) + m).view(bsz * self.num_heads, tgt_len, src_len)
        w_v = F.softmax(w, dim=-1)
        p_v = F.dropout(w_v, p=self.dropout, training=self.training)
        p_l = F.dropout(w_l, p=self.dropout, training=self.training)
        out_v = torch.bmm(p_v, vl)
        out_l = torch.bmm(p_l, vv)
        merge = lambda t, n: t.view(bsz, self.num_heads, n, self.head_dim).transpose(1, 2).reshape(bsz, n, self.embed_dim)
        return merge(out_v, tgt_len), merge(out_l, src_len)

    def forward(self, v, l, attention_mask_l=None):
        q = self.v_proj(v)
        k = self.l_proj(l)
        vv = self.values_v_proj(v)
        vl = self.values_l_proj(l)
        if self._inference(v, l, attention_mask_l) and MSDA.bi_attention_supported(q, k, vv, vl, attention_mask_l, self.num_heads):
            out_v, out_l = MSDA.bi_attention_forward(q, k, vv, vl, attention_mask_l, self.num_heads, self.scale)
        elif (self._own_training(v, l, attention_mask_l)
              and MSDA.bi_attention_train_supported(q, k, vv, vl, attention_mask_l, self.num_heads)):
            if self._dropout_active():
                out_v, out_l = BiAttentionFunction.apply(q, k, vv, vl, attention_mask_l, self.num_heads, self.scale,
                                                         float(self.dropout), MSDA.bi_attention_seed(q.device))[:2]
            else:
                out_v, out_l = BiAttentionFunction.apply(q, k, vv, vl, attention_mask_l, self.num_heads, self.scale)[:2]
        else:
            out_v, out_l = self._core_torch(q * self.scale, k, vv, vl, attention_mask_l)
        return self.out_v_proj(out_v), self.out_l_proj(out_l)


class BiAttentionBlockForCheckpoint(nn.Module):
    def __init__(self, v_dim, l_dim, embed_dim, num_heads, dropout=0.1, drop_path=.0, init_values=1e-4, cfg=None):
        super().__init__()
        self.layer_norm_v = nn.LayerNorm(v_dim)
        self.layer_norm_l = nn.LayerNorm(l_dim)
        self.attn = BiMultiHeadAttention(v_dim=v_dim, l_dim=l_dim, embed_dim=embed_dim, num_heads=num_heads, dropout=dropout,
                                         cfg=cfg)
        if drop_path > 0.:
            raise NotImplementedError("BiAttentionBlockForCheckpoint: drop_path > 0 is not supported (VLFuse passes 0)")
        self.drop_path = nn.Identity()
        self.gamma_v = nn.Parameter(init_values * torch.ones((v_dim)), requires_grad=True)
        self.gamma_l = nn.Parameter(init_values * torch.ones((l_dim)), requires_grad=True)
        self.cfg = cfg

    def forward(self, v, l, attention_mask_l=None, task=None):
        v = self.layer_norm_v(v)
        l = self.layer_norm_l(l)
        delta_v, delta_l = self.attn(v, l, attention_mask_l=attention_mask_l)
        v = v + self.drop_path(self.gamma_v * delta_v)     # the residual starts from the NORMALISED features, as in the reference
        l = l + self.drop_path(self.gamma_l * delta_l)
        return v, l


class VLFuse(nn.Module):
    """Early fusion: bi-directional attention between the flattened image tokens and the text tokens."""

    def __init__(self, cfg):
        super().__init__()
        self.init_configs(cfg)
        self.cfg = cfg
        self.use_checkpoint = cfg.MODEL.VL_FUSION_USE_CHECKPOINT
        self.b_attn = BiAttentionBlockForCheckpoint(v_dim=self.img_dim, l_dim=self.lang_dim, embed_dim=self.embed_dim,
                                                    num_heads=self.n_head, dropout=0.1, drop_path=.0,
                                                    init_values=1.0 / cfg.MODEL.DDETRS.ENC_LAYERS, cfg=cfg)

    def init_configs(self, cfg):
        self.lang_model = cfg.MODEL.LANGUAGE_BACKBONE.MODEL_TYPE
        self.img_dim = cfg.MODEL.DDETRS.HIDDEN_DIM
        self.max_query_len = cfg.MODEL.LANGUAGE_BACKBONE.MAX_QUERY_LEN
        self.n_layers = cfg.MODEL.LANGUAGE_BACKBONE.N_LAYERS
        self.n_head = 8
        self.embed_dim = cfg.MODEL.DDETRS.VL_HIDDEN_DIM
        if self.lang_model in ["bert-base-uncased", "roberta-base", "clip"]:
            self.lang_dim = cfg.MODEL.LANGUAGE_BACKBONE.LANG_DIM
        else:
            self.lang_dim = 1024

    def set_own_training(self, flag, dropout=False):
        """Route the attention core under autograd through the HIP training kernels (BiMultiHeadAttention.own_training) for
        this layer; with dropout=True also when its dropout (0.1) is active (BiMultiHeadAttention.own_dropout): without it a
        stock training run, which has dropout on, stays on the composition."""
        self.b_attn.attn.own_training = bool(flag)
        self.b_attn.attn.own_dropout = bool(dropout)
        return self

    def forward(self, x, task=None):
        visual = x["visual"]
        lang = x["lang"]
        # activation checkpointing only means something when autograd records: the inference route never runs under it
        if self.use_checkpoint and torch.is_grad_enabled():
            fused_visual, fused_lang = checkpoint.checkpoint(self.b_attn, visual, lang["hidden"], lang["masks"], task,
                                                            use_reentrant=False)
        else:
            fused_visual, fused_lang = self.b_attn(visual, lang["hidden"], lang["masks"], task)
        lang["hidden"] = fused_lang
        return {"visual": fused_visual, "lang": lang}
