"""The ViTDet-style ViT backbone with the reference's names and state-dict layout (projects/UNINEXT/uninext/backbone/vit.py and
backbone/utils.py), running its attention core on include/patch_embed_hip.h at inference.

  window_partition, window_unpartition, get_rel_pos, add_decomposed_rel_pos, get_abs_pos      backbone/utils.py:16-157
  Attention        backbone/vit.py:27-83      qkv, proj, rel_pos_h, rel_pos_w
  Mlp              timm's in the reference     fc1, act, fc2
  Block            backbone/vit.py:147-230    norm1, attn, norm2, mlp, window_size (the ConvNeXt Block lives in backbone.py)
  ViT              backbone/vit.py:233-374    patch_embed, pos_embed, blocks, fpn1..3; forward returns {"res3", "res4", "res5"}
  vit_kwargs       the three presets of D2ViT (backbone/vit.py:378-425)

At inference on the GPU in fp32 (Attention.fused_core), Attention.forward is qkv Linear -> ext.vit_attention -> proj: one pass
over the keys per 128 queries, with the decomposed relative positions added to score tiles in registers, so the
[B * heads, S, S] scores, their 5-d view, the softmax and the permute copies of q, k, v and the output are never written.
Under autograd the core can run on the same scheme too (opt-in: Attention.own_training, ViT.set_own_training):
ViTAttentionFunction is ext.vit_attention_train, which also keeps the row log-sum-exp, and ext.vit_attention_backward, which
recomputes the probabilities tile by tile -- neither writes the scores, so a block saves qkv, the core's output and one float
per (head, query) instead of three [B * heads, S, S] tensors.
Everything else -- autograd by default, the CPU, other dtypes, head sizes the kernel lacks -- runs the reference's PyTorch composition.
Window partition, padding and un-partition are PyTorch copies as in the reference; the zero-padded tokens (qkv.bias after the
Linear) take part as keys.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ext
from .backbone import DropPath, PatchEmbed, _fp32_on, _records


def window_partition(x, window_size):
    """[B, H, W, C] -> ([B * windows, window_size, window_size, C], (Hp, Wp)): zeros are appended at the bottom and the right up
    to the next multiples of window_size, then the map is cut into non-overlapping windows, row-major per image."""
    B, H, W, C = x.shape
    bottom, right = (-H) % window_size, (-W) % window_size
    if bottom or right:
        x = F.pad(x, (0, 0, 0, right, 0, bottom))
    Hp, Wp = H + bottom, W + right
    nh, nw = Hp // window_size, Wp // window_size
    tiles = x.reshape(B, nh, window_size, nw, window_size, C).transpose(2, 3)           # [B, nh, nw, ws, ws, C]
    return tiles.reshape(B * nh * nw, window_size, window_size, C), (Hp, Wp)


def window_unpartition(windows, window_size, pad_hw, hw):
    """The inverse of window_partition: [B * windows, window_size, window_size, C] -> [B, H, W, C], the padding cut off."""
    nh, nw = pad_hw[0] // window_size, pad_hw[1] // window_size
    C = windows.shape[-1]
    tiles = windows.reshape(-1, nh, nw, window_size, window_size, C).transpose(2, 3)   # [B, nh, ws, nw, ws, C]
    full = tiles.reshape(tiles.shape[0], pad_hw[0], pad_hw[1], C)
    if tuple(pad_hw) == tuple(hw):
        return full
    return full[:, :hw[0], :hw[1]].contiguous()


def resize_rel_pos(rel_pos, length):
    """A relative-position table [L, C] at `length` rows: itself when L == length, else every channel linearly interpolated
    along the rows (F.interpolate, mode "linear")."""
    if rel_pos.shape[0] == length:
        return rel_pos
    return F.interpolate(rel_pos.t().unsqueeze(0), size=length, mode="linear")[0].t()


def get_rel_pos(q_size, k_size, rel_pos):
    """[q_size, k_size, C]: for every (query, key) coordinate pair the row of the table, resized to 2 * max(q_size, k_size) - 1
    rows, that belongs to their distance.  Equal sizes: row i - j + n - 1.  Unequal sizes: the shorter axis is stretched to the
    longer one's extent before the difference is taken, and the fractional row is truncated."""
    n = max(q_size, k_size)
    table = resize_rel_pos(rel_pos, 2 * n - 1)
    if q_size == k_size:
        steps = torch.arange(n, device=table.device)
        rows = steps[:, None] - steps[None, :] + (n - 1)
    else:
        q_step, k_step = max(k_size / q_size, 1.0), max(q_size / k_size, 1.0)
        q_at = torch.arange(q_size, device=table.device) * q_step
        k_at = torch.arange(k_size, device=table.device) * k_step
        rows = (q_at[:, None] - k_at[None, :] + (k_size - 1) * k_step).long()
    return table[rows]


def add_decomposed_rel_pos(attn, q, rel_pos_h, rel_pos_w, q_size, k_size):
    """attn [B, q_h * q_w, k_h * k_w] plus the decomposed relative positions of MViTv2: the products of every query with the
    height table's rows are shared by all keys of a row, those with the width table's rows by all keys of a column.  The height
    term is added first."""
    (q_h, q_w), (k_h, k_w) = q_size, k_size
    tokens = q.unflatten(1, (q_h, q_w))                                                     # [B, q_h, q_w, C]
    along_h = torch.einsum("byxc,ykc->byxk", tokens, get_rel_pos(q_h, k_h, rel_pos_h))     # [B, q_h, q_w, k_h]
    along_w = torch.einsum("byxc,xkc->byxk", tokens, get_rel_pos(q_w, k_w, rel_pos_w))     # [B, q_h, q_w, k_w]
    scores = attn.unflatten(2, (k_h, k_w)).unflatten(1, (q_h, q_w))                         # [B, q_h, q_w, k_h, k_w]
    scores = scores + along_h.unsqueeze(-1) + along_w.unsqueeze(-2)
    return scores.flatten(3).flatten(1, 2)


def get_abs_pos(abs_pos, has_cls_token, hw):
    """Absolute position embeddings [1, N (+ 1), C] as [1, h, w, C]: the cls entry dropped, and the square grid of the
    pre-training size resized bicubically when it is not h x w."""
    grid = abs_pos[:, 1:] if has_cls_token else abs_pos
    side = math.isqrt(grid.shape[1])
    if side * side != grid.shape[1]:
        raise ValueError("get_abs_pos: %d positions are not a square grid" % grid.shape[1])
    grid = grid.reshape(1, side, side, -1)
    if (side, side) == tuple(hw):
        return grid
    return F.interpolate(grid.permute(0, 3, 1, 2), size=tuple(hw), mode="bicubic", align_corners=False).permute(0, 2, 3, 1)


class Mlp(nn.Module):
    """fc1 -> act -> fc2 (timm's Mlp with its defaults: biases, no dropout, no norm)."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class ViTAttentionFunction(torch.autograd.Function):
    """`apply(qkv, th, tw, heads, hw, scale)` -> the attention core [B', S, heads * D] of qkv [B', S, 3 * heads * D] with the
    tables th [2 * q_h - 1, D], tw [2 * q_w - 1, D] (or both None): ext.vit_attention_train forward, ext.vit_attention_backward
    backward (exact fp32, fixed order, bitwise repeatable).  Saved for backward: qkv, the tables, the output and the row
    log-sum-exp; the probabilities are recomputed."""

    @staticmethod
    def forward(ctx, qkv, th, tw, heads, hw, scale):
        det = lambda t: None if t is None else t.detach().contiguous()
        qkv, th, tw = det(qkv), det(th), det(tw)
        out, lse = ext.vit_attention_train(qkv, th, tw, heads, hw, scale)
        ctx.heads, ctx.hw, ctx.scale = int(heads), (int(hw[0]), int(hw[1])), float(scale)
        ctx.save_for_backward(qkv, th, tw, out, lse)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        qkv, th, tw, out, lse = ctx.saved_tensors
        grad_qkv, grad_th, grad_tw = ext.vit_attention_backward(qkv, th, tw, out, lse, grad_out, ctx.heads, ctx.hw, ctx.scale)
        return grad_qkv, grad_th, grad_tw, None, None, None


class Attention(nn.Module):
    """Multi-head attention with decomposed relative positions (backbone/vit.py:27-83): same constructor and parameter names."""

    # True: at inference (fp32, GPU, no autograd graph, a head size the kernel takes) the core between `qkv` and `proj` is
    # ext.vit_attention; False: the reference's PyTorch composition everywhere.  Unmeasured against the
    # composition, hence opt-in until profiles/r11_vit.txt (tools/vit_bench.py) exists; the default follows that record.
    fused_core = False
    # True: when autograd records (fp32, GPU, no autocast, a head size the kernels take) the core is ViTAttentionFunction -- the
    # fused forward with the row log-sum-exp and its recomputing backward.  False (default): the PyTorch composition whenever
    # autograd records.  Opt-in until measured as a default (profiles/r31_vit_train.txt); ViT.set_own_training sets it per net.
    own_training = False

    def __init__(self, dim, num_heads=8, qkv_bias=True, use_rel_pos=False, rel_pos_zero_init=True, input_size=None):
        super().__init__()
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        self.use_rel_pos = use_rel_pos
        if self.use_rel_pos:
            self.rel_pos_h = nn.Parameter(torch.zeros(2 * input_size[0] - 1, head_dim))
            self.rel_pos_w = nn.Parameter(torch.zeros(2 * input_size[1] - 1, head_dim))
            if not rel_pos_zero_init:
                nn.init.trunc_normal_(self.rel_pos_h, std=0.02)
                nn.init.trunc_normal_(self.rel_pos_w, std=0.02)
        self._tables = None

    def _resized_tables(self, H, W):
        """The two tables at 2H - 1 and 2W - 1 rows, contiguous.  Interpolated ones are kept for the last (H, W) only, until a
        parameter changes."""
        h, w = self.rel_pos_h, self.rel_pos_w
        if h.shape[0] == 2 * H - 1 and w.shape[0] == 2 * W - 1:
            return h.detach().contiguous(), w.detach().contiguous()
        key = (H, W, h.data_ptr(), w.data_ptr(), h._version, w._version, h.device, h.dtype)
        if self._tables is None or self._tables[0] != key:
            with torch.no_grad():
                self._tables = (key, resize_rel_pos(h.detach(), 2 * H - 1).contiguous(), resize_rel_pos(w.detach(), 2 * W - 1).contiguous())
        return self._tables[1], self._tables[2]

    def _kernels_take(self, x):
        """(the kernels take this call, autograd records it): an fp32 GPU input [B, H, W, dim], fp32 parameters on its device, no
        autocast, a head size the kernels have."""
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
            return False, False
        params = [self.qkv.weight, self.qkv.bias, self.proj.weight, self.proj.bias]
        if self.use_rel_pos:
            params += [self.rel_pos_h, self.rel_pos_w]
        if not _fp32_on(x.device, *params) or torch.is_autocast_enabled():
            return False, False
        dim = self.qkv.in_features
        ok = dim % self.num_heads == 0 and dim // self.num_heads in ext._lib.VIT_ATTN_HEAD_DIMS and x.shape[-1] == dim
        return ok, _records(x, *params)

    def _use_hip(self, x):
        """The fused route may be taken: switched on, an fp32 GPU input, fp32 parameters on its device, no autograd graph being
        recorded, no autocast, a head size the kernel has."""
        if not self.fused_core:
            return False
        ok, records = self._kernels_take(x)
        return ok and not records

    def _use_hip_training(self, x):
        """The training route may be taken: own_training, an fp32 GPU input, fp32 parameters on its device, autograd records, no
        autocast, a head size the kernels have."""
        if not self.own_training:
            return False
        ok, records = self._kernels_take(x)
        return ok and records

    def _core_torch(self, qkv, H, W):
        """The PyTorch composition between `qkv` and `proj`: qkv [B, S, 3 * heads * D] -> [B, S, heads * D].  The full
        [B * heads, S, S] scores are formed, q is scaled before the product, the relative positions use the unscaled q."""
        B, S, _ = qkv.shape
        heads = self.num_heads
        split = qkv.view(B, S, 3, heads, -1)
        q, k, v = (split[:, :, j].transpose(1, 2).reshape(B * heads, S, -1) for j in range(3))
        scores = torch.bmm(q * self.scale, k.transpose(1, 2))
        if self.use_rel_pos:
            scores = add_decomposed_rel_pos(scores, q, self.rel_pos_h, self.rel_pos_w, (H, W), (H, W))
        context = torch.bmm(scores.softmax(dim=-1), v)
        return context.view(B, heads, S, -1).transpose(1, 2).reshape(B, S, -1)

    def forward(self, x):
        B, H, W, _ = x.shape
        fused = self._use_hip(x)
        train = self._use_hip_training(x)
        qkv = self.qkv(x).reshape(B, H * W, -1)
        if train and ext.vit_attention_train_supported(qkv, None, None, self.num_heads, (H, W)):   # else (q_w above the limit): PyTorch
            # the tables keep their autograd history: an interpolated table's gradient reaches the parameter through F.interpolate
            th, tw = ((resize_rel_pos(self.rel_pos_h, 2 * H - 1).contiguous(), resize_rel_pos(self.rel_pos_w, 2 * W - 1).contiguous())
                      if self.use_rel_pos else (None, None))
            core = ViTAttentionFunction.apply(qkv, th, tw, self.num_heads, (H, W), self.scale)
            return self.proj(core.view(B, H, W, -1))
        if fused:
            th, tw = self._resized_tables(H, W) if self.use_rel_pos else (None, None)
            fused = ext.vit_attention_supported(qkv, th, tw, self.num_heads, (H, W))
        if fused:
            core = ext.vit_attention(qkv, th, tw, self.num_heads, (H, W), self.scale)
        else:
            core = self._core_torch(qkv, H, W)
        return self.proj(core.view(B, H, W, -1))


class Block(nn.Module):
    """Transformer block with optional window attention (backbone/vit.py:147-230): same constructor and parameter names.  The
    convolutional residual block (use_residual_block=True) is not built: D2ViT passes residual_block_indexes=[]."""

    def __init__(self, dim, num_heads, mlp_ratio=4.0, qkv_bias=True, drop_path=0.0, norm_layer=nn.LayerNorm, act_layer=nn.GELU,
                 use_rel_pos=False, rel_pos_zero_init=True, window_size=0, use_residual_block=False, input_size=None):
        super().__init__()
        if use_residual_block:
            raise ValueError("use_residual_block=True is not built: the D2ViT presets pass residual_block_indexes=[]")
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, use_rel_pos=use_rel_pos, rel_pos_zero_init=rel_pos_zero_init,
                              input_size=input_size if window_size == 0 else (window_size, window_size))
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer)
        self.window_size = window_size
        self.use_residual_block = use_residual_block

    def forward(self, x):
        y = self.norm1(x)
        if self.window_size > 0:
            windows, padded = window_partition(y, self.window_size)
            y = window_unpartition(self.attn(windows), self.window_size, padded, (x.shape[1], x.shape[2]))
        else:
            y = self.attn(y)
        x = x + self.drop_path(y)
        return x + self.drop_path(self.mlp(self.norm2(x)))


class ViT(nn.Module):
    """The ViTDet backbone as UNINEXT uses it (backbone/vit.py:233-374): patch embedding, absolute positions resized to the token
    grid, `depth` blocks (windowed at window_block_indexes), and three outputs from the last block's map: fpn1 (transposed
    convolution, stride 8), fpn2 (identity, stride 16), fpn3 (max pooling, stride 32).  Same constructor and state-dict keys.
    use_act_checkpoint wraps each block's call in torch.utils.checkpoint (the reference takes fairscale's wrapper)."""

    def __init__(self, img_size=1024, patch_size=16, in_chans=3, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.0, qkv_bias=True,
                 drop_path_rate=0.0, norm_layer=nn.LayerNorm, act_layer=nn.GELU, use_abs_pos=True, use_rel_pos=False,
                 rel_pos_zero_init=True, window_size=0, window_block_indexes=(), residual_block_indexes=(), use_act_checkpoint=False,
                 pretrain_img_size=224, pretrain_use_cls_token=True, out_feature="last_feat"):
        super().__init__()
        self.pretrain_use_cls_token = pretrain_use_cls_token
        self.patch_embed = PatchEmbed(kernel_size=(patch_size, patch_size), stride=(patch_size, patch_size), in_chans=in_chans,
                                      embed_dim=embed_dim)
        if use_abs_pos:
            num_patches = (pretrain_img_size // patch_size) * (pretrain_img_size // patch_size)
            self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1 if pretrain_use_cls_token else num_patches, embed_dim))
        else:
            self.pos_embed = None
        rates = torch.linspace(0, drop_path_rate, depth).tolist()
        self.blocks = nn.ModuleList([
            Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, drop_path=rates[i], norm_layer=norm_layer,
                  act_layer=act_layer, use_rel_pos=use_rel_pos, rel_pos_zero_init=rel_pos_zero_init,
                  window_size=window_size if i in window_block_indexes else 0, use_residual_block=i in residual_block_indexes,
                  input_size=(img_size // patch_size, img_size // patch_size)) for i in range(depth)])
        self.use_act_checkpoint = use_act_checkpoint
        self._out_feature_channels = {out_feature: embed_dim}
        self._out_feature_strides = {out_feature: patch_size}
        self._out_features = [out_feature]
        if self.pos_embed is not None:
            nn.init.trunc_normal_(self.pos_embed, std=0.02)
        self.fpn1 = nn.Sequential(nn.ConvTranspose2d(embed_dim, embed_dim // 2, kernel_size=2, stride=2))
        self.fpn2 = nn.Identity()
        self.fpn3 = nn.MaxPool2d(kernel_size=2, stride=2)
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def set_own_training(self, flag=True):
        """Attention.own_training on every block's attention of this backbone, and PatchEmbed.own_exact_training on its patch
        embedding: the training step of both on the project's kernels (opt-in)."""
        for blk in self.blocks:
            blk.attn.own_training = bool(flag)
        self.patch_embed.own_exact_training = bool(flag)
        return self

    def forward(self, x):
        x = self.patch_embed(x)
        if self.pos_embed is not None:
            x = x + get_abs_pos(self.pos_embed, self.pretrain_use_cls_token, (x.shape[1], x.shape[2]))
        for blk in self.blocks:
            if self.use_act_checkpoint and torch.is_grad_enabled():
                from torch.utils import checkpoint
                x = checkpoint.checkpoint(blk, x, use_reentrant=False)
            else:
                x = blk(x)
        xp = x.permute(0, 3, 1, 2)   # B H W C -> B C H W
        return {"res3": self.fpn1(xp), "res4": self.fpn2(xp), "res5": self.fpn3(xp)}


_PRESETS = {"ViT-Base": (768, 12, 0.1, 12), "ViT-Large": (1024, 24, 0.4, 16), "ViT-huge": (1280, 32, 0.5, 16)}


def vit_kwargs(name, in_chans=3, use_act_checkpoint=False):
    """Constructor arguments of ViT for D2ViT's cfg.MODEL.VIT.NAME (backbone/vit.py:378-425): window 14 in blocks 0, 1, 3, 4, 6,
    7, 9, 10 whatever the depth, decomposed relative positions, LayerNorm eps 1e-6."""
    from functools import partial
    if name not in _PRESETS:
        raise ValueError("Unsupported ViT name")
    embed_dim, depth, drop_path_rate, num_heads = _PRESETS[name]
    return dict(img_size=1024, patch_size=16, in_chans=in_chans, embed_dim=embed_dim, depth=depth, num_heads=num_heads,
                drop_path_rate=drop_path_rate, window_size=14, mlp_ratio=4, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6),
                window_block_indexes=[0, 1, 3, 4, 6, 7, 9, 10], residual_block_indexes=[], use_rel_pos=True, out_feature="last_feat",
                use_act_checkpoint=use_act_checkpoint)
