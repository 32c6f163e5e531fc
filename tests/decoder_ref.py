"""Float64 restatement of the decoder's arithmetic from its definition: the self-attention core that
biattn_hip_self_forward_f32 computes, the decoder layer around it, and the decoder / re-id loops.  Plain torch on the CPU,
parameters taken from a reference-keyed state dict."""
import math

import torch
import torch.nn.functional as F


def core(q, k, v, heads, mask=None, scale=None):
    """q, k, v [B, L, E] -> [B, L, E]: per head softmax_j((q scale) . k + mask) v.  mask [L, L]: bool (True = excluded) or float
    (added).  A row with every key excluded is NaN."""
    B, L, E = q.shape
    D = E // heads
    scale = D ** -0.5 if scale is None else scale
    split = lambda t: t.double().reshape(B, L, heads, D).permute(0, 2, 1, 3)
    s = (split(q) * scale) @ split(k).transpose(-1, -2)
    if mask is not None:
        s = s.masked_fill(mask, float("-inf")) if mask.dtype == torch.bool else s + mask.double()
    return (torch.softmax(s, -1) @ split(v)).permute(0, 2, 1, 3).reshape(B, L, E)


def _lin(st, name, x):
    return x @ st[name + ".weight"].double().t() + st[name + ".bias"].double()


def _norm(st, name, x):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * st[name + ".weight"].double() + st[name + ".bias"].double()


def deform_attn(st, pre, query, ref, src, shapes, lsi, padding_mask, heads, n_levels, n_points):
    """Multi-scale deformable attention: every query samples n_points bilinear taps per level and head around its reference
    point (pixel centres at (i + 0.5) / size, zeros outside) and mixes them with softmax weights."""
    B, Lq, C = query.shape
    S, D = src.shape[1], C // heads
    value = _lin(st, pre + "value_proj", src)
    if padding_mask is not None:
        value = value.masked_fill(padding_mask[..., None], 0.0)
    value = value.reshape(B, S, heads, D)
    off = _lin(st, pre + "sampling_offsets", query).reshape(B, Lq, heads, n_levels, n_points, 2)
    w = torch.softmax(_lin(st, pre + "attention_weights", query).reshape(B, Lq, heads, n_levels * n_points), -1)
    w = w.reshape(B, Lq, heads, n_levels, n_points)
    if ref.shape[-1] == 2:
        size_xy = torch.stack([shapes[:, 1], shapes[:, 0]], -1).double()
        loc = ref[:, :, None, :, None, :] + off / size_xy[None, None, None, :, None, :]
    else:
        loc = ref[:, :, None, :, None, :2] + off / n_points * ref[:, :, None, :, None, 2:] * 0.5
    out = torch.zeros(B, Lq, heads, D, dtype=torch.float64)
    for lvl in range(n_levels):
        H, W = int(shapes[lvl, 0]), int(shapes[lvl, 1])
        start = int(lsi[lvl])
        img = value[:, start:start + H * W].permute(0, 2, 3, 1).reshape(B * heads, D, H, W)
        grid = (2 * loc[:, :, :, lvl] - 1).permute(0, 2, 1, 3, 4).reshape(B * heads, Lq, n_points, 2)
        taps = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)    # [B heads, D, Lq, P]
        wl = w[:, :, :, lvl].permute(0, 2, 1, 3).reshape(B * heads, 1, Lq, n_points)
        out += (taps * wl).sum(-1).reshape(B, heads, D, Lq).permute(0, 3, 1, 2)
    return _lin(st, pre + "output_proj", out.reshape(B, Lq, C))


def layer(st, tgt, query_pos, ref, src, shapes, lsi, padding_mask, attn_mask, heads, n_levels=4, n_points=4, pre=""):
    """One decoder layer at inference: self-attention among the queries, deformable cross-attention into src, FFN; each followed
    by a residual add and a LayerNorm."""
    st = {k[len(pre):]: v for k, v in st.items() if k.startswith(pre)}
    tgt, src, ref = tgt.double(), src.double(), ref.double()
    E = tgt.shape[-1]
    pos = 0.0 if query_pos is None else query_pos.double()
    w, b = st["self_attn.in_proj_weight"].double(), st["self_attn.in_proj_bias"].double()
    x = tgt + pos
    q, k, v = x @ w[:E].t() + b[:E], x @ w[E:2 * E].t() + b[E:2 * E], tgt @ w[2 * E:].t() + b[2 * E:]
    tgt = _norm(st, "norm2", tgt + _lin(st, "self_attn.out_proj", core(q, k, v, heads, attn_mask)))
    cross = deform_attn(st, "cross_attn.", tgt + pos, ref, src, shapes, lsi, padding_mask, heads, n_levels, n_points)
    tgt = _norm(st, "norm1", tgt + cross)
    return _norm(st, "norm3", tgt + _lin(st, "linear2", torch.relu(_lin(st, "linear1", tgt))))


def sine_embed(pos, feats=128, temperature=10000):
    """[B, L, n] -> [B, L, n * feats], y's block before x's.  The frequencies are rounded to fp32, as the reference has them."""
    c = torch.arange(feats, dtype=torch.float32)
    dim_t = (temperature ** (2 * torch.div(c, 2, rounding_mode="floor") / feats)).double()
    blocks = []
    for n in range(pos.shape[-1]):
        ang = pos[..., n:n + 1].double() * (2 * math.pi) / dim_t
        e = torch.empty_like(ang)
        e[..., 0::2], e[..., 1::2] = ang[..., 0::2].sin(), ang[..., 1::2].cos()
        blocks.append(e)
    blocks[0], blocks[1] = blocks[1], blocks[0]
    return torch.cat(blocks, -1)


def mlp(st, pre, x, n):
    for j in range(n):
        x = _lin(st, "%slayers.%d" % (pre, j), x)
        if j < n - 1:
            x = torch.relu(x)
    return x


def logit(x, eps=1e-5):
    x = x.clamp(0, 1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


def decoder(st, tgt, ref, src, shapes, lsi, valid_ratios, padding_mask, attn_mask, heads, n_layers, refine):
    """(stack of every layer's output, stack of the reference points after every layer).  refine: bbox_embed is set."""
    out, ref = tgt.double(), ref.double()
    outs, refs = [], []
    vr = torch.cat([valid_ratios, valid_ratios], -1).double()
    for lid in range(n_layers):
        ref_in = ref[:, :, None] * vr[:, None]
        pos = mlp(st, "ref_point_head.", sine_embed(ref_in[:, :, 0, :]), 2)
        out = layer(st, out, pos, ref_in, src, shapes, lsi, padding_mask, attn_mask, heads, pre="layers.%d." % lid)
        if refine:
            ref = torch.sigmoid(mlp(st, "bbox_embed.%d." % lid, out, 3) + logit(ref))
        outs.append(out)
        refs.append(ref)
    return torch.stack(outs), torch.stack(refs)
