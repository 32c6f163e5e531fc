"""Float64 restatement of the text encoder (BertModel without a pooler, transformers 4.x mask semantics) and of its attention
core, in plain torch statements on a state dict: no module of the package and no `transformers`.  As tests/decoder_ref.py."""
import math

import torch


def layer_norm(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)                     # biased
    return (x - mu) / torch.sqrt(var + eps) * w + b


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def additive(mask, dtype=torch.float64):
    """[B, T] or [B, T, T] keep mask -> what is added to the scores [B, heads, T, T]"""
    m = mask.to(dtype)
    m = m[:, None, None, :] if m.dim() == 2 else m[:, None, :, :]
    return (1.0 - m) * torch.finfo(dtype).min


def attention_core(q, k, v, heads, mask=None):
    """q, k, v [B, T, heads * d] -> context [B, T, heads * d]; with it, every entry's MAGNITUDE as tests/attn_parity.py derives
    it for out[i, d] = sum_j p_ij v_jd: (1 + 2 A_i) sum_j p_ij |v_jd|, A_i the largest, over the kept keys of query i, of the
    score's own summed absolute summands sum_d |q_id / sqrt(d)| |k_jd| (a score's fp32 rounding error is a multiple of u times
    that; exp passes it on as a relative error of the term, the normalisation as at most another)."""
    B, T, E = q.shape
    d = E // heads
    split = lambda t: t.reshape(B, T, heads, d).permute(0, 2, 1, 3)
    s = split(q) @ split(k).transpose(-1, -2) / math.sqrt(d)
    amp = split(q).abs() @ split(k).abs().transpose(-1, -2) / math.sqrt(d)
    if mask is not None:
        s = s + additive(mask, s.dtype)
        keep = mask != 0
        amp = amp * (keep[:, None, None, :] if keep.dim() == 2 else keep[:, None, :, :])
    p = torch.softmax(s, -1)
    merge = lambda t: t.permute(0, 2, 1, 3).reshape(B, T, E)
    return merge(p @ split(v)), merge((1.0 + 2.0 * amp.max(-1, keepdim=True)[0]) * (p @ split(v).abs()))


def embeddings(p, ids, tt, eps):
    T = ids.shape[1]
    tt = torch.zeros_like(ids) if tt is None else tt
    x = p["embeddings.word_embeddings.weight"][ids] + p["embeddings.token_type_embeddings.weight"][tt]
    x = x + p["embeddings.position_embeddings.weight"][:T][None]
    return layer_norm(x, p["embeddings.LayerNorm.weight"], p["embeddings.LayerNorm.bias"], eps)


def layer(p, pre, x, heads, mask, eps):
    lin = lambda name, t: t @ p[pre + name + ".weight"].T + p[pre + name + ".bias"]
    ctx, _ = attention_core(lin("attention.self.query", x), lin("attention.self.key", x), lin("attention.self.value", x), heads, mask)
    x = layer_norm(lin("attention.output.dense", ctx) + x, p[pre + "attention.output.LayerNorm.weight"],
                   p[pre + "attention.output.LayerNorm.bias"], eps)
    y = lin("output.dense", gelu(lin("intermediate.dense", x)))
    return layer_norm(y + x, p[pre + "output.LayerNorm.weight"], p[pre + "output.LayerNorm.bias"], eps)


def model(p, cfg, ids, mask=None, tt=None):
    """Every hidden state: the embeddings, then each layer's output."""
    p = {k: v.double() for k, v in p.items()}
    x = embeddings(p, ids, tt, cfg["layer_norm_eps"])
    hidden = [x]
    for n in range(cfg["num_hidden_layers"]):
        x = layer(p, "encoder.layer.%d." % n, x, cfg["num_attention_heads"], mask, cfg["layer_norm_eps"])
        hidden.append(x)
    return hidden


def parallel_det_mask(mask):
    """The reference's loop (bert_model.py:38-43), statement by statement."""
    bs, seq_len = mask.shape
    mask_new = torch.zeros((bs, seq_len, seq_len))
    for b in range(bs):
        mask_new[b, :, :] = mask[b]
        num_valid = int(torch.sum(mask[b]))
        mask_new[b, :num_valid, :num_valid] = torch.eye(num_valid)
    return mask_new
