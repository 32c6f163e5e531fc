"""Float64 restatement of the ViT attention core (include/patch_embed_hip.h: patch_embed_hip_vit_attn_f32) and of the helpers
around it, written from the header's formulas, for the tests of the fused kernel and of uninext_amd/vit.py."""
import torch
import torch.nn.functional as F


def resize_table(table, length):
    """Linear interpolation of a [L, D] table along its rows to `length` rows (half-pixel centres, edges clamped)."""
    L = table.shape[0]
    if L == length:
        return table
    pos = ((torch.arange(length, dtype=torch.float64) + 0.5) * (L / length) - 0.5).clamp(min=0.0)
    lo = pos.floor().long().clamp(max=L - 1)
    hi = (lo + 1).clamp(max=L - 1)
    w = (pos - lo.double()).to(table.dtype)[:, None]
    return table[lo] * (1 - w) + table[hi] * w


def scores(qkv, th, tw, num_heads, q_hw, scale):
    """s[b, h, i, j] in float64.  q is scaled first, in qkv's OWN precision, as the module does; the two relative-position terms
    use the unscaled q."""
    Hq, Wq = q_hw
    B, S, E3 = qkv.shape
    D = E3 // (3 * num_heads)
    t = qkv.reshape(B, S, 3, num_heads, D)
    q, k = t[:, :, 0].permute(0, 2, 1, 3), t[:, :, 1].permute(0, 2, 1, 3)            # [B, H, S, D]
    s = torch.matmul((q * scale).double(), k.double().transpose(-1, -2))
    if th is not None:
        ih = torch.arange(S) // Wq
        iw = torch.arange(S) % Wq
        q64 = q.double()
        rel_h = torch.einsum("bhid,icd->bhic", q64, th.double()[ih[:, None] - torch.arange(Hq)[None, :] + Hq - 1])   # [B, H, S, Hq]
        rel_w = torch.einsum("bhid,icd->bhic", q64, tw.double()[iw[:, None] - torch.arange(Wq)[None, :] + Wq - 1])   # [B, H, S, Wq]
        s = s + rel_h[..., ih] + rel_w[..., iw]
    return s


def core(qkv, th, tw, num_heads, q_hw, scale):
    """qkv [B, S, 3 * heads * D]; th [2 Hq - 1, D], tw [2 Wq - 1, D] or both None.  Returns out [B, S, heads * D] in float64."""
    B, S, E3 = qkv.shape
    D = E3 // (3 * num_heads)
    v = qkv.reshape(B, S, 3, num_heads, D)[:, :, 2].permute(0, 2, 1, 3).double()
    p = torch.softmax(scores(qkv, th, tw, num_heads, q_hw, scale), dim=-1)
    return torch.matmul(p, v).permute(0, 2, 1, 3).reshape(B, S, num_heads * D)


def composition_fp32(qkv, th, tw, num_heads, q_hw, scale):
    """The module's PyTorch composition on an fp32 qkv (the operations of Attention.forward between qkv and proj)."""
    from uninext_amd.vit import add_decomposed_rel_pos
    B, S, _ = qkv.shape
    t = qkv.reshape(B, S, 3, num_heads, -1).permute(2, 0, 3, 1, 4)
    q, k, v = t.reshape(3, B * num_heads, S, -1).unbind(0)
    attn = (q * scale) @ k.transpose(-2, -1)
    if th is not None:
        attn = add_decomposed_rel_pos(attn, q, th, tw, q_hw, q_hw)
    attn = attn.softmax(dim=-1)
    return (attn @ v).view(B, num_heads, S, -1).permute(0, 2, 1, 3).reshape(B, S, -1)


def exact_case(seed, B, heads, q_hw, D, device="cpu"):
    """Small-integer q, k and tables with scale 2^-3 (passed explicitly, whatever D is): every product is a multiple of 2^-3
    below 2^6 and every partial sum of a score stays below 2^14, so each score is the same number in any summation order, in
    fp32 and in float64.  |q|, |k| <= 2 and a quarter of the table entries are +-1, the rest 0: the scores have a spread of about 8,
    a peaked but not one-hot softmax.
    v is a multiple of 2^-10 in [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    Hq, Wq = q_hw
    S = Hq * Wq
    t = torch.zeros(B, S, 3, heads, D)
    t[:, :, 0] = torch.randint(-2, 3, (B, S, heads, D), generator=g).float()
    t[:, :, 1] = torch.randint(-2, 3, (B, S, heads, D), generator=g).float()
    t[:, :, 2] = torch.randint(-1024, 1025, (B, S, heads, D), generator=g).float() / 1024
    th = (torch.randint(-1, 2, (2 * Hq - 1, D), generator=g) * (torch.rand(2 * Hq - 1, D, generator=g) < 0.375)).float()
    tw = (torch.randint(-1, 2, (2 * Wq - 1, D), generator=g) * (torch.rand(2 * Wq - 1, D, generator=g) < 0.375)).float()
    return t.reshape(B, S, 3 * heads * D).to(device), th.to(device), tw.to(device), 0.125


def window_partition(x, ws):
    B, H, W, C = x.shape
    ph, pw = (-H) % ws, (-W) % ws
    x = F.pad(x, (0, 0, 0, pw, 0, ph))
    Hp, Wp = H + ph, W + pw
    x = x.reshape(B, Hp // ws, ws, Wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5)
    return x.reshape(-1, ws, ws, C), (Hp, Wp)
