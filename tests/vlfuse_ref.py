"""Float64 restatement of the bi-directional attention core (include/biattn_hip.h), for the tests of the fused kernels.

It follows the fp32 behaviour of the reference's mask: `masked_fill(mask == 0, -9e15)` on the tokenizer mask leaves the ones in
place, and in fp32 `score + (-9e15)` rounds to exactly -9e15 (|score| <= 50000 after the clamp, far below the spacing of fp32
there), so a masked score IS the constant and a row whose tokens are all masked is uniform over all T tokens.  In float64 the
sum keeps the score, and such a row follows the scores instead: this restatement therefore SETS masked scores to the constant.
"""
import torch

CLAMP = 50000.0
MASKED = -9e15


def split_heads(t, num_heads):
    B, N, E = t.shape
    return t.reshape(B, N, num_heads, E // num_heads).permute(0, 2, 1, 3)          # [B, H, N, D]


def merge_heads(t):
    B, H, N, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, N, H * D)


def scores(q, k, num_heads, q_scale):
    """Clamped scores [B, H, S, T] in float64; q is scaled first, in its OWN precision, as the module does."""
    qs = (q * q_scale).double()
    s = torch.matmul(split_heads(qs, num_heads), split_heads(k.double(), num_heads).transpose(-1, -2))
    return s.clamp(min=-CLAMP, max=CLAMP)


def core(q, k, vv, vl, mask, num_heads, q_scale):
    """q, vv [B, S, E]; k, vl [B, T, E]; mask [B, T] (0 = masked, else the value that is added) or None.
    Returns (out_v [B, S, E], out_l [B, T, E]) in float64."""
    s = scores(q, k, num_heads, q_scale)
    st = s.transpose(-1, -2)
    p_l = torch.softmax((st - st.max(dim=-1, keepdim=True)[0]).clamp(min=-CLAMP), dim=-1)
    out_l = torch.matmul(p_l, split_heads(vv.double(), num_heads))
    if mask is not None:
        m = mask.double()[:, None, None, :]
        s = torch.where(m == 0, torch.full_like(s, MASKED), s + m)
    p_v = torch.softmax(s, dim=-1)
    out_v = torch.matmul(p_v, split_heads(vl.double(), num_heads))
    return merge_heads(out_v), merge_heads(out_l)


def exact_case(seed, B, H, S, T, D=256, device="cpu", big=True):
    """Integer-valued q, k with a power-of-two scale (D = 256: 2^-4): every product is a multiple of 2^-4 and every partial sum
    of a score stays below 2^20, so the scores are identical in any summation order and in fp32 and float64.  With `big`, image
    tokens 0 and S // 2 and text tokens 0 and T - 1 carry the same +-1 pattern at full amplitude: their scores are 65536 before
    the clamp and tie at +50000 on both softmax axes (text token 1, when T > 2, carries the negated pattern: -50000)."""
    g = torch.Generator().manual_seed(seed)
    E = H * D
    q = torch.randint(-8, 9, (B, S, E), generator=g).float()
    k = torch.randint(-8, 9, (B, T, E), generator=g).float()
    if big:
        sgn = (torch.randint(0, 2, (B, 1, E), generator=g) * 2 - 1).float()
        q[:, 0:1] = 512.0 * sgn
        q[:, S // 2:S // 2 + 1] = 512.0 * sgn
        if T > 2:
            k[:, 1:2] = -8.0 * sgn
        k[:, 0:1] = 8.0 * sgn
        k[:, T - 1:T] = 8.0 * sgn
    vv = torch.randint(-1024, 1025, (B, S, E), generator=g).float() / 1024
    vl = torch.randint(-1024, 1025, (B, T, E), generator=g).float() / 1024
    return q.to(device), k.to(device), vv.to(device), vl.to(device), D ** -0.5
