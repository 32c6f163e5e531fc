"""Per-entry float64 parity of the three fused attention cores (uninext_amd/csrc/dec_attn.hip, vit_attn.hip, biattn.hip): the
cases, float64 numpy restatements that return every output entry's VALUE and its MAGNITUDE, the fp32 PyTorch compositions, and
the error measure.  No GPU is needed to import this.  tests/test_attn_parity_cpu.py checks that the measure has teeth,
tests/test_attn_parity_gpu.py holds the kernels to it.

For out[i, d] = sum_j p_ij v_jd the magnitude is s[i, d] = (1 + 2 A_i) sum_j p_ij |v_jd|.  A_i is the largest, over the open
keys of query i, of the score's own summed absolute summands, sum_d |q_id scale| |k_jd| plus |rel_h| + |rel_w| or |mask value|
where one is added: a score's fp32 rounding error is a multiple of u times that, exp passes an error e of a score on as a
relative error e of its term, and the normalisation as at most another e, so the entry moves by at most 2 e sum_j p_ij |v_jd|
to first order; the 1 is the rounding of the second product's own sum.  A score at the +-50000 clamp is exact, and so is a masked
score of the image side of biattn (-9e15 SET, not added: tests/vlfuse_ref.py): both contribute 0 to A_i.  It is derived, not
measured.  An entry is held to entry_bound of tests/parity_measure.py: max(8 x the composition's error, 16 u s).

Every input is seeded and dyadic (a multiple of 2^-10), so fp32 holds exactly what float64 sees; q is scaled in fp32 first, as
the kernels and the existing restatements do, by a scale that is itself a fp32 number.
"""
import functools
import os
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_cases as DC                                                  # noqa: E402
import vlfuse_cases as LC                                                   # noqa: E402
import parity_measure as PM                                                 # noqa: E402
from parity_measure import COMP_MARGIN, SUM_DEPTH, U, entry_bound          # noqa: E402,F401

assert DC.STEP_BITS == 10
dyadic = DC.dyadic
TOL = DC.TOL
TILE = 32
CLAMP, MASKED = 50000.0, -9e15
NEG = float("-inf")
BHS = ((1, 1), (2, 3))                      # batch x heads of every shape
STRESS = ("ascending", "descending", "flat", "sharp")

DEC_D = 32
DEC_LENS = (1,      # one key, one query
            31,     # a tail in the only tile; the second wave owns no tile
            32,     # one full tile: the second wave owns no tile at all
            33,     # a tail of one key in the second wave's only tile, and a second workgroup
            64,     # one full tile per wave, no tail anywhere
            65,     # three tiles, ranges of 2 and 1; the second wave's only tile holds one key
            97,     # four tiles, two per wave
            130)    # five tiles, ranges of 3 and 2
VIT_DS = (64, 80)
VIT_SHAPES = ((1, 1), (4, 8), (3, 11), (8, 16), (3, 43), (14, 14), (40, 1), (1, 40), (20, 23))
BI_D = 256
BI_TS = (1, 32, 33, 65, 96, 97, 129, 224, 256)
BI_SHAPES = tuple((S, T) for T in BI_TS for S in (1, 33, 129)) + tuple((S, T) for S in (32, 128, 1065) for T in (65, 129))
BI_MASKS = ("none", "i64", "f32", "allmasked")


def fp32_scale(D):
    return float(np.float32(D ** -0.5))


# ------------------------------------------------------------------------------------------------------------------- the cases

CASES = {}


def _add(name, **spec):
    assert name not in CASES, name
    CASES[name] = spec


for _B, _H in BHS:
    _bh = "%dx%d" % (_B, _H)
    for _L in DEC_LENS:
        for _kind, _pat in (("none", None), ("bool", "random"), ("f32", "random")):
            _add("dec/L%d/%s/%s" % (_L, _kind, _bh), core="dec", L=_L, B=_B, heads=_H, mask=_kind, pattern=_pat, stress=None)
    for _kind in ("bool", "f32"):
        for _L in (65, 130):
            for _pat in ("dn", "last_open"):
                _add("dec/L%d/%s_%s/%s" % (_L, _kind, _pat, _bh), core="dec", L=_L, B=_B, heads=_H, mask=_kind, pattern=_pat, stress=None)
        _add("dec/L97/%s_row45/%s" % (_kind, _bh), core="dec", L=97, B=_B, heads=_H, mask=_kind, pattern="row45", stress=None)
    for _s in STRESS:
        _add("dec/L130/%s/%s" % (_s, _bh), core="dec", L=130, B=_B, heads=_H, mask="none", pattern=None, stress=_s)
    for _D in VIT_DS:
        for _hw in VIT_SHAPES:
            for _rel in (True, False):
                _add("vit/D%d/%dx%d/%s/%s" % (_D, _hw[0], _hw[1], "rel" if _rel else "norel", _bh), core="vit", D=_D, hw=_hw, B=_B,
                     heads=_H, rel=_rel, stress=None)
        for _s in STRESS:
            _add("vit/D%d/20x23/%s/%s" % (_D, _s, _bh), core="vit", D=_D, hw=(20, 23), B=_B, heads=_H, rel=True, stress=_s)
    for _S, _T in BI_SHAPES:
        for _m in BI_MASKS:
            _add("bi/S%d_T%d/%s/%s" % (_S, _T, _m, _bh), core="bi", S=_S, T=_T, B=_B, heads=_H, mask=_m, stress=None)
    for _s in STRESS:
        _add("bi/S1065_T65/%s/%s" % (_s, _bh), core="bi", S=1065, T=65, B=_B, heads=_H, mask="none", stress=_s)
for _s in ("ascending", "descending"):      # 34 tiles in 22 ranges: the text side rescales inside a range as well
    _add("bi/S1065_T129/%s/2x3" % _s, core="bi", S=1065, T=129, B=2, heads=3, mask="none", stress=_s)


def names(core, **want):
    return [n for n, c in CASES.items() if c["core"] == core and all(c[k] == v for k, v in want.items())]


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _ramp(r, sign, streamed, step):
    """channel 0 of every head: `step` per tile of 32 rows on the streamed side, 4 on the owned side"""
    n = r.shape[-3]
    if streamed:
        r[..., 0] = (sign * step * (torch.arange(n) // TILE).double())[:, None]
    else:
        r[..., 0] = 4.0
    return r.reshape(*r.shape[:-2], -1)


def _qk(g, B, n_q, n_k, heads, D, stress, streamed, step):
    """(q [B, n_q, E], k [B, n_k, E]) float64 dyadic.  streamed: "q" or "k", the side that is tiled."""
    if stress in ("ascending", "descending"):
        sign = 1.0 if stress == "ascending" else -1.0
        q = dyadic(torch.randn(B, n_q, heads * D, generator=g), 0.5).view(B, n_q, heads, D)
        k = dyadic(torch.randn(B, n_k, heads * D, generator=g), 0.5).view(B, n_k, heads, D)
        return _ramp(q, sign, streamed == "q", step), _ramp(k, sign, streamed == "k", step)
    q = dyadic(torch.randn(B, n_q, heads * D, generator=g))
    k = dyadic(torch.randn(B, n_k, heads * D, generator=g))
    if stress == "flat":
        q = torch.zeros_like(q)
    elif stress == "sharp":
        q, k = q * 4.0, k * 4.0
    else:
        assert stress is None
    return q, k


def dec_mask(name):
    c = CASES[name]
    L, kind, pat = c["L"], c["mask"], c["pattern"]
    if kind == "none":
        return None
    g = torch.Generator().manual_seed(zlib.crc32(("mask/%d/%s/%s" % (L, kind, pat)).encode()))
    if pat in ("random", "row45"):
        if kind == "bool":
            m = torch.rand(L, L, generator=g) < 0.3
            m[:, 0] = False                                     # no row is empty
        else:
            m = DC.float_mask(g, L)                             # dyadic values, a quarter -inf, column 0 open
        if pat == "row45":
            m[45] = True if kind == "bool" else NEG
        return m
    if pat == "dn":                                             # queries from L // 2 rounded down to a tile: leading tiles wholly excluded
        m = DC.dn_mask(L, L // 2 // TILE * TILE, 2)
    else:
        m = torch.ones(L, L, dtype=torch.bool)                  # a single open key, the last one of the last tile
        m[:, L - 1] = False
    return m if kind == "bool" else torch.zeros(L, L, dtype=torch.float64).masked_fill(m, NEG)


def bi_mask(name):
    """[B, T] int64 or float64 (0 = masked, else the value that is added), or None.  allmasked: the last image has no token."""
    c = CASES[name]
    B, T, kind = c["B"], c["T"], c["mask"]
    if kind == "none":
        return None
    keep = torch.arange(T)[None, :] < torch.tensor([max(1, (2 * T + 2) // 3), max(1, T // 2)])[:B, None]     # tokenizer-like
    if kind == "allmasked":
        keep[B - 1] = False
    if kind in ("i64", "allmasked"):
        return keep.long()
    vals = torch.tensor([1.0, 0.5, 2.0, 1.0, -0.25], dtype=torch.float64)[torch.arange(T) % 5]
    return keep.double() * vals[None, :]


@functools.lru_cache(maxsize=64)
def inputs(name):
    """Float64 dyadic inputs of a case from its name; left unchanged."""
    c = CASES[name]
    g = _gen(name)
    B, heads, stress = c["B"], c["heads"], c["stress"]
    if c["core"] == "dec":
        L = c["L"]
        q, k = _qk(g, B, L, L, heads, DEC_D, stress, "k", 3.0)
        x = dict(q=q, k=k, v=dyadic(torch.randn(B, L, heads * DEC_D, generator=g)), mask=dec_mask(name), scale=fp32_scale(DEC_D))
        floats = ("q", "k", "v")
    elif c["core"] == "vit":
        D, (Hq, Wq) = c["D"], c["hw"]
        S = Hq * Wq
        q, k = _qk(g, B, S, S, heads, D, stress, "k", 6.0)
        v = dyadic(torch.randn(B, S, heads * D, generator=g))
        qkv = torch.stack([t.view(B, S, heads, D) for t in (q, k, v)], 2).reshape(B, S, 3 * heads * D)
        x = dict(qkv=qkv, th=None, tw=None, scale=fp32_scale(D))
        floats = ("qkv",)
        if c["rel"]:
            gain = 0.3 if stress is None else 0.0625 if stress in ("ascending", "descending") else 0.3
            x["th"] = dyadic(torch.randn(2 * Hq - 1, D, generator=g), gain)
            x["tw"] = dyadic(torch.randn(2 * Wq - 1, D, generator=g), gain)
            if stress in ("ascending", "descending"):           # the ramp's constant on q meets no table entry
                x["th"][:, 0] = 0.0
                x["tw"][:, 0] = 0.0
            floats += ("th", "tw")
    else:
        S, T = c["S"], c["T"]
        g = _gen("bi/S%d_T%d/%s/%dx%d" % (S, T, stress, B, heads))      # the same tensors under every mask
        q, k = _qk(g, B, S, T, heads, BI_D, stress, "q", 12.0)      # the text side streams the image tokens
        x = dict(q=q, k=k, vv=dyadic(torch.randn(B, S, heads * BI_D, generator=g)),
                 vl=dyadic(torch.randn(B, T, heads * BI_D, generator=g)), mask=bi_mask(name), scale=fp32_scale(BI_D))
        floats = ("q", "k", "vv", "vl")
    for key in floats:
        x[key] = x[key] + 0.0                                   # rounding to the dyadic grid leaves -0.0 behind: +0.0
        assert torch.equal(x[key].float().double(), x[key]), (name, key)      # fp32 holds what float64 sees
    m = x.get("mask")
    if m is not None and m.dtype == torch.float64:
        assert torch.equal(m.float().double(), m), (name, "mask")
    return x


# ------------------------------------------------------------------------------------------------------------ the restatements

def _np(t):
    return t.numpy().astype(np.float64)


def _scaled(q, scale):
    """q * scale in fp32, taken to float64"""
    return (q.astype(np.float32) * np.float32(scale)).astype(np.float64)


def _split(t, heads):
    B, N, E = t.shape
    return t.reshape(B, N, heads, E // heads).transpose(0, 2, 1, 3)            # [B, H, N, D]


def _merge(t):
    B, H, N, D = t.shape
    return t.transpose(0, 2, 1, 3).reshape(B, N, H * D)


def softmax_pv(s, amp, v):
    """s, amp [..., Q, K]: the scores (-inf = excluded) and their summed absolute summands (0 where the score is exact);
    v [..., K, Dv].  Returns (out, mag) [..., Q, Dv]; a row with every key excluded is NaN in both."""
    with np.errstate(invalid="ignore"):
        e = np.exp(s - s.max(-1, keepdims=True))
        p = e / e.sum(-1, keepdims=True)
    A = np.where(np.isfinite(s), amp, 0.0).max(-1)
    return p @ v, (1.0 + 2.0 * A)[..., None] * (p @ np.abs(v))


def dec_scores(q, k, heads, mask, scale):
    """(s, amp) [B, H, L, L] float64 of the decoder's self-attention: (q scale) . k + mask"""
    qs, kh = _split(_scaled(q, scale), heads), _split(k, heads)
    s = qs @ kh.transpose(0, 1, 3, 2)
    amp = np.abs(qs) @ np.abs(kh).transpose(0, 1, 3, 2)
    if mask is not None:
        if mask.dtype == np.bool_:
            s = np.where(mask, NEG, s)
        else:
            s = s + mask
            amp = amp + np.where(np.isfinite(mask), np.abs(mask), 0.0)
    return s, amp


def dec_core(q, k, v, heads, mask, scale):
    """q, k, v [B, L, E] float64 numpy, mask [L, L] bool (True = excluded) or float64 (added) or None -> (out, mag) [B, L, E]."""
    s, amp = dec_scores(q, k, heads, mask, scale)
    out, mag = softmax_pv(s, amp, _split(v, heads))
    return _merge(out), _merge(mag)


def vit_key_hw(q_hw):
    Hq, Wq = q_hw
    j = np.arange(Hq * Wq)
    return j // Wq, j % Wq


def vit_scores(qkv, th, tw, heads, q_hw, scale, scaled=_scaled):
    """(s, amp, v) of the ViT core: (q scale) . k + q . th[ih - jh + Hq - 1] + q . tw[iw - jw + Wq - 1], the height term first.
    scaled: how q is scaled (in fp32, as the kernels do; tests/vit_bwd_parity.py also asks for the float64 product)"""
    Hq, Wq = q_hw
    B, S, E3 = qkv.shape
    D = E3 // (3 * heads)
    t = qkv.reshape(B, S, 3, heads, D)
    q, k, v = (t[:, :, n].transpose(0, 2, 1, 3) for n in range(3))
    qs = scaled(q, scale)
    s = qs @ k.transpose(0, 1, 3, 2)
    amp = np.abs(qs) @ np.abs(k).transpose(0, 1, 3, 2)
    if th is not None:
        ih, iw = vit_key_hw(q_hw)
        rel_h = np.einsum("bhid,icd->bhic", q, th[ih[:, None] - np.arange(Hq)[None, :] + Hq - 1])      # [B, H, S, Hq]
        rel_w = np.einsum("bhid,icd->bhic", q, tw[iw[:, None] - np.arange(Wq)[None, :] + Wq - 1])      # [B, H, S, Wq]
        s = (s + rel_h[..., ih]) + rel_w[..., iw]
        amp = amp + np.abs(rel_h)[..., ih] + np.abs(rel_w)[..., iw]
    return s, amp, v


def vit_core(qkv, th, tw, heads, q_hw, scale):
    """qkv [B, S, 3 heads D]; th [2 Hq - 1, D], tw [2 Wq - 1, D] or both None -> (out, mag) [B, S, heads D]."""
    s, amp, v = vit_scores(qkv, th, tw, heads, q_hw, scale)
    out, mag = softmax_pv(s, amp, v)
    return _merge(out), _merge(mag)


def swapped_tables_differ(name):
    """For q_h != q_w: the restatement with the two tables exchanged (each resized to the other's rows) is far outside the
    project's bound, so a transposed lookup cannot pass.  False for a square shape (nothing to tell apart)."""
    import vit_ref
    c, x = CASES[name], inputs(name)
    Hq, Wq = c["hw"]
    if Hq == Wq:
        return False
    want = reference(name)["out"][0]
    th, tw = vit_ref.resize_table(x["tw"], 2 * Hq - 1), vit_ref.resize_table(x["th"], 2 * Wq - 1)
    swapped, _ = vit_core(_np(x["qkv"]), _np(th), _np(tw), c["heads"], c["hw"], x["scale"])
    assert np.abs(swapped - want).max() > 100 * TOL * np.abs(want).max(), name
    return True


def bi_scores(q, k, heads, scale):
    """(clamped s, amp) [B, H, S, T]; amp is 0 where the clamp bites"""
    qs, kh = _split(_scaled(q, scale), heads), _split(k, heads)
    raw = qs @ kh.transpose(0, 1, 3, 2)
    amp = np.where(np.abs(raw) >= CLAMP, 0.0, np.abs(qs) @ np.abs(kh).transpose(0, 1, 3, 2))
    return np.clip(raw, -CLAMP, CLAMP), amp


def bi_core(q, k, vv, vl, mask, heads, scale):
    """q, vv [B, S, E]; k, vl [B, T, E]; mask [B, T] (0 = masked, else the value that is added) or None.
    Returns (out_v, mag_v [B, S, E], out_l, mag_l [B, T, E])."""
    s, amp = bi_scores(q, k, heads, scale)
    st = s.transpose(0, 1, 3, 2)
    zt = np.maximum(st - st.max(-1, keepdims=True), -CLAMP)
    out_l, mag_l = softmax_pv(zt, amp.transpose(0, 1, 3, 2), _split(vv, heads))
    if mask is not None:
        m = mask.astype(np.float64)[:, None, None, :]
        s = np.where(m == 0, MASKED, s + m)                                   # SET, as fp32 has it
        amp = np.where(m == 0, 0.0, amp + np.abs(m))
    out_v, mag_v = softmax_pv(s, amp, _split(vl, heads))
    return _merge(out_v), _merge(mag_v), _merge(out_l), _merge(mag_l)


def _npmask(m):
    return None if m is None else m.numpy()


@functools.lru_cache(maxsize=64)
def reference(name):
    """{output: (value, mag)} of a case: computed once, shared, left unchanged."""
    c, x = CASES[name], inputs(name)
    if c["core"] == "dec":
        return {"out": dec_core(_np(x["q"]), _np(x["k"]), _np(x["v"]), c["heads"], _npmask(x["mask"]), x["scale"])}
    if c["core"] == "vit":
        th, tw = (None, None) if x["th"] is None else (_np(x["th"]), _np(x["tw"]))
        return {"out": vit_core(_np(x["qkv"]), th, tw, c["heads"], c["hw"], x["scale"])}
    ov, mv, ol, ml = bi_core(_np(x["q"]), _np(x["k"]), _np(x["vv"]), _np(x["vl"]), _npmask(x["mask"]), c["heads"], x["scale"])
    return {"out_v": (ov, mv), "out_l": (ol, ml)}


def existing_restatement(name):
    """{output: value} by tests/decoder_ref.py, vit_ref.py, vlfuse_ref.py on the same inputs (q scaled in fp32 first)."""
    import decoder_ref
    import vit_ref
    import vlfuse_ref
    c, x = CASES[name], inputs(name)
    if c["core"] == "dec":      # decoder_ref.core scales in the precision it is given: hand it the fp32 product, scale 1
        qs = (x["q"].float() * x["scale"]).double()
        return {"out": decoder_ref.core(qs, x["k"], x["v"], c["heads"], x["mask"], 1.0).numpy()}
    if c["core"] == "vit":
        th, tw = (None, None) if x["th"] is None else (x["th"].float(), x["tw"].float())
        return {"out": vit_ref.core(x["qkv"].float(), th, tw, c["heads"], c["hw"], x["scale"]).numpy()}
    ov, ol = vlfuse_ref.core(x["q"].float(), x["k"].float(), x["vv"].float(), x["vl"].float(), x["mask"], c["heads"], x["scale"])
    return {"out_v": ov.numpy(), "out_l": ol.numpy()}


def tile_maxima(name):
    """[N, owned tokens, tiles]: the largest float64 score of every tile of 32 streamed tokens, as the running softmax meets
    them (biattn: the text side's, over the image tokens)."""
    c, x = CASES[name], inputs(name)
    if c["core"] == "dec":
        s, _ = dec_scores(_np(x["q"]), _np(x["k"]), c["heads"], _npmask(x["mask"]), x["scale"])
    elif c["core"] == "vit":
        th, tw = (None, None) if x["th"] is None else (_np(x["th"]), _np(x["tw"]))
        s, _, _ = vit_scores(_np(x["qkv"]), th, tw, c["heads"], c["hw"], x["scale"])
    else:
        s = bi_scores(_np(x["q"]), _np(x["k"]), c["heads"], x["scale"])[0].transpose(0, 1, 3, 2)
    n = s.shape[-1]
    pad = (-n) % TILE
    s = np.concatenate((s, np.full(s.shape[:-1] + (pad,), NEG)), -1)
    return s.reshape(-1, s.shape[-2], (n + pad) // TILE, TILE).max(-1), s[..., :n]


def stress_property(name):
    """Asserts, on the float64 scores, the property that names a stress case."""
    c = CASES[name]
    tmax, s = tile_maxima(name)
    assert tmax.shape[-1] >= 5, (name, "many tiles")
    if c["stress"] == "ascending":          # every tile's largest score exceeds every earlier one: a rescale at every tile
        assert (np.diff(tmax, axis=-1) > 0).all(), name
    elif c["stress"] == "descending":       # ... stays below the first tile's: the running max never moves, the skip is taken
        assert (np.diff(tmax, axis=-1) < 0).all(), name
    elif c["stress"] == "flat":
        assert (s == 0).all(), name
    else:
        assert c["stress"] == "sharp"
        with np.errstate(under="ignore"):
            p = np.exp(s - s.max(-1, keepdims=True))
        assert (p < U).mean() > 0.5, (name, "most probabilities are below fp32's reach of the largest")


# ----------------------------------------------------------------------------------------------------------- the compositions

@functools.lru_cache(maxsize=None)
def _bi_module(E, heads, device):
    from uninext_amd.modules.vl_fusion import BiMultiHeadAttention
    from types import SimpleNamespace as NS
    m = BiMultiHeadAttention(8, 8, E, heads, dropout=0.1, cfg=NS(MODEL=NS(DYHEAD=NS(FUSE_CONFIG=LC.fuse_cfg()))))
    return m.to(device).eval()


def composition(name, device="cpu"):
    """{output: float64 numpy} of the fp32 PyTorch composition on `device`; it never runs the kernels."""
    c, x = CASES[name], inputs(name)
    heads, scale = c["heads"], x["scale"]
    dev = lambda t: None if t is None else (t.float() if t.dtype == torch.float64 else t).to(device)
    back = lambda t: t.detach().cpu().double().numpy()
    with torch.no_grad():
        if c["core"] == "dec":      # F.multi_head_attention_forward: q scaled, baddbmm with the float mask, softmax, bmm
            q, k, v, mask = dev(x["q"]), dev(x["k"]), dev(x["v"]), dev(x["mask"])
            B, L, E = q.shape
            split = lambda t: t.view(B, L, heads, E // heads).transpose(1, 2).reshape(B * heads, L, E // heads)
            q, k, v = split(q * scale), split(k), split(v)
            if mask is not None and mask.dtype == torch.bool:
                mask = torch.zeros(L, L, dtype=torch.float32, device=device).masked_fill(mask, NEG)
            w = torch.bmm(q, k.transpose(-2, -1)) if mask is None else torch.baddbmm(mask, q, k.transpose(-2, -1))
            out = torch.bmm(torch.softmax(w, dim=-1), v)
            assert out.dtype == torch.float32
            return {"out": back(out.view(B, heads, L, -1).transpose(1, 2).reshape(B, L, E))}
        if c["core"] == "vit":      # the torch route of vit.Attention's core
            from uninext_amd import vit
            D, (Hq, Wq) = c["D"], c["hw"]
            m = vit.Attention(heads * D, num_heads=heads, use_rel_pos=c["rel"], input_size=(Hq, Wq))
            assert float(np.float32(m.scale)) == scale
            if c["rel"]:
                m.rel_pos_h.copy_(x["th"].float())
                m.rel_pos_w.copy_(x["tw"].float())
            m = m.to(device).eval()
            assert not vit.Attention.fused_core
            out = m._core_torch(dev(x["qkv"]), Hq, Wq)
            assert out.dtype == torch.float32
            return {"out": back(out)}
        m = _bi_module(heads * BI_D, heads, device)
        assert float(np.float32(m.scale)) == scale
        out_v, out_l = m._core_torch(dev(x["q"]) * m.scale, dev(x["k"]), dev(x["vv"]), dev(x["vl"]), dev(x["mask"]))
        assert out_v.dtype == torch.float32 and out_l.dtype == torch.float32
        return {"out_v": back(out_v), "out_l": back(out_l)}


# ---------------------------------------------------------------------------------------------------------- the error measure

HEAD = "%-40s %-8s %10s %10s %10s %8s" % ("case", "output", "kernel err", "comp err", "bound", "ratio")
_T = PM.Table(HEAD, env="ATTN_PARITY_TABLE")
TABLE, WORST, report = _T.lines, _T.worst, _T.report        # WORST: (core, output) -> (ratio, table line)


def measure(case, what, got, want, mag, comp, check=True):
    """Every entry of `got` within entry_bound(the composition's error at the entry, s) of `want`, and the project's bound on top.
    Returns the largest error / bound; check=False only returns it (inf when the NaN rows differ) and adds no line.
    Non-finite: NaN only as whole rows, the same rows in `got`, `want` and `comp`.
    WORST: (core, output).  Line: case, output, the worst entry's errors relative to its own magnitude; a dash line and 0.0
    for a tensor that is NaN throughout.  Tolerance: TOL * max|want|."""
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape == comp.shape == mag.shape, (case, what, got.shape, want.shape, comp.shape, mag.shape)
    nan = np.isnan(want)
    assert np.array_equal(nan.any(-1), nan.all(-1)), (case, what, "NaN is a whole row")
    assert np.array_equal(np.isnan(comp), nan), (case, what, "the composition's NaN rows")
    same_nan = np.array_equal(np.isnan(got), nan)
    if check:
        assert same_nan, (case, what, "NaN rows", np.argwhere(np.isnan(got) != nan)[:8].tolist())
    elif not same_nan:
        return float("inf")
    fin = lambda a: np.where(nan, 0.0, a)
    e = PM.errors(fin(got), fin(want), fin(mag), fin(comp))
    if not check:
        return e.worst
    if nan.all():
        _T.add("%-40s %-8s %10s %10s %10s %8s" % (case, what, "-", "-", "-", "-"))
        return 0.0
    _T.add("%-40s %-8s %10.2e %10.2e %10.2e %8.3f" % ((case, what) + e.row()), (case.split("/")[0], what), e.worst)
    e.check(case, what)
    assert float(e.err.max()) <= TOL * float(e.size.max()), (case, what, "the project's bound", float(e.err.max()), float(e.size.max()))
    return e.worst


# -------------------------------------------------------------------------------------- shapes as the kernels' hosts have them

def bi_nj(T):
    """The biattn_image instantiation of T text tokens: the number of 32-token tiles, rounded up to 1, 2, 4 or 8."""
    tiles = -(-T // TILE)
    return next(nj for nj in (1, 2, 4, 8) if tiles <= nj)


def bi_ranges(BH, S, T):
    """(TP, NC): text tokens rounded up to 32, and the number of ranges of S the text side is split into: enough for 256
    workgroups of 128 text tokens, at most 64, at most one per tile of 32 image tokens."""
    TP = -(-T // TILE) * TILE
    per = BH * -(-TP // (4 * TILE))
    tiles = -(-S // TILE)
    return TP, max(1, min(-(-256 // per), 64, tiles))
