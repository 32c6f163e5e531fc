"""No GPU: the error measure of tests/attn_parity.py has teeth.

A numpy fp32 emulation of the streamed-attention scheme, written from its description (tiles of 32 streamed tokens, a running
max and sum with rescaling, sums in register order and then the other lane half, dec_attn's two-range combine, biattn's
range-order combine and its all-scores-in-registers image side), is held to the measure against the float64 restatement with
the fp32 PyTorch composition on the CPU as `comp`: the correct emulation stays within the bound on EVERY case of the sweep, and
each wrong variant is over it on the case named in WRONG.  The restatements of attn_parity agree with tests/decoder_ref.py,
vit_ref.py and vlfuse_ref.py to 1e-12 of the output's largest value on every case.

Worst error / bound of the correct emulation over the sweep: 0.208 (bi/S1065_T129/ascending/2x3 out_l; dec 0.104, vit 0.163).
Of each wrong variant on its named case (inf: NaN where a number belongs):
    (a) tail_at_0          dec/L33/none/1x1               3.7e+04
    (b) no_rescale         dec/L130/ascending/1x1         2.1e+05
    (c) rescale_inverted   vit/D64/20x23/ascending/1x1    1.4e+05
    (d) cut10              bi/S33_T33/none/1x1            43
    (e) first_max          bi/S1065_T65/ascending/1x1     inf
    (f) rel_w_next_key     vit/D64/3x11/rel/1x1           6.0e+05
    (g) empty_tile_at_0    bi/S33_T65/none/1x1            8.6e+03
(e) is the same number in exact arithmetic: the weights exp(m_c - M) only exceed 1.  It is wrong where they overflow, and the
ascending ramp of 3 per tile over 34 ranges (99 > log of fp32's largest number) is the case that shows it.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_parity as P     # noqa: E402

F32 = np.float32
NEG = F32("-inf")
# register v of a lane holds row 8 (v / 4) + 4 half + v % 4 of a 32-row tile
ROWS = [[8 * (v // 4) + 4 * half + v % 4 for v in range(16)] for half in (0, 1)]
SWITCHES = ("tail_at_0", "no_rescale", "rescale_inverted", "cut10", "first_max", "rel_w_next_key", "empty_tile_at_0")

# variant -> the case of the sweep on which it must exceed the bound
WRONG = {
    "tail_at_0": "dec/L33/none/1x1",                    # (a) 31 keys that do not exist enter the second tile's sum
    "no_rescale": "dec/L130/ascending/1x1",             # (b) the max rises at every tile
    "rescale_inverted": "vit/D64/20x23/ascending/1x1",  # (c)
    "cut10": "bi/S33_T33/none/1x1",                     # (d)
    "first_max": "bi/S1065_T65/ascending/1x1",          # (e) the last range's max is 99 above the first's: exp overflows
    "rel_w_next_key": "vit/D64/3x11/rel/1x1",           # (f)
    "empty_tile_at_0": "bi/S33_T65/none/1x1",           # (g) NJ = 4, the fourth tile has no row
}


def f32(t):
    return None if t is None else t.numpy().astype(F32)


def cut(x, on):
    """mantissa cut to 10 bits"""
    return (np.ascontiguousarray(x).view(np.uint32) & np.uint32(0xFFFFE000)).view(F32) if on else x


def dot32(a, b, sw):
    """a [..., Q, D] . b [..., K, D] -> [..., Q, K] in fp32, one product at a time in the order of the reduction steps: of every 8
    floats the first of each lane half, then the second, ..."""
    a, b = cut(a, "cut10" in sw), cut(b, "cut10" in sw)
    D = a.shape[-1]
    acc = np.zeros(a.shape[:-1] + (b.shape[-2],), F32)
    for ss in range(D // 8):
        for t in range(4):
            for half in (0, 1):
                d = 8 * ss + 4 * half + t
                acc = acc + a[..., :, None, d] * b[..., None, :, d]
    assert acc.dtype == F32
    return acc


def chain32(a, b):
    """sum_d a[..., d] b[..., d] as one fp32 chain in d order"""
    acc = np.zeros(np.broadcast_shapes(a.shape, b.shape)[:-1], F32)
    for d in range(a.shape[-1]):
        acc = acc + a[..., d] * b[..., d]
    return acc


def seqsum(p):
    """sum over the last axis in index order, fp32"""
    acc = np.zeros(p.shape[:-1], F32)
    for n in range(p.shape[-1]):
        acc = acc + p[..., n]
    return acc


def pad_keys(X, V, fill):
    """X [N, Q, K] -> K rounded up to 32 with `fill`; V [N, K, Dv] with zero rows"""
    pad = (-X.shape[-1]) % P.TILE
    X = np.concatenate((X, np.full(X.shape[:-1] + (pad,), fill, F32)), -1)
    V = np.concatenate((V, np.zeros((V.shape[0], pad, V.shape[2]), F32)), 1)
    return X, V


def stream(X, V, tiles, sw):
    """The running softmax of every owned token over the tiles `tiles` of its streamed side.  X [N, Q, 32 n] fp32 scores with
    everything added (-inf: not there), V [N, 32 n, Dv].  A wave is 32 consecutive owned tokens.  Returns (max, sum, accumulator)."""
    N, Q, _ = X.shape
    m = np.full((N, Q), NEG, F32)
    l = np.zeros((N, Q), F32)
    acc = np.zeros((N, Q, V.shape[-1]), F32)
    wave = np.arange(Q) // P.TILE
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for t in tiles:
            x = X[:, :, P.TILE * t:P.TILE * (t + 1)]
            v = cut(V[:, P.TILE * t:P.TILE * (t + 1)], "cut10" in sw)
            m_new = np.maximum(m, x.max(-1))
            m_use = np.where(m_new == NEG, F32(0), m_new)               # nothing open so far: against 0, never -inf - -inf
            alpha = np.exp(m - m_use)
            p = np.exp(x - m_use[..., None])
            l = l * alpha + (seqsum(p[..., ROWS[0]]) + seqsum(p[..., ROWS[1]]))
            m = m_new
            need = np.zeros((N, wave[-1] + 1), bool)
            np.logical_or.at(need, (slice(None), wave), alpha != 1)     # some lane of the wave has a factor other than 1
            apply = ~need if "rescale_inverted" in sw else np.zeros_like(need) if "no_rescale" in sw else need
            acc = np.where(apply[:, wave, None], acc * alpha[..., None], acc)
            pc = cut(p, "cut10" in sw)
            for r in range(16):
                for half in (0, 1):
                    j = ROWS[half][r]
                    acc = acc + pc[:, :, j, None] * v[:, None, j, :]
    assert acc.dtype == F32 and l.dtype == F32
    return m, l, acc


def heads_of(t, heads):
    B, n, E = t.shape
    return t.reshape(B, n, heads, E // heads).transpose(0, 2, 1, 3).reshape(B * heads, n, E // heads)


def merged(t, B):
    N, n, D = t.shape
    return t.reshape(B, N // B, n, D).transpose(0, 2, 1, 3).reshape(B, n, -1)


def emulate_dec(name, sw=()):
    c, x = P.CASES[name], P.inputs(name)
    B, L, heads = c["B"], c["L"], c["heads"]
    q, k, v = (heads_of(f32(x[n]), heads) for n in ("q", "k", "v"))
    X = dot32(q * F32(x["scale"]), k, sw)
    mask = x["mask"]
    if mask is not None:
        X = np.where(mask.numpy(), NEG, X) if mask.dtype != P.torch.float64 else X + f32(mask)
    X, v = pad_keys(X, v, F32(0) if "tail_at_0" in sw else NEG)
    tiles = X.shape[-1] // P.TILE
    per = -(-tiles // 2)
    (m0, l0, a0), (m1, l1, a1) = stream(X, v, range(0, per), sw), stream(X, v, range(per, tiles), sw)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = m0 if "first_max" in sw else np.maximum(m0, m1)
        m_use = np.where(m == NEG, F32(0), m)
        w0, w1 = np.exp(m0 - m_use), np.exp(m1 - m_use)
        inv = F32(1) / (l0 * w0 + l1 * w1)
        out = (a0 * w0[..., None] + a1 * w1[..., None]) * inv[..., None]
    return {"out": merged(out, B)}


def emulate_vit(name, sw=()):
    c, x = P.CASES[name], P.inputs(name)
    B, heads, D, (Hq, Wq) = c["B"], c["heads"], c["D"], c["hw"]
    S = Hq * Wq
    t = f32(x["qkv"]).reshape(B, S, 3, heads, D)
    q, k, v = (t[:, :, n].transpose(0, 2, 1, 3).reshape(B * heads, S, D) for n in range(3))
    X = dot32(q * F32(x["scale"]), k, sw)
    if c["rel"]:
        th, tw = f32(x["th"]), f32(x["tw"])
        ih, iw = P.vit_key_hw((Hq, Wq))
        rel_h = chain32(q[:, :, None, :], th[ih[:, None] - np.arange(Hq)[None, :] + Hq - 1][None])        # [N, S, Hq]
        rel_w = chain32(q[:, :, None, :], tw[iw[:, None] - np.arange(Wq)[None, :] + Wq - 1][None])        # [N, S, Wq]
        jw = iw[np.minimum(np.arange(S) + 1, S - 1)] if "rel_w_next_key" in sw else iw
        X = (X + rel_h[:, :, ih]) + rel_w[:, :, jw]
    X, v = pad_keys(X, v, F32(0) if "tail_at_0" in sw else NEG)
    _, l, acc = stream(X, v, range(X.shape[-1] // P.TILE), sw)
    return {"out": merged(acc * (F32(1) / l)[..., None], B)}


@functools.lru_cache(maxsize=4)
def _bi_text_side(name, sw):
    """(out_l [N, T, D], image-side scores before the mask [N, S, T]) of a case: the mask plays no part in either"""
    c, x = P.CASES[name], P.inputs(name)
    B, heads, S, T = c["B"], c["heads"], c["S"], c["T"]
    q, k, vv = (heads_of(f32(x[n]), heads) for n in ("q", "k", "vv"))
    qs = q * F32(x["scale"])
    clamp = lambda s: np.minimum(np.maximum(s, F32(-P.CLAMP)), F32(P.CLAMP))
    # the text side: a wave owns 32 text tokens and streams the image tokens of one range; the ranges are combined in order
    Xt, vvp = pad_keys(clamp(dot32(k, qs, sw)), vv, F32(0) if "tail_at_0" in sw else NEG)
    tiles = Xt.shape[-1] // P.TILE
    _, NC = P.bi_ranges(B * heads, S, T)
    parts = [stream(Xt, vvp, range(tiles * n // NC, tiles * (n + 1) // NC), sw) for n in range(NC)]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        M = parts[0][0]
        if "first_max" not in sw:
            for m, _, _ in parts[1:]:
                M = np.maximum(M, m)
        Ls, o = np.zeros_like(M), np.zeros_like(parts[0][2])
        for m, l, acc in parts:
            w = np.exp(m - M)
            Ls = Ls + l * w
            o = o + acc * w[..., None]
        out_l = o / Ls[..., None]
    return out_l, clamp(dot32(qs, k, sw))


def emulate_bi(name, sw=()):
    c, x = P.CASES[name], P.inputs(name)
    B, heads, S, T = c["B"], c["heads"], c["S"], c["T"]
    vl = heads_of(f32(x["vl"]), heads)
    out_l, Xi = _bi_text_side(name.replace("/%s/" % c["mask"], "/none/") if c["stress"] is None else name, tuple(sw))
    # the image side: all scores of a token in registers, NJ tiles of 32 text tokens
    if x["mask"] is not None:
        mk = np.repeat(x["mask"].numpy(), heads, 0)[:, None, :]                                   # [N, 1, T]
        Xi = Xi + np.where(mk == 0, F32(P.MASKED), mk.astype(F32))
        assert Xi.dtype == F32
    Xi, vlp = pad_keys(Xi, vl, F32(0) if "tail_at_0" in sw else NEG)
    NJ = P.bi_nj(T)
    empty = NJ * P.TILE - Xi.shape[-1]
    Xi = np.concatenate((Xi, np.full(Xi.shape[:-1] + (empty,), F32(0) if "empty_tile_at_0" in sw else NEG, F32)), -1)
    vlp = np.concatenate((vlp, np.zeros((vlp.shape[0], empty, vlp.shape[2]), F32)), 1)
    order = [[P.TILE * jt + r for jt in range(NJ) for r in ROWS[half]] for half in (0, 1)]
    with np.errstate(under="ignore"):
        p = np.exp(Xi - Xi.max(-1, keepdims=True))
        p = p * (F32(1) / (seqsum(p[..., order[0]]) + seqsum(p[..., order[1]])))[..., None]
        p, vlp = cut(p, "cut10" in sw), cut(vlp, "cut10" in sw)
        out_v = np.zeros(Xi.shape[:-1] + (vlp.shape[-1],), F32)
        for n in range(16 * NJ):
            for half in (0, 1):
                j = order[half][n]
                out_v = out_v + p[:, :, j, None] * vlp[:, None, j, :]
    assert out_v.dtype == F32 and out_l.dtype == F32
    return {"out_v": merged(out_v, B), "out_l": merged(out_l, B)}


EMULATE = {"dec": emulate_dec, "vit": emulate_vit, "bi": emulate_bi}


def worst_ratio(name, sw=(), check=True):
    ref, comp = P.reference(name), P.composition(name, "cpu")
    got = EMULATE[P.CASES[name]["core"]](name, sw)
    return max(P.measure(name, what, got[what].astype(np.float64), want, mag, comp[what], check=check) for what, (want, mag) in ref.items())


def agrees_with_the_existing_restatement(name):
    for what, value in P.existing_restatement(name).items():
        want = P.reference(name)[what][0]
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(value), nan), (name, what)
        assert np.abs(np.where(nan, 0.0, value - want)).max() <= 1e-12 * np.abs(np.where(nan, 0.0, want)).max(), (name, what)


def sweep(core, **want):
    return [n for n in P.names(core, **want)]


def _chunks():
    """the sweep in pieces of one core and one batch x heads, so that no test takes long"""
    out = []
    for core in ("dec", "vit", "bi"):
        for B, H in P.BHS:
            out.append(pytest.param(core, B, H, id="%s-%dx%d" % (core, B, H)))
    return out


@pytest.mark.parametrize("core,B,heads", _chunks())
def test_correct_emulation_within_the_bound_and_restatements_agree(core, B, heads):
    since = len(P.TABLE)
    worst = 0.0
    for name in P.names(core, B=B, heads=heads):
        agrees_with_the_existing_restatement(name)
        if P.CASES[name]["stress"]:
            P.stress_property(name)
        worst = max(worst, worst_ratio(name))
    P.report(since)
    print("worst error / bound of the correct emulation: %.3f" % worst)
    assert worst <= 1.0


def test_every_case_of_the_issue_is_in_the_sweep():
    assert len(P.names("dec", stress=None, pattern=None)) == 2 * len(P.DEC_LENS)
    assert len(P.names("dec", pattern="random")) == 2 * 2 * len(P.DEC_LENS)
    assert len(P.names("vit", stress=None)) == 2 * 2 * 2 * len(P.VIT_SHAPES)
    assert len(P.names("bi", stress=None)) == 2 * 4 * (27 + 6)
    assert {P.bi_nj(T) for T in P.BI_TS} == {1, 2, 4, 8}
    assert [P.bi_nj(T) for T in P.BI_TS] == [1, 1, 2, 4, 4, 4, 8, 8, 8]
    for T in (65, 96, 129, 224):                                   # a tile with no row
        assert P.bi_nj(T) * P.TILE - T >= P.TILE
    assert P.bi_ranges(1, 1065, 65) == (96, 34) and P.bi_ranges(6, 1065, 129) == (160, 22)
    for name in WRONG.values():
        assert name in P.CASES


@pytest.mark.parametrize("variant", SWITCHES)
def test_wrong_variant_exceeds_the_bound_on_its_named_case(variant):
    name = WRONG[variant]
    assert worst_ratio(name) <= 1.0                                # the correct emulation passes the same case
    ratio = worst_ratio(name, (variant,), check=False)
    print("%-18s %-32s error / bound %.3g" % (variant, name, ratio))
    assert ratio > 1.0, (variant, name, ratio)


def test_swapped_tables_give_another_answer():
    checked = [P.swapped_tables_differ(name) for name in P.names("vit", rel=True, stress=None, B=1, heads=1)]
    assert sum(checked) == 2 * sum(h != w for h, w in P.VIT_SHAPES)
