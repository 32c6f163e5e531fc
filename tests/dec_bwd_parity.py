"""Per-entry float64 parity of the decoder self-attention core's training route (uninext_amd/csrc/dec_attn_bwd.hip: attn_lse,
bwd_q, bwd_kv, each in the mask variants none, bool and f32): the cases, a float64 numpy restatement of the forward's lse and of
the backward that returns every entry's VALUE and its MAGNITUDE, the fp32 PyTorch composition, and the error measure.  No GPU
and no built package is needed to import this.  tests/test_dec_bwd_parity_cpu.py checks that the measure has teeth,
tests/test_dec_bwd_parity_gpu.py holds the kernels to it through the C ABI.

Inputs are seeded by the case's name (crc32) and dyadic (multiples of 2^-10): q, k, v, g and the finite values of a float mask,
so fp32 holds exactly what float64 sees.  q is scaled in fp32 first by fp32_scale(32), which is no power of two: the rounding
is real.  The scores and their summed absolute summands `amp` are attn_parity.dec_scores'.

The restatement is written out analytically (include/biattn_hip.h), not through autograd, with g the upstream gradient and
m the mask's element (0, a finite float, or -inf), tests/vit_bwd_parity.py's formulas without the relative-position terms:
    s_ij = qs_i . k_j + m_ij       lse_i = log sum_j exp(s_ij)     p_ij = exp(s_ij - lse_i)     o_i = sum_j p_ij v_j
    delta_i = g_i . o_i            dv_j = sum_i p_ij g_i           ds_ij = p_ij (g_i . v_j - delta_i)
    dk_j = sum_i ds_ij qs_i        dq_i = scale sum_j ds_ij k_j
It agrees with decoder_train_cases.reference_grads (float64 autograd of core64, which rounds q * scale in fp32 as well) to
1e-12 of each group's largest value on every case (agrees_with_autograd).

THE MAGNITUDES are vit_bwd_parity's, unchanged in form; u = 2^-24, nothing was fitted to what a kernel gives, and no term was
added after the run on the MI355X.  Per (b, h), over the OPEN keys of query i (those with s_ij > -inf):
  A_i = max_j amp_ij, amp including |m_ij| of a finite float mask element;    L_i = max(|lse_i|, max_j |s_ij|)
  lse: 1 + A_i + |lse_i|                                 R_i = 1 + 2 A_i + 3 L_i
  dv[j, d] = sum_i R_i p_ij |g_id|                       P_ij = sum_d |g_id| |v_jd|
  Delta_i = sum_d |g_id| (1 + 2 A_i) sum_j p_ij |v_jd|   T_ij = p_ij (R_i |dp_ij - delta_i| + P_ij + Delta_i)
  dk[j, d] = sum_i T_ij |qs_id|                          dq[i, d] = scale sum_j T_ij |k_jd|
(their derivations: vit_bwd_parity's docstring).  An excluded pair has p = 0 and enters nothing.

A DEAD query (every key excluded): its lse is -inf and the kernel must give exactly -inf; every channel of its dq row must be
NaN and no other entry of any group may be NaN; its contribution to dk and dv is dropped from the values and the magnitudes
(include/biattn_hip.h, for a finite grad_out row).  A key that no live query attends to has dk = dv = 0 with magnitude 0: the
kernel must give an exact zero of either sign.  measure() decides these and hands only finite arrays to parity_measure.errors.

An entry is held to parity_measure.entry_bound: max(8 x the fp32 composition's error at the entry, 16 u x the magnitude); the
composition is decoder_train_cases.composition32 under fp32 autograd, and where it is NaN (a dead row poisons its whole
(batch, head)) its term drops and the derived term stands alone.  decoder_cases.TOL of the group's largest value sits on top
(of dv's for a group that is exactly zero in float64: L = 1), for every group but those of RESIDUE_GROUPS: stress cases' groups
whose largest value is below RESIDUE of their largest magnitude, what a cancellation left over, which has no scale that fp32
arithmetic, the composition's included, can be held to 1e-4 of.  No case goes without the per-entry bound.
"""
import functools
import os
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_parity as AP                                                    # noqa: E402
import parity_measure as PM                                                 # noqa: E402
from parity_measure import U                                                # noqa: E402

TOL = AP.TOL
TILE = AP.TILE
D = AP.DEC_D
NEG = AP.NEG
BHS = AP.BHS
GROUPS = ("lse", "dq", "dk", "dv")
STRESS = AP.STRESS                          # on L = 130 without a mask, built as attn_parity._qk builds them
STRESS_OWN = ("late", "large")              # tests/test_decoder_train_gpu.py's late-maximum and +-1e4-score inputs, v and g dyadic
RESIDUE = 1e-6
# The groups that go without the project's TOL on top, by case: every one is a stress case's, and residue_groups() asserts that
# each is below RESIDUE of its largest magnitude and that no other group of any case is.  late: p is one-hot to 1e-7 and
# dp - delta cancels to 1e-9 of its terms.  large: the keys that carry all the probability have the same k, so dq = k sum_j ds_ij
# cancels to float64's own rounding while its summands are 100 times dv's size (k is 100 times v): neither the residue nor dv
# is a scale for it (the correct fp32 emulation is 1.1e-4 of dv's largest value off there: 98 summands of size 3 in fp32).
RESIDUE_GROUPS = {
    "L130/late/1x1": ("dq", "dk"), "L130/late/2x3": ("dq", "dk"),
    "L130/large/1x1": ("dq",), "L130/large/2x3": ("dq",),
}
# +-1e4 scores: lse = 1e4 + log(n+), n+ the number of keys with the positive score, is ONE fp32 number per query (the ABI); fp32's
# spacing at 1e4 is 2^-10, so a random n+ leaves a rounding of up to 4.9e-4 that exp(s - lse) turns into a common relative error
# of every probability of the (batch, head).  The per-entry bound allows it (the L_i term of R_i); TOL = 1e-4 of the group's
# largest value cannot, for any kernel with this ABI (include/biattn_hip.h records the limit; vit_bwd_parity's docstring has the
# same finding).  So that TOL can stay on dk and dv of this case, the number of positive keys is FIXED to the n+ <= 130 for
# which 1e4 + log(n+) lies closest to a multiple of 2^-10 (large_positive_keys(), from the number format alone); which keys
# they are is still seeded.
LARGE_L = 130


def large_positive_keys(L=LARGE_L):
    """(n+, |1e4 + log n+ - the nearest multiple of 2^-10|) with the smallest distance over 2 <= n+ < L"""
    n = np.arange(2, L)
    x = (1e4 + np.log(n)) * 1024.0
    d = np.abs(x - np.round(x)) / 1024.0
    return int(n[np.argmin(d)]), float(d.min())


# ------------------------------------------------------------------------------------------------------------------- the cases

CASES = {}


def _add(name, **spec):
    assert name not in CASES, name
    spec.setdefault("stress", None)
    spec.setdefault("pattern", None)
    CASES[name] = spec


def _both(L, tag, **spec):
    for _B, _H in BHS:
        _add("L%d/%s/%dx%d" % (L, tag, _B, _H), L=L, B=_B, heads=_H, **spec)


# lengths: 1 gives dq = dk = 0 exactly with a positive magnitude; L <= 32 leaves wave 1 without a tile; 65 and 130 give wave 1
# fewer tiles than wave 0 (2 + 1, 3 + 2); 33 and 65 put one row in the tail tile and in the tail workgroup (AP.DEC_LENS)
for _L in AP.DEC_LENS:
    for _kind in ("none", "bool", "f32"):
        _both(_L, _kind, mask=_kind, pattern=None if _kind == "none" else "random", group="len")
# mask patterns, bool and as -inf f32
PATTERNS = (
    ("dn", (65, 130)),          # leading tiles wholly excluded for the matching queries; 65: the smallest with a whole dead tile
    ("last_open", (65, 130)),   # only key L - 1: wave 0 has no live tile in bwd_q; every bwd_kv workgroup but the last stores zeros
    ("first_open", (65, 130)),  # only key 0: wave 1 has no live tile in bwd_q; 130: wave 1 owns two dead tiles
    ("one_pair", (65, 97)),     # one streamed tile with ONE open pair, on a lane with half == 1 and r32 != 0, in both passes;
                                # 65: the tile is wave 0's in both passes; 97: wave 0's in bwd_q, wave 1's in bwd_kv
    ("closed_key", (65, 97)),   # key 37 is attended by no query: dk = dv = 0 exactly in one row of a live workgroup
    ("closed_tile", (65, 97)),  # keys 32..63 are attended by no query: that bwd_kv workgroup skips every tile and stores zeros
)
for _pat, _Ls in PATTERNS:
    for _L in _Ls:
        for _kind in ("bool", "f32"):
            _both(_L, "%s_%s" % (_kind, _pat), mask=_kind, pattern=_pat, group="pattern")
# finite float masks, no -inf.  asym: m[i, j] != m[j, i] almost everywhere, catches a transposed read or a float mask read as
# open / closed; 65: the smallest with both waves busy and a tail, 97: two tiles per wave.  near_sym: symmetric but for ONE pair
# that differs by 2^-10, at a key that three queries attend to: the transposed read that a one-number measure lets through.
for _L in (65, 97):
    _both(_L, "f32_asym", mask="f32", pattern="asym", group="float")
_both(65, "f32_near_sym", mask="f32", pattern="near_sym", group="float")
# dead queries, on the random masks
DEAD = (
    ("row45", 97),          # one dead query inside a live tile of wave 0's range of the key pass
    ("last_row", 65),       # the only row of the tail tile and the tail workgroup; wave 1's only tile of the key pass is all dead
    ("dead_tile", 97),      # rows 32..63: bwd_kv skips that query tile, that bwd_q workgroup has no live tile and stores NaN only
    ("row70", 97),          # a dead query in wave 1's streamed range of the key pass (tiles 2 and 3)
)
for _pat, _L in DEAD:
    for _kind in ("bool", "f32"):
        _both(_L, "%s_%s" % (_kind, _pat), mask=_kind, pattern=_pat, group="dead")
# stress, L = 130 (five tiles, 3 + 2) without a mask
for _s in STRESS + STRESS_OWN:
    _both(130, _s, mask="none", stress=_s, group="stress")
# bh -> (b, h) by division, at the smallest L with two workgroups
for _B, _H in ((7, 1), (1, 7)):
    for _kind in ("none", "bool", "f32"):
        _add("L33/%s/%dx%d" % (_kind, _B, _H), L=33, B=_B, heads=_H, mask=_kind, pattern=None if _kind == "none" else "random", group="bh")

ONE_PAIR = {65: (32 + 13, 22), 97: (64 + 13, 32 + 22)}     # (query, key): rows 13 and 22 of their tiles, both with row % 8 >= 4
CLOSED_KEY = 37
NEAR_SYM = dict(key=40, queries=(5, 40, 50), pair=(5, 40), value=-2.0)


def names(**want):
    return [n for n, c in CASES.items() if all(c[k] == v for k, v in want.items())]


def _as_f32_mask(m):
    return torch.zeros(m.shape, dtype=torch.float64).masked_fill(m, NEG)


@functools.lru_cache(maxsize=None)
def mask_of(L, kind, pattern):
    """None, [L, L] bool (True = excluded) or float64 (added; dyadic finite values and -inf)."""
    if kind == "none":
        return None
    ap = lambda k, p=None: AP.dec_mask("dec/L%d/%s%s/1x1" % (L, k, "_" + p if p else "")).clone()
    if pattern == "random" or (pattern in ("dn", "last_open", "row45") and "dec/L%d/%s_%s/1x1" % (L, kind, pattern) in AP.CASES):
        return ap(kind, None if pattern == "random" else pattern)
    if pattern in ("asym", "near_sym"):
        assert kind == "f32"
        r = PM.rng("dec_bwd/mask/%s/%d" % (pattern, L))
        m = np.clip(PM.dy(r.randn(L, L), 3.0).astype(np.float64), -8.0, 8.0)
        if pattern == "near_sym":
            m = np.triu(m) + np.triu(m, 1).T
            c, rows, (pi, pj) = NEAR_SYM["key"], NEAR_SYM["queries"], NEAR_SYM["pair"]
            keep = np.zeros(L, bool)
            keep[list(rows)] = True
            m[~keep, c] = NEG
            m[c, ~keep] = NEG
            m[pj, pi] = NEAR_SYM["value"]
            m[pi, pj] = m[pj, pi] + 2.0 ** -10
        return torch.from_numpy(m)
    if pattern in ("last_row", "dead_tile", "row70"):
        m = ap(kind)
        rows = {"last_row": [L - 1], "dead_tile": list(range(32, 64)), "row70": [70]}[pattern]
        m[rows] = True if kind == "bool" else NEG
        return m
    # the bool patterns, and their -inf form
    if pattern == "first_open":
        m = torch.ones(L, L, dtype=torch.bool)
        m[:, 0] = False
    elif pattern == "one_pair":
        i, j = ONE_PAIR[L]
        m = torch.zeros(L, L, dtype=torch.bool)
        m[i // TILE * TILE:i // TILE * TILE + TILE, j // TILE * TILE:j // TILE * TILE + TILE] = True
        m[:, j] = True                      # key j is attended by query i alone
        m[i, j] = False
    elif pattern == "closed_key":
        m = ap("bool")
        m[:, CLOSED_KEY] = True
    else:
        assert pattern == "closed_tile", pattern
        m = ap("bool")
        m[:, 32:64] = True
    return m if kind == "bool" else _as_f32_mask(m)


def dead_rows(mask):
    """the queries with every key excluded"""
    if mask is None:
        return ()
    closed = mask if mask.dtype == torch.bool else mask == NEG
    return tuple(int(i) for i in torch.nonzero(closed.all(1)).flatten())


def delta_bytes(B, heads, L):
    """dec_attn_bwd.hip's delta_bytes: B heads roundup(L, 32) floats, rounded up to 256 bytes, at least 256"""
    return max(256, -(-(B * heads * (-(-L // TILE) * TILE) * 4) // 256) * 256)


@functools.lru_cache(maxsize=32)
def inputs(name):
    """{q, k, v, g [B, L, heads 32] float64 dyadic tensors, mask, scale, dead}; left unchanged."""
    c = CASES[name]
    gen = torch.Generator().manual_seed(zlib.crc32(("dec_bwd/" + name).encode()))
    B, heads, L, stress = c["B"], c["heads"], c["L"], c["stress"]
    E = heads * D
    scale = AP.fp32_scale(D)
    if stress in STRESS_OWN:
        q, k = torch.zeros(B, L, heads, D, dtype=torch.float64), torch.zeros(B, L, heads, D, dtype=torch.float64)
        if stress == "late":            # every query's largest score is its last key's, 16 above the next
            q[..., 0] = 4.0
            k[:, 0, :, 0] = 8.0
            k[:, L - 1, :, 0] = 40.0
            scale = 0.125
        else:                           # scores of +-1e4, n+ of them positive (large_positive_keys), at seeded keys
            n_pos, _ = large_positive_keys(L)
            q[..., 0] = 100.0
            for b in range(B):
                for h in range(heads):
                    k[b, :, h, 0] = -100.0
                    k[b, torch.randperm(L, generator=gen)[:n_pos], h, 0] = 100.0
            scale = 1.0
        q, k = q.reshape(B, L, E), k.reshape(B, L, E)
    else:
        q, k = AP._qk(gen, B, L, L, heads, D, stress, "k", 3.0)
    v = AP.dyadic(torch.randn(B, L, E, generator=gen))
    g = AP.dyadic(torch.randn(B, L, E, generator=gen))
    mask = mask_of(L, c["mask"], c["pattern"])
    if c["pattern"] == "one_pair":      # the pair's score is far below the query's others: a probability of 1e-7 or so
        i, j = ONE_PAIR[L]
        k[:, j] = -2.0 * q[:, i]
    x = dict(q=q, k=k, v=v, g=g, mask=mask, scale=scale, dead=dead_rows(mask))
    for key in ("q", "k", "v", "g"):
        x[key] = x[key] + 0.0                                   # rounding to the dyadic grid leaves -0.0 behind: +0.0
        assert torch.equal(x[key].float().double(), x[key]) and PM.is_dyadic(x[key].numpy()), (name, key)
    if mask is not None and mask.dtype == torch.float64:
        fin = mask[torch.isfinite(mask)].numpy()
        assert PM.is_dyadic(fin) and not bool(torch.isnan(mask).any()) and not bool((mask == float("inf")).any()), (name, "mask")
    assert float(np.float32(scale)) == scale
    return x


def mask_property(name):
    """Asserts, on the mask, the property that names a pattern case."""
    c, x = CASES[name], inputs(name)
    L, pat, m = c["L"], c["pattern"], x["mask"]
    if m is None:
        return
    closed = (m if m.dtype == torch.bool else m == NEG).numpy()
    op = ~closed
    dead = closed.all(1)
    assert tuple(np.nonzero(dead)[0]) == x["dead"]
    tiles = -(-L // TILE)
    tile_open = np.array([[op[a * TILE:(a + 1) * TILE, b * TILE:(b + 1) * TILE].sum() for b in range(tiles)] for a in range(tiles)])
    if pat == "random":
        assert not dead.any() and op.any(0).all()
    elif pat == "dn":
        assert not dead.any() and (tile_open == 0).any(), (name, "a wholly excluded tile")
    elif pat == "last_open":
        assert op[:, L - 1].all() and op.sum() == L
    elif pat == "first_open":
        assert op[:, 0].all() and op.sum() == L
    elif pat == "one_pair":
        i, j = ONE_PAIR[L]
        assert tile_open[i // TILE, j // TILE] == 1 and op[i, j] and op[:, j].sum() == 1 and not dead.any()
        assert (i % TILE) % 8 >= 4 and (j % TILE) % 8 >= 4 and i % TILE != 0 and j % TILE != 0, (name, "lanes with half == 1, r32 != 0")
    elif pat == "closed_key":
        assert not op[:, CLOSED_KEY].any() and not dead.any() and (op.any(0).sum() == L - 1)
    elif pat == "closed_tile":
        assert not op[:, 32:64].any() and not dead.any() and op.any(0).sum() == L - 32
    elif pat == "asym":
        mm = m.numpy()
        assert np.isfinite(mm).all() and np.abs(mm).max() <= 8.0
        off = ~np.eye(L, dtype=bool)
        assert (mm != mm.T)[off].mean() > 0.99, (name, "m[i, j] != m[j, i] almost everywhere")
    elif pat == "near_sym":
        mm = m.numpy()
        differ = np.argwhere(mm != mm.T)
        pi, pj = NEAR_SYM["pair"]
        assert sorted(map(tuple, differ.tolist())) == sorted([(pi, pj), (pj, pi)]) and mm[pi, pj] - mm[pj, pi] == 2.0 ** -10
        assert tuple(np.nonzero(op[:, NEAR_SYM["key"]])[0]) == NEAR_SYM["queries"] and not dead.any()
    else:
        want = {"row45": [45], "last_row": [L - 1], "dead_tile": list(range(32, 64)), "row70": [70]}[pat]
        assert list(x["dead"]) == want, name
        per_wave = -(-tiles // 2)
        if pat == "row70":
            assert 70 // TILE >= per_wave, (name, "wave 1's streamed range of the key pass")


# -------------------------------------------------------------------------------------------------------------- the restatement

def scores(name):
    """(s, amp) [B, H, L, L] float64 of a case: attn_parity.dec_scores"""
    c, x = CASES[name], inputs(name)
    return AP.dec_scores(AP._np(x["q"]), AP._np(x["k"]), c["heads"], AP._npmask(x["mask"]), x["scale"])


def restate(name):
    """{group: (value, mag)}: lse [B heads, L]; dq, dk, dv [B, L, heads 32].  A dead query's lse is -inf and its dq row NaN,
    both with magnitude 0."""
    c, x = CASES[name], inputs(name)
    B, heads, L, scale = c["B"], c["heads"], c["L"], x["scale"]
    s, amp = scores(name)
    op = np.isfinite(s)
    qs, k, v, g = (AP._split(a, heads) for a in (AP._scaled(AP._np(x["q"]), scale), AP._np(x["k"]), AP._np(x["v"]), AP._np(x["g"])))
    dead = np.zeros(L, bool)
    dead[list(x["dead"])] = True
    assert np.array_equal(~op.any(-1), np.broadcast_to(dead, s.shape[:-1])), name
    T_ = lambda a: a.transpose(0, 1, 3, 2)

    m = np.where(dead, 0.0, s.max(-1))[..., None]
    e = np.exp(s - m)                                           # an excluded pair: exp(-inf) = 0
    l = e.sum(-1, keepdims=True)
    with np.errstate(divide="ignore"):
        lse = np.where(dead, NEG, (m + np.log(l))[..., 0])
    p = e / np.where(l > 0, l, 1.0)                             # a dead query: p = 0, it enters nothing below
    delta = (g * (p @ v)).sum(-1)
    diff = g @ T_(v) - delta[..., None]
    ds = p * diff
    dv, dk, dq = T_(p) @ g, T_(ds) @ qs, scale * (ds @ k)

    A = np.where(op, amp, 0.0).max(-1)
    Ls = np.maximum(np.where(dead, 0.0, np.abs(lse)), np.where(op, np.abs(s), 0.0).max(-1))
    R = 1.0 + 2.0 * A + 3.0 * Ls
    Rp = R[..., None] * p
    P = np.abs(g) @ T_(np.abs(v))
    Delta = (np.abs(g) * ((1.0 + 2.0 * A)[..., None] * (p @ np.abs(v)))).sum(-1)
    Tm = Rp * np.abs(diff) + p * (P + Delta[..., None])
    m_dv, m_dk, m_dq = T_(Rp) @ np.abs(g), T_(Tm) @ np.abs(qs), scale * (Tm @ np.abs(k))
    m_lse = np.where(dead, 0.0, 1.0 + A + np.where(dead, 0.0, np.abs(lse)))

    dq, m_dq = AP._merge(dq), AP._merge(m_dq)
    dq[:, dead] = np.nan
    m_dq[:, dead] = 0.0
    out = {"lse": (lse.reshape(B * heads, L), m_lse.reshape(B * heads, L)), "dq": (dq, m_dq),
           "dk": (AP._merge(dk), AP._merge(m_dk)), "dv": (AP._merge(dv), AP._merge(m_dv))}
    for key, (val, mag) in out.items():
        fin = np.isfinite(val)
        assert np.isfinite(mag).all() and (mag[fin] >= np.abs(val[fin])).all(), (name, key, "the magnitude is at least the value")
        gone = np.zeros(val.shape, bool)
        if key in ("lse", "dq"):
            gone[:, dead] = True
        assert np.array_equal(~fin, gone) and (mag[gone] == 0).all(), (name, key, "only a dead query's lse and dq are not finite")
    return out


@functools.lru_cache(maxsize=8)
def reference(name):
    """{group: (value, mag)} of a case: computed once, shared, left unchanged."""
    return restate(name)


def _torch_inputs(name, device="cpu"):
    """fp32 (qk [B, L, 2 E], v, mask, g) as decoder_train_cases takes them"""
    x = inputs(name)
    m = x["mask"]
    m = None if m is None else (m if m.dtype == torch.bool else m.float()).to(device)
    return torch.cat([x["q"], x["k"]], -1).float().to(device), x["v"].float().to(device), m, x["g"].float().to(device)


def agrees_with_autograd(name):
    """The restatement's gradients against decoder_train_cases.reference_grads (float64 autograd of core64 on the same fp32
    inputs; a dead query's upstream gradient zeroed) to 1e-12 of each group's largest value (of dv's for an exactly-zero group
    and for a residue group); the lse against torch.logsumexp of float64 scores formed with torch.  dq over the live queries."""
    import decoder_train_cases as T
    c, x = CASES[name], inputs(name)
    B, heads, L = c["B"], c["heads"], c["L"]
    qk, v, mask, g = _torch_inputs(name)
    auto, _ = T.reference_grads(qk, v, heads, mask, g, x["scale"], dead=x["dead"])
    auto = {k: t.numpy() for k, t in auto.items()}
    split = lambda t: t.double().reshape(B, L, heads, D).permute(0, 2, 1, 3)
    s = split((x["q"].float() * np.float32(x["scale"]))) @ split(x["k"]).transpose(-1, -2)
    if mask is not None:
        s = s.masked_fill(mask, NEG) if mask.dtype == torch.bool else s + mask.double()
    auto["lse"] = torch.logsumexp(s, -1).reshape(B * heads, L).numpy()
    mine = restate(name)
    assert sorted(auto) == sorted(mine) == sorted(GROUPS), name
    live = np.ones(L, bool)
    live[list(x["dead"])] = False
    dv = np.abs(auto["dv"]).max()
    for k, want in auto.items():
        val, mag = mine[k]
        if k == "lse":
            assert np.array_equal(want == NEG, val == NEG), (name, k)
            want, val = want[:, live], val[:, live]
        elif k == "dq":
            assert (want[:, ~live] == 0).all() and np.isnan(val[:, ~live]).all(), (name, k)
            want, val = want[:, live], val[:, live]
        size = np.abs(want).max() if want.size else 0.0
        if size <= 1e-12 * dv or size < RESIDUE * mag.max():
            assert k != "dv"
            size = dv
        assert want.size == 0 or np.abs(val - want).max() <= 1e-12 * size, (name, k, np.abs(val - want).max(), size)


def residue_groups(name):
    """The groups of a case whose largest value is below RESIDUE of their largest magnitude (vit_bwd_parity's rule).  In a
    stress case they must be RESIDUE_GROUPS' entry; in any other case such a group is exactly zero (one open key per query,
    L = 1 or first_open / last_open: p = 1, dp = delta), below 1e-12 of dv's largest value, keeps TOL of dv's scale on top,
    and is not returned."""
    got = []
    for k, (val, mag) in reference(name).items():
        size = np.where(np.isfinite(val), np.abs(val), 0.0).max()
        if 0 < mag.max() and size < RESIDUE * mag.max():
            got.append(k)
    if CASES[name]["group"] != "stress":
        assert name not in RESIDUE_GROUPS
        for k in got:
            assert np.abs(reference(name)[k][0]).max() <= 1e-12 * np.abs(reference(name)["dv"][0]).max(), (name, k)
            assert CASES[name]["L"] == 1 or CASES[name]["pattern"] in ("last_open", "first_open"), (name, k, "one open key per query")
        return ()
    assert tuple(got) == RESIDUE_GROUPS.get(name, ()), (name, got)
    return tuple(got)


def stress_property(name):
    """Asserts, on the float64 scores, the property that names a stress case."""
    c = CASES[name]
    s = scores(name)[0]
    n = s.shape[-1]
    kind = c["stress"]
    if kind in ("ascending", "descending"):     # every tile's largest score above (below) every earlier tile's, for every query
        pad = (-n) % TILE
        tmax = np.concatenate((s, np.full(s.shape[:-1] + (pad,), -np.inf)), -1).reshape(s.shape[:-1] + (-1, TILE)).max(-1)
        assert tmax.shape[-1] >= 5, (name, "many tiles")
        d = np.diff(tmax, axis=-1)
        assert (d > 0).all() if kind == "ascending" else (d < 0).all(), name
    elif kind == "flat":
        assert (s == 0).all(), name
    elif kind == "sharp":
        with np.errstate(under="ignore"):
            p = np.exp(s - s.max(-1, keepdims=True))
        assert (p < U).mean() > 0.5, (name, "most probabilities are below fp32's reach of the largest")
    elif kind == "late":                        # the largest score is the last key's, 16 above every other
        assert (s.argmax(-1) == n - 1).all() and (s[..., n - 1:] - s[..., :n - 1] >= 16).all(), name
    else:
        n_pos, dist = large_positive_keys(n)
        assert kind == "large" and (np.abs(s) == 1e4).all() and ((s > 0).sum(-1) == n_pos).all() and dist < 1e-5, (name, n_pos, dist)


# ------------------------------------------------------------------------------------------------------------- the composition

def composition(name, device="cpu"):
    """{group: float64 numpy} of the fp32 PyTorch composition on `device` (decoder_train_cases.composition32 under autograd,
    its lse torch.logsumexp of the same fp32 scores); it never runs the kernels.  A dead query makes its (batch, head) NaN."""
    import decoder_train_cases as T
    c, x = CASES[name], inputs(name)
    B, heads, L, scale = c["B"], c["heads"], c["L"], x["scale"]
    qk, v, mask, g = _torch_inputs(name, device)
    if mask is not None and mask.dtype == torch.bool:       # composition32's own fill, made on the device
        mask = torch.zeros(L, L, dtype=torch.float32, device=device).masked_fill(mask, NEG)
    E = heads * D
    q, k, v = (t.clone().requires_grad_(True) for t in (qk[..., :E], qk[..., E:], v))
    out = T.composition32(q, k, v, heads, mask, scale)
    (out * g).sum().backward()
    got = {"dq": q.grad, "dk": k.grad, "dv": v.grad}
    with torch.no_grad():
        sp = lambda t: t.reshape(B, L, heads, D).permute(0, 2, 1, 3).reshape(B * heads, L, D)
        qh, kh = sp(q * scale), sp(k)
        w = torch.bmm(qh, kh.transpose(1, 2)) if mask is None else torch.baddbmm(mask, qh, kh.transpose(1, 2))
        got["lse"] = torch.logsumexp(w, dim=-1)
    for key, t in got.items():
        assert t.dtype == torch.float32, (name, key)
    return {key: t.detach().cpu().double().numpy() for key, t in got.items()}


# ---------------------------------------------------------------------------------------------------------- the error measure

HEAD = "%-28s %-4s %10s %10s %10s %8s" % ("case", "grp", "kernel err", "comp err", "bound", "ratio")
_T = PM.Table(HEAD, env="DEC_BWD_PARITY_TABLE")
TABLE, WORST, report = _T.lines, _T.worst, _T.report        # WORST: group -> (ratio, table line)


def measure(case, what, got, want, mag, comp, check=True):
    """Every entry of `got` within entry_bound(the composition's error at the entry, its magnitude) of `want`, and the project's
    bound on top: TOL of the group's largest value, of dv's for a group that is exactly zero in float64, none for a group of
    RESIDUE_GROUPS.  Returns the largest error / bound; check=False only returns it (inf where the non-finite entries differ
    from the reference's) and adds no line.
    Non-finite: lse is -inf exactly where the reference is (dead queries), dq is NaN exactly there, nothing else is non-finite;
    those entries then leave the arithmetic (their magnitude is 0).  An entry of magnitude 0 (a key no live query attends to,
    dk at q = 0) must be an exact zero of either sign.
    WORST: the group.  Line: case, group, the worst entry's kernel error, composition error and bound, each relative to the
    entry's MAGNITUDE, and their ratio."""
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape == comp.shape == mag.shape, (case, what, got.shape, want.shape, comp.shape, mag.shape)
    out = ~np.isfinite(want)                                    # the dead queries' entries of lse (-inf) and dq (NaN)
    assert (mag >= 0).all() and (mag[out] == 0).all() and (what in ("lse", "dq") or not out.any()), (case, what)
    if what == "lse":
        same = np.array_equal(got == NEG, out) and np.isfinite(got[~out]).all()
    else:
        same = np.array_equal(np.isnan(got), out) and np.isfinite(got[~out]).all()
    zero = (mag == 0) & ~out
    exact = bool((got[zero] == 0).all())
    if check:
        assert same, (case, what, "non-finite entries", np.argwhere(~np.isfinite(got) != out)[:8].tolist())
        assert exact, (case, what, "an entry of magnitude 0 is not an exact zero", np.argwhere(zero & (got != 0))[:8].tolist())
    elif not (same and exact):
        return float("inf")
    fin = lambda a: np.where(out, 0.0, a)
    e = PM.errors(fin(got), fin(want), mag, np.where(out, 0.0, comp))
    if not check:
        return e.worst
    i = e.at
    unit = mag[i] or 1.0
    _T.add("%-28s %-4s %10.2e %10.2e %10.2e %8.3f" % (case, what, e.err[i] / unit, e.cerr[i] / unit, e.bound[i] / unit, e.ratio[i]),
           what, e.worst)
    e.check(case, what)
    if what in RESIDUE_GROUPS.get(case, ()):
        assert CASES[case]["group"] == "stress" and float(e.size.max()) < RESIDUE * float(mag.max()), (case, what)
        return e.worst              # what a cancellation left over: no scale to take TOL of, the per-entry bound stands alone
    size = float(e.size.max())
    dv = float(np.abs(reference(case)["dv"][0]).max())
    if what == "lse":
        assert size > 0 or out.all(), (case, what)
    elif size <= 1e-12 * dv:
        size = dv
    assert float(e.err.max()) <= TOL * size, (case, what, "the project's bound", float(e.err.max()), size)
    return e.worst


def group_err(got, want, live=None):
    """decoder_train_cases.group_err in numpy: per gradient group, max abs error over the group's max abs (dv's for an exactly
    zero group); the measure tests/test_decoder_train_gpu.py holds every group to.  dq over the live queries."""
    errs = {}
    pick = lambda k, a: a[:, live] if (k == "dq" and live is not None) else a
    dv = float(np.abs(want["dv"]).max())
    for k in ("dq", "dk", "dv"):
        w, g = pick(k, want[k]), pick(k, got[k])
        scale = float(np.abs(w).max())
        scale = scale if scale > 1e-12 * dv else dv
        with np.errstate(invalid="ignore"):
            d = np.abs(g - w)
        errs[k] = float("inf") if not np.isfinite(d).all() else float(d.max() / scale)
    return errs
