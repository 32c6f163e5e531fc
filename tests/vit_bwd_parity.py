"""Per-entry float64 parity of the ViT attention core's training route (uninext_amd/csrc/vit_attn_bwd.hip: attn_lse, bwd_q,
bwd_kv, dtables, dtables_reduce): the cases, a float64 numpy restatement of the forward's lse and of the backward that returns
every entry's VALUE and its MAGNITUDE, the fp32 PyTorch composition, and the error measure.  No GPU and no built package is
needed to import this.  tests/test_vit_bwd_parity_cpu.py checks that the measure has teeth, tests/test_vit_bwd_parity_gpu.py
holds the kernels to it through the C ABI.

Inputs are seeded by the case's name and dyadic (multiples of 2^-10): fp32 holds exactly what float64 sees.  q is scaled in
fp32 first, by a scale that is a fp32 number; the scores and their summed absolute summands `amp` are attn_parity.vit_scores'.

The restatement is written out analytically (include/patch_embed_hip.h), not through autograd, with g the upstream gradient:
    lse_i = log sum_j exp(s_ij)        p_ij = exp(s_ij - lse_i)        o_i = sum_j p_ij v_j        delta_i = g_i . o_i
    dv_j = sum_i p_ij g_i              ds_ij = p_ij (g_i . v_j - delta_i)                            dk_j = sum_i ds_ij qs_i
    rh_ic = sum_{j: jh = c} ds_ij      rw_ic = sum_{j: jw = c} ds_ij
    dq_i = scale sum_j ds_ij k_j + sum_c rh_ic th[ih - c + Hq - 1] + sum_c rw_ic tw[iw - c + Wq - 1]
    dth[r] = sum_{b, h} sum_{(i, c): ih - c + Hq - 1 = r} rh_ic q_i (unscaled q), dtw likewise with the axes exchanged.
It agrees with vit_train_cases.reference_grads (float64 autograd of vit_ref.core) to 1e-12 of each group's largest value on
every case (agrees_with_autograd): autograd of a float64 qkv scales q in float64, so that comparison runs the restatement
with scaled="f64"; at D = 64 and in the 9x15 stress cases the scale is a power of two and both scalings are the same bits,
which the check asserts, at D = 80 the two restatements differ in that one line.

THE MAGNITUDES, derived; u = 2^-24, and nothing here was fitted to what a kernel gives.  Per (b, h):
  A_i = max_j amp_ij   the summed absolute summands of the query's largest-amplitude score: a fp32 score errs by a multiple
                       of u A_i (attn_parity's docstring).
  L_i = max(|lse_i|, max_j |s_ij|).
  lse: 1 + A_i + |lse_i|.  lse is a weighted mean of the scores plus a log of a sum of terms <= 1: an error e on the scores
       moves it by at most e (A_i), storing it in fp32 rounds by u |lse_i|, and the log and the running sum's own rounding are
       of order u times a number of order 1 (the 1).
  R_i = 1 + 2 A_i + 3 L_i, the relative amplitude of the RECOMPUTED probability exp(s_ij - lse_i): exp passes an absolute error
       of its argument on as a relative error.  The argument's error: the score's own (A_i), the error of lse through the
       forward's scores (A_i again), the fp32 rounding of the stored lse (<= L_i), the rounding of the difference s - lse
       (|s - lse| <= 2 L_i); the 1 is exp's own rounding.
  dv[j, d] = sum_i R_i p_ij |g_id|: every summand p_ij g_id carries p's relative amplitude; the sum's own rounding is part of
       it since R_i >= 1.
  P_ij = sum_d |g_id| |v_jd|, the summands behind dp_ij = g_i . v_j.
  Delta_i = sum_d |g_id| (1 + 2 A_i) sum_j p_ij |v_jd|: delta is computed from the kernel's own fp32 `out`, whose entry d errs
       by u times the forward sweep's magnitude (1 + 2 A_i) sum_j p_ij |v_jd| (attn_parity's docstring); that magnitude is at
       least |o_id|, so the rounding of the sum g . o itself is covered.
  T_ij = p_ij (R_i |dp_ij - delta_i| + P_ij + Delta_i): ds_ij = p_ij (dp_ij - delta_i) is a product of p (relative amplitude
       R_i) and a difference whose two terms err by u P_ij and u Delta_i.  To first order its error is p's error times the
       difference, R_i p_ij |dp_ij - delta_i|, plus p_ij times the difference's error, p_ij (P_ij + Delta_i); the product's
       own rounding is inside the first (R_i >= 1).  The second term keeps the cancellation p (dp - delta) honest: the entry
       may be small, its magnitude is not.  (Bounding |dp - delta| by P + Delta instead would give R_i p_ij (P_ij + Delta_i),
       which is also derived but R_i times looser wherever the scores are large; the first-order form is kept.)
  dk[j, d] = sum_i T_ij |qs_id|.
  dq[i, d] = scale sum_j T_ij |k_jd| + sum_c Th_ic |th[ih - c + Hq - 1, d]| + sum_c Tw_ic |tw[iw - c + Wq - 1, d]| with
       Th_ic = sum_{j: jh = c} T_ij and Tw_ic = sum_{j: jw = c} T_ij, the magnitudes of the bins rh and rw (plain sums of ds).
  dth[r, d] = sum_{b, h} sum_{(i, c): ih - c + Hq - 1 = r} Th_ic |q_id|, dtw the same with Tw.  The table sums run in float64
       and are rounded once: only the bins' own errors remain.
A group that is exactly zero in float64 arithmetic (dth at q_h = 1, dtw at q_w = 1: one bin holds sum_j ds_ij = 0; dq and dk
at S = 1: p = 1 and dp = delta) still has a positive magnitude: the kernel's dp and delta are two fp32 sums of the same
products in different orders.  Such a group is held to a bound of its own, 16 u of that magnitude or 8 x the composition's
error.  (The float64 VALUE of such an entry is float64's own rounding noise, 1e-17 or so; the table therefore prints errors
relative to the entry's magnitude, not to its value.)

An entry is held to parity_measure.entry_bound: max(COMP_MARGIN x the fp32 composition's error at the entry, SUM_DEPTH u x the
magnitude).  The project's bound sits on top: vit_cases.TOL of the group's largest value (of dv's for a group that is exactly
zero, as vit_train_cases.group_err has it; none for a 9x15 stress case's group that is a cancellation's residue: RESIDUE below).
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
import vit_cases as VC                                                      # noqa: E402
from parity_measure import COMP_MARGIN, SUM_DEPTH, U, entry_bound          # noqa: E402,F401

TOL = VC.TOL
TILE = AP.TILE
DS = (64, 80)
BHS = AP.BHS                                # batch x heads of every shape unless noted
GROUPS = ("lse", "dq", "dk", "dv", "dth", "dtw")
STRESS = AP.STRESS                          # on 20x23, with tables, built as attn_parity._qk builds them
STRESS_9X15 = ("late", "flat0", "large")    # on 9x15 without tables: tests/test_vit_train_gpu.py's inputs, v made dyadic

# (q_h, q_w) and the hazard each is the smallest to reach
SHAPES = ((1, 1),       # one key: p = 1, dq = dk = 0 exactly, one wave with one query
          (1, 2),       # one width bin per lane half (both halves zero and store bins c = half, half + 2, ..)
          (1, 3),       # an odd number of width bins: half 0 owns two, half 1 one
          (4, 8),       # S = 32: one full tile, no tail anywhere
          (3, 11),      # S = 33: a one-key tail tile, a second wave owning one query
          (8, 16),      # S = 128: exactly one workgroup; two key rows per tile
          (3, 43),      # S = 129: a second workgroup owning one query
          (2, 32),      # a key row ends exactly on the tile boundary: the height bin closes at a tile's first key
          (5, 64),      # a key row spans two tiles: the running height bin is carried across tiles
          (40, 1),      # q_w = 1: the div_w branch without the magic number, every key starts a new height bin
          (1, 40),      # q_h = 1: the height bin is stored only by the epilogue
          (14, 14),     # a key tail of 4 in the 7th tile, a query tail in the second workgroup
          (20, 23))     # four workgroups per head, rows ending mid-tile
CHUNK_HW = (3, 5)
CHUNK_BHS = ((16, 1),   # NC = 16, one bh per chunk: the last BH without a second round
             (17, 1),   # chunk 0 owns bh 0 and 16, the others one
             (1, 17),   # the same over heads: bh -> (b, h) by division
             (11, 3))   # BH = 33: chunk 0 owns three, the others two; b and h both move inside a chunk
K_CHUNKS = 16
# agrees_with_autograd: a group whose largest value is below this fraction of its largest magnitude is what a cancellation left
# over, in float64 autograd as much as here (both are good to 2^-53 of the uncancelled terms, not of the residue), and like an
# exactly-zero group it has no scale of its own to take 1e-12 of: dv's scale stands in.  Only the late-maximum stress cases'
# dq and dk are such groups (p is one-hot to 1e-7, dp - delta cancels to 1e-9 of its terms), and the +-1e4-score cases' dq (the
# keys that carry all the probability have the same k: sum_j ds_ij k_j = 0 exactly).  measure() puts no project's bound on top
# of such a group of the 9x15 stress cases for the same reason: neither the residue nor dv (k is 100 times v's size there) is
# a scale that fp32 arithmetic, the composition's included, can be held to 1e-4 of.  The per-entry bound stands alone there.
# The +-1e4-score cases' gradients get no project's bound on top at all: lse is ONE fp32 number per query (the ABI), at
# |lse| = 1e4 its rounding is 5e-4, and exp(s - lse) carries that as a relative error of every probability -- the L_i term of
# R_i.  The emulation's dk is 4.5e-4 of the group's largest value off there, by construction of the scheme, not by a slip.
RESIDUE = 1e-6


# ------------------------------------------------------------------------------- what the host of the kernels computes

def chunks(BH):
    """NC of dtables: min(BH, 16); chunk c sums bh = c, c + NC, .."""
    return min(BH, K_CHUNKS) if BH else 1


def pitch(D):
    """floats per LDS tile row: D rounded up to 32, plus 4"""
    return -(-D // 32) * 32 + 4


def bwd_q_lds_bytes(D, q_w):
    """the launcher's expression: 4 waves x [q_w][32] width bins and two tiles of 32 rows"""
    return 4 * q_w * TILE * 4 + 2 * TILE * pitch(D) * 4


def needs_opt_in(D, q_w):
    return bwd_q_lds_bytes(D, q_w) > 64 * 1024


def last_static_w(D):
    """the largest q_w launched without the large-LDS opt-in"""
    return max(w for w in range(1, 257) if not needs_opt_in(D, w))


def align256(n):
    return -(-n // 256) * 256


def workspace_layout(B, heads, Hq, Wq, D):
    """(offsets of rel, drel, delta, part; total bytes) of the backward's workspace: rel | drel | delta | part"""
    S = Hq * Wq
    SP, BH = -(-S // TILE) * TILE, B * heads
    rel = align256(BH * (Hq + Wq) * SP * 4)
    part = 2 * rel + align256(BH * SP * 4)
    total = part + align256(chunks(BH) * (2 * Hq - 1 + 2 * Wq - 1) * D * 8)
    return (0, rel, 2 * rel, part), max(total, 256)


# ------------------------------------------------------------------------------------------------------------------- the cases

CASES = {}


def _add(name, **spec):
    assert name not in CASES, name
    CASES[name] = spec


def _name(D, hw, tag, B, H):
    return "D%d/%dx%d/%s/%dx%d" % (D, hw[0], hw[1], tag, B, H)


for _D in DS:
    for _hw in SHAPES:
        for _rel in (True, False):
            for _B, _H in BHS:
                _add(_name(_D, _hw, "rel" if _rel else "norel", _B, _H), D=_D, hw=_hw, B=_B, heads=_H, rel=_rel, stress=None, group="shape")
    for _w in (last_static_w(_D), last_static_w(_D) + 1):       # both sides of the large-LDS opt-in, from the launcher's expression
        for _B, _H in BHS:
            _add(_name(_D, (1, _w), "rel", _B, _H), D=_D, hw=(1, _w), B=_B, heads=_H, rel=True, stress=None, group="lds")
    _add(_name(_D, (2, 256), "rel", 1, 1), D=_D, hw=(2, 256), B=1, heads=1, rel=True, stress=None, group="lds")     # the route's limit
    for _B, _H in CHUNK_BHS:
        _add(_name(_D, CHUNK_HW, "rel", _B, _H), D=_D, hw=CHUNK_HW, B=_B, heads=_H, rel=True, stress=None, group="chunk")
    for _B, _H in BHS:
        for _s in STRESS:
            _add(_name(_D, (20, 23), _s, _B, _H), D=_D, hw=(20, 23), B=_B, heads=_H, rel=True, stress=_s, group="stress")
        for _s in STRESS_9X15:
            _add(_name(_D, (9, 15), _s, _B, _H), D=_D, hw=(9, 15), B=_B, heads=_H, rel=False, stress=_s, group="stress")


def names(**want):
    return [n for n, c in CASES.items() if all(c[k] == v for k, v in want.items())]


@functools.lru_cache(maxsize=32)
def inputs(name):
    """{qkv [B, S, 3 heads D], th, tw (or None), g [B, S, heads D], scale}: float64 dyadic tensors; left unchanged."""
    c = CASES[name]
    gen = torch.Generator().manual_seed(zlib.crc32(("vit_bwd/" + name).encode()))
    B, heads, D, (Hq, Wq), stress = c["B"], c["heads"], c["D"], c["hw"], c["stress"]
    S = Hq * Wq
    scale = AP.fp32_scale(D)
    if stress in STRESS_9X15:
        t = torch.zeros(B, S, 3, heads, D, dtype=torch.float64)
        t[:, :, 2] = AP.dyadic(torch.randn(B, S, heads, D, generator=gen))
        if stress == "late":        # every query's largest score is its last key's, 16 above the next
            t[:, :, 0, :, 0] = 4.0
            t[:, 0, 1, :, 0] = 8.0
            t[:, S - 1, 1, :, 0] = 40.0
            scale = 0.125
        elif stress == "flat0":     # k = 0: every score is 0
            t[:, :, 0, :, 0] = 4.0
            scale = 0.125
        else:                       # scores of +-1e4
            t[:, :, 0, :, 0] = 100.0
            t[:, :, 1, :, 0] = (torch.randint(0, 2, (B, S, heads), generator=gen) * 2 - 1).double() * 100.0
            scale = 1.0
        qkv = t.reshape(B, S, 3 * heads * D)
    else:
        q, k = AP._qk(gen, B, S, S, heads, D, stress, "k", 6.0)
        v = AP.dyadic(torch.randn(B, S, heads * D, generator=gen))
        qkv = torch.stack([t.view(B, S, heads, D) for t in (q, k, v)], 2).reshape(B, S, 3 * heads * D)
    x = dict(qkv=qkv, th=None, tw=None, scale=scale)
    floats = ["qkv", "g"]
    if c["rel"]:
        gain = 0.0625 if stress in ("ascending", "descending") else 0.3
        x["th"] = AP.dyadic(torch.randn(2 * Hq - 1, D, generator=gen), gain)
        x["tw"] = AP.dyadic(torch.randn(2 * Wq - 1, D, generator=gen), gain)
        if stress in ("ascending", "descending"):               # the ramp's constant on q meets no table entry
            x["th"][:, 0] = 0.0
            x["tw"][:, 0] = 0.0
        floats += ["th", "tw"]
    x["g"] = AP.dyadic(torch.randn(B, S, heads * D, generator=gen))
    for key in floats:
        x[key] = x[key] + 0.0                                   # rounding to the dyadic grid leaves -0.0 behind: +0.0
        assert torch.equal(x[key].float().double(), x[key]) and PM.is_dyadic(x[key].numpy()), (name, key)
    assert float(np.float32(scale)) == scale
    return x


# -------------------------------------------------------------------------------------------------------------- the restatement

def _f64_scaled(q, scale):
    return q * scale


def table_rows(hw):
    """(idx_h [S, Hq], idx_w [S, Wq]): the table row of query i and key row / column c"""
    Hq, Wq = hw
    ih, iw = AP.vit_key_hw(hw)
    return ih[:, None] - np.arange(Hq)[None, :] + Hq - 1, iw[:, None] - np.arange(Wq)[None, :] + Wq - 1


def scores(name, scaled="f32"):
    """(s, amp, v) [B, H, S, S] float64 of a case"""
    c, x = CASES[name], inputs(name)
    th, tw = (None, None) if x["th"] is None else (AP._np(x["th"]), AP._np(x["tw"]))
    return AP.vit_scores(AP._np(x["qkv"]), th, tw, c["heads"], c["hw"], x["scale"], AP._scaled if scaled == "f32" else _f64_scaled)


def restate(name, scaled="f32"):
    """{group: (value, mag)}: lse [B heads, S]; dq, dk, dv [B, S, heads D]; dth [2 Hq - 1, D], dtw [2 Wq - 1, D] with tables."""
    c, x = CASES[name], inputs(name)
    B, heads, D, (Hq, Wq), scale = c["B"], c["heads"], c["D"], c["hw"], x["scale"]
    S = Hq * Wq
    s, amp, v = scores(name, scaled)
    t = AP._np(x["qkv"]).reshape(B, S, 3, heads, D)
    q, k = (t[:, :, n].transpose(0, 2, 1, 3) for n in range(2))
    qs = AP._scaled(q, scale) if scaled == "f32" else _f64_scaled(q, scale)
    g = AP._split(AP._np(x["g"]), heads)
    T_ = lambda a: a.transpose(0, 1, 3, 2)

    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    l = e.sum(-1, keepdims=True)
    lse = (m + np.log(l))[..., 0]
    p = e / l
    delta = (g * (p @ v)).sum(-1)
    diff = g @ T_(v) - delta[..., None]
    ds = p * diff
    dv, dk, dq = T_(p) @ g, T_(ds) @ qs, scale * (ds @ k)

    A = amp.max(-1)
    L = np.maximum(np.abs(lse), np.abs(s).max(-1))
    R = 1.0 + 2.0 * A + 3.0 * L
    Rp = R[..., None] * p
    P = np.abs(g) @ T_(np.abs(v))
    Delta = (np.abs(g) * ((1.0 + 2.0 * A)[..., None] * (p @ np.abs(v)))).sum(-1)
    Tm = Rp * np.abs(diff) + p * (P + Delta[..., None])
    m_dv, m_dk, m_dq = T_(Rp) @ np.abs(g), T_(Tm) @ np.abs(qs), scale * (Tm @ np.abs(k))

    out = {"lse": (lse.reshape(B * heads, S), (1.0 + A + np.abs(lse)).reshape(B * heads, S))}
    if c["rel"]:
        th, tw = AP._np(x["th"]), AP._np(x["tw"])
        idx_h, idx_w = table_rows((Hq, Wq))
        bins = lambda a: (a.reshape(B, heads, S, Hq, Wq).sum(-1), a.reshape(B, heads, S, Hq, Wq).sum(-2))
        (rh, rw), (Th, Tw) = bins(ds), bins(Tm)
        dq = dq + np.einsum("bhic,icd->bhid", rh, th[idx_h]) + np.einsum("bhic,icd->bhid", rw, tw[idx_w])
        m_dq = m_dq + np.einsum("bhic,icd->bhid", Th, np.abs(th)[idx_h]) + np.einsum("bhic,icd->bhid", Tw, np.abs(tw)[idx_w])
        for key, idx, r, Tr, rows in (("dth", idx_h, rh, Th, 2 * Hq - 1), ("dtw", idx_w, rw, Tw, 2 * Wq - 1)):
            val, mag = np.zeros((rows, D)), np.zeros((rows, D))
            np.add.at(val, idx, np.einsum("bhic,bhid->icd", r, q))
            np.add.at(mag, idx, np.einsum("bhic,bhid->icd", Tr, np.abs(q)))
            out[key] = (val, mag)
    out.update(dq=(AP._merge(dq), AP._merge(m_dq)), dk=(AP._merge(dk), AP._merge(m_dk)), dv=(AP._merge(dv), AP._merge(m_dv)))
    for key, (val, mag) in out.items():
        assert np.isfinite(val).all() and np.isfinite(mag).all() and (mag >= np.abs(val)).all(), (name, key, "the magnitude is at least the value")
        assert mag.max() > 0 or c["stress"] in ("flat", "flat0"), (name, key, "a positive magnitude (flat: q or k is zero, exact zeros)")
    return out


@functools.lru_cache(maxsize=8)
def reference(name):
    """{group: (value, mag)} of a case: computed once, shared, left unchanged."""
    return restate(name)


def groups_of(name):
    return tuple(k for k in GROUPS if CASES[name]["rel"] or k not in ("dth", "dtw"))


def _autograd(name, th, tw):
    import vit_train_cases as T
    c, x = CASES[name], inputs(name)
    got, _ = T.reference_grads(x["qkv"], th, tw, c["heads"], c["hw"], x["scale"], x["g"])
    B, S = x["g"].shape[:2]
    return {k: (v.reshape(B, S, -1) if k in ("dq", "dk", "dv") else v).numpy() for k, v in got.items()}


def agrees_with_autograd(name):
    """The restatement's gradients against float64 autograd of vit_ref.core on the same float64 qkv, to 1e-12 of each group's
    largest value (of dv's for an exactly-zero group); the lse against torch.logsumexp of vit_ref.scores."""
    import vit_ref
    c, x = CASES[name], inputs(name)
    mine = restate(name, scaled="f64")
    auto = _autograd(name, x["th"], x["tw"])
    auto["lse"] = torch.logsumexp(vit_ref.scores(x["qkv"], x["th"], x["tw"], c["heads"], c["hw"], x["scale"]), -1).reshape(-1, x["g"].shape[1]).numpy()
    assert sorted(auto) == sorted(mine) == sorted(groups_of(name)), name
    dv = np.abs(auto["dv"]).max()
    for k, want in auto.items():
        size = np.abs(want).max()
        if size <= 1e-12 * dv or size < RESIDUE * mine[k][1].max():
            assert k != "dv"
            size = dv
        assert np.abs(mine[k][0] - want).max() <= 1e-12 * size, (name, k, np.abs(mine[k][0] - want).max(), size)
    if c["D"] == 64 or c["stress"] in STRESS_9X15:      # a power-of-two scale: the fp32-scaled restatement is the same bits
        for k, (val, mag) in reference(name).items():
            assert np.array_equal(val, mine[k][0]) and np.array_equal(mag, mine[k][1]), (name, k)


def swapped_tables_differ(name):
    """For q_h != q_w: the restatement with the two tables exchanged (each resized to the other's rows) moves dq, dk and dv far
    outside the project's bound, so a transposed lookup cannot pass.  False for a square shape (nothing to tell apart), for a
    case without tables and for a stress case."""
    import vit_ref
    c, x = CASES[name], inputs(name)
    Hq, Wq = c["hw"]
    if Hq == Wq or not c["rel"] or c["stress"]:     # flat: q = 0 meets no table
        return False
    swapped = _autograd(name, vit_ref.resize_table(x["tw"], 2 * Hq - 1), vit_ref.resize_table(x["th"], 2 * Wq - 1))
    for k in ("dq", "dk", "dv"):
        want = reference(name)[k][0]
        if np.abs(want).max() > 1e-12 * np.abs(reference(name)["dv"][0]).max():     # S = 1 has no dq, dk to move
            assert np.abs(swapped[k] - want).max() > 100 * TOL * np.abs(want).max(), (name, k)
    return True


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
    elif kind in ("flat", "flat0"):
        assert (s == 0).all(), name
    elif kind == "sharp":
        with np.errstate(under="ignore"):
            p = np.exp(s - s.max(-1, keepdims=True))
        assert (p < U).mean() > 0.5, (name, "most probabilities are below fp32's reach of the largest")
    elif kind == "late":                        # the largest score is the last key's, 16 above every other
        assert (s.argmax(-1) == n - 1).all() and (s[..., n - 1:] - s[..., :n - 1] >= 16).all(), name
    else:
        assert kind == "large" and (np.abs(s) == 1e4).all() and (s > 0).any(-1).all() and (s < 0).any(-1).all(), name


# ------------------------------------------------------------------------------------------------------------- the composition

def composition(name, device="cpu"):
    """{group: float64 numpy} of the fp32 PyTorch composition on `device` (vit_ref.composition_fp32 under autograd, its lse
    torch.logsumexp of the same fp32 scores); it never runs the kernels."""
    import vit_train_cases as T
    from uninext_amd.vit import add_decomposed_rel_pos
    c, x = CASES[name], inputs(name)
    heads, hw, scale = c["heads"], c["hw"], x["scale"]
    dev = lambda t: None if t is None else t.float().to(device)
    qkv, th, tw, g = dev(x["qkv"]), dev(x["th"]), dev(x["tw"]), dev(x["g"])
    B, S, _ = qkv.shape
    got = T.composition_grads(qkv, th, tw, heads, hw, scale, g)
    with torch.no_grad():       # the scores as vit_ref.composition_fp32 forms them
        t = qkv.reshape(B, S, 3, heads, -1).permute(2, 0, 3, 1, 4)
        q, k, _ = t.reshape(3, B * heads, S, -1).unbind(0)
        attn = (q * scale) @ k.transpose(-2, -1)
        if th is not None:
            attn = add_decomposed_rel_pos(attn, q, th, tw, hw, hw)
        got["lse"] = torch.logsumexp(attn, dim=-1)
    for k, v in got.items():
        assert v.dtype == torch.float32, (name, k)
    return {k: (v.reshape(B, S, -1) if k in ("dq", "dk", "dv") else v).detach().cpu().double().numpy() for k, v in got.items()}


# ---------------------------------------------------------------------------------------------------------- the error measure

HEAD = "%-34s %-4s %10s %10s %10s %8s" % ("case", "grp", "kernel err", "comp err", "bound", "ratio")
_T = PM.Table(HEAD, env="VIT_BWD_PARITY_TABLE")
TABLE, WORST, report = _T.lines, _T.worst, _T.report        # WORST: group -> (ratio, table line)


def measure(case, what, got, want, mag, comp, check=True):
    """Every entry of `got` within entry_bound(the composition's error at the entry, its magnitude) of `want`, and the project's
    bound on top: TOL of the group's largest value, of dv's for a group that is exactly zero in float64.  Returns the largest
    error / bound; check=False only returns it (inf for a non-finite entry) and adds no line.
    WORST: the group.  Line: case, group, the worst entry's kernel error, composition error and bound, each relative to the
    entry's MAGNITUDE (an exactly-zero group has no value to be relative to), and their ratio."""
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape == comp.shape == mag.shape, (case, what, got.shape, want.shape, comp.shape, mag.shape)
    assert np.isfinite(want).all() and np.isfinite(comp).all() and (mag >= 0).all(), (case, what)
    if not np.isfinite(got).all():
        assert not check, (case, what, "non-finite entries", np.argwhere(~np.isfinite(got))[:8].tolist())
        return float("inf")
    e = PM.errors(got, want, mag, comp)
    if not check:
        return e.worst
    i = e.at
    unit = mag[i] or 1.0
    _T.add("%-34s %-4s %10.2e %10.2e %10.2e %8.3f" % (case, what, e.err[i] / unit, e.cerr[i] / unit, e.bound[i] / unit, e.ratio[i]),
           what, e.worst)
    e.check(case, what)
    size = float(e.size.max())
    dv = float(np.abs(reference(case)["dv"][0]).max())
    if what == "lse":
        assert size > 0, (case, what)
    elif CASES[case]["stress"] == "large" or (CASES[case]["stress"] in STRESS_9X15 and size < RESIDUE * float(mag.max())):
        return e.worst              # what a cancellation left over: no scale to take TOL of, the per-entry bound stands alone
    elif size <= 1e-12 * dv:
        size = dv
    assert float(e.err.max()) <= TOL * size, (case, what, "the project's bound", float(e.err.max()), size)
    return e.worst
