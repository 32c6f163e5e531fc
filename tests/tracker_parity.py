"""Per-entry parity of the online tracker's kernels (uninext_amd/csrc/tracker.hip: memo_embed, feats_rows, cols_final,
associate, update) at their wave, workgroup and ring edges: the cases, the restatements, the fp32 PyTorch composition and the
error measure.  No GPU is needed to import this.  tests/test_tracker_parity_cpu.py checks the input conditions, pins the
restatements to tests/tracker_ref.py and shows that the measure has teeth; tests/test_tracker_parity_gpu.py holds the three
entry points to it through the C ABI.

Banks are built DIRECTLY, field by field (blank_state / the *_inputs functions), not by driving a sequence.  Floats are
multiples of 2^-10 (tests/decoder_cases.py: dyadic), so float64 sees exactly what fp32 holds; the one exception is the temporal
table, whose entries float32((k + 1) / length) are fp32 numbers by definition.  `capacity` is M + n + 3.  Everything of a bank
the contract does not call live -- slots >= M, ring entries >= long_len, `embed` under long_match, the rings without it, the
unused entries of the temporal table -- holds NaN in floats and INT_GARBAGE / LONG_GARBAGE in integers, so any use shows.

scores64: the magnitude.  u = 2^-24; an output's bound is SUM_DEPTH u s (entry_bound of tests/parity_measure.py), s in
units of u, to first order:
  * memo (long_match): w_k = score_k + table_k rounds once, a product ring_kd w_k once, the sum of len terms len - 1 times:
    acc_d carries (len + 2) A_d, A_d = sum_k |ring_kd| w_k.  wsum carries len of itself, the division one more:
        s_memo = (len + 2) A_d / wsum + (len + 1) |memo_d|;     without long_match the memo is `embed`, exact: 0
  * feats_im: a dot product of D terms in any order carries (D + 2) sum_d |e_d| |m_d|, plus what the memo hands on:
        F_im = (D + 2) sum_d |e_d| |m_d| + sum_d |e_d| s_memo_md
  * the row maximum is the exact maximum of the fp32 feats:  s_max_i = max_k F_ik
  * a softmax entry p_j over a set J moves by at most p_j 2 max_J F when its logits move by F (the common shift cancels).
    Its own arithmetic on the fp32 logits: the argument f_j - max rounds once (|f_j - max| relative to t_j = exp(f_j - max)),
    expf is good to 2 u: g_j = |f_j - max| + 2.  The sum S of |J| terms carries sum_j t_j g_j + |J| S, the division one:
        s_p = p_j (2 max_J F + g_j + sum_j t_j g_j / S + |J| + 1),      s_S = S (2 max_J F + sum_j t_j g_j / S + |J|)
    (S is not shift-invariant: its arguments move with the maximum, hence the 2 max F).  J is the M columns for the row
    softmax p and the KEPT rows for the column softmax q.
  * score = (p + q) * 0.5: the sum rounds once, the halving is exact:   s = (s_p + s_q + p + q) / 2
The form is derived, not measured, and no term was fitted.  On top the project's bound 1e-4 max(1, max|ref|) is asserted.
What the measure can and cannot see: s carries the worst-case depth factors (D + 2, |J| + 1) and is multiplied by SUM_DEPTH on
top, so the relative bound of a score is about 1e-4 at D <= 8 and several 1e-3 at D = 256, a thousand times the rounding an
fp32 route shows there.  It rejects STRUCTURAL mistakes (a softmax over the wrong set, a wrong table row, a dropped term: the
mutants of tests/test_tracker_parity_cpu.py); a bi-softmax wrong by 1e-4 relative passes it at most widths.  And with dyadic
inputs and |feats| <= 8 every dot product of `plain` and `equal` is exact in fp32: only `wide` and `long` round in it.

associate_exact and update_exact restate the two exact-fp32 kernels in integers and np.float32, one IEEE operation per
operation of the kernel: they are compared bitwise, without a tolerance.  Both report the events they meet, as tracker_ref.
"""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_cases as DC                                                  # noqa: E402
import tracker_ref                                                          # noqa: E402
import parity_measure as PM                                                 # noqa: E402
from parity_measure import COMP_MARGIN, SUM_DEPTH, U, entry_bound          # noqa: E402,F401

assert DC.STEP_BITS == 10
TOL = DC.TOL
F32, F64 = np.float32, np.float64
STEP = 1024.0
INT_GARBAGE, LONG_GARBAGE = -0x5A5A5A5A, -0x5A5A5A5A5A5A5A5A
BOX = 5
FIELDS = (("meta", np.int64, lambda C, D, L: (2,)), ("id", np.int64, lambda C, D, L: (C,)), ("label", np.int64, lambda C, D, L: (C,)),
          ("bbox", F32, lambda C, D, L: (C, BOX)), ("velocity", F32, lambda C, D, L: (C, BOX)),
          ("last_frame", np.int32, lambda C, D, L: (C,)), ("acc_frame", np.int32, lambda C, D, L: (C,)),
          ("exist_frame", np.int32, lambda C, D, L: (C,)), ("long_len", np.int32, lambda C, D, L: (C,)),
          ("long_score", F32, lambda C, D, L: (C, L)), ("embed", F32, lambda C, D, L: (C, D)),
          ("long_embed", F32, lambda C, D, L: (C, L, D)))
FLOAT_FIELDS = tuple(k for k, t, _ in FIELDS if t is F32)


def blank_state(C, D, L, M=0, num_tracklets=0):
    """A bank of nothing but NaN and garbage, with its two counters."""
    s = {}
    for name, dtype, shape in FIELDS:
        fill = np.nan if dtype is F32 else (LONG_GARBAGE if dtype is np.int64 else INT_GARBAGE)
        s[name] = np.full(shape(C, D, L), fill, dtype=dtype)
    s["meta"][:] = (M, num_tracklets)
    return s


_rng, dy, is_dyadic = PM.rng, PM.dy, PM.is_dyadic        # seeded by name; float32 multiples of 2^-10 (never -0.0)


def temporal_table(L):
    """[L + 1, L] fp32: row `length` holds float32((k + 1) / length) for k < length (tests/test_tracker_cpu.py pins the
    package's table to this); everything else NaN, no kernel may read it."""
    t = np.full((L + 1, L), np.nan, dtype=F32)
    for length in range(1, L + 1):
        t[length, :length] = (np.arange(1, length + 1, dtype=F64) / length).astype(F32)
    return t


# =========================================================================================================== scores: the cases

PLAIN_RANGE, WIDE_RANGE = 8.0, 40.0
# name: D, M, n, keep pattern, stress, L (0: no long_match), temporal, embeds offset by one float
_S = [(1, 1, 1, "all", "plain"), (3, 3, 2, "all", "plain"), (4, 4, 2, "first", "plain"), (12, 5, 63, "last", "plain"),
      (63, 255, 65, "alt", "plain"), (65, 256, 2, "one", "plain"), (252, 257, 63, "all", "plain"), (256, 513, 257, "alt", "plain"),
      (8, 5, 65, "all", "plain", 0, False, True), (256, 257, 65, "none", "plain"), (3, 5, 2, "none", "plain"),
      (4, 1, 257, "all", "plain"), (256, 3, 1, "all", "plain"), (65, 513, 1, "one", "plain"),
      (256, 257, 65, "alt", "wide"), (3, 5, 63, "all", "wide"), (12, 513, 2, "first", "wide"), (252, 256, 257, "last", "wide"),
      (256, 257, 2, "all", "equal"), (63, 4, 65, "alt", "equal"),
      (4, 5, 2, "all", "long", 1, False), (3, 3, 2, "all", "long", 1, True), (12, 257, 63, "alt", "long", 3, False),
      (256, 5, 65, "first", "long", 3, True), (63, 255, 2, "all", "long", 10, True), (252, 4, 63, "last", "long", 10, False),
      (256, 256, 2, "all", "long", 64, True), (1, 513, 1, "all", "long", 64, False), (8, 5, 65, "alt", "long", 10, True, True),
      (4, 4, 2, "none", "long", 3, False)]
SCORES = {}
for _c in _S:
    _D, _M, _n, _keep, _stress = _c[:5]
    _L, _temporal, _off = (list(_c[5:]) + [0, False, False][len(_c) - 5:])
    _name = "D%d%s_M%d_n%d_%s/%s%s" % (_D, "off" if _off else "", _M, _n, _keep, _stress, ("%d%s" % (_L, "t" if _temporal else "")) if _L else "")
    assert _name not in SCORES
    SCORES[_name] = dict(D=_D, M=_M, n=_n, keep=_keep, stress=_stress, L=max(_L, 1), long=_L > 0, temporal=_temporal, offset=_off)
SCORE_DS, SCORE_MS, SCORE_NS, SCORE_LS = (1, 3, 4, 8, 12, 63, 65, 252, 256), (1, 3, 4, 5, 255, 256, 257, 513), (1, 2, 63, 65, 257), (1, 3, 10, 64)
KEEPS = ("all", "first", "last", "alt", "one", "none")


def keep_pattern(kind, n):
    k = np.ones(n, dtype=np.uint8)
    if kind == "first":
        k[0] = 0
    elif kind == "last":
        k[-1] = 0
    elif kind == "alt":
        k[1::2] = 0
    elif kind == "one":
        k[:] = 0
        k[n // 2] = 1
    elif kind == "none":
        k[:] = 0
    else:
        assert kind == "all"
    return k


def _rows(g, base, noise, radius):
    """dyadic rows of norm `radius` (before rounding) around the rows of `base`"""
    v = base + noise * g.standard_normal(base.shape) / np.sqrt(base.shape[-1])
    return dy(radius * v / np.linalg.norm(v, axis=-1, keepdims=True))


@functools.lru_cache(maxsize=4)
def score_inputs(name):
    """dict(state, embeds [n, D] fp32, keep [n] uint8, temporal or None, M, C, D, L, long): left unchanged by its callers."""
    c, g = SCORES[name], _rng(name)
    D, M, n, L = c["D"], c["M"], c["n"], c["L"]
    C = M + n + 3
    radius = 0.98 * np.sqrt(WIDE_RANGE if c["stress"] == "wide" else PLAIN_RANGE)
    K = max(M, n)
    keys = g.standard_normal((K, D))
    keys /= np.linalg.norm(keys, axis=1, keepdims=True)
    state = blank_state(C, D, L, M, 7)
    embeds = _rows(g, keys[np.arange(n) % K], 0.3, radius)
    slot_keys = keys[np.zeros(M, dtype=int)] if c["stress"] == "equal" else keys[np.arange(M) % K]
    if c["long"]:
        lens = 1 + np.arange(M) % L                                  # 1 .. L across the slots
        state["long_len"][:M] = lens
        for m in range(M):
            state["long_embed"][m, :lens[m]] = _rows(g, np.repeat(slot_keys[m][None], lens[m], 0), 0.3, radius)
            state["long_score"][m, :lens[m]] = g.randint(1, 1025, lens[m]) / STEP        # dyadic in (0, 1]
    else:
        rows = _rows(g, slot_keys, 0.0 if c["stress"] == "equal" else 0.3, radius)
        state["embed"][:M] = rows
    return dict(state=state, embeds=embeds, keep=keep_pattern(c["keep"], n), temporal=temporal_table(L) if c["temporal"] else None,
                M=M, C=C, D=D, L=L, long=c["long"])


# =================================================================================================== scores: the restatement

def scores64(state, embeds, keep, long_match, temporal, mutant=None):
    """dict of float64 arrays: memo [M, D], feats [n, M], rstat [n, 2] (row maximum, row sum of exponentials), scores [n, M],
    and mag_memo, mag_feats, mag_rstat, mag_scores, the magnitudes of the module docstring (units of u).  Rows the pre-NMS
    dropped hold NaN in rstat and scores.  `mutant`: a deliberately wrong variant for test_tracker_parity_cpu.py."""
    M = int(state["meta"][0])
    E = np.asarray(embeds, dtype=F64)
    n, D = E.shape
    L = state["long_score"].shape[1]
    memo, s_memo = np.zeros((M, D)), np.zeros((M, D))
    if long_match:
        for m in range(M):
            ln = min(max(int(state["long_len"][m]), 0), L)
            w = state["long_score"][m, :ln].astype(F64)
            if temporal is not None:
                row = ln - 1 if mutant == "temporal_len_minus_1" else ln
                w = w + np.nan_to_num(temporal[row, :ln].astype(F64))
            ring = state["long_embed"][m, :ln].astype(F64)
            memo[m] = (ring * w[:, None]).sum(0) / w.sum()
            s_memo[m] = (ln + 2) * (np.abs(ring) * w[:, None]).sum(0) / w.sum() + (ln + 1) * np.abs(memo[m])
    else:
        memo[:] = state["embed"][:M].astype(F64)
    Ed = E.copy()
    if mutant == "drop_term":
        Ed[:, D - 1] = 0.0
    feats = Ed @ memo.T
    Fm = (D + 2) * (np.abs(E) @ np.abs(memo).T) + np.abs(E) @ s_memo.T
    kept = np.flatnonzero(np.asarray(keep))
    rstat, s_rstat = np.full((n, 2), np.nan), np.full((n, 2), np.nan)
    scores, s_scores = np.full((n, M), np.nan), np.full((n, M), np.nan)
    if len(kept) and M:
        f, Fk = feats[kept], Fm[kept]
        mx = f.max(1, keepdims=True)
        t = np.exp(f - mx)
        S = t.sum(1, keepdims=True)
        Fr = Fk.max(1, keepdims=True)
        g = np.abs(f - mx) + 2.0
        T = (t * g).sum(1, keepdims=True) / S
        p = t / S
        s_p = p * (2 * Fr + g + T + M + 1)
        rstat[kept] = np.concatenate([mx, S], 1)
        s_rstat[kept] = np.concatenate([Fr, S * (2 * Fr + T + M)], 1)
        col = np.arange(n) if mutant == "col_all_rows" else kept     # the set of rows the column softmax runs over
        fc, J = feats[col], len(col)
        cmx = fc.max(0, keepdims=True)
        tc = np.exp(fc - cmx)
        Sc = tc.sum(0, keepdims=True)
        Fc = Fm[col].max(0, keepdims=True)
        gc = np.abs(fc - cmx) + 2.0
        Tc = (tc * gc).sum(0, keepdims=True) / Sc
        q = np.exp(f - cmx) / Sc
        s_q = q * (2 * Fc + np.abs(f - cmx) + 2.0 + Tc + J + 1)
        scores[kept] = (p + q) / 2
        s_scores[kept] = (s_p + s_q + p + q) / 2
    return dict(memo=memo, feats=feats, rstat=rstat, scores=scores, mag_memo=s_memo, mag_feats=Fm, mag_rstat=s_rstat,
                mag_scores=s_scores, kept=kept)


@functools.lru_cache(maxsize=4)
def score_reference(name):
    x = score_inputs(name)
    return scores64(x["state"], x["embeds"], x["keep"], x["long"], x["temporal"])


def score_composition(name, device="cpu"):
    """The fp32 PyTorch composition on the kept rows, as float64 numpy.  It is a COPY of the package's lines, not a call: the
    memo by stack / product / sum / division per slot as IDOL_Tracker.memo forms it (tests/test_tracker_parity_cpu.py pins this
    copy bitwise to that property), then `torch.mm` and `(feats.softmax(dim=1) + feats.softmax(dim=0)) / 2` as
    _match_composition has them, which cannot be called apart from its pre-NMS and its update; max and exp-sum for the row
    statistics.  It never runs the kernels."""
    x = score_inputs(name)
    st, M, n = x["state"], x["M"], len(x["keep"])
    with torch.no_grad():
        if x["long"]:
            rows = []
            for m in range(M):
                ln = int(st["long_len"][m])
                w = torch.from_numpy(st["long_score"][m, :ln].copy())
                if x["temporal"] is not None:
                    w = w + torch.from_numpy(x["temporal"][ln, :ln].copy())
                rows.append((torch.from_numpy(st["long_embed"][m, :ln].copy()) * w.unsqueeze(1)).sum(0) / w.sum())
            memo = torch.stack(rows)
        else:
            memo = torch.from_numpy(st["embed"][:M].copy())
        kept = np.flatnonzero(x["keep"])
        out = dict(memo=memo.double().numpy(), rstat=np.full((n, 2), np.nan), scores=np.full((n, M), np.nan))
        if len(kept):
            e = torch.from_numpy(x["embeds"][kept]).to(device)
            feats = torch.mm(e, memo.to(device).t())
            sc = (feats.softmax(dim=1) + feats.softmax(dim=0)) / 2
            mx = feats.max(dim=1, keepdim=True)[0]
            assert sc.dtype == torch.float32
            out["scores"][kept] = sc.cpu().double().numpy()
            out["rstat"][kept] = torch.cat([mx, (feats - mx).exp().sum(1, keepdim=True)], 1).cpu().double().numpy()
    return out


# ========================================================================================================== the error measure

HEAD = "%-12s %-40s %10s %10s %10s %8s" % ("output", "case", "kernel err", "comp err", "bound", "ratio")
_T = PM.Table(HEAD, env="TRACKER_PARITY_TABLE")
TABLE, WORST, report = _T.lines, _T.worst, _T.report        # WORST: (output, stress) -> (ratio, table line)


def measure(case, what, stress, got, want, mag, comp, check=True):
    """Every entry of `got` within entry_bound(the composition's error at the entry, s) of `want`, and the project's bound on top.
    Returns the largest error / bound; check=False only returns it (inf for a NaN in `got`) and adds no line.
    Non-finite: an entry where `want` is NaN (a row that is not kept) is not compared; no NaN among the rest, in `comp`, `mag` or `got`.
    WORST: (output, stress).  Line: output, case, the worst entry's errors relative to its own magnitude.
    Tolerance: TOL * max(1, max|want|)."""
    got = np.asarray(got, dtype=F64)
    assert got.shape == want.shape == comp.shape == mag.shape, (case, what, got.shape, want.shape, comp.shape, mag.shape)
    live = ~np.isnan(want)
    assert not np.isnan(comp[live]).any() and not np.isnan(mag[live]).any(), (case, what)
    if not live.any():
        return 0.0
    got, want, comp, mag = got[live], want[live], comp[live], mag[live]
    if np.isnan(got).any():
        assert not check, (case, what, "NaN entries", int(np.isnan(got).sum()))
        return float("inf")
    e = PM.errors(got, want, mag * 1.0, comp)
    if not check:
        return e.worst
    _T.add("%-12s %-40s %10.2e %10.2e %10.2e %8.3f" % ((what, case) + e.row()), (what, stress), e.worst)
    e.check(case, what)
    tol = TOL * max(1.0, float(e.size.max()))
    assert float(e.err.max()) <= tol, (case, what, "the project's bound", float(e.err.max()), tol)
    return e.worst


def measure_scores(name, got, comp, check=True):
    """got: dict(memo, rstat, scores) of one case against score_reference; the largest error / bound of the three outputs."""
    ref, stress = score_reference(name), SCORES[name]["stress"]
    return max(measure(name, k, stress, got[k], ref[k], ref["mag_" + k], comp[k], check) for k in ("memo", "rstat", "scores"))


def worst_table():
    return "\n".join("%-7s %s" % (k[1], WORST[k][1]) for k in sorted(WORST))


# ======================================================================================================= associate, exactly

TIE_COLUMNS = (5, 69, 261, 300)       # lanes 5 and 44, waves 0 and 1, strided passes 0 and 1 of the 256 threads


def iou32(inter, area_i, area_j):
    """(float32(inter) + 1e-6f) / (float32(union) + 1e-6f), one rounding per operation"""
    it, un = F32(inter), F32(int(area_i) + int(area_j) - int(inter))
    return F32(F32(it + F32(1e-6)) / F32(un + F32(1e-6)))


def associate_exact(scores, keep, bboxes, inter, area, state, capacity, frame_weight, match_thr, new_thr, nms_thr, frame_id,
                    tracklet_frames, mutant=None):
    """(plan [2 capacity + n] int32, INT_GARBAGE where the kernel writes nothing; result [3 n + 2] int64; next meta [2]; the
    events met) of track_hip_associate_f32, operation for operation in integers and np.float32."""
    M, nxt = int(state["meta"][0]), int(state["meta"][1])
    n, C = len(keep), capacity
    match_thr, new_thr, nms_thr, half = F32(match_thr), F32(new_thr), F32(nms_thr), F32(0.5)
    gt = lambda which, a, b: a >= b if mutant == "ge_" + which else a > b      # the kernel's comparisons are strict
    events = set()
    kept = np.asarray(keep) != 0
    ids = np.full(n, -2, dtype=np.int64)
    taken = np.zeros(M, dtype=np.int64)
    exist = state["exist_frame"][:M].astype(np.int64)
    existf = state["exist_frame"][:M].astype(F32)
    for i in range(n if M > 0 else 0):
        if not kept[i]:
            continue
        raw = np.asarray(scores[i], dtype=F32)
        v = np.where(taken > 0, F32(0), raw)
        if (raw[taken > 0] > match_thr).any():
            events.add("rival")
        if frame_weight:
            hits = gt("half", v, half)
            if (v == half).any():
                events.add("fw_eq_half")
            cnt = int(hits.sum())
            if ((raw > half) & (taken > 0)).any():
                events.add("fw_taken_hit")
            events.add("fw_cnt%s" % (cnt if cnt < 3 else "_more"))
            if gt("cnt", cnt, 1):
                esum = int(exist[hits].sum())
                mean = F32(F32(esum) / F32(cnt))
                if float(mean) * cnt != esum:
                    events.add("fw_inexact_mean")
                plain = int(np.argmax(v))
                v = np.where(hits, v * existf, v * mean).astype(F32)
                if int(np.argmax(v)) != plain:
                    events.add("fw_changed_winner")
        best = v.max()
        tied = np.flatnonzero(v == best)
        bi = int(tied[-1] if mutant == "tie_highest" else tied[0])
        if len(tied) > 1 and best != 0:
            events.add("tie")
            waves, passes = (tied % 256) // 64, tied // 256
            if len(set(passes)) > 1:
                events.add("tie_across_passes")
            if len(set(waves)) > 1:
                events.add("tie_across_waves")
            if (waves[1:] < waves[0]).any():
                events.add("tie_lowest_in_later_wave")
            if len(set(tied % 64)) > 1:
                events.add("tie_across_lanes")
        if best == match_thr:
            events.add("eq_match_thr")
        if gt("match", best, match_thr):
            ids[i] = state["id"][bi]
            taken[bi] = i + 1
            events.add("matched")
    fresh = np.zeros(n, dtype=bool)
    for i in range(n):
        if kept[i] and ids[i] == -2:
            if bboxes[i, 4] == new_thr:
                events.add("eq_new_thr")
            if gt("new", bboxes[i, 4], new_thr):
                ids[i], fresh[i] = nxt, True
                nxt += 1
                events.add("new")
                if i in (63, 64, 65):
                    events.add("new_at_%d" % i)
    area = np.asarray(area)
    for i in range(n):
        if not kept[i] or ids[i] != -2:
            continue
        js = np.flatnonzero(kept[:i])
        overlaps = False
        if len(js):
            it = inter[i, js].astype(F32)
            un = (int(area[i]) + area[js].astype(np.int64) - inter[i, js]).astype(F32)
            iou = ((it + F32(1e-6)) / (un + F32(1e-6))).astype(F32)
            if (iou == nms_thr).any():
                events.add("eq_nms_thr")
            overlaps = bool((~((iou <= nms_thr) if mutant == "ge_nms" else (iou < nms_thr))).any())
        if overlaps:
            events.add("left_unselected")
        else:
            ids[i] = -1
            events.add("backdrop")
    plan = np.full(2 * C + n, INT_GARBAGE, dtype=np.int32)
    count = 0
    for m in range(M):
        row = int(taken[m]) - 1
        age = 0 if row >= 0 else frame_id - int(state["last_frame"][m])
        alive = age <= tracklet_frames if mutant == "ge_age" else age < tracklet_frames
        if row < 0 and age == tracklet_frames - 1:
            events.update(("age_edge_survives", "age_edge_survives_at_%d" % m))
        if row < 0 and age == tracklet_frames:
            events.update(("age_edge_expires", "age_edge_expires_at_%d" % m))
        if row >= 0 and frame_id - int(state["last_frame"][m]) >= tracklet_frames and alive:
            events.add("matched_rescued")
        plan[m] = row
        plan[C + m] = count if alive else -1
        if alive and count < m:
            events.add("moved_lower")
        if not alive:
            events.add("expired")
            if mutant == "dst_off_by_one":
                count += 1
        count += 1 if alive else 0
    for i in range(n):
        alive = bool(fresh[i]) and 0 < tracklet_frames
        plan[2 * C + i] = count if alive and count < C else -1
        count += 1 if alive else 0
    count = min(count, C)
    if count == 0:
        events.add("all_expire")
    result = np.zeros(3 * n + 2, dtype=np.int64)
    result[:n] = kept
    result[n:2 * n] = np.where(kept, ids, -3)
    result[2 * n], result[2 * n + 1] = count, nxt
    rows = np.flatnonzero(kept)
    result[2 * n + 2:2 * n + 2 + len(rows)] = rows
    return plan, result, np.asarray([count, nxt], dtype=np.int64), events


ASSOC_FRAME, MATCH_THR, NEW_THR = 20, 0.5, 0.5
NMS_THR_EQ = float(iou32(3, 8, 5))        # the fp32 IoU of inter 3, areas 8 and 5, handed over as nms_thr_post
# name: M, n, frame_weight, memo_tracklet_frames, keep with holes
_A = [(0, 1, 0, 4, 0), (0, 65, 0, 4, 1), (0, 64, 0, 0, 0), (1, 1, 0, 4, 0), (1, 64, 1, 4, 0), (63, 65, 0, 4, 0), (64, 64, 0, 4, 1),
      (65, 257, 1, 4, 0), (65, 65, 0, 0, 0), (255, 65, 0, 4, 0), (256, 1, 0, 4, 0), (257, 64, 1, 4, 1), (513, 257, 0, 4, 0),
      (513, 1024, 0, 3, 1), (257, 1024, 1, 4, 0), (513, 65, 1, 2, 0)]
ASSOC = {"M%d_n%d%s%s%s" % (M, n, "_fw" if fw else "", "_tf%d" % tf if tf != 4 else "", "_holes" if h else ""):
         dict(M=M, n=n, fw=bool(fw), tf=tf, holes=bool(h)) for M, n, fw, tf, h in _A}
ASSOC_MS, ASSOC_NS = (0, 1, 63, 64, 65, 255, 256, 257, 513), (1, 64, 65, 257, 1024)
ASSOC_EVENTS = ("tie", "tie_across_lanes", "tie_across_waves", "tie_across_passes", "tie_lowest_in_later_wave", "eq_match_thr",
                "eq_new_thr", "eq_nms_thr", "rival", "fw_cnt1", "fw_cnt2", "fw_cnt_more", "fw_taken_hit", "fw_changed_winner",
                "fw_inexact_mean", "fw_eq_half", "age_edge_survives", "age_edge_expires", "matched_rescued", "moved_lower", "expired",
                "all_expire", "new", "new_at_63", "new_at_64", "new_at_65", "backdrop", "left_unselected", "matched")
EDGE_SLOTS = (62, 63, 64, 65, 66, 254, 255, 256, 257, 258)


@functools.lru_cache(maxsize=4)
def assoc_inputs(name):
    """dict(scores, keep, bboxes, inter, area, state, C, args, planted): the inputs of one association and the events planted
    in them.  Unplanted scores lie in [0, 0.25), unplanted detection scores in {0.25, 0.375, 0.75, 0.875}, unplanted IoUs
    near 0."""
    c, g = ASSOC[name], _rng(name)
    M, n, fw, tf = c["M"], c["n"], c["fw"], c["tf"]
    C, D, L = M + n + 3, 1, 1
    frame_id = ASSOC_FRAME
    scores = (g.randint(0, 256, (n, M)) / STEP).astype(F32)
    keep = np.ones(n, dtype=np.uint8)
    if c["holes"]:
        keep[g.rand(n) < 0.2] = 0
        keep[[0, n - 1]] = (0, 1)
    bboxes = np.concatenate([g.randint(0, 4096, (n, 4)) / 8.0, g.choice([0.25, 0.375, 0.75, 0.875], (n, 1))], 1).astype(F32)
    area = g.randint(40, 200, n).astype(np.int32)
    inter = np.zeros((n, n), dtype=np.int32)
    state = blank_state(C, D, L, M, 5000)
    ms = np.arange(M)
    state["id"][:M] = 1000 + 3 * ms
    state["exist_frame"][:M] = 1 + (ms * 7) % 5
    age = np.asarray([1, 2, tf - 1, tf, tf + 3])[ms % 5] if M else np.zeros(0, dtype=int)
    for m in EDGE_SLOTS:                                                # odd slots survive at the last age, even ones expire at
        if m < M:                                                       # the first: both kinds on both sides of 63 | 64 and 255 | 256
            age[m] = tf - 1 if m % 2 else tf
    state["last_frame"][:M] = frame_id - np.maximum(age, 1)
    planted = set()
    reserved = [i for i in (62, 63, 64, 65, 66) if i < n and keep[i]]
    for i in reserved:                                                  # new tracklets around the ballot's edge
        bboxes[i, 4] = 0.875
    queue = [i for i in np.flatnonzero(keep) if i not in reserved]
    ties = [c_ for c_ in TIE_COLUMNS if c_ < M]
    if len(ties) < 2 and M >= 2:
        ties = [0, M - 1]
    # the columns a planted row may match: never an edge slot (a matched slot is alive whatever its age, and the ages planted
    # at the ballots' edges would go unused), and the slots that would expire come first, so that a match rescues some
    pool = [m for m in range(M) if m not in ties and m not in EDGE_SLOTS]
    pool = [m for m in pool if age[m] >= tf] + [m for m in pool if age[m] < tf]
    take = lambda: queue.pop(0) if queue else None
    col = lambda: pool.pop(0) if pool else None

    def role(rows=1, cols=0):
        return len(queue) >= rows and len(pool) >= cols

    if len(ties) >= 2 and role(1):
        i = take()
        scores[i, ties] = 0.625
        state["exist_frame"][ties] = 3
        planted.add("tie")
        if len(ties) == 4 and role(2):                                  # 69 against 300 (wave 1 against wave 0), then 261 against 300
            i, j = take(), take()
            scores[i, [69, 300]] = 0.625
            scores[j, [261, 300]] = 0.625
            planted.update(("tie_lowest_in_later_wave", "tie_across_passes"))
    if role(1, 1):
        scores[take(), col()] = 0.5
        planted.add("eq_match_thr")
    if role(2, 1):
        i, j, m = take(), take(), col()
        scores[i, m] = scores[j, m] = 0.75
        bboxes[j, 4] = 0.875
        planted.add("rival")
    if fw:
        if role(1, 1):
            i, m = take(), col()
            scores[i, m] = 0.5625
            state["exist_frame"][m] = 0        # no tracker gets here; it is what makes `cnt > 1` against `cnt >= 1` visible
            planted.add("fw_cnt1")
        if role(1, 2):
            i, a, b = take(), col(), col()
            scores[i, a], scores[i, b] = 0.625, 0.5625
            state["exist_frame"][[a, b]] = (1, 5)
            planted.update(("fw_cnt2", "fw_changed_winner"))
        if role(1, 2):
            i, a, b = take(), col(), col()
            scores[i, a], scores[i, b] = 0.625, 0.5                     # 0.5 is no hit: one hit, no weighting, a wins
            state["exist_frame"][[a, b]] = (1, 5)                       # were it one, b would win with 2.5
            planted.add("fw_eq_half")
        if role(1, 3):
            i, a, b, d = take(), col(), col(), col()
            scores[i, [a, b, d]] = (0.75, 0.625, 0.5625)
            state["exist_frame"][[a, b, d]] = (1, 2, 4)
            planted.update(("fw_cnt_more", "fw_inexact_mean"))
        if role(2, 2):
            i, j, a, b = take(), take(), col(), col()
            scores[i, a] = 0.75
            scores[j, a], scores[j, b] = 0.75, 0.5625                   # a is taken when j comes: one hit is left, not two
            planted.add("fw_taken_hit")
    for _ in range(12):                                                 # plain matches
        if role(3, 1):
            scores[take(), col()] = 0.75
    if len(queue) >= 3:
        i = queue.pop()                                                 # a late row: the threshold itself is not above it
        bboxes[i, 4] = NEW_THR
        planted.add("eq_new_thr")
        i, j = queue.pop(), queue.pop(0)
        assert j < i
        bboxes[i, 4], bboxes[j, 4] = 0.25, 0.25
        area[i], area[j] = 8, 5
        inter[i, j] = inter[j, i] = 3
        planted.update(("eq_nms_thr", "left_unselected"))
    inter[np.arange(n), np.arange(n)] = area
    args = dict(capacity=C, frame_weight=fw, match_thr=MATCH_THR, new_thr=NEW_THR, nms_thr=NMS_THR_EQ, frame_id=frame_id,
                tracklet_frames=tf)
    return dict(scores=scores, keep=keep, bboxes=bboxes, inter=inter, area=area, state=state, C=C, D=D, L=L, M=M, n=n, args=args,
                planted=planted)


def assoc_expected(name, mutant=None):
    x = assoc_inputs(name)
    return associate_exact(x["scores"], x["keep"], x["bboxes"], x["inter"], x["area"], x["state"], mutant=mutant, **x["args"])


# =========================================================================================================== update, exactly

def update_exact(embeds, bboxes, labels, plan, result, state, capacity, keep_weight, momentum, frame_id, mutant=None):
    """(the next bank, the events): track_hip_update_f32 in np.float32 and integers, in the kernel's operation order; what the
    kernel does not write is NaN / garbage, and `meta` is the association's."""
    C, L, D = capacity, state["long_score"].shape[1], state["embed"].shape[1]
    M, n = int(state["meta"][0]), len(labels)
    kw, mo = F32(keep_weight), F32(momentum)
    b = blank_state(C, D, L, int(result[2 * n]), int(result[2 * n + 1]))
    events = set()
    for i in range(n):
        dst = int(plan[2 * C + i])
        if dst < 0:
            continue
        events.add("new")
        b["embed"][dst] = embeds[i]
        b["long_embed"][dst, 0] = embeds[i]
        b["bbox"][dst] = bboxes[i]
        b["velocity"][dst] = 0
        b["long_score"][dst, 0] = bboxes[i, 4]
        b["id"][dst], b["label"][dst] = result[n + i], labels[i]
        b["last_frame"][dst], b["acc_frame"][dst], b["exist_frame"][dst], b["long_len"][dst] = frame_id, 0, 1, 1
    for m in range(M):
        dst, row = int(plan[C + m]), int(plan[m])
        if dst < 0:
            events.add("expiring")
            continue
        ln = min(max(int(state["long_len"][m]), 0), L)
        if row < 0:
            events.add("unseen_moves_lower" if dst < m else "unseen")
            b["embed"][dst] = state["embed"][m]
            b["long_embed"][dst, :ln] = state["long_embed"][m, :ln]
            b["long_score"][dst, :ln] = state["long_score"][m, :ln]
            for k in ("bbox", "velocity", "id", "label", "last_frame", "acc_frame", "exist_frame"):
                b[k][dst] = state[k][m]
            b["long_len"][dst] = ln
            continue
        events.add("seen_full_ring" if ln == L else "seen_short_ring")
        e = embeds[row]
        drop = 1 if ln == L else 0
        kl = ln - drop
        b["embed"][dst] = ((kw * state["embed"][m]).astype(F32) + (mo * e).astype(F32)).astype(F32)
        lo, hi = (0, kl) if mutant == "drop_newest" and drop else (drop, ln)
        b["long_embed"][dst, :kl] = state["long_embed"][m, lo:hi]
        b["long_score"][dst, :kl] = state["long_score"][m, lo:hi]
        b["long_embed"][dst, kl] = e
        b["long_score"][dst, kl] = bboxes[row, 4]
        acc, gap = int(state["acc_frame"][m]), frame_id - int(state["last_frame"][m])
        events.add("gap_%d" % gap)
        events.add("acc_0" if acc == 0 else ("acc_large" if acc > 1 << 24 else "acc"))
        nb = bboxes[row]
        v = ((nb - state["bbox"][m]).astype(F32) / F32(gap)).astype(F32)
        div = F32(acc if mutant == "velocity_by_acc" and acc else acc + 1)
        b["velocity"][dst] = (((state["velocity"][m] * F32(acc)).astype(F32) + v).astype(F32) / div).astype(F32)
        b["bbox"][dst] = nb
        b["id"][dst], b["label"][dst] = state["id"][m], labels[row]
        b["last_frame"][dst], b["acc_frame"][dst] = frame_id, acc + 1
        b["exist_frame"][dst], b["long_len"][dst] = int(state["exist_frame"][m]) + 1, kl + 1
    return b, events


def live_fields(bank):
    """{field: the live part of a bank as a flat array}: slots [0, count), of each ring the entries [0, long_len)."""
    count = int(bank["meta"][0])
    lens = bank["long_len"][:count]
    L = bank["long_score"].shape[1]
    ring = np.arange(L)[None, :] < lens[:, None]
    out = {k: bank[k][:count].reshape(-1) for k, _, _ in FIELDS if k not in ("meta", "long_score", "long_embed")}
    out["meta"] = bank["meta"]
    out["long_score"] = bank["long_score"][:count][ring]
    out["long_embed"] = bank["long_embed"][:count][ring].reshape(-1)
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == F32 else a


def assert_banks_bitwise(got, want, what):
    g, w = live_fields(got), live_fields(want)
    for k in w:
        assert g[k].shape == w[k].shape, (what, k, g[k].shape, w[k].shape)
        assert not (w[k].dtype == F32 and np.isnan(w[k]).any()), (what, k, "the restatement leaves a live entry unwritten")
        bad = np.flatnonzero(bits(g[k]) != bits(w[k]))
        assert bad.size == 0, (what, k, "entries differ", bad[:8].tolist(), g[k][bad[:4]].tolist(), w[k][bad[:4]].tolist())


# name: D, L, M, memo_tracklet_frames, momentum
UPDATES = {"D1_L1": (1, 1, 10, 4, 0.5), "D8_L2": (8, 2, 10, 4, 0.5), "D255_L3": (255, 3, 12, 4, 0.3), "D256_L64": (256, 64, 10, 4, 0.8125),
           "D8_L64_M70": (8, 64, 70, 4, 0.3), "D256_L3_allnew": (256, 3, 0, 4, 0.5), "D8_L2_allexpire": (8, 2, 6, 1, 0.5),
           "D255_L1_M70": (255, 1, 70, 4, 0.5)}
UPDATE_DS, UPDATE_LS = (1, 8, 255, 256), (1, 2, 3, 64)
UPDATE_EVENTS = ("new", "expiring", "unseen", "unseen_moves_lower", "seen_full_ring", "seen_short_ring", "gap_1", "gap_3", "acc_0",
                 "acc_large")


@functools.lru_cache(maxsize=4)
def update_inputs(name):
    """The inputs of one update: a bank whose slot m is, by m % 5, seen with a short ring (a full one at L = 1), seen with a full
    ring, not seen, expiring, not seen behind the expired one; one detection per seen slot in shuffled order, two new tracklets
    and a backdrop.  The plan and the result are associate_exact's."""
    D, L, M, tf, momentum = UPDATES[name]
    g = _rng(name)
    seen = [m for m in range(M) if m % 5 < 2] if "allexpire" not in name else []
    n = len(seen) + 3
    C, frame_id = M + n + 3, ASSOC_FRAME
    state = blank_state(C, D, L, M, 900)
    ms = np.arange(M)
    state["id"][:M], state["label"][:M] = 100 + 2 * ms, ms % 7
    state["bbox"][:M] = dy(g.randint(0, 4096, (M, BOX)) / 8.0)
    state["velocity"][:M] = dy(g.standard_normal((M, BOX)), 4.0)
    state["acc_frame"][:M] = np.asarray([0, 3, (1 << 24) + 1])[ms % 3]
    state["exist_frame"][:M] = 1 + ms % 4
    state["embed"][:M] = dy(g.standard_normal((M, D)))
    role = ms % 5
    age = np.where(role < 2, np.where(ms % 2 == 0, 1, 3), np.where(role == 3, tf + 1, min(2, max(tf - 1, 1))))
    if "allexpire" in name:
        age[:] = 1 + ms % 3
    state["last_frame"][:M] = frame_id - age
    lens = np.where(role == 0, 1 + ms % max(L - 1, 1), np.where(role == 1, L, 1 + (ms * 3) % L))
    state["long_len"][:M] = lens
    for m in range(M):
        state["long_embed"][m, :lens[m]] = dy(g.standard_normal((lens[m], D)))
        state["long_score"][m, :lens[m]] = g.randint(1, 1025, lens[m]) / STEP
    embeds = dy(g.standard_normal((n, D)))
    bboxes = np.concatenate([g.randint(0, 4096, (n, 4)) / 8.0, g.randint(600, 1000, (n, 1)) / STEP], 1).astype(F32)
    labels = g.randint(0, 40, n).astype(np.int64)
    rows = list(g.permutation(n))
    scores = (g.randint(0, 256, (n, M)) / STEP).astype(F32)
    for m in seen:
        scores[rows.pop(), m] = 0.75
    bboxes[rows.pop(), 4] = 0.25                                        # a backdrop; the other two start tracklets
    keep = np.ones(n, dtype=np.uint8)
    area = np.full(n, 50, dtype=np.int32)
    inter = np.diag(area).astype(np.int32)
    plan, result, meta, _ = associate_exact(scores, keep, bboxes, inter, area, state, C, False, MATCH_THR, NEW_THR, 0.3, frame_id, tf)
    return dict(embeds=embeds, bboxes=bboxes, labels=labels, plan=plan, result=result, state=state, C=C, D=D, L=L, M=M, n=n,
                keep_weight=float(1 - momentum), momentum=float(momentum), frame_id=frame_id, tf=tf)


def update_expected(name, mutant=None):
    x = update_inputs(name)
    return update_exact(x["embeds"], x["bboxes"], x["labels"], x["plan"], x["result"], x["state"], x["C"], x["keep_weight"],
                        x["momentum"], x["frame_id"], mutant=mutant)


def update64(name):
    """The next bank's memo in float64 by tests/tracker_ref.py: RefTracker.update on the tracklets of the input bank."""
    x = update_inputs(name)
    st, M, n = x["state"], x["M"], x["n"]
    ref = tracker_ref.RefTracker(memo_tracklet_frames=x["tf"], memo_momentum=x["momentum"], memory_len=x["L"])
    for m in range(M):
        ln = int(st["long_len"][m])
        ref.tracklets[int(st["id"][m])] = dict(
            bbox=st["bbox"][m].astype(F64), embed=st["embed"][m].astype(F64), long_embed=[r.astype(F64) for r in st["long_embed"][m, :ln]],
            long_score=[F64(v) for v in st["long_score"][m, :ln]], label=int(st["label"][m]), last_frame=int(st["last_frame"][m]),
            velocity=st["velocity"][m].astype(F64), acc_frame=int(st["acc_frame"][m]), exist_frame=int(st["exist_frame"][m]))
    ref.update([int(v) for v in x["result"][n:2 * n]], x["bboxes"].astype(F64), x["embeds"].astype(F64), x["labels"], x["frame_id"])
    return ref


def bank_memo(bank):
    """The memo of a bank in the layout of tracker_ref.RefTracker.memo (long_match off)."""
    count = int(bank["meta"][0])
    lens = bank["long_len"][:count].astype(np.int64)
    ring = np.arange(bank["long_score"].shape[1])[None, :] < lens[:, None]
    f = lambda a: np.asarray(a, dtype=F64)
    return dict(bboxes=f(bank["bbox"][:count]), labels=bank["label"][:count].astype(np.int64), embeds=f(bank["embed"][:count]),
                ids=bank["id"][:count].astype(np.int64), vs=f(bank["velocity"][:count]), long_embeds=f(bank["long_embed"][:count][ring]),
                long_score=f(bank["long_score"][:count][ring])[:, None], long_len=lens,
                exist_frame=bank["exist_frame"][:count].astype(np.int64))
