"""No GPU: the conditions on the inputs of tests/tracker_parity.py, its restatements against tests/tracker_ref.py, and the
teeth of the measure.

Conditions (none is a tolerance): every input is a multiple of 2^-10 (the temporal table aside: fp32 numbers by definition);
|feats| <= 8 on `plain`, `equal` and `long`, above 20 and at most 40 on `wide`, where every exp(f - max) of every row and of
every column over the kept rows is a normal fp32 number; the case lists reach every D, M, n, L and keep pattern the sweep
names; every event planted in an association is met by associate_exact, every event of ASSOC_EVENTS and UPDATE_EVENTS by some
case, and the planted equalities are exact fp32 numbers.

Restatements: scores64 -> associate_exact -> update_exact chained over the eight sequences of tests/tracker_cases.py give
RefTracker's ids on every frame and its memo after every frame within 1e-6; update_exact is within 8 u of RefTracker.update
on every update case; an honest fp32 emulation of the scores (sequential sums in np.float32) meets the measure on every case,
with the magnitude as derived.

The fp32 composition's memo is bitwise IDOL_Tracker.memo on a long_match case with temporal weights.

Teeth: every mutant of MUTANTS is rejected on the case named there, the scores' by the measure (error / bound above 1), the
others by the exact comparison."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracker_cases as C       # noqa: E402
import tracker_parity as P      # noqa: E402
import tracker_ref              # noqa: E402

F32, F64 = np.float32, np.float64
MIN_NORMAL = 2.0 ** -126


# ------------------------------------------------------------------------------------------------------- the input conditions

@pytest.mark.parametrize("name", list(P.SCORES))
def test_score_inputs_are_dyadic_and_in_range(name):
    c, x, ref = P.SCORES[name], P.score_inputs(name), P.score_reference(name)
    st, M = x["state"], x["M"]
    assert x["C"] > M + c["n"] and P.is_dyadic(x["embeds"])
    if c["long"]:
        ring = np.arange(x["L"])[None, :] < st["long_len"][:M, None]
        assert set(st["long_len"][:M]) == set(range(1, min(M, x["L"]) + 1))
        assert P.is_dyadic(st["long_embed"][:M][ring]) and P.is_dyadic(st["long_score"][:M][ring])
        assert (st["long_score"][:M][ring] > 0).all() and (st["long_score"][:M][ring] <= 1).all()
        assert np.isnan(st["embed"]).all() and np.isnan(st["long_embed"][:M][~ring]).all()
    else:
        assert P.is_dyadic(st["embed"][:M]) and np.isnan(st["long_embed"]).all()
    assert np.isnan(st["embed"][M:]).all() and (st["long_len"][M:] == P.INT_GARBAGE).all()
    top = float(np.abs(ref["feats"]).max())
    if c["stress"] == "wide":
        assert 20.0 < top <= P.WIDE_RANGE, top
        kept = ref["kept"]
        f = ref["feats"][kept]
        assert np.exp(f - f.max(1, keepdims=True)).min() >= 4 * MIN_NORMAL and np.exp(f - f.max(0, keepdims=True)).min() >= 4 * MIN_NORMAL
    else:
        assert top <= P.PLAIN_RANGE, top
    if c["stress"] == "equal":
        assert (st["embed"][:M] == st["embed"][0]).all()
    assert not np.isnan(ref["memo"]).any() and not np.isnan(ref["feats"]).any()


def test_the_case_lists_reach_every_named_value():
    S = P.SCORES.values()
    assert {c["D"] for c in S} == set(P.SCORE_DS) and {c["M"] for c in S} == set(P.SCORE_MS) and {c["n"] for c in S} == set(P.SCORE_NS)
    assert {c["L"] for c in S if c["long"]} == set(P.SCORE_LS) and {c["keep"] for c in S} == set(P.KEEPS)
    assert any(c["offset"] and c["D"] == 8 for c in S) and {c["stress"] for c in S} == {"plain", "wide", "equal", "long"}
    for L in P.SCORE_LS:
        assert {c["temporal"] for c in S if c["long"] and c["L"] == L} == {False, True}
    assert 25 <= len(P.SCORES) <= 35
    A = P.ASSOC.values()
    assert {c["M"] for c in A} == set(P.ASSOC_MS) and {c["n"] for c in A} == set(P.ASSOC_NS)
    assert any(c["tf"] == 0 and c["M"] for c in A) and any(c["holes"] for c in A) and any(c["fw"] for c in A)
    assert {u[0] for u in P.UPDATES.values()} == set(P.UPDATE_DS) and {u[1] for u in P.UPDATES.values()} == set(P.UPDATE_LS)
    assert any(u[2] == 0 for u in P.UPDATES.values())


def test_the_temporal_table_is_the_packages():
    from uninext_amd.tracker import temporal_table
    for L in (1, 3, 64):
        ours, theirs = P.temporal_table(L), temporal_table(L).numpy()
        used = ~np.isnan(ours)
        assert np.array_equal(ours[used], theirs[used]) and used.sum() == L * (L + 1) // 2


def test_the_composition_memo_is_the_packages():
    """score_composition copies IDOL_Tracker.memo's arithmetic; here the copy is held bitwise to the property itself."""
    import torch
    from uninext_amd.tracker import IDOL_Tracker
    name = "D256_M5_n65_first/long3t"
    x = P.score_inputs(name)
    st = x["state"]
    tracker = IDOL_Tracker(fused=False, long_match=True, temporal_weight=True, memory_len=x["L"])
    t = lambda a: torch.from_numpy(np.array(a))
    tracker.tracklets = {m: dict(bbox=torch.zeros(5), embed=torch.zeros(x["D"]), label=torch.tensor(0), velocity=torch.zeros(5),
                                 long_embed=list(t(st["long_embed"][m, :st["long_len"][m]]).unbind(0)),
                                 long_score=list(t(st["long_score"][m, :st["long_len"][m]]).unbind(0)),
                                 last_frame=0, acc_frame=0, exist_frame=1) for m in range(x["M"])}
    theirs = tracker.memo[2].double().numpy()
    assert np.array_equal(theirs, P.score_composition(name)["memo"])


@pytest.mark.parametrize("name", list(P.ASSOC))
def test_every_planted_event_occurs(name):
    x = P.assoc_inputs(name)
    assert x["C"] > x["M"] + x["n"]
    assert P.is_dyadic(x["scores"]) and P.is_dyadic(x["bboxes"])
    assert np.array_equal(x["inter"], x["inter"].T) and (np.diag(x["inter"]) == x["area"]).all()
    assert (x["inter"] <= np.minimum(x["area"][:, None], x["area"][None, :])).all()
    plan, result, meta, events = P.assoc_expected(name)
    assert x["planted"] <= events, (name, sorted(x["planted"] - events))
    if "eq_match_thr" in x["planted"]:
        assert (x["scores"] == F32(P.MATCH_THR)).any()
    if "eq_nms_thr" in x["planted"]:
        assert F32(P.NMS_THR_EQ) == P.iou32(3, 8, 5) and float(F32(P.NMS_THR_EQ)) == P.NMS_THR_EQ
    M, C_, tf = x["M"], x["C"], P.ASSOC[name]["tf"]
    for m in P.EDGE_SLOTS:                     # unmatched, at the last age that survives (odd) or the first that expires (even)
        if m < M and tf > 0:
            kind = "survives" if m % 2 else "expires"
            assert plan[m] == -1 and (plan[C_ + m] >= 0) == bool(m % 2), (name, m, plan[m], plan[C_ + m])
            assert "age_edge_%s_at_%d" % (kind, m) in events, (name, m)
    if P.ASSOC[name]["tf"] == 0:
        assert "all_expire" in events and meta[0] == 0 and (plan[2 * x["C"]:] == -1).all()


def test_every_event_is_met_by_some_case():
    met = set()
    for name in P.ASSOC:
        met |= P.assoc_expected(name)[3]
    assert set(P.ASSOC_EVENTS) <= met, sorted(set(P.ASSOC_EVENTS) - met)
    for name in ("M513_n257", "M513_n1024_tf3_holes", "M513_n65_fw_tf2"):       # both ballot edges in one association
        ev = P.assoc_expected(name)[3]
        assert {"age_edge_survives_at_63", "age_edge_expires_at_64", "age_edge_survives_at_255", "age_edge_expires_at_256"} <= ev, name
    met = set()
    for name in P.UPDATES:
        x = P.update_inputs(name)
        assert all(P.is_dyadic(x[k]) for k in ("embeds", "bboxes")) and x["C"] > x["M"] + x["n"]
        met |= P.update_expected(name)[1]
    assert set(P.UPDATE_EVENTS) <= met, sorted(set(P.UPDATE_EVENTS) - met)
    assert P.update_expected("D8_L2_allexpire")[1] == {"new", "expiring"}
    assert P.update_expected("D256_L3_allnew")[1] == {"new"}


# --------------------------------------------------------------------------------------- the restatements against what exists

def chain(name):
    """The three restatements as a tracker over a sequence of tracker_cases: per frame (ids, indices, kept) and the memo."""
    kw = C.CASES[name][3]
    p = tracker_ref.RefTracker(**kw)
    D, L, cap = C.CASES[name][1], p.memory_len, 256
    state = P.blank_state(cap, D, L, 0, 0)
    temporal = P.temporal_table(L) if p.temporal_weight else None
    frames, memos = [], []
    for fr in C.frames(name):
        flat = (fr["masks"].numpy()[:, 0] > 0).reshape(len(fr["indices"]), -1).astype(np.int32)
        n, inter, area = len(flat), flat @ flat.T, flat.sum(1).astype(np.int32)
        keep = np.ones(n, dtype=np.uint8)
        for i in range(n):
            for j in range(i + 1, n):
                if keep[i] and keep[j] and (inter[i, j] + 1e-6) / (area[i] + area[j] - inter[i, j] + 1e-6) > p.nms_thr_pre:
                    keep[j] = 0
        M = int(state["meta"][0])
        emb, bb = fr["embeds"].numpy(), fr["bboxes"].numpy()
        scores = P.scores64(state, emb, keep, p.long_match, temporal)["scores"].astype(F32)
        plan, result, _, _ = P.associate_exact(scores, keep, bb, inter, area, state, cap, p.frame_weight, p.match_score_thr,
                                               p.addnew_score_thr if M else p.init_score_thr, p.nms_thr_post, fr["frame_id"],
                                               p.memo_tracklet_frames)
        state, _ = P.update_exact(emb, bb, fr["labels"].numpy(), plan, result, state, cap, 1 - p.memo_momentum, p.memo_momentum,
                                  fr["frame_id"])
        kept = [i for i in range(n) if keep[i]]
        assert list(result[2 * n + 2:2 * n + 2 + len(kept)]) == kept
        frames.append(([int(result[n + i]) for i in kept], [fr["indices"][i] for i in kept], len(kept)))
        memo = None
        if state["meta"][0]:
            memo = P.bank_memo(state)
            if p.long_match:
                memo["embeds"] = P.scores64(state, np.zeros((1, D)), [1], True, temporal)["memo"]
        memos.append(memo)
    return frames, memos


@pytest.mark.parametrize("name", list(C.CASES))
def test_chained_restatements_reproduce_the_float64_tracker(name):
    ref = tracker_ref.run(name, C)
    frames, memos = chain(name)
    assert len(frames) == len(ref["frames"]) == len(ref["memos"])
    for t, (got, want) in enumerate(zip(frames, ref["frames"])):
        assert got == (list(want[0]), list(want[1]), want[2]), (name, t, got, want)
    for t, (got, want) in enumerate(zip(memos, ref["memos"])):
        assert (got is None) == (want is None), (name, t)
        if want is not None:
            C.assert_memo_close(got, want, "%s frame %d" % (name, t), tol=1e-6)


@pytest.mark.parametrize("name", list(P.UPDATES))
def test_update_exact_is_within_a_few_u_of_float64(name):
    bank, _ = P.update_expected(name)
    ref = P.update64(name)
    assert len(ref.tracklets) == int(bank["meta"][0])
    if ref.tracklets:
        C.assert_memo_close(P.bank_memo(bank), ref.memo(), name, tol=8 * P.U)
        lasts = [v["last_frame"] for v in ref.tracklets.values()], [v["acc_frame"] for v in ref.tracklets.values()]
        count = len(ref.tracklets)
        assert list(bank["last_frame"][:count]) == lasts[0] and list(bank["acc_frame"][:count]) == lasts[1]


def emulate32(name):
    """The scores in np.float32 with plainly sequential sums: an honest fp32 route that is neither the kernels' nor PyTorch's."""
    x = P.score_inputs(name)
    st, M, D, L, keep = x["state"], x["M"], x["D"], x["L"], x["keep"]
    n = len(keep)
    if x["long"]:
        memo = np.zeros((M, D), dtype=F32)
        for m in range(M):
            ln = int(st["long_len"][m])
            w = st["long_score"][m, :ln] + x["temporal"][ln, :ln] if x["temporal"] is not None else st["long_score"][m, :ln]
            acc, ws = np.zeros(D, dtype=F32), F32(0)
            for k in range(ln):
                acc, ws = acc + st["long_embed"][m, k] * w[k], F32(ws + w[k])
            memo[m] = acc / ws
    else:
        memo = st["embed"][:M]
    kept = np.flatnonzero(keep)
    out = dict(memo=memo.astype(F64), rstat=np.full((n, 2), np.nan), scores=np.full((n, M), np.nan))
    if len(kept):
        e = x["embeds"][kept]
        feats = np.zeros((len(kept), M), dtype=F32)
        for d in range(D):
            feats += e[:, d, None] * memo[None, :, d]
        assert feats.dtype == F32
        mx, cmx = feats.max(1, keepdims=True), feats.max(0, keepdims=True)
        t, tc = np.exp(feats - mx), np.exp(feats - cmx)
        S, Sc = np.cumsum(t, 1, dtype=F32)[:, -1:], np.cumsum(tc, 0, dtype=F32)[-1:]
        out["rstat"][kept] = np.concatenate([mx, S], 1)
        out["scores"][kept] = (t / S + tc / Sc) * F32(0.5)
    return out


def test_an_honest_fp32_route_meets_the_measure_on_every_case():
    since = len(P.TABLE)
    worst = max(P.measure_scores(name, emulate32(name), P.score_composition(name)) for name in P.SCORES)
    print(P.HEAD + "\n" + "\n".join(P.TABLE[since:]))
    del P.TABLE[since:]
    P.WORST.clear()
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------------ the teeth

MUTANTS = {
    "col_all_rows": ("scores", "D63_M255_n65_alt/plain"),
    "temporal_len_minus_1": ("scores", "D63_M255_n2_all/long10t"),
    "drop_term": ("scores", "D256_M257_n65_alt/wide"),
    "tie_highest": ("assoc", "M513_n257"),
    "ge_match": ("assoc", "M63_n65"),
    "ge_new": ("assoc", "M63_n65"),
    "ge_nms": ("assoc", "M63_n65"),
    "ge_age": ("assoc", "M255_n65"),
    "ge_cnt": ("assoc", "M65_n257_fw"),
    "ge_half": ("assoc", "M65_n257_fw"),
    "dst_off_by_one": ("assoc", "M255_n65"),
    "drop_newest": ("update", "D8_L2"),
    "velocity_by_acc": ("update", "D255_L3"),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_each_mutant_is_rejected(mutant):
    kind, name = MUTANTS[mutant]
    if kind == "scores":
        x = P.score_inputs(name)
        wrong = P.scores64(x["state"], x["embeds"], x["keep"], x["long"], x["temporal"], mutant=mutant)
        comp = P.score_composition(name)
        assert P.measure_scores(name, comp, comp, check=False) <= 1.0
        ratio = P.measure_scores(name, wrong, comp, check=False)
        print(mutant, name, "error / bound", ratio)
        assert ratio > 1.0
    elif kind == "assoc":
        want, wrong = P.assoc_expected(name), P.assoc_expected(name, mutant)
        assert not (np.array_equal(want[0], wrong[0]) and np.array_equal(want[1], wrong[1]))
    else:
        want, wrong = P.update_expected(name)[0], P.update_expected(name, mutant)[0]
        with pytest.raises(AssertionError):
            P.assert_banks_bitwise(wrong, want, name)
        P.assert_banks_bitwise(want, want, name)


def test_drop_term_is_also_rejected_on_the_scalar_path_width():
    x = P.score_inputs("D3_M3_n2_all/plain")
    wrong = P.scores64(x["state"], x["embeds"], x["keep"], x["long"], x["temporal"], mutant="drop_term")
    assert P.measure_scores("D3_M3_n2_all/plain", wrong, P.score_composition("D3_M3_n2_all/plain"), check=False) > 1.0
