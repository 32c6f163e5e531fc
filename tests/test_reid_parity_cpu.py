"""No GPU: the conditions the cases of tests/reid_parity.py claim, its restatements against what exists, and the teeth of the
measure.

Conditions (none is a tolerance): inputs are dyadic (the named exceptions aside: the 2^-45 entries, the merge pair, the +inf and
NaN plants); the planted ties are equal fp32 numbers; the merge pair merges under + 100000 and decides the answer; the
integer-sum column sums to 3 in float64 and in fp32, its neighbour to 3 - 2^-10; every other column of a plain image keeps its
candidate sums off the integers by at least 2^-10 (they are exact, so any order gives the same k); every edge query of the loss
cases is sampled; the case lists reach every size the sweep names.

Pins: the selection wrapper equals tests/reid_ref.py's select on the six cases of tests/reid_cases.py; the float64 restatement
gives the fixtures' losses and gradients (tests/golden/reid/*.npz) and the float64 composition's on all six.

Teeth: every mutant of MUTANTS exceeds the bound on the case named there.  The measure alone: the fp32 PyTorch composition on
the CPU meets the DERIVED term by itself (the composition term set to zero) on every case, nothing excluded."""
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import reid_cases as C      # noqa: E402
import reid_parity as P     # noqa: E402
import reid_ref as R        # noqa: E402

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------- the input conditions

def _sums(col, k):
    top = np.sort(col.astype(F64))[::-1][:k]
    s32 = F32(0)
    for v in top.astype(F32):
        s32 = F32(s32 + v)
    return float(top.sum()), float(s32)


@pytest.mark.parametrize("name", list(P.SELECT))
def test_selection_inputs_hold_their_conditions(name):
    x = P.select_inputs(name)
    Q = x["Q"]
    assert Q >= 100 and len(x["images"]) <= 64
    for im in x["images"]:
        cost, iou = im["cost"], im["iou"]
        assert cost.dtype == F32 and iou.dtype == F32 and cost.shape == iou.shape == im["flags"].shape
        fin = np.isfinite(cost)
        assert P.is_dyadic(cost[fin], 1024.0 if not im["plain"] else 64.0, 64.0) and (cost[fin] >= 0).all()
        ok = ~np.isnan(iou)
        assert P.is_dyadic(iou[ok]) and (iou[ok] >= 0).all() and (iou[ok] <= 1).all()
        if im["plain"]:
            assert fin.all() and ok.all()
            for t in np.flatnonzero(im["valid"]):
                for k in (10, 100):
                    s64, s32 = _sums(iou[:, t], k)
                    assert s64 == s32 and abs(s64 - round(s64)) >= 2.0 ** -10, (name, t, k, s64)


def test_selection_plants_are_what_they_claim():
    x, want = P.select_inputs("q100_plants"), P.select_expected("q100_plants")
    Q, off = x["Q"], x["off"]
    intsum, tie_iou, tie_cost, merge, nan = x["images"]
    pos = [P.block(want["pos"], off, Q, b) for b in range(5)]
    neg = [P.block(want["neg"], off, Q, b) for b in range(5)]
    # the integer sum and its neighbour, in both precisions and for both candidate counts
    for k in (10, 100):
        assert _sums(intsum["iou"][:, 0], k) == (3.0, 3.0) and _sums(intsum["iou"][:, 1], k) == (3.0 - 2.0 ** -10,) * 2
    alone = P.select_exact(intsum["cost"][:, :1], intsum["iou"][:, :1], intsum["flags"][:, :1], [1])
    assert alone["n_pos"][0] == 3 and Q - alone["n_neg"][0] == 3
    alone = P.select_exact(intsum["cost"][:, 1:2], intsum["iou"][:, 1:2], intsum["flags"][:, 1:2], [1])
    assert alone["n_pos"][0] == 2
    # fifteen equal IoUs through the cut
    col = tie_iou["iou"][:, 0]
    assert (col == F32(0.25)).sum() == 15 and (col[col != F32(0.25)] == 0).all()
    assert _sums(col, 10)[0] == 2.5 and _sums(col, 100)[0] == 3.75
    # equal costs: top-k, argmin, repair
    c = tie_cost["cost"]
    assert len(set(c[list(P.TIE_ROWS), 0].tolist())) == 1 and (np.delete(c[:, 0], P.TIE_ROWS) > 1.0).all()
    assert np.flatnonzero(pos[2][:, 0]).tolist() == list(P.TIE_ROWS[:3])
    assert c[50, 1] == c[50, 2] == c[:, 1].min() == c[:, 2].min() and pos[2][50].tolist() == [0, 1, 0]
    assert c[60, 2] == c[70, 2] and (np.delete(c[:, 2], [50, 60, 70]) > c[60, 2]).all() and np.flatnonzero(pos[2][:, 2]).tolist() == [60]
    # the merge
    a, b = merge["cost"][P.MERGE_A, 2], merge["cost"][P.MERGE_B, 2]
    assert a > b and F32(a + O_TAKEN) == F32(b + O_TAKEN) and P.MERGE_A < P.MERGE_B
    assert pos[3][P.MERGE_A, 2] == 1 and pos[3][P.MERGE_B, 2] == 0
    apart = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in merge.items()}
    apart["cost"][P.MERGE_A, 2] = 5.0 + 2.0 ** -6                              # a pair that survives the + 100000: row B wins
    assert F32(apart["cost"][P.MERGE_A, 2] + O_TAKEN) != F32(b + O_TAKEN)
    # (row B takes it, is reset to its cheaper column 0 as the stale row it is, and the target stays without a query: one round
    # shows it; the merged pair is settled within that round)
    r = P.select_exact(apart["cost"], apart["iou"], apart["flags"], apart["valid"], 1)
    assert r["first_status"] == 2 and not r["pos"][:, 2].any()
    r = P.select_exact(merge["cost"], merge["iou"], merge["flags"], merge["valid"], 1)
    assert r["first_status"] == 0 and r["pos"][P.MERGE_A, 2] == 1
    assert r["status"] == 0 and want["status"].tolist() == [0] * 5
    # NaN: k = 1 for the column with a NaN IoU
    assert np.isnan(nan["iou"][:, 0]).sum() == 1 and np.isnan(nan["cost"][7]).all() and np.isnan(nan["cost"][:, 2]).sum() == 3
    first = P.select_exact(nan["cost"][:, :1], nan["iou"][:, :1], nan["flags"][:, :1], [1])
    assert first["n_pos"][0] == 1


O_TAKEN = F32(100000.0)


def test_the_repair_case_carries_its_rows_over_and_is_cut_off():
    x = P.select_inputs("q100_dup")
    im = x["images"][0]
    carried = P.select_exact(im["cost"], im["iou"], im["flags"], im["valid"], P.MAX_ROUNDS)
    fresh = P.select_exact(im["cost"], im["iou"], im["flags"], im["valid"], P.MAX_ROUNDS, carry=False)
    assert carried["repaired"] and carried["status"] == 0
    assert np.array_equal(carried["pos"], fresh["pos"]) and not np.array_equal(carried["neg"], fresh["neg"])
    assert P.select_expected("q100_dup")["status"].tolist() == [0]
    # the first run needs exactly one round: max_rounds = 0 cuts it off (bit 2 from the first run), max_rounds = 1 does not
    for name, status in (("q100_dup_rounds0", 2), ("q100_dup_rounds1", 0)):
        y = P.select_inputs(name)
        assert all(np.array_equal(y["images"][0][k], im[k]) for k in ("cost", "iou", "flags"))
        assert P.select_expected(name)["status"].tolist() == [status], name
    assert np.array_equal(P.select_expected("q100_dup_rounds1")["neg"], P.select_expected("q100_dup")["neg"])
    cut0 = P.select_exact(im["cost"], im["iou"], im["flags"], im["valid"], 0)
    cut1 = P.select_exact(im["cost"], im["iou"], im["flags"], im["valid"], 1)
    print("first-run status with max_rounds 0, 1:", cut0["first_status"], cut1["first_status"])
    assert cut0["first_status"] == 2 and cut1["first_status"] == 0


def test_status_bit_2_comes_from_one_run_alone():
    """max_rounds = 0 on two hand-built images: the first run settles and the second is cut off; and the other way round.  A
    kernel that kept only one run's status would return 0 for one of them."""
    x, want = P.select_inputs("q100_split_rounds0"), P.select_expected("q100_split_rounds0")
    assert x["max_rounds"] == 0 and want["status"].tolist() == [2, 2]
    r30, r40, r50 = P.SPLIT_ROWS
    for im, second in zip(x["images"], (True, False)):
        wide = 0 if second else 1
        assert P.is_dyadic(im["iou"]) and _sums(im["iou"][:, wide], 10) == (1.25, 1.25) and _sums(im["iou"][:, wide], 100) == (2.65625, 2.65625)
        assert not im["iou"][:, 1 - wide].any() and (im["flags"] == 1).all()
        r = P.select_exact(im["cost"], im["iou"], im["flags"], im["valid"], 0)
        assert (r["first_status"], r["second_status"]) == ((0, 2) if second else (2, 0))
        assert not r["repaired"] and np.array_equal(r["cost"], im["cost"])              # (cut off before any + 100000)
        if second:
            assert np.argwhere(r["pos"]).tolist() == [[r30, 0], [r40, 1]] and np.argwhere(r["neg"]).tolist() == [[r30, 0], [r40, 0]]
        else:
            assert np.argwhere(r["pos"]).tolist() == [[r40, 0]] and np.argwhere(r["neg"]).tolist() == [[r40, 0], [r50, 1]]
        settled = P.select_exact(im["cost"], im["iou"], im["flags"], im["valid"], P.MAX_ROUNDS)
        assert settled["status"] == 0


def test_keys_flags_and_the_case_lists():
    want = P.select_expected("q100_keys_flags")
    assert want["status"].tolist() == [0, 8, 4, 8]
    assert (want["counts"][1] == -1).all() and (want["counts"][0] >= 0).all()
    x = P.select_inputs("q128_valid_patterns")
    assert [im["valid"].tolist() for im in x["images"]][3] == [0] * 16 and x["images"][0]["valid"].tolist() == [1] + [0] * 15
    assert x["images"][1]["valid"].tolist() == [0] * 16 + [1] and x["images"][2]["valid"][:3].tolist() == [1, 0, 1]
    want = P.select_expected("q128_valid_patterns")
    assert not P.block(want["pos"], x["off"], 128, 3).any() and want["status"].tolist() == [0] * 5
    b64 = P.select_inputs("q100_batch64")
    assert len(b64["images"]) == 64 and 0 in b64["sizes"][1:-1] and b64["sizes"][0] == 0
    assert {P.SELECT[n]["Q"] for n in P.SELECT} == set(P.SELECT_QS)
    assert set(P.SELECT_GS) <= {G for n in P.SELECT for G in P.select_inputs(n)["sizes"]}
    assert {c["Q"] for c in P.LOSS.values()} == set(P.LOSS_QS)
    assert {c["Q"] for c in P.BACKWARD.values()} == set(P.BACKWARD_QS) and {c["C"] for c in P.BACKWARD.values()} == set(P.BACKWARD_CS)
    assert {c["grads"] for c in P.BACKWARD.values()} == set(P.BACKWARD_GRADS)
    assert {v[0] for v in P.SCORES.values()} == set(P.SCORE_QS) and {v[1] for v in P.SCORES.values()} == set(P.SCORE_CS)
    assert {G for v in P.SCORES.values() for G in v[2]} == set(P.SCORE_GS)


@pytest.mark.parametrize("name", list(P.LOSS))
def test_loss_inputs_hold_their_conditions(name):
    p, c = P.problem("loss", name), P.LOSS[name]
    ls = P.reference("loss", name)["ls"]
    Q = p["Q"]
    assert P.is_dyadic(p["dot"]) and P.is_dyadic(p["cos"]) and np.abs(p["cos"]).max() <= 1
    roles = ls["roles"]
    edge = p["planted"]["edge_queries"]
    assert set(edge) == {q for q in P.EDGE_QUERIES if q < Q} | {Q - 1}
    assert all(roles[0, q] == 6 for q in edge) and int(((roles[0] & 4) != 0).sum()) == len(edge) == p["meta"][0, 3]      # item A: every edge query
    isneg = (roles[0] & 2) != 0
    rank = np.cumsum(isneg) - 1
    assert sorted(p["ranks"][:len(edge)].tolist()) == [int(rank[q]) for q in edge] and int(rank[Q - 1]) == int(isneg.sum()) - 1
    assert all(int(rank[q]) != q for q in edge if q > 1)                          # the positives before them shift the ranks
    assert not (roles[1] & 1).any() and (roles[1] & 2).any()                      # B: no positive
    assert not (roles[2] & 2).any() and (roles[2] & 1).any() and p["meta"][2, 3] == 0        # C: no negative, rcnt = 0
    d = len(p["meta"]) - 2
    assert p["meta"][d, 1] == p["off"][2] + P.INTERIOR and 0 < P.INTERIOR < 16
    assert ((roles[d] & 2) != 0).sum() == ((roles[d] & 4) != 0).sum() == p["meta"][d, 3] > 0         # D: every negative sampled
    assert p["meta"][-1, 3] == 0
    if c.get("nan_item"):
        assert p["meta"][-1, 4] == 0 and np.isnan(ls["stats"][-1, 1]) and np.isnan(ls["losses"][1]) and np.isfinite(ls["losses"][0])
    else:
        assert np.isfinite(ls["losses"]).all()
    assert bool(p["malformed"]) == bool(c.get("malformed"))
    for i in p["malformed"]:
        assert not roles[i].any() and not ls["stats"][i].any()
    if c.get("extreme"):
        mn, mp = ls["stats"][0, 2], ls["stats"][0, 3]
        assert mn == 80.0 and mp == 80.0
        with np.errstate(over="ignore"):
            assert np.isinf(F32(np.exp(F32(mn))) * F32(np.exp(F32(mp))))           # the unshifted product is no fp32 number
        assert np.isfinite(ls["stats"][0]).all() and ls["stats"][0, 0] > 160
    else:
        assert np.abs(p["dot"]).max() <= 8


@pytest.mark.parametrize("kind,name", [("scores", n) for n in P.SCORES] + [("backward", n) for n in P.BACKWARD])
def test_embedding_inputs_hold_their_conditions(kind, name):
    p = P.problem(kind, name)
    ref, key = p["ref"].copy(), p["key"].copy()
    for b, q in p["zero_rows"]["ref"]:
        assert float(np.sqrt((ref[b, q].astype(F64) ** 2).sum())) in (0.0, P.TINY)
        ref[b, q] = 0
    for b, q in p["zero_rows"]["key"]:
        assert float(np.sqrt((key[b, q].astype(F64) ** 2).sum())) in (0.0, P.TINY)
        key[b, q] = 0
    assert P.TINY < P.EPS and P.is_dyadic(ref) and P.is_dyadic(key)
    rows = [(int(m[0]), P.key_row(p["keys"], int(m[1]), p["Qk"])) for m in p["meta"]]
    assert set(p["zero_rows"]["key"]) <= set(rows)                   # a valid target points at the zero and at the sub-eps key row
    if kind == "backward":
        assert p["item_counts"] == [4, 0, 3] and p["valid"][0] == 0
        assert rows[0] == rows[1] and rows[4] == rows[5] == rows[6] and rows[2] == (0, p["Qk"] - 1) and rows[3] == (0, 1)
        assert (p["keys"] < 0).any() and len(p["zero_rows"]["key"]) == 2 and (len(p["zero_rows"]["ref"]) == 2) == (p["Q"] >= 4)
        ls = P.reference(kind, name)["ls"]
        assert np.isfinite(ls["losses"]).all() and all((ls["roles"][i] != 0).any() for i in range(7))
        if p["Q"] >= 4:
            assert all(ls["roles"][i, 0] & 1 and ls["roles"][i, 1] == 6 for i in (4, 5, 6))
    elif max(p["sizes"]) >= 16:
        b = int(np.argmax(np.asarray(p["sizes"]) >= 16))
        v = p["valid"][p["off"][b]:p["off"][b + 1]]
        assert v[0] == 0 and v[1] == 1 and (p["keys"] < 0).any()
        assert len(set(rows)) < len(rows) and len(p["zero_rows"]["key"]) == 2


# --------------------------------------------------------------------------------------- the restatements against what exists

def old_case(name):
    """One of the six cases of tests/reid_cases.py as a problem of reid_parity: the selection by reid_ref.select, the ranks by
    replaying the reference's random.sample calls.  -> (problem, the wrapper's selection per image, reid_ref's)"""
    cfg = C.CASES[name]
    flat = C.make_inputs(cfg)
    bs, Q = len(cfg["images"]), cfg["Q"]
    sizes = [len(flat["valid_%d" % b]) for b in range(bs)]
    off = P.offsets(sizes)
    mpos, mneg, meta, ranks, counts, mine, theirs = [], [], [], [], [], [], []
    random.seed(C.SEED)
    for b in range(bs):
        valid = flat["valid_%d" % b]
        table = R.focal_table(flat["ref_cls"][b])
        want = R.select(table, flat["ref_box"][b], flat["boxes_%d" % b], flat["pm_%d" % b], valid) if sizes[b] else None
        theirs.append(want)
        if sizes[b]:
            cost, iou, flags = R.O.cost_terms(table, flat["ref_box"][b], flat["boxes_%d" % b], flat["pm_%d" % b])
            mine.append(P.select_exact(cost, iou, flags, valid))
        else:
            mine.append(None)
        count = 0
        if want is None:
            mpos.append(np.zeros((Q, sizes[b]), np.uint8)); mneg.append(np.zeros((Q, sizes[b]), np.uint8)); counts.append(0)
            continue
        for t in np.flatnonzero(valid):
            n_pos, n_neg = int(want["n_pos"][t]), int(want["n_neg"][t])
            drawn = random.sample(list(range(0, n_neg)), R.num_sample_neg(n_pos, n_neg))
            meta.append((b, off[b] + t, len(ranks), len(drawn), n_pos + len(drawn)))
            ranks.extend(drawn)
            count += 1
        mpos.append(want["pos"]); mneg.append(want["neg"]); counts.append(count)
    p = dict(name=name, Q=Q, Qk=cfg["Qk"], C=cfg["C"], sizes=sizes, off=off, ref=flat["hs_ref"], key=flat["hs_key"],
             valid=P.pack([flat["valid_%d" % b] for b in range(bs)], np.uint8), keys=P.pack([flat["idx_%d" % b] for b in range(bs)], np.int64),
             mpos=P.pack(mpos, np.uint8), mneg=P.pack(mneg, np.uint8), meta=np.asarray(meta, np.int32).reshape(-1, P.META),
             ranks=np.asarray(ranks or [0], np.int32), item_counts=counts, grads=np.asarray((1, 1), F32), hand_scores=False)
    return p, mine, theirs


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_restatements_equal_the_fixtures_and_the_float64_composition(name):
    from uninext_amd import reid
    from torch import nn
    p, mine, theirs = old_case(name)
    for a, b in zip(mine, theirs):                                   # the wrapper against reid_ref.select
        assert (a is None) == (b is None)
        if a is not None:
            assert all(np.array_equal(a[k], b[k]) for k in ("pos", "neg", "n_pos", "n_neg")) and a["status"] == b["status"] == 0
            assert a["repaired"] == b["repaired"]
    cfg = C.CASES[name]
    args = C.rebuild(C.make_inputs(cfg), len(cfg["images"]), embed_dtype=torch.float64)
    args[4].requires_grad_(True); args[5].requires_grad_(True)
    random.seed(C.SEED)
    items = reid.select_pos_neg(args[0], args[1], args[2], args[3], nn.Identity(), args[4], args[5], args[6], fused=False)
    losses = reid.loss_reid({"pred_qd": items, "reid_params": args[5].sum()}, None, None, 1.0)
    assert len(items) == len(p["meta"])
    sc = P.scores64(p)
    ls = P.loss64(p, sc)
    fixture = C.load_fixture(name) if cfg["fixture"] else None
    # (the reference normalises the auxiliary rows in fp32 -- `.float()` -- also when everything else is float64: its auxiliary
    # loss carries fp32 cosines, (C + 8) u each to first order)
    tol = (1e-11, (cfg["C"] + 8) * P.U)
    close = lambda got, want: float(np.abs(np.asarray(got) - np.asarray(want)).max()) <= tol[j] * max(1.0, float(np.abs(want).max()))
    for j, (key, grads) in enumerate((("loss_reid", (1, 0)), ("loss_reid_aux", (0, 1)))):
        bw = P.backward64(p, sc, ls, grads=grads)
        g_ref, g_key = torch.autograd.grad(losses[key], [args[5], args[4]], retain_graph=True)
        assert close(ls["losses"][j], float(losses[key].detach())) and close(bw["grad_ref"], g_ref.numpy()) and close(bw["grad_key"], g_key.numpy()), (name, key)
        if fixture is not None:
            assert close(ls["losses"][j], float(fixture[key])) and close(bw["grad_ref"], fixture["grad_ref." + key]), (name, key)
            assert close(bw["grad_key"], fixture["grad_key." + key]), (name, key)


# ------------------------------------------------------------------------------------------------------------------ the measure

FLOAT_CASES = [("scores", n) for n in P.SCORES] + [("loss", n) for n in P.LOSS] + [("backward", n) for n in P.BACKWARD]


def run_measure(kind, name, got, comp, check, which=None):
    p, ref = P.problem(kind, name), P.reference(kind, name)
    worst = []
    if kind != "loss" and (which in (None, "scores")):
        worst.append(P.measure_scores(name, p, got, ref["sc"], comp if comp is not None else ref["sc"], check))
    if kind != "scores" and (which in (None, "loss")):
        worst.append(P.measure_loss(name, got, ref["ls"], comp if comp is not None else ref["ls"], check))
    if kind == "backward" and (which in (None, "backward")):
        worst.append(P.measure_backward(name, got, ref["bw"], comp if comp is not None else ref["bw"], check))
    return max(worst)


@pytest.mark.parametrize("kind,name", FLOAT_CASES)
def test_the_fp32_composition_meets_the_derived_term_alone(kind, name):
    """The composition as `got`, the reference itself as `comp`: the composition term of the bound is zero, only SUM_DEPTH u s is
    left, and the project's bound on top.  No case is excluded and no entry but the unwritten norms."""
    p, ref = P.problem(kind, name), P.reference(kind, name)
    since = len(P.TABLE)
    got = P.composition(p, ref["ls"]["roles"], grads=None if kind == "backward" else False)
    worst = run_measure(kind, name, got, None, True)
    print(P.HEAD + "\n" + "\n".join(P.TABLE[since:]))
    del P.TABLE[since:]
    P.WORST.clear()
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------------ the teeth

MUTANTS = {
    "drop_own": ("backward", "q257_c64_g0_1"),
    "key_wrong_row": ("backward", "q4_c192_g0_1"),
    "rank_pass": ("loss", "q513"),
    "max_all": ("loss", "q257_extreme"),
    "first_valid_0": ("scores", "q15_c192_g16"),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_each_mutant_is_rejected(mutant):
    kind, name = MUTANTS[mutant]
    p, ref = P.problem(kind, name), P.reference(kind, name)
    comp = P.composition(p, ref["ls"]["roles"], grads=None if kind == "backward" else False)
    assert run_measure(kind, name, comp, comp, False) <= 1.0
    if kind == "scores":
        wrong = P.scores64(p, mutant=mutant)
    elif kind == "loss":
        wrong = P.loss64(p, None, mutant=mutant)
        if mutant == "rank_pass":
            assert not np.array_equal(wrong["roles"], ref["ls"]["roles"]) and np.array_equal(wrong["roles"][:, :256], ref["ls"]["roles"][:, :256])
    else:
        wrong = dict(ref["ls"], **P.backward64(p, ref["sc"], ref["ls"], mutant=mutant))
        wrong.update({k: ref["sc"][k] for k in P.SCORE_OUTPUTS})
    ratio = run_measure(kind, name, wrong, comp, False)
    print(mutant, name, "error / bound", ratio)
    assert ratio > 1.0


def test_drop_own_is_rejected_on_a_row_far_below_the_largest():
    """What the aggregate measure lets through: the mutant's largest error relative to the LARGEST entry of grad_ref is below the
    project's 1e-4 on some case's row, while that row is wrong by more than its own bound."""
    kind, name = MUTANTS["drop_own"]
    p, ref = P.problem(kind, name), P.reference(kind, name)
    wrong = P.backward64(p, ref["sc"], ref["ls"], mutant="drop_own")
    err = np.abs(wrong["grad_ref"] - ref["bw"]["grad_ref"])
    over = err > P.entry_bound(0.0, ref["bw"]["mag_grad_ref"])
    assert over.any()
    small = over & (err <= 1e-4 * np.abs(ref["bw"]["grad_ref"]).max())
    print("entries over their own bound: %d, of them under 1e-4 of the tensor's scale: %d" % (over.sum(), small.sum()))
    assert small.any()
