"""CPU: the PyTorch composition of uninext_amd/reid.py and the numpy restatement tests/reid_ref.py against the fixtures the
reference's select_pos_neg / loss_reid minted (tests/golden/make_reid_golden.py), the public names and signatures, the
criterion classes, the zero-item exit and the `random` contract.

Integers (positive sets, negative masks, sampled ranks) are held to equality.  Losses and gradients are float32 here against
float64 in the fixtures: scaled_error <= 1e-4 (tests/criterion_cases.py)."""
import hashlib
import inspect
import json
import os
import random
import sys

import numpy as np
import pytest
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import reid_cases as C  # noqa: E402
import reid_ref as R  # noqa: E402

REF_FILE = os.path.join(os.environ.get("UNINEXT_REFERENCE", "/root/reference"), "projects/UNINEXT/uninext/models/pos_neg_select.py")


def run_composition(name, dtype=torch.float32):
    from uninext_amd import reid
    cfg = C.CASES[name]
    g = C.load_fixture(name)
    bs = len(cfg["images"])
    ref_box, all_indices, targets, det_targets, hs_key, hs_ref, ref_cls = C.rebuild(g, bs, embed_dtype=dtype)
    hs_key.requires_grad_(True)
    hs_ref.requires_grad_(True)
    random.seed(C.SEED)
    items = reid.select_pos_neg(ref_box, all_indices, targets, det_targets, nn.Identity(), hs_key, hs_ref, ref_cls)
    return g, items, hs_key, hs_ref


@pytest.mark.parametrize("name", C.FIXTURES)
def test_composition_reproduces_the_fixture(name):
    from uninext_amd import reid
    g, items, hs_key, hs_ref = run_composition(name)
    assert len(items) == len(g["item_image"])
    assert hashlib.sha256(repr(random.getstate()).encode()).hexdigest() == str(g["state_hash"])      # the generator is where the reference left it
    for i, it in enumerate(items):
        b = int(g["item_image"][i])
        pos, neg = np.nonzero(g["pos"][i])[0], np.nonzero(g["neg"][i])[0]
        ranks = g["ranks"][g["rank_off"][i]:g["rank_off"][i + 1]]
        key = hs_key[b, int(g["idx_%d" % b][g["item_target"][i]])]
        # the rows behind the item are the fixture's queries, index for index: rebuilt from them the scores are bitwise the item's
        rows = torch.cat([hs_ref[b][pos], hs_ref[b][neg]])
        assert torch.equal(it["contrast"][:, 0], torch.einsum("nc,kc->nk", [rows, key[None]])[:, 0])
        assert it["label"].tolist() == [1.0] * len(pos) + [0.0] * len(neg)
        aux_rows = nn.functional.normalize(torch.cat([hs_ref[b][pos], hs_ref[b][neg][ranks.tolist()]]), dim=1)
        assert torch.equal(it["aux_consin"][:, 0], torch.einsum("nc,kc->nk", [aux_rows, nn.functional.normalize(key[None], dim=1)])[:, 0])
        assert it["aux_label"].tolist() == [1.0] * len(pos) + [0.0] * len(ranks)
        want = g["contrast"][g["score_off"][i]:g["score_off"][i + 1]]
        assert C.scaled_error(it["contrast"].detach().numpy().reshape(-1), want) <= C.TOLERANCE
        want = g["aux_consin"][g["aux_off"][i]:g["aux_off"][i + 1]]
        assert C.scaled_error(it["aux_consin"].detach().numpy().reshape(-1), want) <= C.TOLERANCE
    losses = reid.loss_reid({"pred_qd": items, "reid_params": hs_ref.sum()}, None, None, 1.0)
    assert sorted(losses) == ["loss_reid", "loss_reid_aux"]
    for key in losses:
        g_ref, g_key = torch.autograd.grad(losses[key], [hs_ref, hs_key], retain_graph=True)
        errs = (C.scaled_error(float(losses[key]), g[key]), C.scaled_error(g_ref.numpy(), g["grad_ref." + key]),
                C.scaled_error(g_key.numpy(), g["grad_key." + key]))
        print("%s %s: composition loss %.3e grad_ref %.3e grad_key %.3e (scaled errors against float64)" % ((name, key) + errs))
        assert max(errs) <= C.TOLERANCE, errs


@pytest.mark.parametrize("name", C.FIXTURES)
def test_restatement_integers_equal_the_fixture(name):
    g = C.load_fixture(name)
    cfg = C.CASES[name]
    i = 0
    for b in range(len(cfg["images"])):
        valid = g["valid_%d" % b]
        got = R.select(R.focal_table(g["ref_cls"][b]), g["ref_box"][b], g["boxes_%d" % b], g["pm_%d" % b], valid)
        if got is None:
            assert not valid.any()
            continue
        assert got["status"] == 0
        for t in np.nonzero(valid)[0]:
            assert (int(g["item_image"][i]), int(g["item_target"][i])) == (b, t)
            assert np.array_equal(got["pos"][:, t], g["pos"][i]) and np.array_equal(1 - got["neg"][:, t], g["neg"][i])
            assert (got["n_pos"][t], got["n_neg"][t]) == (g["pos"][i].sum(), g["neg"][i].sum())
            assert g["rank_off"][i + 1] - g["rank_off"][i] == R.num_sample_neg(int(got["n_pos"][t]), int(got["n_neg"][t]))
            i += 1
    assert i == len(g["item_image"])


def test_case_table_covers_what_it_claims():
    """The repair case's first run repairs, and the carried-over rows change the second run against a fresh cost matrix; the
    all-negatives case samples every negative of an item; every fixture keeps its IoU sums clear of the integers."""
    g = C.load_fixture("reid_q160_repair_c64")
    changed = 0
    for b in range(2):
        args = (R.focal_table(g["ref_cls"][b]), g["ref_box"][b], g["boxes_%d" % b], g["pm_%d" % b], g["valid_%d" % b])
        carried, fresh = R.select(*args), R.select(*args, carry=False)
        assert carried["repaired"]
        assert np.array_equal(carried["pos"], fresh["pos"])
        changed += int(not np.array_equal(carried["neg"], fresh["neg"]))
    assert changed == 2
    for name in C.FIXTURES:
        g = C.load_fixture(name)
        assert C.candidate_sum_margin(g, len(C.CASES[name]["images"])) > 1e-3
        for key, value in C.make_inputs(C.CASES[name]).items():
            assert np.array_equal(value, g[key]), (name, key)           # the fixture's inputs are the case table's
    g = C.load_fixture("reid_q130_allneg_c64")
    n_pos, n_neg, drawn = g["pos"].sum(1), g["neg"].sum(1), np.diff(g["rank_off"])
    assert any(10 * p >= n and d == n for p, n, d in zip(n_pos, n_neg, drawn))
    g = C.load_fixture("reid_q130_mixed_c64")
    assert g["valid_1"].tolist() == [False, True, False, True, True, False] and g["idx_1"][1] == g["idx_1"][3]


def test_signatures_equal_the_references():
    """Names, order and defaults against the signatures recorded at mint time (and against the reference itself where it is at
    hand); `fused=None` is the one addition, last."""
    import ast
    from uninext_amd import reid
    want = json.load(open(os.path.join(C.GOLDEN, "signatures.json")))
    assert sorted(want) == ["dynamic_k_matching", "get_in_boxes_info", "get_pos_idx", "loss_reid", "select_pos_neg"]
    if os.path.exists(REF_FILE):
        for n in ast.parse(open(REF_FILE).read()).body:
            if isinstance(n, ast.FunctionDef) and n.name in want:
                a = n.args
                defaults = [None] * (len(a.args) - len(a.defaults)) + [ast.literal_eval(d) for d in a.defaults]
                assert [[x.arg, d] for x, d in zip(a.args, defaults)] == want[n.name], n.name
    for name, sig in want.items():
        mine = [[p.name, None if p.default is p.empty else p.default] for p in inspect.signature(getattr(reid, name)).parameters.values()]
        if name == "loss_reid":
            sig = sig[1:]                      # a function here: no self
        if name == "select_pos_neg":
            assert mine[-1] == ["fused", None]
            mine = mine[:-1]
        assert mine == sig, name
    assert reid.FUSED is True              # the default follows profiles/r21_reid.txt


def test_video_criteria_accept_reid_and_return_the_two_keys():
    import uninext_amd
    from uninext_amd import reid
    from uninext_amd.criterion import DINOCriterion, SetCriterion
    with pytest.raises(NotImplementedError):
        SetCriterion(None, {}, ["labelsVL", "reid"])
    crit = uninext_amd.VideoSetCriterion(None, {}, ["labelsVL", "reid"])
    assert isinstance(crit, SetCriterion) and crit.losses == ["labelsVL", "reid"]
    assert issubclass(uninext_amd.VideoDINOCriterion, DINOCriterion)
    assert uninext_amd.VideoDINOCriterion(None, {}, ["reid"]).losses == ["reid"]
    g, items, hs_key, hs_ref = run_composition("reid_q100_c64")
    outputs = {"pred_qd": items, "reid_params": hs_ref.sum()}
    got = crit.get_loss("reid", outputs, None, None, 1.0)
    want = reid.loss_reid(outputs, None, None, 1.0)
    assert sorted(got) == ["loss_reid", "loss_reid_aux"] and all(torch.equal(got[k], want[k]) for k in got)
    for name in ("select_pos_neg", "get_pos_idx", "get_in_boxes_info", "dynamic_k_matching", "loss_reid"):
        assert getattr(uninext_amd, name) is getattr(reid, name)


def test_zero_items_exit():
    from uninext_amd import reid
    cfg = {"seed": 7, "Q": 100, "Qk": 4, "C": 64, "T": 8, "images": [C._img(0), C._img(2, valid=[0, 0])]}
    flat = C.make_inputs(cfg)
    ref_box, all_indices, targets, det_targets, hs_key, hs_ref, ref_cls = C.rebuild(flat, 2)
    items = reid.select_pos_neg(ref_box, all_indices, targets, det_targets, nn.Identity(), hs_key, hs_ref, ref_cls)
    assert items == []
    params = torch.ones((), requires_grad=True)
    losses = reid.loss_reid({"pred_qd": items, "reid_params": params}, None, None, 1.0)
    assert float(losses["loss_reid"]) == 0.0 and float(losses["loss_reid_aux"]) == 0.0 and losses["loss_reid"].requires_grad


def test_generator_state_follows_the_references_sample_calls():
    """After the call the generator is where the reference's sequence of random.sample calls leaves it: the same population and
    k per item, in item order."""
    g, items, _, _ = run_composition("reid_q130_mixed_c64")
    after = random.getstate()
    random.seed(C.SEED)
    for i in range(len(items)):
        n_pos, n_neg = int(g["pos"][i].sum()), int(g["neg"][i].sum())
        drawn = random.sample(list(range(0, n_neg)), R.num_sample_neg(n_pos, n_neg))
        assert drawn == g["ranks"][g["rank_off"][i]:g["rank_off"][i + 1]].tolist()
    assert random.getstate() == after


def test_fewer_than_100_queries_raise_what_topk_raises():
    from uninext_amd import reid
    cfg = {"seed": 8, "Q": 99, "Qk": 4, "C": 64, "T": 8, "images": [C._img(2)]}
    ref_box, all_indices, targets, det_targets, hs_key, hs_ref, ref_cls = C.rebuild(C.make_inputs(cfg), 1)
    with pytest.raises(RuntimeError):
        reid.select_pos_neg(ref_box, all_indices, targets, det_targets, nn.Identity(), hs_key, hs_ref, ref_cls)
