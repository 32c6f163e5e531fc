"""Two-stage query selection on the CPU: state-dict keys, the composition route in float64 against the reference's fixtures
(tests/golden/query_selection/, minted by tests/golden/make_query_selection_golden.py), the last-bit validity rule, and the new
rows of the binding's signature table against the header."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import query_selection_cases as C          # noqa: E402
import test_binding_signatures_cpu as SIG   # noqa: E402

EXACT = 1e-10
OUTPUTS = ("reference_points", "topk_coords_unact", "topk_proposals", "enc_outputs_class", "enc_outputs_coord_unact")


def case(name):
    fx = C.load(name)
    cfg, states, x = C.make_case(name, int(fx["seed"]))
    assert C.digest(states) == float(fx["digest"])
    assert np.array_equal(x["memory"].numpy(), fx["memory"].astype(np.float64)) and np.array_equal(x["mask"].numpy(), fx["mask"])
    assert np.array_equal(x["lang_feat_pool"].numpy(), fx["lang_feat_pool"].astype(np.float64))
    return fx, cfg, states, x


def same(got, want, tol=EXACT):
    """Equal infinities in equal places, finite entries within tol (absolute)."""
    got, want = got.detach().double().numpy(), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf])
    assert not np.isnan(got).any()
    assert float(np.abs(got[~inf] - want[~inf]).max()) <= tol


@pytest.mark.parametrize("name", list(C.FIXTURES))
def test_state_dict_keys_and_shapes_are_the_references(name):
    fx, cfg, states, x = case(name)
    mods = C.build(cfg, states, torch.float64)           # a strict load
    recorded = C.recorded_keys(fx)
    assert set(recorded) == set(mods)
    for k, m in mods.items():
        assert [[n, list(v.shape)] for n, v in m.state_dict().items()] == recorded[k], k


@pytest.mark.parametrize("name", list(C.FIXTURES))
def test_composition_in_float64_reproduces_the_fixture(name):
    from uninext_amd import modules as M
    fx, cfg, states, x = case(name)
    mods = C.build(cfg, states, torch.float64)
    out = C.run(cfg, mods, x)
    for k, got in zip(OUTPUTS, out):
        if k == "topk_proposals":
            assert got.dtype == torch.long and np.array_equal(got.numpy(), fx[k])
        else:
            same(got, fx[k])
    assert C.run(cfg, mods, x, all_coords=False)[4] is None
    with torch.no_grad():
        memory, proposals = M.gen_encoder_output_proposals(x["memory"], x["mask"], x["shapes"], mods["enc_output"],
                                                           mods["enc_output_norm"])
    assert proposals.dtype == torch.float32               # the proposals are fp32 whatever the memory's type
    same(proposals, fx["output_proposals"], 0.0)
    same(memory[:, torch.as_tensor(fx["memory_rows"])], fx["output_memory"])
    # a list of (H, W) is read like the tensor
    with torch.no_grad():
        again = M.gen_encoder_output_proposals(x["memory"], x["mask"], [tuple(s) for s in x["shapes"].tolist()],
                                               mods["enc_output"], mods["enc_output_norm"])
    assert torch.equal(again[0], memory) and torch.equal(again[1], proposals)


def test_pooling_helper_and_general_head():
    from uninext_amd import modules as M
    fx, cfg, states, x = case("vl_align")
    feats, tokens = torch.from_numpy(fx["agg_features"]), torch.from_numpy(fx["agg_mask"])
    same(M.agg_lang_feat(feats, tokens, "average"), fx["agg_average"])
    same(M.agg_lang_feat(feats, tokens, "max"), fx["agg_max"], 0.0)
    with pytest.raises(ValueError):
        M.agg_lang_feat(feats, tokens, "median")
    mods = C.build(cfg, states, torch.float64)
    with torch.no_grad():
        memory, _ = M.gen_encoder_output_proposals(x["memory"], x["mask"], x["shapes"], mods["enc_output"], mods["enc_output_norm"])
        same(mods["class_embed"](memory[:, :9], feats), fx["align_general"])


def test_width_50_puts_columns_0_and_49_out_on_the_last_bit():
    from uninext_amd.modules.query_selection import encoder_output_proposals
    assert np.float32(0.5) / np.float32(50) == np.float32(0.01) and np.float32(49.5) / np.float32(50) == np.float32(0.99)
    for W, out in ((50, [0, 49]), (49, []), (51, [0, 50]), (100, [0, 99])):
        proposals, valid = encoder_output_proposals(torch.zeros(1, 2 * W, dtype=torch.bool), [(2, W)])
        assert proposals.dtype == torch.float32
        cols = sorted(set((~valid[0, :, 0]).nonzero().flatten().remainder(W).tolist()))
        assert cols == out, (W, cols)
    fx = C.load("vl_align")
    dead0 = np.isinf(fx["output_proposals"][0]).any(-1)
    assert sorted(dead0.nonzero()[0].tolist()) == [0, 49, 50, 99, 100, 149]        # image 0: nothing else is out


def test_fused_is_ignored_on_the_cpu():
    from uninext_amd import modules as M
    assert M.TwoStageQuerySelection.fused in (False, True)
    fx, cfg, states, x = case("one_level")
    mods = C.build(cfg, states, torch.float64)
    plain, fused = C.run(cfg, mods, x, fused=False), C.run(cfg, mods, x, fused=True)
    for a, b in zip(plain, fused):
        assert torch.equal(a, b)
    out = M.select_queries(x["memory"], x["mask"], x["shapes"], mods["enc_output"], mods["enc_output_norm"], mods["class_embed"],
                           mods["bbox_embed"], x["lang_feat_pool"], cfg["topk"], fused=True)
    assert out[0].requires_grad and out[4] is None         # autograd records: PyTorch's composition
    same(out[0], fx["reference_points"])


def test_new_signature_rows_parse_against_the_header():
    from uninext_amd import _lib
    declared = SIG.prototypes(os.path.join(SIG.ROOT, "include", "dynmask_hip.h"))
    group = _lib._SIGNATURES["dynmask_hip.h"]
    for name in ("qsel_scores_hip_f32", "qsel_boxes_hip_f32", "qsel_hip_last_kernel"):
        assert name in declared and name in group and name in _lib.DYNMASK_EXPORTS
        restype, argtypes = group[name]
        row = (SIG.ctypes_kind(restype, name), [SIG.ctypes_kind(t, name) for t in argtypes])
        assert row == declared[name], (name, row, declared[name])
    assert group["qsel_hip_last_kernel"] == (ctypes.c_char_p, [])
    assert declared["qsel_scores_hip_f32"][1][-1] == "pointer" and declared["qsel_boxes_hip_f32"][1][-1] == "pointer"   # the stream
    assert _lib.ABI_VERSION == 2


def restated(fx, cfg, states, x):
    """tests/query_selection_ref.py on a fixture's inputs, its proposal logit rounded to fp32 as the fixture's generator did."""
    import query_selection_ref as R
    n = lambda t: t.double().numpy()
    enc, norm, box = states["enc_output"], states["enc_output_norm"], states["bbox_embed"]
    terms = R.vl_align_terms({k: n(v) for k, v in states["class_embed"].items()}, n(x["lang_feat_pool"])) \
        if cfg["head"] == "vl_align" else R.still_terms({k: n(v) for k, v in states["class_embed"].items()})
    mlp = [n(box["layers.%d.%s" % (i, k)]) for i in range(3) for k in ("weight", "bias")]
    return R.select(n(x["memory"]), x["mask"].numpy(), cfg["levels"], (n(enc["weight"]), n(enc["bias"])),
                    (n(norm["weight"]), n(norm["bias"])), 1e-5, terms, mlp, cfg["topk"], fp32_logit=True)


@pytest.mark.parametrize("name", list(C.FIXTURES))
def test_float64_restatement_reproduces_the_fixture(name):
    fx, cfg, states, x = case(name)
    r = restated(fx, cfg, states, x)
    t = torch.from_numpy
    same(t(r["logits"]).unsqueeze(-1), fx["enc_outputs_class"])
    same(t(r["output_memory"][:, fx["memory_rows"]]), fx["output_memory"])
    same(t(r["coords"]), fx["enc_outputs_coord_unact"])
    same(t(r["output_proposals"]), fx["output_proposals"])
    assert np.array_equal(r["topk"], fx["topk_proposals"])                          # exactly, in order
    same(t(np.take_along_axis(r["coords"], r["topk"][..., None], 1)), fx["topk_coords_unact"])
    same(t(np.take_along_axis(r["points"], r["topk"][..., None], 1)), fx["reference_points"])
    assert np.array_equal(r["live"], ~np.isinf(fx["output_proposals"]).any(-1))
    # the magnitudes dominate the values they belong to
    assert (r["mag_logits"] >= np.abs(r["logits"]) * (1 - 1e-12)).all()
    assert (r["mag_memory"] >= np.abs(r["output_memory"]) * (1 - 1e-12)).all()
    live = r["live"]
    assert (r["mag_coords"][live] >= np.abs(r["coords"][live]) * (1 - 1e-12)).all()


def test_restatement_and_module_agree_on_every_validity_bit_of_the_grid():
    """Every pair (x, valid) with x < valid <= 128, as a column and as a row: the restatement's numpy fp32 division against the
    module's torch fp32 division on the CPU.  The grid holds quotients that ARE fp32(0.01) and fp32(0.99), where the strict
    comparison decides on the last bit."""
    import query_selection_ref as R
    from uninext_amd.modules.query_selection import encoder_output_proposals, valid_sizes
    mask, levels = R.validity_grid()
    assert mask.shape == (128, 256) and sum(h * w for h, w in levels) == 256
    q = R.grid_quotients()
    assert (q == R.LO).any() and (q == R.HI).any() and q[49, 0] == R.LO and q[49, 49] == R.HI
    cx, cy, wh, live, valid_wh = R.proposals(mask, levels)
    proposals, valid = encoder_output_proposals(torch.from_numpy(mask), levels)
    assert proposals.dtype == torch.float32
    assert np.array_equal(live, valid[..., 0].numpy())          # a padded token of the grid has x >= valid: out by the rule itself
    assert np.array_equal(np.stack((cx, cy, wh, wh), -1)[~mask], proposals.numpy()[~mask])      # the quotients themselves, bitwise
    assert np.array_equal(valid_wh, valid_sizes(torch.from_numpy(mask), levels).numpy())
    # what the grid decides: x = 0 is out from valid = 50 on (0.5 / 50 rounds to fp32(0.01) itself), and so is x = valid - 1
    want = ~np.isnan(q) & (q > R.LO) & (q < R.HI)
    assert np.array_equal(live[:, :128], want) and np.array_equal(live[:, 128:], want)
    assert not want[49, 0] and not want[49, 49] and want[48, 0] and want[48, 48]
