"""No GPU: the conditions the cases of tests/loss_parity.py claim, its restatements against what exists, and the teeth of the
measure.

Conditions (none is a tolerance): every input is a number float64 sees exactly (dyadic logits, targets and similarities, the
planted thresholds, quarter-valued images whose pooling is exact); the case lists reach every size the sweep names; the ties sit
where the plants say; the last slice of the two large mask cases is empty by the restated slice formula and no smaller case has
one; the LDS widths are the limit of tile_bytes; the excluded share of every output is 0.

Pins: the restatements equal the float64 evaluation of the compositions on the generic cases of tests/criterion_cases.py and
tests/boxinst_cases.py, the stored targets of tests/golden/boxinst/targets.npz (bitmasks exactly, similarities within the project's
bound), and the fp32 compositions on the CPU meet the bound on every small case.

Teeth: every mutant of MUTANTS, rounded to fp32, exceeds the per-entry bound against the true restatement on the case named
there; the test prints which of them the aggregate scaled_error <= 1e-4 would have let through."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import boxinst_cases as BC      # noqa: E402
import criterion_cases as CC    # noqa: E402
import loss_parity as P         # noqa: E402

F32, F64 = np.float32, np.float64


def close(got, want, rel=1e-11):
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    assert got.shape == want.shape
    assert np.all(np.abs(got - want) <= rel * np.maximum(np.abs(want), np.abs(want).max() * 1e-3 + 1e-300)), float(np.abs(got - want).max())


# ---------------------------------------------------------------------------------------------------------------- the conditions

def test_the_constants_are_imported_not_redefined():
    import query_selection_ref as Q
    assert (P.U, P.SUM_DEPTH, P.COMP_MARGIN, P.TOL) == (Q.U, Q.SUM_DEPTH, Q.COMP_MARGIN, CC.MARGIN) and P.entry_bound is Q.entry_bound
    assert P.UNWRITTEN == {}                                    # nothing is excluded from any comparison


def test_token_cases_hold_their_conditions():
    assert {c["T"] for c in P.TOKEN.values()} == set(P.TOKEN_TS) and {c["B"] * c["Q"] for c in P.TOKEN.values()} >= set(P.TOKEN_ROWS)
    assert {c["mask"] for c in P.TOKEN.values()} == {"none", "int64", "bool"}
    assert any(c["B"] == 3 and c["Q"] == 3 for c in P.TOKEN.values())
    assert all(c["T"] % 4 == 0 for c in P.TOKEN.values() if c["misaligned"]) and sum(c["misaligned"] for c in P.TOKEN.values()) == 2
    seen, targets = set(), set()
    for name in P.TOKEN:
        p = P.token_inputs(name)
        assert P.is_dyadic(p["logits"]) and P.is_dyadic(p["pm"]) and p["pm"].min() >= 0 and p["pm"].max() <= 1
        seen |= set(np.abs(p["logits"][np.abs(p["logits"]) >= 10]).tolist())
        targets |= set(p["row_target"].reshape(-1).tolist())
        ref = P.token64(p)
        if p["mask"] is not None:                               # a masked token: value 0, s 0
            dead = ~ref["counted"]
            assert dead.any() or p["logits"].shape[2] < 3
            assert not ref["grad"][dead].any() and not ref["mag_grad"][dead].any()
        assert np.isfinite(ref["mag_grad"]).all() and (ref["mag_grad"][ref["counted"]] > 0).all()
    assert seen == {10.0, 17.0, 30.0, 88.0, 100.0} and targets == {-1, 0, 1, 2, P.TOKEN_G}
    assert np.exp(F32(-88.0)) < 2.0 ** -126 < np.exp(F32(-87.0))          # where expf leaves the normal range


def test_mask_cases_hold_their_conditions():
    small = [n for n in P.MASK if not n.startswith("empty")]
    assert {c["F"] * c["h"] * c["w"] for n, c in P.MASK.items() if n in small} == set(P.MASK_PS)
    assert {c["stride"] for c in P.MASK.values()} == {1, 2, 3, 4}
    for P_ in (1024, 2048):
        assert {c["w"] % 4 == 0 for n, c in P.MASK.items() if n in small and c["F"] * c["h"] * c["w"] == P_} == {True, False}
    assert P.mask_slices(4, 1023)[0] == P.mask_slices(4, 1024)[0] == 1 and P.mask_slices(4, 1025) == (2, 516)
    for name in small:
        c = P.MASK[name]
        assert not P.empty_slices(c["n"], c["F"] * c["h"] * c["w"]), name
        p = P.mask_inputs(name)
        assert P.is_dyadic(p["src"]) and p["gt_row"].tolist() == [0, c["F"], -1, c["F"] + 1] and p["gt"].shape[0] == 2 * c["F"]
        start = c["stride"] // 2
        assert p["gt"].shape[1:] == (start + c["stride"] * (c["h"] - 1) + 1, start + c["stride"] * (c["w"] - 1) + 1)
        ref = P.mask64(p)
        assert ref["t"][1].all() and not ref["t"][2].any() and not ref["t"][3].any() and 0 < ref["t"][0].mean() < 1
        assert {10.0, 100.0} <= set(np.abs(p["src"][1]).reshape(-1).tolist()) and {10.0, 100.0} <= set(np.abs(p["src"][2]).reshape(-1).tolist())
        slices, chunk = P.mask_slices(c["n"], c["F"] * c["h"] * c["w"])
        inside = any(f * c["h"] * c["w"] % chunk for f in range(1, c["F"]))     # a frame boundary inside a slice ...
        assert inside != (c["F"] * c["h"] * c["w"] == 2048)                     # ... but at F = 2, P = 2048, where it IS the slice edge


def test_the_empty_slice_cases_are_the_smallest_of_the_restated_formula():
    # below 512 * 1024 pixels `most` = ceil(P / 1024) decides the slices and each holds pixels: sampled there, searched beyond
    assert not any(P.empty_slices(4, P_) for P_ in range(1, 4096))
    lo = next(P_ for P_ in range(512 * 1024 - 8, 512 * 1024 + 64) if P.empty_slices(4, P_))
    lo4 = next(P_ for P_ in range(512 * 1024 - 8, 512 * 1024 + 64) if P_ % 4 == 0 and P.empty_slices(4, P_))
    assert not any(P.empty_slices(4, P_) for P_ in range(1, 512 * 1024 - 8, 997)) and (lo, lo4) == (524289, 524292)
    for name, P_ in (("empty_slice_scalar", lo), ("empty_slice_vec4", lo4)):
        c = P.MASK[name]
        assert (c["n"], c["h"], c["stride"], c["F"] * c["h"] * c["w"]) == (4, 3, 1, P_) and (c["w"] % 4 == 0) == name.endswith("vec4")
        slices, chunk = P.mask_slices(4, P_)
        assert P.empty_slices(4, P_) == [slices - 1] and (slices - 2) * chunk < P_


def test_box_cases_hold_their_conditions():
    combos = {(c["d"], c["h"]) for c in P.BOX.values() if c["plant"] is None}
    assert combos >= {(d, h) for d in P.BOX_DS for h in P.BOX_HS}
    assert {c["stride"] for c in P.BOX.values()} == {1, 2, 3, 4}
    assert any(c["h"] < c["d"] and c["w"] < c["d"] for c in P.BOX.values()) and any(c["w"] < c["d"] <= c["h"] for c in P.BOX.values())
    assert any(c["h"] < c["d"] <= c["w"] for c in P.BOX.values())
    # the LDS limit, from tile_bytes
    assert (P.widest(1), P.widest(8), P.widest(2)) == (716, 298, 597)
    assert (P.BOX["lds_d1_w716"]["w"], P.BOX["lds_d8_w298"]["w"]) == (716, 298)
    assert P.tile_bytes(717, 1) > P.LDS_BYTES >= P.tile_bytes(716, 1) and P.tile_bytes(299, 8) > P.LDS_BYTES >= P.tile_bytes(298, 8)
    below = np.nextafter(P.THRESH, F32(0))
    for name, c in P.BOX.items():
        p = P.box_inputs(name)
        assert P.is_dyadic(p["src"]), name
        plain = (p["sim"] != P.THRESH) & (p["sim"] != below)
        assert P.is_dyadic(p["sim"][plain]) and (~plain).sum() >= 2 and (p["sim"] == P.THRESH).any() and (p["sim"] == below).any()
        assert len(set(p["inst"].tolist())) == len(p["inst"])                 # distinct rows: the contract
    ref = P.box64(P.box_inputs("d2_h17"))
    p = P.box_inputs("d2_h17")
    at = (p["sim"][p["img"]] == P.THRESH) & (ref["t"][:, None] != 0)
    assert at.any() and ref["weights"][at].all() and not ref["weights"][(p["sim"][p["img"]] == below)].any()


def test_the_ties_sit_where_the_plants_say():
    p = P.box_inputs("ties_h17_w200")
    ref, high = P.box64(p), P.box64(p, "tie_high")
    h = 17
    for i, r in enumerate(p["inst"]):
        x = p["src"][r, 0]
        for row, cols in P.TIE_ROWS.items():
            assert np.flatnonzero(x[row] == x[row].max()).tolist() == list(cols) and ref["pos"][i, row] == cols[0] and high["pos"][i, row] == cols[1]
        for col, rows in P.TIE_COLS.items():
            assert np.flatnonzero(x[:, col] == x[:, col].max()).tolist() == list(rows) and ref["pos"][i, h + col] == rows[0]
        others = [y for y in range(h) if y not in P.TIE_ROWS]
        assert all((x[y] == x[y].max()).sum() == 1 for y in others)
    (a, b), (c, d), (e, f) = (P.TIE_ROWS[k] for k in (0, 1, 2))
    assert a // 64 == b // 64 and a % 64 != b % 64 and c % 64 == d % 64 and c // 64 != d // 64 and e // 64 != f // 64 and e % 64 > f % 64 and e < f
    (a, b), (c, d), (e, f) = (P.TIE_COLS[k] for k in (0, 1, 2))
    assert a // 8 == b // 8 == 0 and (c // 8, d // 8) == (0, 1) and (e // 8, f // 8) == (1, 2)
    q = P.box_inputs("all_equal")
    ref = P.box64(q)
    assert len(set(q["src"].reshape(-1).tolist())) == 1 and not ref["pos"].any()


def test_the_weight_plants_are_what_they_claim():
    for name, rows in (("w_band_first_row", {8}), ("w_band_last_row", {15})):
        ref = P.box64(P.box_inputs(name))
        assert set(np.argwhere(ref["weights"].sum(1) > 0)[:, 1].tolist()) == rows and ref["totals"][1] > 0
    ref = P.box64(P.box_inputs("w_border_only"))
    inner = ref["weights"][:, :, 1:-1, 1:-1]
    assert not inner.any() and ref["totals"][1] > 0
    for name in ("no_weight", "img_out_of_range"):
        ref = P.box64(P.box_inputs(name))
        assert ref["totals"].tolist() == [0.0, 0.0] and ref["losses"][1] == 0 and not ref["grad_pair"].any() and not ref["mag_grad_pair"].any()
        assert ref["grad_prj"].any()
    p = P.box_inputs("rows_out_of_range")
    ref = P.box64(p)
    assert not ref["t"][2].any() and not ref["pos"][1].any() and not ref["grad_prj"][1].any() and not ref["mag_grad_prj"][1].any()
    # a pixel without a weighted term that is no maximum: value 0, s 0
    ref = P.box64(P.box_inputs("w_band_first_row"))
    quiet = ~ref["row_max"] & ~ref["col_max"]
    assert quiet.any() and not ref["grad_prj"][:, 0][quiet].any() and not ref["mag_grad_prj"][:, 0][quiet].any()
    assert (ref["grad_pair"] == 0).any() and not ref["mag_grad_pair"][ref["grad_pair"] == 0].any()


def test_colour_cases_hold_their_conditions():
    assert {(c["h"], c["w"]) for c in P.COLOR.values()} == {(h, w) for h in P.COLOR_HS for w in P.COLOR_WS}
    assert {(c["d"], c["stride"]) for c in P.COLOR.values()} == {(d, s) for d in P.COLOR_DS for s in P.COLOR_STRIDES}
    bytes_seen, quarter = set(), False
    for name, c in P.COLOR.items():
        for kind in ("u8", "f32"):
            p = P.color_inputs(name, kind)
            img = p["images"].astype(F64)
            assert np.all(img * 4 == np.round(img * 4)) and img.min() >= 0 and img.max() <= 255 and (kind == "f32" or p["images"].dtype == np.uint8)
            byte, mean = P.pooled_bytes(p["images"], c["stride"])
            assert np.all(mean * 64 == np.round(mean * 64))                     # the pooling is exact in any order
            s32 = p["images"].astype(F32).reshape(2, 3, c["h"], c["stride"], c["w"], c["stride"]).sum((3, 5), dtype=F32) / F32(c["stride"] ** 2)
            assert np.array_equal(s32.astype(F64), mean)
            bytes_seen |= set(byte.reshape(-1).tolist())
            y, x = p["blocks"][-1]
            if kind == "f32" and (c["w"] > 1 or c["h"] // 3 not in (0, c["h"] // 2, c["h"] - 1)):
                quarter |= bool(np.all(mean[:, :, y, x] == 76.75) and np.all(byte[:, :, y, x] == 76))
            ref = P.color64(p)
            alone = P.color64(p, keep=p["honest"])              # only the strided holes matter
            assert np.array_equal(ref["sim"], alone["sim"]) and (c["stride"] == 1 or not np.array_equal(p["keep"], p["honest"]))
            assert (p["honest"] == 0).any()
            outside = ref["sim"] == 0                           # a neighbour outside the image or not kept: value 0, s 0
            assert outside.any() and not ref["mag_sim"][outside].any()
    assert {0, 255, 77, P.GREY_BELOW, P.GREY_ABOVE} <= bytes_seen and quarter
    grey = np.full((1, 3, 1, 2), P.GREY_BELOW)
    grey[..., 1] = P.GREY_ABOVE
    _, xyz = P.lab64(grey)
    assert (xyz[..., 0] < 0.008856).all() and (xyz[..., 1] > 0.008856).all()


def test_bitmask_boxes_hold_their_conditions():
    for W in P.BITMASK_WS:
        b = P.bitmask_boxes(W)
        assert np.isnan(b).any() and np.isinf(b).any() and {-0.5, -1.0, -1.5} <= set(b[np.isfinite(b)].tolist())
        assert (b[:, 2] == W - 1).any() and (b[:, 2] == W).any() and (b[:, 2] < b[:, 0]).any() and ((b[:, 2] == b[:, 0]) & (b[:, 3] == b[:, 1])).any()
        want = P.bitmasks_exact(b, P.BITMASK_H, W)
        assert want[0].all() and not want[3:5].any() and want[5, 1:4, 1:].all() and want[5].sum() == 3 * (W - 1)      # a NaN far end: the edge
        assert want[6, 1:, 1:6].all() and want[6].sum() == 5 * (P.BITMASK_H - 1) and want[7, :3].all() and not want[7, 3:].any() and not want[8].any()
        assert want[11].sum() == want[12].sum() == want[13].sum() == 12 and int(want[18].sum()) == 1 and int(want[19].sum()) == 1
        assert not want[14:18].any() and not want[20].any()
        # the slice of the reference's composition, where it is defined (finite, non-negative coordinates)
        for slot, box in zip(want, b):
            if np.isfinite(box).all() and (box >= 0).all():
                ref = np.zeros((P.BITMASK_H, W), np.uint8)
                ref[int(box[1]):int(F32(box[3] + 1)), int(box[0]):int(F32(box[2] + 1))] = 1
                assert np.array_equal(slot, ref)
    assert {W % 16 == 0 for W in P.BITMASK_WS} == {True, False}


# ---------------------------------------------------------------------------------------------------------------------- the pins

@pytest.mark.parametrize("variant", ["int64", "bool", "unmatched", "fractional", "bool_fractional_extreme"])
def test_token_restatement_equals_the_float64_composition(variant):
    logits, mask, row_target, pm, want_loss, want_grad = CC.token_case(3, 130, 77, variant)
    p = dict(logits=logits.numpy(), mask=None if mask is None else mask.numpy().astype(np.int64), row_target=row_target.numpy(), pm=pm.numpy(),
             alpha=CC.ALPHA, scale=1.0)
    ref = P.token64(p)
    close(ref["loss"], want_loss)
    big = np.abs(logits.numpy()) < 20                           # (the composition's float64 1 - p has lost its digits beyond)
    close(ref["grad"][big], want_grad.numpy()[big], 1e-7)
    assert CC.scaled_error(ref["grad"], want_grad.numpy()) < 1e-12


@pytest.mark.parametrize("geometry", [(3, 1, 7, 9, 4), (2, 2, 13, 21, 4), (1, 1, 1, 1, 1)])
def test_mask_restatement_equals_the_float64_composition(geometry):
    src, gt, gt_row, want, want_grad = CC.mask_case(*geometry)
    p = dict(src=src.numpy(), gt=gt.view(-1, *gt.shape[-2:]).numpy().astype(np.uint8), gt_row=gt_row.numpy(), stride=geometry[4],
             num_boxes=CC.MASK_NUM_BOXES)
    a, b = P.mask64(p, (1.0, 0.0)), P.mask64(p, (0.0, 1.0))
    close(a["losses"], np.asarray(want))
    close(a["grad"] + 2.0 * b["grad"], want_grad.numpy(), 1e-9)
    tgt = CC.target_pixels(gt.view(-1, *gt.shape[-2:]), gt_row, *geometry[1:4], geometry[4])
    assert np.array_equal(a["t"] != 0, tgt.numpy()) and np.array_equal(a["sums"][:, 3], tgt.flatten(1).sum(1).numpy())


@pytest.mark.parametrize("geometry,variant", [((3, 17, 33), "plain"), ((2, 40, 68), "plain"), ((3, 17, 33), "bad_gt_row"), ((2, 5, 4), "subset"),
                                              ((3, 17, 33), "second_image"), ((2, 5, 4), "no_weight"), ((1, 3, 5), "thresh_negative")])
def test_boxinst_restatement_equals_the_float64_composition(geometry, variant):
    case = BC.kernel_case(*geometry, variant)
    gt = case["gt"]
    p = dict(src=case["src"].numpy(), inst=case["inst"].numpy(), gt=gt.view(-1, *gt.shape[-2:]).numpy().astype(np.uint8), gt_row=case["gt_row"].numpy(),
             sim=case["sim"].numpy(), img=case["img"].numpy(), thresh=case["thresh"], d=BC.DILATION, stride=BC.STRIDE, warmup=BC.WARMUP)
    ref = P.box64(p)
    close(ref["losses"], np.asarray(case["want"]), 1e-10)
    assert ref["totals"][1] == case["sum_w"] and np.array_equal(ref["t"] != 0, case["tgt"][:, 0].numpy())
    want = case["want_grad"].numpy()
    got = ref["grad_prj"] + 2.0 * ref["grad_pair"]
    assert CC.scaled_error(got, want) < 1e-9
    x = case["src"][case["inst"].long()][:, 0]
    h = geometry[1]
    assert np.array_equal(ref["pos"][:, :h], x.argmax(dim=2).numpy()) and np.array_equal(ref["pos"][:, h:], x.argmax(dim=1).numpy())


def _padded_fixture():
    images, heights, boxes = BC.make_target_inputs()
    H = max(-(-im.shape[1] // 32) * 32 for im in images)
    W = max(-(-im.shape[2] // 32) * 32 for im in images)
    batch, keep = np.zeros((len(images), 3, H, W), np.uint8), np.zeros((len(images), H, W), np.uint8)
    for b, (im, ht) in enumerate(zip(images, heights)):
        batch[b, :, :im.shape[1], :im.shape[2]] = im.numpy()
        removed = int(10 * float(im.shape[1]) / float(ht))
        keep[b, :im.shape[1] - removed, :im.shape[2]] = 1
    return batch, keep, boxes, H, W


def test_target_restatements_equal_the_stored_fixture():
    stored = BC.load_targets()
    batch, keep, boxes, H, W = _padded_fixture()
    ref = P.color64(dict(images=batch, keep=keep, stride=BC.STRIDE, d=BC.DILATION))
    for b in range(len(boxes)):
        assert np.array_equal(P.bitmasks_exact(boxes[b].numpy(), H, W) != 0, stored["masks.%d" % b].numpy())
        BC.within(ref["sim"][b], stored["sim.%d" % b].numpy().astype(F64), "sim")


def test_colour_restatement_equals_the_projects_composition():
    from uninext_amd.boxinst import rgb2lab
    p = P.color_inputs("h17_w16", "u8")
    ref, comp = P.color64(p), P.color_composition(p)
    byte = ref["byte"]
    close(ref["lab"], rgb2lab(byte[:, [2, 1, 0]].transpose(0, 2, 3, 1).astype(np.uint8)).transpose(0, 3, 1, 2), 1e-12)
    assert P.measure("color", "sim", "h17_w16", comp["sim"].astype(F32), ref["sim"], ref["mag_sim"]) <= 1.0
    table = P.srgb_table()
    assert table[0] == 0 and table[255] == 1 and table[10] == 10 / 255 / 12.92 and np.all(np.diff(table) > 0)


# ---------------------------------------------------------------------------- the fp32 compositions on the CPU meet the measure

@pytest.mark.parametrize("name", list(P.TOKEN))
def test_token_composition_meets_the_bound(name):
    p = P.token_inputs(name)
    ref, comp = P.token64(p), P.token_composition(p)
    P.measure("token", "loss", name, comp["loss"], ref["loss"], ref["mag_loss"], comp["loss"], aggregate=False)
    for sl, where in P.token_slices(p, ref).items():
        P.measure("token", sl, name, comp["grad"], ref["grad"], ref["mag_grad"], comp["grad"], where, aggregate=False)
    assert not comp["grad"][~ref["counted"]].any()


@pytest.mark.parametrize("name", [n for n in P.MASK if not n.startswith("empty")])
def test_mask_composition_meets_the_bound(name):
    p = P.mask_inputs(name)
    focal, dice = P.mask64(p, (1.0, 0.0)), P.mask64(p, (0.0, 1.0))
    comp = P.mask_composition(p, focal["t"])
    P.measure("mask", "losses", name, comp["losses"], focal["losses"], focal["mag_losses"], comp["losses"], aggregate=False)
    P.measure("mask", "focal", name, comp["grad_focal"], focal["grad"], focal["mag_grad"], comp["grad_focal"], aggregate=False)
    P.measure("mask", "dice", name, comp["grad_dice"], dice["grad"], dice["mag_grad"], comp["grad_dice"], aggregate=False)
    assert np.array_equal(comp["sums"][:, 3], focal["sums"][:, 3])


@pytest.mark.parametrize("name", [n for n in P.BOX if not n.startswith("lds")])
def test_boxinst_composition_meets_the_bound(name):
    p = P.box_inputs(name)
    ref = P.box64(p)
    comp = P.box_composition(p, ref)
    P.measure("boxinst", "losses", name, comp["losses"], ref["losses"], ref["mag_losses"], comp["losses"], aggregate=False)
    P.measure("boxinst", "prj", name, comp["grad_prj"], ref["grad_prj"], ref["mag_grad_prj"], comp["grad_prj"], aggregate=False)
    P.measure("boxinst", "pairwise", name, comp["grad_pair"], ref["grad_pair"], ref["mag_grad_pair"], comp["grad_pair"], aggregate=False)
    sl = P.box_slices(ref)
    assert not ref["grad_prj"][sl["neither"]].any() and not comp["grad_prj"][sl["neither"]].any()


# --------------------------------------------------------------------------------------------------------------------- the teeth

def r32(a):
    return np.asarray(a, F64).astype(F32).astype(F64)


def _token(name, mutant):
    p = P.token_inputs(name)
    ref, bad, comp = P.token64(p), P.token64(p, mutant), P.token_composition(p)
    return [("grad", r32(bad["grad"]), ref["grad"], ref["mag_grad"], comp["grad"])]


def _mask(name, mutant, grads, what="grad"):
    p = P.mask_inputs(name)
    ref, bad = P.mask64(p, grads), P.mask64(p, grads, mutant)
    comp = P.mask_composition(p, ref["t"])
    c = grads[0] * comp["grad_focal"] + grads[1] * comp["grad_dice"]
    return [("grad", r32(bad["grad"]), ref["grad"], ref["mag_grad"], c), ("sums", r32(bad["sums"]), ref["sums"], ref["mag_sums"], None),
            ("losses", r32(bad["losses"]), ref["losses"], ref["mag_losses"], comp["losses"])]


def _box(name, mutant):
    p = P.box_inputs(name)
    ref, bad = P.box64(p), P.box64(p, mutant)
    comp = P.box_composition(p, ref)
    return [("grad_prj", r32(bad["grad_prj"]), ref["grad_prj"], ref["mag_grad_prj"], comp["grad_prj"]),
            ("grad_pair", r32(bad["grad_pair"]), ref["grad_pair"], ref["mag_grad_pair"], comp["grad_pair"]),
            ("losses", r32(bad["losses"]), ref["losses"], ref["mag_losses"], comp["losses"])]


def _color(name, mutant):
    p = P.color_inputs(name, "u8")
    ref, bad, comp = P.color64(p), P.color64(p, mutant=mutant), P.color_composition(p)
    return [("sim", r32(bad["sim"]), ref["sim"], ref["mag_sim"], comp["sim"])]


# stride / 2 rounded up differs from stride / 2 at the odd strides: 3 among the loss cases, 1 among the colour cases (1, 2, 4)
STRIDE3 = next(n for n, c in P.BOX.items() if c["stride"] == 3 and c["plant"] is None and c["h"] >= 9)
COLOR_STRIDE1 = next(n for n, c in P.COLOR.items() if c["stride"] == 1 and c["w"] > 1)
# (kernel, mutant) -> the named case it has to fail on
MUTANTS = {
    ("boxinst", "nbr_order"): lambda: _box("d3_h17", "nbr_order"),
    ("color", "nbr_order"): lambda: _color("h17_w17", "nbr_order"),
    ("boxinst", "centre_weight"): lambda: _box("d2_h17", "centre_weight"),
    ("boxinst", "drop_halo"): lambda: _box("d7_h25", "drop_halo"),
    ("boxinst", "tie_high"): lambda: _box("ties_h17_w200", "tie_high"),
    ("mask", "start_up"): lambda: _mask("p1023_f3_11x31_s3", "start_up", (1.0, 0.0)),
    ("boxinst", "start_up"): lambda: _box(STRIDE3, "start_up"),
    ("color", "start_up"): lambda: _color(COLOR_STRIDE1, "start_up"),
    ("mask", "skip_last_slice"): lambda: _mask("p1025_f5_5x41_s2", "skip_last_slice", (0.0, 1.0)),
    ("color", "unstrided_mask"): lambda: _color("h16_w16", "unstrided_mask"),
    ("mask", "den_no_plus1"): lambda: _mask("p2048_f2_8x128_s2", "den_no_plus1", (0.0, 1.0)),
    ("token", "alpha_swap"): lambda: _token("b3_q3_t65_bool", "alpha_swap"),
    ("mask", "alpha_swap"): lambda: _mask("p1024_f2_16x32_s4", "alpha_swap", (1.0, 0.0)),
}




def test_every_mutant_is_rejected_per_entry():
    assert P.BOX["d7_h25"]["h"] > 8 + 7
    passed_aggregate, lines = [], []
    for (kernel, mutant), build in MUTANTS.items():
        worst, aggregate = 0.0, 0.0
        for what, got, want, mag, comp in build():
            worst = max(worst, P.measure(kernel, what, mutant, got, want, mag, comp, check=False))
            aggregate = max(aggregate, CC.scaled_error(got, want))
        lines.append("%-8s %-16s per-entry error / bound %10.3g   aggregate scaled_error %9.2e %s"
                     % (kernel, mutant, worst, aggregate, "(the aggregate measure accepts it)" if aggregate <= P.TOL else ""))
        if aggregate <= P.TOL:
            passed_aggregate.append((kernel, mutant))
        assert worst > 1.0, (kernel, mutant, worst)
    print("\n".join(lines))
    print("mutants the aggregate scaled_error <= 1e-4 lets through: %s" % (passed_aggregate or "none"))


def test_the_excluded_share_is_zero():
    """measure() takes a report slice, never an exclusion: the slices of a group partition its entries"""
    p = P.token_inputs("b3_q3_t65_bool")
    ref = P.token64(p)
    cover = sum(w.astype(int) for w in P.token_slices(p, ref).values())
    assert np.array_equal(cover, ref["counted"].astype(int)) and not ref["grad"][~ref["counted"]].any()
    ref = P.box64(P.box_inputs("d2_h17"))
    assert (sum(w.astype(int) for w in P.box_slices(ref).values()) == 1).all()
