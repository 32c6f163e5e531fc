"""The criterion without a GPU: the composition (`fused = False`) against the reference's loss dictionaries
(tests/golden/criterion/*.npz, minted by tests/golden/make_criterion_golden.py), the restated giou_loss on hand-built boxes, the
"last pair wins" rule of the matched rows, the exported names and signatures against the reference checkout's by `ast`, and the
losses that are not part of this repository."""
import ast
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import criterion_cases as C   # noqa: E402

REF = os.environ.get("UNINEXT_REFERENCE", "/root/reference")
REF_DIR = os.path.join(REF, "projects/UNINEXT/uninext/models/deformable_detr")


def test_fixtures_are_the_documented_ones():
    stored = sorted(os.path.splitext(f)[0] for f in os.listdir(C.GOLDEN) if f.endswith(".npz"))
    assert stored == sorted(C.CASES)
    for name, cfg in C.CASES.items():
        flat, expect = C.load(name)
        again = C.make_inputs(cfg)                              # the generator has not drifted from the stored inputs
        assert set(again) == set(flat)
        for k in flat:
            assert torch.equal(again[k], flat[k]), (name, k)
        assert ("loss_ce_dn" in expect) == cfg["dn"] and "loss_ce_enc" in expect and "loss_mask_0" in expect
        assert int(flat["out.text_masks"].sum()) < flat["out.text_masks"].numel()          # trailing zeros


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_composition_reproduces_the_reference(name):
    _, expect = C.load(name)
    got = C.run_fixture(name, fused=False)
    assert set(got) == set(expect)
    for key, want in expect.items():
        C.within(float(got[key]), want, key)            # 1e-4 of the value itself


def test_fused_on_the_cpu_is_the_composition():
    """The switch never selects a kernel for CPU tensors: the same numbers, bit for bit."""
    a, b = C.run_fixture("ota_dn", fused=False), C.run_fixture("ota_dn", fused=True)
    for key in a:
        assert torch.equal(a[key], b[key]), key


def test_giou_loss_on_hand_built_boxes():
    from uninext_amd.criterion import giou_loss
    f = lambda rows: torch.tensor(rows, dtype=torch.float64)
    eps = 1e-7
    # identical: iou = 4 / (4 + eps), no excess hull
    same = giou_loss(f([[0, 0, 2, 2]]), f([[0, 0, 2, 2]]))
    assert abs(float(same) - (1 - 4 / (4 + eps))) < 1e-15
    # disjoint: no intersection, union 2, hull 3 x 1: 1 + (3 - 2) / (3 + eps)
    apart = giou_loss(f([[0, 0, 1, 1]]), f([[2, 0, 3, 1]]))
    assert abs(float(apart) - (1 + 1 / (3 + eps))) < 1e-15
    # touching edges are not an intersection (strict inequalities): union 2, hull 2: loss exactly 1
    assert float(giou_loss(f([[0, 0, 1, 1]]), f([[1, 0, 2, 1]]))) == 1.0
    # nested: intersection 1, union 16, hull 16
    nested = giou_loss(f([[0, 0, 4, 4]]), f([[1, 1, 2, 2]]))
    assert abs(float(nested) - (1 - 1 / (16 + eps))) < 1e-15
    # degenerate zero-area against itself: 0 / eps and 0 / eps: loss 1, finite
    assert float(giou_loss(f([[1, 1, 1, 1]]), f([[1, 1, 1, 1]]))) == 1.0
    # zero-area point inside a box: union 4, hull 4: loss 1
    assert float(giou_loss(f([[1, 1, 1, 1]]), f([[0, 0, 2, 2]]))) == 1.0
    both = giou_loss(f([[0, 0, 2, 2], [0, 0, 1, 1]]), f([[0, 0, 2, 2], [2, 0, 3, 1]]))
    assert both.shape == (2,)
    assert abs(float(giou_loss(f([[0, 0, 2, 2], [0, 0, 1, 1]]), f([[0, 0, 2, 2], [2, 0, 3, 1]]), reduction="sum")) - float(both.sum())) < 1e-15
    assert abs(float(giou_loss(f([[0, 0, 2, 2], [0, 0, 1, 1]]), f([[0, 0, 2, 2], [2, 0, 3, 1]]), reduction="mean")) - float(both.mean())) < 1e-15
    assert float(giou_loss(torch.zeros(0, 4), torch.zeros(0, 4), reduction="mean")) == 0.0
    with pytest.raises(AssertionError):
        giou_loss(f([[2, 0, 1, 1]]), f([[0, 0, 1, 1]]))


def test_a_query_listed_twice_keeps_its_last_pair():
    from uninext_amd.criterion import matched_rows
    idx = lambda *v: torch.tensor(v, dtype=torch.int64)
    indices = [(idx(3, 1, 3, 0, 3), idx(0, 1, 2, 1, 1)), (idx(), idx()), (idx(2, 2), idx(1, 0))]
    rows = matched_rows(indices, [0, 3, 3], 4, torch.device("cpu"))
    assert rows.dtype == torch.int32
    # the reference's loop, pair after pair
    want = torch.full((3, 4), -1, dtype=torch.int32)
    for b, (src, tgt) in enumerate(indices):
        for s, t in zip(src.tolist(), tgt.tolist()):
            want[b, s] = [0, 3, 3][b] + t
    assert torch.equal(rows, want)
    assert rows.tolist() == [[1, 1, -1, 1], [-1, -1, -1, -1], [-1, -1, 3, -1]]
    assert torch.equal(matched_rows([(idx(), idx())], [0], 5, torch.device("cpu")), torch.full((1, 5), -1, dtype=torch.int32))


def test_duplicates_in_the_module_follow_the_loop():
    """loss_labelsVL with a query matched twice: the one-hot row is the LAST pair's positive map."""
    from uninext_amd.criterion import SetCriterion, token_sigmoid_binary_focal_loss
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(1, 4, 6, generator=g)
    pm = torch.tensor([[1, 0, 0, 0, 0, 0], [0, 0, 1, 1, 0, 0]], dtype=torch.bool)
    crit = SetCriterion(None, {}, ["labelsVL"], ota=True)
    got = crit.loss_labelsVL({"pred_logits": logits, "text_masks": None}, [{"positive_map": pm}],
                             [(torch.tensor([2, 2]), torch.tensor([0, 1]))], 1)["loss_ce"]
    onehot = torch.zeros(1, 4, 6)
    onehot[0, 2] = pm[1].float()
    assert torch.equal(got, token_sigmoid_binary_focal_loss(logits, onehot) / 2)


def _ref_defs(path, names):
    tree = ast.parse(open(path).read())
    return {n.name: n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names}


def _ast_signature(fn):
    a = fn.args
    assert not a.posonlyargs and not a.kwonlyargs and a.vararg is None
    defaults = [None] * (len(a.args) - len(a.defaults)) + [ast.literal_eval(d) for d in a.defaults]
    return [(arg.arg, d) for arg, d in zip(a.args, defaults)], a.kwarg.arg if a.kwarg else None


def _our_signature(fn):
    out, kwarg = [], None
    for p in inspect.signature(fn).parameters.values():
        if p.kind == p.VAR_KEYWORD:
            kwarg = p.name
        else:
            assert p.kind == p.POSITIONAL_OR_KEYWORD
            out.append((p.name, None if p.default is p.empty else p.default))
    return out, kwarg


@pytest.mark.skipif(not os.path.isdir(REF_DIR), reason="needs the reference checkout")
def test_names_and_signatures_equal_the_references():
    from uninext_amd import criterion as ours
    functions = {**_ref_defs(os.path.join(REF_DIR, "segmentation.py"), ["dice_loss", "sigmoid_focal_loss", "token_sigmoid_binary_focal_loss"]),
                 **_ref_defs(os.path.join(REF_DIR, "deformable_detr.py"), ["compute_box_iou", "dice_coefficient"])}
    assert len(functions) == 5
    for name, node in functions.items():
        assert _our_signature(getattr(ours, name)) == _ast_signature(node), name
    classes = _ref_defs(os.path.join(REF_DIR, "deformable_detr.py"), ["SetCriterion", "DINOCriterion"])
    assert [b.id for b in classes["DINOCriterion"].bases] == ["SetCriterion"] and issubclass(ours.DINOCriterion, ours.SetCriterion)
    checked = 0
    for cls_name, node in classes.items():
        for method in (m for m in node.body if isinstance(m, ast.FunctionDef)):
            mine = getattr(ours, cls_name).__dict__.get(method.name)
            assert mine is not None, (cls_name, method.name)
            assert _our_signature(mine) == _ast_signature(method), (cls_name, method.name)
            checked += 1
    assert checked >= 14          # twelve methods of SetCriterion, two of DINOCriterion
    assert inspect.signature(ours.giou_loss).parameters["eps"].default == 1e-7          # fvcore's


def test_reid_and_boxinst_name_themselves():
    from uninext_amd.criterion import SetCriterion
    for loss in ("reid", "masks_boxinst"):
        with pytest.raises(NotImplementedError, match=loss):
            SetCriterion(None, {}, ["labelsVL", loss])
        with pytest.raises(NotImplementedError, match=loss):
            SetCriterion(None, {}, ["labelsVL"]).get_loss(loss, {}, [], [], 1)
    with pytest.raises(AssertionError):
        SetCriterion(None, {}, ["labelsVL"]).get_loss("labels", {}, [], [], 1)


def test_fused_is_a_class_attribute_on_by_default():
    """On since profiles/r18_criterion.txt; an instance can turn it off for itself."""
    from uninext_amd.criterion import DINOCriterion, SetCriterion
    assert SetCriterion.fused is True and DINOCriterion.fused is True
    crit = DINOCriterion(None, {}, [])
    crit.fused = False
    assert SetCriterion.fused is True


def test_kernel_cases_are_what_they_claim():
    """The seeded kernel inputs: masks, extremes and shared rows are there, and the float64 yardstick is finite."""
    logits, mask, rows, pm, loss, grad = C.token_case(2, 65, 255, "extreme")
    assert {30.0, -30.0, 100.0, -100.0} <= set(logits.view(-1).tolist()) and np.isfinite(loss) and bool(torch.isfinite(grad).all())
    assert bool((grad[:, :, mask[0] == 0][0] == 0).all())
    assert C.token_case(2, 65, 255, "unmatched")[2].max() == -1
    assert C.token_case(3, 130, 77, "zero_image")[1][2].sum() == 0
    frac = C.token_case(2, 64, 256, "fractional")[3]
    assert bool(((frac > 0) & (frac < 1)).any())
    src, gt, gt_row, (lm, ld), grad = C.mask_case(3, 1, 7, 9, 4)
    tgt = C.target_pixels(gt.view(-1, 28, 36), gt_row, 1, 7, 9, 4)
    assert int(gt_row[1]) == int(gt_row[2]) and not tgt[0].any() and tgt[2].all() and np.isfinite(lm) and np.isfinite(ld)


def test_target_pixels_are_get_target_masks_gathered():
    from uninext_amd.criterion import SetCriterion
    flat, _ = C.load("ota_dn")
    _, targets, indices_list, _ = C.rebuild(flat, C.CASES["ota_dn"])
    crit = SetCriterion(None, {}, ["masks"], mask_out_stride=C.STRIDE)
    src = torch.zeros(1, 1, *C.MASK_HW)
    dense = crit.get_target_masks(targets, src)
    tgt_idx = crit._get_tgt_permutation_idx(indices_list[-1])
    want = dense.reshape(C.BS, -1, 1, *C.MASK_HW)[tgt_idx]
    from uninext_amd.criterion import pad_masks
    gt = pad_masks([t["masks"] for t in targets])
    gt_row = (tgt_idx[0] * gt.shape[1] + tgt_idx[1]).int()
    got = C.target_pixels(gt.view(-1, *gt.shape[-2:]), gt_row, 1, *C.MASK_HW, C.STRIDE)
    assert torch.equal(got.float(), want)
