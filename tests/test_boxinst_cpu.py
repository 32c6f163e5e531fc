"""BoxInst without a GPU: the composition (`fused` off) against the reference's fixtures (tests/golden/boxinst/*.npz, minted by
tests/golden/make_boxinst_golden.py), `rgb2lab` on anchor colours, the exported names and signatures against the reference checkout's
by `ast`, the state-dict key, the consumption of `random`, and the seeded kernel cases of tests/boxinst_cases.py."""
import ast
import inspect
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boxinst_cases as B   # noqa: E402
from test_criterion_cpu import _ast_signature, _our_signature   # noqa: E402

REF = os.environ.get("UNINEXT_REFERENCE", "/root/reference")
DDETR = os.path.join(REF, "projects/UNINEXT/uninext/models/deformable_detr/deformable_detr.py")
IMG = os.path.join(REF, "projects/UNINEXT/uninext/uninext_img.py")


def test_fixtures_are_the_documented_ones():
    stored = sorted(os.path.splitext(f)[0] for f in os.listdir(B.GOLDEN) if f.endswith(".npz"))
    assert stored == sorted(list(B.LOSS_CASES) + ["targets"])
    for name, cfg in B.LOSS_CASES.items():
        flat, expect = B.load_loss(name)
        again = B.make_loss_inputs(cfg)                         # the generator has not drifted from the stored inputs
        assert set(again) == set(flat) and set(expect) == {"loss_prj", "loss_pairwise", "iter"}
        for k in flat:
            assert torch.equal(again[k], flat[k]), (name, k)
    assert B.load_loss("over_topk")[1]["loss_pairwise"] > 0.1 and B.load_loss("warmup_mid")[1]["loss_pairwise"] > 0.1
    assert B.load_loss("no_weight")[1]["loss_pairwise"] == 0.0 and B.load_loss("no_weight")[1]["loss_prj"] > 0.1
    assert sum(B.LOSS_CASES["over_topk"]["pairs"]) > B.LOSS_CASES["over_topk"]["topk"]


def test_targets_reproduce_the_reference():
    """Padding, the bottom band, pooling, BGR -> RGB, .byte(), the strided mask, the bitmask rule: against the reference's own code
    (with this module's rgb2lab in skimage's place, see make_boxinst_golden.py)."""
    from uninext_amd.boxinst import boxinst_targets
    images, heights, boxes = B.make_target_inputs()
    stored = B.load_targets()
    for fused in (False, True):                                  # on CPU tensors the switch changes nothing
        got = boxinst_targets(images, heights, boxes, fused=fused)
        for b, t in enumerate(got):
            assert t["masks"].dtype == torch.bool and torch.equal(t["masks"], stored["masks.%d" % b])
            sim = t["image_color_similarity"]
            assert sim.shape == (len(boxes[b]), 8, 16, 24) and sim.dtype == torch.float32
            assert sim.stride(0) == 0                            # ONE [8, h, w] tensor handed out as a view
            B.within(sim[0], stored["sim.%d" % b], "sim")
    as_float = boxinst_targets([im.float() for im in images], heights, boxes)
    assert torch.equal(as_float[1]["image_color_similarity"], got[1]["image_color_similarity"])
    # what the fixture exercises: a non-zero bottom band, boxes clamped at the far edges, both sides of the threshold
    # int(10 * 64 / 128) = 5 rows removed: pooled row 15 (sampled at pixel 62) is no neighbour, row 14 (pixel 58) is one
    assert not stored["sim.0"][3:5, 15].any() and not stored["sim.0"][5:, 13].any() and stored["sim.0"][5:, 12].any()
    assert int(stored["masks.0"][3].sum()) == (64 - 50) * (96 - 80) and int(stored["masks.0"][4].sum()) == 1
    assert bool((stored["sim.0"] >= 0.3).any()) and bool((stored["sim.0"] < 0.3).any())
    assert int(stored["masks.0"][0].sum()) == 96 and int(stored["masks.0"][1].sum()) == 61


@pytest.mark.parametrize("name", sorted(B.LOSS_CASES))
def test_composition_reproduces_the_reference(name):
    _, expect = B.load_loss(name)
    got, crit = B.run_loss_fixture(name, fused=False)
    assert set(got) == {"loss_prj", "loss_pairwise"}
    for key in got:
        B.within(float(got[key]), expect[key], key)            # 1e-4 of the value itself
    assert float(crit._iter) == expect["iter"]


def test_fused_on_the_cpu_is_the_composition():
    for name in ("over_topk", "warmup_mid"):
        a, _ = B.run_loss_fixture(name, fused=False)
        b, _ = B.run_loss_fixture(name, fused=True)
        for key in a:
            assert torch.equal(a[key], b[key]), key


def test_rgb2lab_on_anchor_colours():
    """Published CIE Lab values (D65, 2 degrees) of the sRGB primaries: all the anchoring available without skimage."""
    from uninext_amd.boxinst import rgb2lab
    rgb = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0]], dtype=np.uint8)
    lab = rgb2lab(rgb)
    assert lab.dtype == np.float64 and lab.shape == (5, 3)
    want = [(53.2408, 80.0925, 67.2032), (87.7347, -86.1827, 83.1793), (32.2970, 79.1875, -107.8602)]
    assert np.max(np.abs(lab[:3] - np.array(want))) < 5e-3, lab[:3]
    assert abs(lab[3, 0] - 100.0) < 5e-3 and abs(lab[3, 1]) < 0.01 and abs(lab[3, 2]) < 0.01
    assert np.max(np.abs(lab[4])) < 1e-9
    as_tensor = rgb2lab(torch.from_numpy(rgb).view(5, 1, 3))
    assert torch.is_tensor(as_tensor) and as_tensor.dtype == torch.float64 and np.array_equal(as_tensor.view(5, 3).numpy(), lab)


def _defs(path, names):
    tree = ast.parse(open(path).read())
    found = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names}
    for cls in (n for n in tree.body if isinstance(n, ast.ClassDef)):
        found.update({(cls.name, n.name): n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in names})
    return found


@pytest.mark.skipif(not os.path.isdir(os.path.dirname(DDETR)), reason="needs the reference checkout")
def test_names_and_signatures_equal_the_references():
    import uninext_amd
    from uninext_amd import boxinst as ours
    functions = {**_defs(DDETR, ["unfold_wo_center", "compute_project_term", "compute_pairwise_term"]),
                 **_defs(IMG, ["get_images_color_similarity"])}
    assert len(functions) == 4
    for name, node in functions.items():
        assert _our_signature(getattr(ours, name)) == _ast_signature(node), name
        assert getattr(uninext_amd, name) is getattr(ours, name)                       # re-exported
    methods = _defs(DDETR, ["__init__", "loss_masks_boxinst"])
    for cls in (ours.BoxInstSetCriterion, ours.BoxInstDINOCriterion):
        assert _our_signature(cls.__init__) == _ast_signature(methods[("SetCriterion", "__init__")])
        assert _our_signature(cls.loss_masks_boxinst) == _ast_signature(methods[("SetCriterion", "loss_masks_boxinst")])
    for name in ("rgb2lab", "boxinst_targets", "BoxInstSetCriterion", "BoxInstDINOCriterion", "BoxInstLossesFunction"):
        assert getattr(uninext_amd, name) is getattr(ours, name)


def test_state_dict_key_defaults_and_dispatch():
    from uninext_amd.boxinst import BoxInstDINOCriterion, BoxInstSetCriterion
    from uninext_amd.criterion import DINOCriterion, SetCriterion
    crit = BoxInstSetCriterion(None, {}, ["labelsVL", "masks_boxinst"])
    assert list(crit.state_dict()) == ["_iter"] and crit._iter.shape == (1,) and crit._iter.dtype == torch.float32
    assert crit.losses == ["labelsVL", "masks_boxinst"]
    assert (crit.pairwise_size, crit.pairwise_dilation, crit.pairwise_color_thresh, crit._warmup_iters, crit.boxinst_topk,
            crit.bottom_pixels_removed) == (3, 2, 0.3, 10000, 64, 10)
    cfg = B.boxinst_cfg(B.LOSS_CASES["over_topk"])
    assert BoxInstDINOCriterion(None, {}, ["masks_boxinst"], cfg=cfg).boxinst_topk == 3
    assert issubclass(BoxInstDINOCriterion, DINOCriterion) and issubclass(BoxInstSetCriterion, SetCriterion)
    from uninext_amd import boxinst
    assert BoxInstSetCriterion.fused_boxinst is True and boxinst.FUSED is True            # on since profiles/r26_boxinst.txt
    assert SetCriterion.fused is True and not hasattr(SetCriterion, "fused_boxinst")
    # dispatched through get_loss, `_iter` counted before the early exits
    flat, _ = B.load_loss("scalar_pred")
    outputs, targets, indices = B.rebuild_loss(flat, B.LOSS_CASES["scalar_pred"])
    got = crit.get_loss("masks_boxinst", outputs, targets, indices, 3.0)
    assert set(got) == {"loss_prj", "loss_pairwise"} and float(crit._iter) == 1.0
    flat, _ = B.load_loss("no_gt")
    outputs, targets, indices = B.rebuild_loss(flat, B.LOSS_CASES["no_gt"])
    crit.get_loss("masks_boxinst", outputs, targets, indices, 3.0)
    assert float(crit._iter) == 2.0
    with pytest.raises(NotImplementedError, match="masks_boxinst"):                        # the base class keeps raising
        SetCriterion(None, {}, ["masks_boxinst"])


def test_random_is_consumed_exactly_once_per_over_topk_call(monkeypatch):
    calls = []
    real = random.sample

    def counting(population, k):
        calls.append((population, k))
        return real(population, k)

    monkeypatch.setattr(random, "sample", counting)
    for fused in (False, True):
        B.run_loss_fixture("over_topk", fused=fused)
    assert calls == [(range(5), 3), (range(5), 3)]
    calls.clear()
    B.run_loss_fixture("plain", fused=False)
    assert calls == []
    # the same pairs as the reference drew: the generator is left where the reference leaves it
    B.run_loss_fixture("over_topk", fused=False)
    after = random.random()
    random.seed(B.LOSS_CASES["over_topk"]["rseed"])
    real(range(5), 3)
    assert random.random() == after


def test_kernel_cases_are_what_they_claim():
    """Unique row and column maxima in sigmoid space (the kernels take them of the logits), weights on both sides, and a finite
    float64 yardstick."""
    assert len(set(B.KERNEL_CASES)) == len(B.KERNEL_CASES) and len(B.KERNEL_GEOMETRIES) == len(set(B.KERNEL_GEOMETRIES))
    for (n, h, w), variant in B.KERNEL_CASES:
        case = B.kernel_case(n, h, w, variant)
        p = case["src"].double()[case["inst"].long()].sigmoid()
        for dim in (2, 3):
            top = p.max(dim=dim, keepdim=True)[0]
            assert bool(((p == top).sum(dim=dim) == 1).all()), ((n, h, w), variant, dim)
        assert np.isfinite(case["want"]).all() and bool(torch.isfinite(case["want_grad"]).all())
        assert (case["sum_w"] == 0) == (variant == "no_weight"), ((n, h, w), variant, case["sum_w"])
        assert len(set(case["inst"].tolist())) == case["inst"].numel()
    extreme = B.kernel_case(3, 17, 33, "extreme")["src"]
    assert {30.0, -30.0, 100.0, -100.0} <= set(extreme.view(-1).tolist())
    assert not B.kernel_case(2, 5, 4, "bad_gt_row")["tgt"][-1].any() and B.kernel_case(2, 5, 4, "bad_gt_row")["inst"].numel() == 3
    assert B.kernel_case(3, 17, 33, "subset")["src"].shape[0] == 5 and B.kernel_case(3, 17, 33, "subset")["inst"].numel() == 3
    assert bool((B.kernel_case(2, 40, 68, "second_image")["img"] == 1).all())
