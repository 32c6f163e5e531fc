"""Decoder prediction heads on the CPU: the composition route of DetectionHeads in float64 against the reference's fixtures
(tests/golden/pred_heads/, minted by tests/golden/make_pred_heads_golden.py), the state-dict keys, the layout of inference()'s
outputs, the task check, and the `fused` flag on tensors the HIP route does not take."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pred_heads_cases as C          # noqa: E402

EXACT = 1e-12         # of the reference output's largest magnitude


def case(name):
    fx = C.load(name)
    cfg, states, x = C.make_case(name)
    assert int(fx["seed"]) == cfg["seed"] and C.digest(states) == float(fx["digest"])
    return fx, cfg, states, x


def same(got, want, what):
    got, want = got.detach().double().numpy(), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert float(np.abs(got - want).max()) <= EXACT * float(np.abs(want).max()), what


@pytest.mark.parametrize("name", list(C.FIXTURES))
def test_composition_in_float64_reproduces_the_fixture(name):
    fx, cfg, states, x = case(name)
    out = C.run(cfg, C.build(cfg, states, torch.float64), x)
    assert set(out) == {k for k in C.OUTPUTS if k in fx}
    assert ("pred_boxious" in out) == cfg["iou"]
    for k, v in out.items():
        same(v, fx[k], k)


@pytest.mark.parametrize("name", list(C.FIXTURES))
def test_state_dict_keys_and_shapes_are_the_references(name):
    fx, cfg, states, x = case(name)
    heads = C.build(cfg, states, torch.float64)          # a strict load of every submodule
    recorded = C.recorded_keys(fx)
    assert set(recorded) == set(states)
    for k, want in recorded.items():
        assert [[n, list(v.shape)] for n, v in getattr(heads, k).state_dict().items()] == want, k
    # below the module the keys carry the attribute names, and nothing else is there
    assert sorted(heads.state_dict()) == sorted("%s.%s" % (k, n) for k, want in recorded.items() for n, _ in want)
    if cfg["head"] == "vl_align":
        assert "class_embed.1.dot_product_projection_text.weight" in heads.state_dict()
    assert "bbox_embed.0.layers.2.bias" in heads.state_dict() and "controller.layers.2.weight" in heads.state_dict()
    assert ("iou_head.1.weight" in heads.state_dict()) == cfg["iou"] and (heads.iou_head is None) != cfg["iou"]


def test_given_modules_are_kept_not_copied():
    from torch import nn
    from uninext_amd import modules as M
    boxes = nn.ModuleList(M.MLP(256, 256, 4, 3) for _ in range(2))
    classes = nn.ModuleList(M.Still_Classifier(256) for _ in range(2))
    controller = M.MLP(256, 256, 9, 3)
    heads = M.DetectionHeads(classes, boxes, None, controller)
    assert heads.bbox_embed is boxes and heads.class_embed is classes and heads.controller is controller and heads.iou_head is None
    assert heads.bbox_embed[1].layers[0].weight is boxes[1].layers[0].weight


@pytest.mark.parametrize("name", ["detection", "ref2_plain"])
def test_inference_layout_of_points_and_parameters(name):
    fx, cfg, states, x = case(name)
    heads = C.build(cfg, states, torch.float64)
    out = C.run(cfg, heads, x)
    assert tuple(out["reference_points"].shape) == (1, C.B * C.Q, 2)
    assert tuple(out["mask_head_params"].shape) == (1, C.B * C.Q, cfg["P"])
    # image-major rows; the points are those of inter_references[-2] in (x, y) pixels of each image
    for b, (h, w) in enumerate(x["image_sizes"]):
        rows = slice(b * C.Q, (b + 1) * C.Q)
        want = x["inter_references"][-2][b, :, :2] * torch.tensor([w, h], dtype=torch.float64)
        assert torch.equal(out["reference_points"][0, rows], want)
        same(out["reference_points"][0, rows], fx["reference_points"][0, rows], "points of image %d" % b)
    with torch.no_grad():
        level = heads.forward_level(C.LEVELS - 1, x["hs"][-1], x["inter_references"][C.LEVELS - 2], x["hidden"])
        assert torch.equal(level[3].reshape(1, -1, cfg["P"]), out["mask_head_params"])
        assert torch.equal(level[0], out["pred_logits"]) and torch.equal(level[1], out["pred_boxes"])
        assert (level[2] is None) == (not cfg["iou"])
        assert heads.forward_level(0, x["hs"][0], x["init_reference"], x["hidden"], want_controller=False)[3] is None
        # level 0 has its own heads
        assert not torch.equal(heads.forward_level(0, x["hs"][-1], x["inter_references"][C.LEVELS - 2], x["hidden"])[1], level[1])


def test_a_bad_task_raises():
    fx, cfg, states, x = case("grounding")
    heads = C.build(cfg, states, torch.float64)
    for task in ("grounding", "sot"):
        same(C.run(dict(cfg, task=task), heads, x)["pred_logits"], fx["pred_logits"], task)
    with pytest.raises(ValueError, match="task must be detection or grounding"):
        C.run(dict(cfg, task="vos"), heads, x)


def test_fused_is_ignored_on_the_cpu():
    from uninext_amd import modules as M
    assert M.DetectionHeads.fused in (False, True)
    fx, cfg, states, x = case("detection")
    heads = C.build(cfg, states, torch.float64)
    plain, fused = C.run(cfg, heads, x, fused=False), C.run(cfg, heads, x, fused=True)
    assert all(torch.equal(plain[k], fused[k]) for k in plain)
    heads32 = C.build(cfg, states, torch.float32)           # fp32 on the CPU, and autograd recording: PyTorch's composition
    heads32.fused = True
    hs, init_reference, inter_references, text = C.inputs(x, torch.float32)
    out = heads32.inference(hs, init_reference, inter_references, text, cfg["task"], x["image_sizes"])
    assert out["pred_boxes"].requires_grad and out["mask_head_params"].requires_grad
    assert C.QC.rel_err(out["pred_boxes"], fx["pred_boxes"]) <= C.TOL
