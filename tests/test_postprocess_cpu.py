"""Detection post-processing without a GPU: the PyTorch composition of uninext_amd/postprocess.py against the reference's
fixtures, the restatement of torchvision's batched_nms on hand-built cases, the vectorised class-logit conversion against a
literal loop, and the binding of the detpost_* entry points."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import postprocess_cases as P   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("detpost_scores_hip_f32", "detpost_nms_hip_f32", "detpost_hip_last_kernel")


def test_the_fixtures_are_the_ones_the_generator_mints():
    assert P.FIXTURES == P.EXPECTED_FIXTURES
    for name in P.FIXTURES:
        assert os.path.getsize(os.path.join(P.GOLDEN, name + ".npz")) <= 640 * 1024
        assert sorted(P.load(name)["runs"]) == sorted(run for n, run in P.RUNS if n == name)


@pytest.mark.parametrize("name,run", P.RUNS)
def test_composition_reproduces_the_reference(name, run):
    from uninext_amd.postprocess import DetectionPostProcess
    P.check_against_fixture(lambda ota, demo: DetectionPostProcess(ota=ota, fused=False, demo_only=demo), name, run)


def test_a_threshold_run_returns_fewer_than_a_hundred_and_one_reaches_the_invalid_entries():
    few = P.load("thres_few_q300_t64")["runs"]["ota"][1]
    assert all(0 < len(e["scores"]) < 100 and (e["scores"] > 0.3).all() for e in few)
    reached = P.load("coco_q300_t256")["runs"]["thres_reaches_invalid"][1]
    assert all((e["scores"] == -1.0).any() for e in reached)


@pytest.mark.parametrize("case", sorted(P.hand_cases()))
def test_batched_nms_hand_built(case):
    from uninext_amd.postprocess import batched_nms
    boxes, scores, classes, expect = P.hand_cases()[case]
    keep = batched_nms(boxes, scores, torch.tensor(classes), 0.5)
    assert keep.dtype == torch.int64 and keep.tolist() == expect


def test_batched_nms_empty_input():
    from uninext_amd.postprocess import batched_nms, nms
    keep = batched_nms(torch.zeros(0, 4), torch.zeros(0), torch.zeros(0, dtype=torch.long), 0.5)
    assert keep.dtype == torch.int64 and keep.shape == (0,)
    assert nms(torch.zeros(0, 4), torch.zeros(0), 0.5).shape == (0,)


def test_batched_nms_routes_agree_across_the_4000_element_switch():
    """1000 boxes are 4000 elements (the offset route), 1001 are 4004 (class by class): the first 1000 of the larger input
    are the smaller input, the extra box is far away from everything, and every IoU keeps the margin on both routes."""
    from uninext_amd import postprocess as pp
    boxes, scores, cls, expect = P.nms_case(1000, 1)
    xyxy = pp.box_cxcywh_to_xyxy(boxes[0])
    assert xyxy.numel() == pp.COORDINATE_TRICK_MAX_NUMEL
    small = pp.batched_nms(xyxy, scores[0], cls[0], 0.7)
    assert small.tolist() == expect[0][0].tolist()
    far = torch.tensor([[5.0, 5.0, 5.5, 5.5]])
    big = pp.batched_nms(torch.cat([xyxy, far]), torch.cat([scores[0], torch.tensor([-1.0])]),
                         torch.cat([cls[0], torch.tensor([0], dtype=cls.dtype)]), 0.7)
    assert big.tolist() == expect[1][0].tolist() + [1000]
    assert sorted(big.tolist()[:-1]) == sorted(small.tolist()) and 0 < len(small) < 1000


@pytest.mark.parametrize("Q,C,T", [(1, 1, 1), (65, 80, 256), (300, 365, 256)])
def test_convert_equals_a_literal_loop(Q, C, T):
    from uninext_amd.postprocess import convert_grounding_to_od_logits
    logits, _, pm, _ = P.scores_case(Q, C, T)
    got = convert_grounding_to_od_logits(logits, C, pm)
    want = P.literal_convert(logits, C, pm)
    assert got.shape == want.shape == (2, Q, C)
    np.testing.assert_array_equal(got.numpy(), want.numpy())
    if C > 2:
        assert (got[:, :, 1] == 0).all() and len(pm[3]) == 6      # the class without tokens, the class with six


def test_convert_follows_the_reference_on_label_order_and_range():
    from uninext_amd.postprocess import convert_grounding_to_od_logits
    logits = torch.arange(12, dtype=torch.float32).view(1, 2, 6)
    pm = {1: [0, 1], 3: [2], 0: [5]}            # label 0 addresses the last class, as the reference's index -1 does
    np.testing.assert_array_equal(convert_grounding_to_od_logits(logits, 3, pm).numpy(), P.literal_convert(logits, 3, pm).numpy())
    with pytest.raises(IndexError):
        convert_grounding_to_od_logits(logits, 3, {1: [6]})
    with pytest.raises(NotImplementedError):
        convert_grounding_to_od_logits(logits, 3, pm, score_agg="MAX")


def test_any_other_task_raises_the_references_error():
    from uninext_amd.postprocess import DetectionPostProcess
    fx = P.load("grounding_q300_t64")
    with pytest.raises(ValueError, match="task must be detection or grounding"):
        DetectionPostProcess()(fx["box_cls"], fx["box_pred"], fx["iou_pred"], fx["image_sizes"], fx["positive_map"], 1, task="sot")


def test_fused_is_the_default_and_takes_the_composition_off_the_gpu():
    from uninext_amd.postprocess import DetectionPostProcess
    assert DetectionPostProcess.fused is True and DetectionPostProcess(fused=False).fused is False      # profiles/r15_postprocess.txt
    P.check_against_fixture(lambda ota, demo: DetectionPostProcess(ota=ota, demo_only=demo), "grounding_q300_t64", "ota")


def test_new_names_are_declared_bound_and_exported():
    from uninext_amd import _lib
    header = open(os.path.join(ROOT, "include", "dynmask_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib._SIGNATURES["dynmask_hip.h"] and name in _lib.DYNMASK_EXPORTS
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert getattr(raw, name) is not None and getattr(lib, name).argtypes is not None
    assert _lib.last_kernel("detpost") == "" or _lib.last_kernel("detpost").startswith("detpost_")
    for macro, value in (("DETPOST_HIP_MAX_CLASSES", _lib.DETPOST_MAX_CLASSES), ("DETPOST_HIP_MAX_TOKENS", _lib.DETPOST_MAX_TOKENS),
                         ("DETPOST_HIP_MAX_QUERIES", _lib.DETPOST_MAX_QUERIES)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, header).group(1)) == value


def test_sizes_the_kernels_refuse_come_back_as_error_codes():
    """The entry points check their sizes before they touch a pointer or the device."""
    from uninext_amd import _lib
    lib = _lib.load()
    assert lib.detpost_nms_hip_f32(None, None, None, 0.7, 0, 1, _lib.DETPOST_MAX_QUERIES + 1, None, None, None, None) == -5
    assert "1024" in _lib.last_error()
    assert lib.detpost_scores_hip_f32(None, None, None, None, 0, 0.0, 1, 1, 1, _lib.DETPOST_MAX_TOKENS + 1, None, None, None, None, None) == -5
    assert lib.detpost_scores_hip_f32(None, None, None, None, 0, 0.0, 1, 1, _lib.DETPOST_MAX_CLASSES + 1, 1, None, None, None, None, None) == -5
    assert lib.detpost_scores_hip_f32(None, None, None, None, 0, 0.0, 1, 1, 1, 1, None, None, None, None, None) == -1
    assert lib.detpost_nms_hip_f32(None, None, None, 0.7, 2, 1, 1, None, None, None, None) == -2
