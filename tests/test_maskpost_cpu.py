"""Mask post-processing on the CPU: the composition of PyTorch ops against the reference's fixtures (exactly), the pinned
nearest-index rule against F.interpolate, the fixtures' own margins, the refusals of the C ABI (no GPU is touched: every call
here is refused, or answered as empty, before any HIP runtime call) and the unchanged face of DetectionPostProcess."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maskpost_cases as M   # noqa: E402
import postprocess_cases as P   # noqa: E402


@pytest.mark.parametrize("name", sorted(M.BINARIZE_CASES))
def test_composition_reproduces_the_reference_masks(name):
    from uninext_amd.postprocess import MaskPostProcess, postprocess_masks, segmentation_postprocess
    c = M.binarize_case(name)
    assert MaskPostProcess.fused in (False, True)
    got = postprocess_masks(c["planes"].unsqueeze(1), c["rows"], c["crop"], c["out"], c["stride"], c["thres"], fused=False)
    assert got.dtype == torch.uint8 and torch.equal(got, c["expect"])
    at_image = postprocess_masks(c["planes"], c["rows"], c["crop"], None, c["stride"], c["thres"], fused=False)
    assert tuple(at_image.shape) == (len(c["rows"]),) + c["crop"]
    if c["out"] == c["crop"]:
        assert torch.equal(at_image, c["expect"])
    # the two steps apart, as the reference takes them: inference()'s masks, then segmentation_postprocess on the result
    n = len(c["rows"])
    result = {"scores": torch.ones(n), "pred_boxes": torch.tensor([[0.0, 0.0, c["crop"][1], c["crop"][0]]]).repeat(n, 1),
              "pred_masks": at_image}
    assert torch.equal(segmentation_postprocess(result, *c["out"])["pred_masks"], c["expect"])


@pytest.mark.parametrize("name", sorted(M.BINARIZE_CASES))
def test_fixture_keeps_its_margin(name):
    """Assertion (a) of the generator, on the committed files: few pixels in the band, the float64 decision elsewhere."""
    c = M.binarize_case(name)
    assert float(c["excluded"].float().mean()) <= M.MAX_EXCLUDED_SHARE
    assert not bool(((c["expect"] != c["decide"]) & ~c["excluded"]).any())


def test_a_crop_past_the_plane_ends_with_the_plane():
    from uninext_amd.postprocess import postprocess_masks
    c = M.binarize_case("identity")
    got = postprocess_masks(c["planes"], c["rows"], (1000, 1000), None, 4, 0.5, fused=False)
    assert tuple(got.shape) == (7, 100, 168)
    assert torch.equal(got[:, :97, :161], c["expect"])
    assert tuple(postprocess_masks(c["planes"], c["rows"][:0], (97, 161), (5, 6), 4, 0.5).shape) == (0, 5, 6)


@pytest.mark.parametrize("size,out", [(800, 480), (1344, 1920), (800, 1080), (37, 101), (101, 37), (5, 1), (1, 5), (7, 7)])
def test_fp32_nearest_rule_is_f_interpolate(size, out):
    want = F.interpolate(torch.arange(size, dtype=torch.float32).view(1, 1, 1, size), size=(1, out), mode="nearest").view(-1)
    np.testing.assert_array_equal(M.nearest_index(out, size), want.long().numpy())
    want = F.interpolate(torch.arange(size, dtype=torch.float32).view(1, 1, size, 1), size=(out, 1), mode="nearest").view(-1)
    np.testing.assert_array_equal(M.nearest_index(out, size), want.long().numpy())


def test_a_float64_rule_would_pick_other_pixels():
    """Why the rule is pinned in fp32: the two size pairs the GPU cases carry."""
    for size, out, off in ((1344, 1920, 34), (800, 1080, 5)):
        f64 = np.minimum(np.floor(np.arange(out) * (size / out)).astype(np.int64), size - 1)
        assert int((f64 != M.nearest_index(out, size)).sum()) == off


@pytest.mark.parametrize("name", M.NMS_CASES + list(M.NMS_HAND))
def test_mask_nms_composition_reproduces_the_reference(name):
    from uninext_amd.postprocess import MASK_NMS_FUSED, mask_iou, mask_nms
    c = M.nms_case(name)
    n = len(c["keep"])
    assert MASK_NMS_FUSED in (False, True)
    masks = c["logits"].sigmoid() > 0.5
    assert torch.equal(masks.view(n, -1), c["masks"])                    # the rebuilt inputs are the generator's
    assert mask_nms(c["logits"], [0.0] * n, None, nms_thr=c["thr"], fused=False) == c["keep"]
    assert mask_nms(c["logits"][:, 0], torch.zeros(n), nms_thr=c["thr"], fused=False) == c["keep"]
    area, inter, keep, margin = M.mask_nms_restated(c["logits"], c["thr"])
    assert [bool(k) for k in keep] == c["keep"] and margin >= M.IOU_MARGIN
    if n >= 2:
        iou = mask_iou(masks[0], masks[1])
        assert iou.shape == (1,) and abs(float(iou) - (inter[0, 1] + 1e-6) / (area[0] + area[1] - inter[0, 1] + 1e-6)) < 1e-6


def test_mask_nms_of_nothing_is_an_empty_list():
    from uninext_amd.postprocess import mask_nms
    assert mask_nms(torch.zeros(0, 1, 25, 42), [], None) == []


@pytest.fixture(scope="module")
def lib():
    from uninext_amd import build, _lib
    build.build()
    return _lib.load()


def test_binding_rows_and_limits(lib):
    from uninext_amd import _lib
    for name in ("maskpost_binarize_hip_f32", "maskpost_pack_hip_f32", "maskpost_nms_hip_u32", "maskpost_hip_last_kernel"):
        assert name in _lib.DYNMASK_EXPORTS and getattr(lib, name).argtypes is not None
    assert _lib.last_kernel("maskpost") == "" or _lib.last_kernel("maskpost").startswith("maskpost_")
    header = open(os.path.join(os.path.dirname(M.HERE), "include", "dynmask_hip.h")).read()
    for macro, value in (("MASKPOST_HIP_MAX_WIDTH", _lib.MASKPOST_MAX_WIDTH), ("MASKPOST_HIP_MAX_MASKS", _lib.MASKPOST_MAX_MASKS)):
        assert "#define %s %d\n" % (macro, value) in header


def test_c_abi_refusals(lib):
    from uninext_amd import _lib
    buf = ctypes.create_string_buffer(64)       # a non-null address; a refused call reads nothing behind it
    ok = ctypes.addressof(buf)

    def binarize(logits=ok, rows=ok, Q=2, h=25, w=42, n=1, stride=4, crop_h=97, crop_w=161, out_h=60, out_w=100, thres=0.5, out=ok):
        return lib.maskpost_binarize_hip_f32(logits, rows, Q, h, w, n, stride, crop_h, crop_w, out_h, out_w, thres, out, None)

    def answer(code, text):
        assert code < 0 and _lib.last_error() == text
        return code

    assert answer(binarize(stride=3), "maskpost_binarize: stride must be 1, 2, 4 or 8") == -5
    assert answer(binarize(stride=0), "maskpost_binarize: stride must be 1, 2, 4 or 8") == -5
    assert answer(binarize(stride=16), "maskpost_binarize: stride must be 1, 2, 4 or 8") == -5
    for thres in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert answer(binarize(thres=thres), "maskpost_binarize: thres must lie in (0, 1)") == -5
    assert answer(binarize(crop_h=101), "maskpost_binarize: crop beyond the upsampled plane") == -2
    assert answer(binarize(crop_w=169), "maskpost_binarize: crop beyond the upsampled plane") == -2
    assert answer(binarize(stride=2, crop_h=51, crop_w=84), "maskpost_binarize: crop beyond the upsampled plane") == -2
    assert answer(binarize(crop_h=0), "maskpost_binarize: bad dimensions") == -2
    assert answer(binarize(out_w=0), "maskpost_binarize: bad dimensions") == -2
    assert answer(binarize(n=-1), "maskpost_binarize: bad dimensions") == -2
    assert answer(binarize(w=_lib.MASKPOST_MAX_WIDTH + 1, crop_w=8), "maskpost_binarize: at most 8192 logits per row") == -5
    assert answer(binarize(n=1 << 20, out_h=1 << 10, out_w=1 << 11), "maskpost_binarize: problem too large") == -2
    for null in ("logits", "rows", "out"):
        assert answer(binarize(**{null: None}), "maskpost_binarize: null pointer argument") == -1
    assert binarize(n=0, logits=None, rows=None, out=None) == 0                       # nothing to do: no launch

    assert answer(lib.maskpost_pack_hip_f32(ok, ok, 2, 0, 42, 1, ok, ok, None), "maskpost_pack: bad dimensions") == -2
    assert answer(lib.maskpost_pack_hip_f32(ok, ok, 1 << 12, 1 << 10, 1 << 10, 1, ok, ok, None), "maskpost_pack: problem too large") == -2
    assert answer(lib.maskpost_pack_hip_f32(ok, None, 2, 25, 42, 1, ok, ok, None), "maskpost_pack: null pointer argument") == -1
    assert answer(lib.maskpost_pack_hip_f32(ok, ok, 2, 25, 42, 1, ok, None, None), "maskpost_pack: null pointer argument") == -1
    assert lib.maskpost_pack_hip_f32(None, None, 2, 25, 42, 0, None, None, None) == 0

    assert answer(lib.maskpost_nms_hip_u32(ok, ok, _lib.MASKPOST_MAX_MASKS + 1, 33, 0.5, ok, ok, None), "maskpost_nms: at most 1024 masks") == -5
    assert answer(lib.maskpost_nms_hip_u32(ok, ok, 3, 0, 0.5, ok, ok, None), "maskpost_nms: bad dimensions") == -2
    assert answer(lib.maskpost_nms_hip_u32(ok, ok, -1, 33, 0.5, ok, ok, None), "maskpost_nms: bad dimensions") == -2
    assert answer(lib.maskpost_nms_hip_u32(ok, None, 3, 33, 0.5, ok, ok, None), "maskpost_nms: null pointer argument") == -1
    assert answer(lib.maskpost_nms_hip_u32(ok, ok, 3, 33, 0.5, ok, None, None), "maskpost_nms: null pointer argument") == -1
    assert lib.maskpost_nms_hip_u32(None, None, 0, 33, 0.5, None, None, None) == 0


def test_supported_sizes_follow_the_c_abi():
    from uninext_amd import ext
    assert ext.maskpost_supported(25, 42, 4, (97, 161), (60, 100), 0.5)
    assert ext.maskpost_supported(200, 336, 4, (800, 1333), (800, 1333), 0.5, 900, 100)
    assert not ext.maskpost_supported(25, 42, 3, (70, 100), (60, 100), 0.5)
    assert not ext.maskpost_supported(25, 42, 4, (101, 161), (60, 100), 0.5)
    assert not ext.maskpost_supported(25, 42, 4, (97, 161), (60, 100), 1.0)
    assert not ext.maskpost_supported(25, 42, 4, (97, 161), (0, 100), 0.5)
    assert not ext.maskpost_supported(2, 8193, 1, (2, 8193), (2, 8193), 0.5)
    assert not ext.maskpost_supported(25, 42, 4, (97, 161), (1 << 10, 1 << 11), 0.5, 7, 1 << 20)


def test_launchers_refuse_cpu_tensors():
    from uninext_amd import ext
    c = M.binarize_case("single")
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.maskpost_binarize(c["planes"], c["rows"], 4, c["crop"], c["out"], 0.5)
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.maskpost_pack(c["planes"], c["rows"])


def test_detection_postprocess_keeps_its_keys_and_gains_masks_on_request():
    from uninext_amd.postprocess import DetectionPostProcess, postprocess_masks
    fx = P.load("grounding_q300_t64")
    args = (fx["box_cls"], fx["box_pred"], fx["iou_pred"], fx["image_sizes"], fx["positive_map"], fx["num_classes"])
    post = DetectionPostProcess(ota=True, fused=False)
    plain = post(*args, task="grounding")
    assert all(sorted(r) == ["pred_boxes", "pred_classes", "query_index", "scores"] for r in plain)
    B, Q = fx["box_cls"].shape[:2]
    mask_pred = torch.randn(B, Q, 1, 9, 13, generator=torch.Generator().manual_seed(3))
    sizes = [(33, 50), (30, 41)]
    with_masks = post(*args[:3], sizes, *args[4:], task="grounding", mask_pred=mask_pred, output_sizes=[(48, 64), (33, 50)])
    for b, (r, p) in enumerate(zip(with_masks, plain)):
        assert sorted(r) == ["pred_boxes", "pred_classes", "pred_masks", "query_index", "scores"]
        assert torch.equal(r["query_index"], p["query_index"])
        want = postprocess_masks(mask_pred[b], r["query_index"], sizes[b], [(48, 64), (33, 50)][b], fused=False)
        assert torch.equal(r["pred_masks"], want) and tuple(want.shape) == (1,) + [(48, 64), (33, 50)][b]
    at_image = post(*args[:3], sizes, *args[4:], task="grounding", mask_pred=mask_pred)
    assert [tuple(r["pred_masks"].shape) for r in at_image] == [(1, 33, 50), (1, 30, 41)]


def test_segmentation_postprocess_scales_clips_and_drops():
    from uninext_amd.postprocess import segmentation_postprocess
    result = {"scores": torch.tensor([0.9, 0.8, 0.7]), "pred_classes": torch.tensor([1, 2, 3]), "query_index": torch.tensor([4, 5, 6]),
              "pred_boxes": torch.tensor([[10.0, 20.0, 50.0, 60.0], [90.0, 10.0, 130.0, 30.0], [120.0, 5.0, 140.0, 9.0]]),
              "pred_masks": (torch.arange(3 * 40 * 100).view(3, 40, 100) % 3 == 0).byte()}
    out = segmentation_postprocess(result, 80, 50)       # 100 wide -> 50: x halves; 40 high -> 80: y doubles
    assert out["scores"].tolist() == pytest.approx([0.9, 0.8]) and out["query_index"].tolist() == [4, 5]
    np.testing.assert_allclose(out["pred_boxes"].numpy(), [[5, 40, 25, 80], [45, 20, 50, 60]])       # clipped; the third is empty
    want = F.interpolate(result["pred_masks"][:2].unsqueeze(1).float(), size=(80, 50), mode="nearest")[:, 0].byte()
    assert torch.equal(out["pred_masks"], want)
    assert len(result["scores"]) == 3 and result["pred_boxes"][0, 0] == 10.0          # the input is left as it was
    boxes_only = segmentation_postprocess({k: v for k, v in result.items() if k != "pred_masks"}, 80, 50, image_size=(40, 100))
    assert sorted(boxes_only) == ["pred_boxes", "pred_classes", "query_index", "scores"] and len(boxes_only["scores"]) == 2
