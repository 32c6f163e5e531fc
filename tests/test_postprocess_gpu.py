"""Detection post-processing on the GPU: the two detpost kernels against the PyTorch composition and the CPU restatement of
NMS (given identical scores and classes, so the kept indices are compared exactly), the fused DetectionPostProcess against
the reference's fixtures, and the kernels' own contracts: repeatability, independence of the other images of a batch, guard
bands around every output, error codes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import postprocess_cases as P   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 256                                     # guard elements on either side of an output
SENTINEL = {torch.float32: 12345.0, torch.int32: 0x5A5A5A5A, torch.uint8: 0x5A}


class Guarded:
    """Outputs carved out of larger buffers filled with a sentinel; check() asserts the bands are as they were."""

    def __init__(self):
        self.bufs = []

    def __call__(self, shape, dtype):
        n = int(np.prod(shape))
        buf = torch.full((BAND + n + BAND,), SENTINEL[dtype], dtype=dtype, device=DEV)
        self.bufs.append((buf, n))
        return buf[BAND:BAND + n].view(shape)

    def check(self):
        for buf, n in self.bufs:
            assert bool((buf[:BAND] == SENTINEL[buf.dtype]).all()) and bool((buf[BAND + n:] == SENTINEL[buf.dtype]).all())


def csr_of(pm, C, T):
    from uninext_amd.postprocess import positive_map_csr
    csr = positive_map_csr(pm, C, T, torch.device(DEV))
    assert csr is not None and csr[0].numel() == C + 1
    return csr


@pytest.mark.parametrize("Q,C,T", [(1, 1, 1), (65, 80, 256), (300, 365, 256), (900, 80, 256)])
def test_scores_kernel_equals_the_composition(Q, C, T):
    from uninext_amd import _lib, ext
    logits, iou, pm, expect = P.scores_case(Q, C, T)
    B = logits.shape[0]
    cls_ptr, tok_idx = csr_of(pm, C, T)
    for (with_iou, thres), (prob, mx, arg, valid) in expect.items():
        guard = Guarded()
        out = (guard((B, Q, C), torch.float32), guard((B, Q), torch.float32), guard((B, Q), torch.int32), guard((B, Q), torch.int32))
        got = ext.detpost_scores(logits.to(DEV), iou.to(DEV) if with_iou else None, cls_ptr, tok_idx, thres, out=out)
        torch.cuda.synchronize()
        guard.check()
        assert _lib.last_kernel("detpost") == ("detpost_scores<iou>" if with_iou else "detpost_scores")
        g_prob, g_max, g_arg, g_valid = (t.cpu() for t in got)
        np.testing.assert_array_equal((g_prob == -1.0).numpy(), (prob == -1.0).numpy())
        np.testing.assert_allclose(g_prob.numpy(), prob.numpy(), rtol=0, atol=P.MARGIN)
        np.testing.assert_allclose(g_max.numpy(), mx.numpy(), rtol=0, atol=P.MARGIN)
        np.testing.assert_array_equal(g_arg.numpy(), arg.numpy())
        np.testing.assert_array_equal(g_valid.numpy(), valid.numpy())
        assert int(g_valid.sum()) == int(valid.sum())
        np.testing.assert_array_equal(g_max.numpy(), g_prob.max(-1)[0].numpy())          # the kernel's own maximum, exactly


def run_nms(boxes, scores, cls, threshold, per_class):
    from uninext_amd import ext
    B, Q = scores.shape
    guard = Guarded()
    out = (guard((B, Q), torch.int32), guard((B,), torch.int32), guard((B, Q), torch.uint8))
    keep, n_keep, kept_mask = ext.detpost_nms(boxes.to(DEV).contiguous(), scores.to(DEV).contiguous(), cls.int().to(DEV).contiguous(),
                                              threshold, per_class=per_class, out=out)
    torch.cuda.synchronize()
    guard.check()
    return keep.cpu(), n_keep.cpu(), kept_mask.cpu()


def assert_nms(got, expect, Q):
    keep, n_keep, kept_mask = got
    for b, want in enumerate(expect):
        n = len(want)
        assert int(n_keep[b]) == n
        np.testing.assert_array_equal(keep[b, :n].numpy(), want.numpy())
        assert bool((keep[b, n:] == -1).all())                     # the padded tail
        mask = torch.zeros(Q, dtype=torch.uint8)
        mask[want] = 1
        np.testing.assert_array_equal(kept_mask[b].numpy(), mask.numpy())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Q", [1, 63, 64, 65, 128, 900, 1024])
def test_nms_kernel_equals_the_cpu_restatement(Q, B):
    from uninext_amd import _lib
    boxes, scores, cls, expect = P.nms_case(Q, B)       # asserts the IoU margin on the CPU first
    for per_class in (0, 1):
        got = run_nms(boxes, scores, cls, 0.7, per_class)
        assert _lib.last_kernel("detpost") == ("detpost_nms<per_class>" if per_class else "detpost_nms<offset>")
        assert_nms(got, expect[per_class], Q)
        assert 0 < int(got[1].min()) and (Q < 63 or int(got[1].max()) < Q)


@pytest.mark.parametrize("case", sorted(P.hand_cases()))
def test_nms_kernel_hand_built(case):
    xyxy, scores, classes, expect = P.hand_cases()[case]
    boxes = P.xyxy_to_cxcywh(xyxy).unsqueeze(0)         # small integers and halves: the conversion back is exact
    for per_class in (0, 1):
        got = run_nms(boxes, scores.unsqueeze(0), torch.tensor([classes]), 0.5, per_class)
        assert_nms(got, [torch.tensor(expect)], len(classes))


def test_more_than_1024_queries_is_an_error_code_and_the_module_takes_the_composition():
    from uninext_amd import _lib, ext
    from uninext_amd.postprocess import DetectionPostProcess
    Q = _lib.DETPOST_MAX_QUERIES + 1
    g = torch.Generator().manual_seed(5)
    boxes = torch.cat([0.2 + 0.6 * torch.rand(1, Q, 2, generator=g), 0.05 + 0.1 * torch.rand(1, Q, 2, generator=g)], -1)
    with pytest.raises(RuntimeError, match=r"code -5"):
        ext.detpost_nms(boxes.to(DEV), torch.rand(1, Q, generator=g).to(DEV), torch.zeros(1, Q, dtype=torch.int32, device=DEV), 0.7)
    logits = torch.randn(1, Q, 8, generator=g)
    pm = {1: [0, 1], 2: [3], 3: [4, 5, 6]}
    ext.detpost_scores(logits.to(DEV), None, *csr_of(pm, 3, 8))
    before = _lib.last_kernel("detpost")
    args = ([(480, 640)], pm, 3)
    got = DetectionPostProcess(fused=True)(logits.to(DEV), boxes.to(DEV), None, *args)
    assert _lib.last_kernel("detpost") == before == "detpost_scores"      # no detpost kernel ran for the module
    want = DetectionPostProcess(fused=False)(logits, boxes, None, *args)
    assert len(got[0]["scores"]) == len(want[0]["scores"]) == 100
    np.testing.assert_allclose(got[0]["scores"].cpu().numpy(), want[0]["scores"].numpy(), rtol=0, atol=P.MARGIN)


@pytest.mark.parametrize("name,run", P.RUNS)
def test_fused_reproduces_the_reference(name, run):
    from uninext_amd import _lib
    from uninext_amd.postprocess import DetectionPostProcess
    P.check_against_fixture(lambda ota, demo: DetectionPostProcess(ota=ota, fused=True, demo_only=demo), name, run, device=DEV)
    want = "detpost_nms<offset>" if P.load(name)["runs"][run][0]["ota"] else "detpost_scores"
    assert _lib.last_kernel("detpost").startswith(want)


def test_fused_is_repeatable_and_an_image_does_not_depend_on_its_batch():
    from uninext_amd.postprocess import DetectionPostProcess
    fx = P.load("coco_q300_t256")
    post = DetectionPostProcess(ota=True, fused=True)
    x = [fx[k].to(DEV) for k in ("box_cls", "box_pred", "iou_pred")]
    rest = (fx["positive_map"], fx["num_classes"])
    first = post(*x, fx["image_sizes"], *rest, score_thres=0.6)
    again = post(*x, fx["image_sizes"], *rest, score_thres=0.6)
    alone = post(*(t[1:2].contiguous() for t in x), fx["image_sizes"][1:2], *rest, score_thres=0.6)
    for key in ("scores", "pred_classes", "pred_boxes", "query_index"):
        for a, b in zip(first, again):
            assert torch.equal(a[key], b[key])
        assert torch.equal(first[1][key], alone[0][key])
    assert 0 < len(first[1]["scores"]) <= 100
