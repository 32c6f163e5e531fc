"""Mask post-processing on the GPU: the fused binarise-and-resize kernel against the reference's fixtures and against the
composition of PyTorch ops on the GPU (both outside the float64 band of tests/maskpost_cases.py, which may hold at most 1e-4 of
a case's pixels), the pack / pair / scan kernels of the mask NMS against torch's integer sums and the reference's keep flags,
and the kernels' own contracts: guard bands around every output, repeatability, the name of the kernel that ran."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maskpost_cases as M   # noqa: E402
import postprocess_cases as P   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 256                                     # sentinel bytes (elements) on either side of an output
SENTINEL = {torch.int32: 0x5A5A5A5A, torch.uint8: 0x5A}


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


def run_binarize(c):
    from uninext_amd import ext
    guard = Guarded()
    out = guard((len(c["rows"]),) + c["out"], torch.uint8)
    got = ext.maskpost_binarize(c["planes"].to(DEV), c["rows"].to(DEV), c["stride"], c["crop"], c["out"], c["thres"], out=out)
    torch.cuda.synchronize()
    guard.check()
    return got


@pytest.mark.parametrize("name", sorted(M.BINARIZE_CASES))
def test_binarize_kernel_gives_the_reference_masks(name):
    from uninext_amd import _lib
    from uninext_amd.postprocess import postprocess_masks
    c = M.binarize_case(name)
    got = run_binarize(c)
    assert _lib.last_kernel("maskpost") == "maskpost_binarize"
    assert not bool((got == SENTINEL[torch.uint8]).any())            # every byte was written
    M.check_masks(got, c, name + ": kernel against the fixture")
    assert torch.equal(run_binarize(c), got)                          # two runs, the same bytes
    composed = postprocess_masks(c["planes"].to(DEV), c["rows"].to(DEV), c["crop"], c["out"], c["stride"], c["thres"], fused=False)
    M.check_masks(composed, c, name + ": composition on the GPU against the fixture")
    fused = postprocess_masks(c["planes"].unsqueeze(1).to(DEV), c["rows"].to(DEV), c["crop"], c["out"], c["stride"], c["thres"],
                              fused=True)
    assert torch.equal(fused, got)
    wrong = int(((got != composed).cpu() & ~c["excluded"]).sum())
    assert wrong == 0


def test_binarize_row_start_alignments_and_an_unaligned_base():
    """Rows of 13, 100, 161 and 333 bytes start at every residue of 16; here the base itself is off by 1..15 bytes as well."""
    from uninext_amd import ext
    c = M.binarize_case("down_60x100")
    want = run_binarize(c)
    n, numel = len(c["rows"]), want.numel()
    for shift in (1, 7, 15):
        buf = torch.full((BAND + shift + numel + BAND,), SENTINEL[torch.uint8], dtype=torch.uint8, device=DEV)
        out = buf[BAND + shift:BAND + shift + numel].view(n, *c["out"])
        ext.maskpost_binarize(c["planes"].to(DEV), c["rows"].to(DEV), c["stride"], c["crop"], c["out"], c["thres"], out=out)
        assert torch.equal(out, want)
        assert bool((buf[:BAND + shift] == 0x5A).all()) and bool((buf[BAND + shift + numel:] == 0x5A).all())


def test_binarize_of_no_instance_launches_nothing_and_a_row_outside_q_is_an_empty_mask():
    from uninext_amd import _lib, ext
    c = M.binarize_case("single")
    run_binarize(c)
    ext.maskpost_pack(c["planes"].to(DEV), c["rows"].to(DEV))
    assert _lib.last_kernel("maskpost") == "maskpost_pack"
    got = ext.maskpost_binarize(c["planes"].to(DEV), c["rows"][:0].to(DEV), 4, c["crop"], c["out"], 0.5)
    assert tuple(got.shape) == (0,) + c["out"] and _lib.last_kernel("maskpost") == "maskpost_pack"
    rows = torch.tensor([3, 7, -1], dtype=torch.int64, device=DEV)
    got = ext.maskpost_binarize(c["planes"].to(DEV), rows, 4, c["crop"], c["out"], 0.5)
    assert torch.equal(got[0].cpu(), c["expect"][0]) and int(got[1:].sum()) == 0


def test_unsupported_sizes_are_error_codes_and_the_module_takes_the_composition():
    from uninext_amd import _lib, ext
    from uninext_amd.postprocess import postprocess_masks
    c = M.binarize_case("single")
    planes, rows = c["planes"].to(DEV), c["rows"].to(DEV)
    with pytest.raises(RuntimeError, match=r"code -5"):
        ext.maskpost_binarize(planes, rows, 3, (70, 120), (70, 120), 0.5)
    with pytest.raises(RuntimeError, match=r"code -2"):
        ext.maskpost_binarize(planes, rows, 4, (101, 161), (97, 161), 0.5)
    ext.maskpost_pack(planes, rows)
    got = postprocess_masks(planes, rows, (70, 120), None, 3, 0.5, fused=True)                # stride 3: the composition
    assert _lib.last_kernel("maskpost") == "maskpost_pack" and tuple(got.shape) == (1, 70, 120)
    got = postprocess_masks(planes.half(), rows, c["crop"], None, 4, 0.5, fused=True)         # fp16: the composition
    assert _lib.last_kernel("maskpost") == "maskpost_pack" and got.dtype == torch.uint8


def run_nms(logits, thr):
    from uninext_amd import _lib, ext
    n, _, h, w = logits.shape
    words = (h * w + 31) // 32
    guard = Guarded()
    packed = (guard((n, words), torch.int32), guard((n,), torch.int32))
    rows = torch.arange(n, dtype=torch.int64, device=DEV)
    bits, area = ext.maskpost_pack(logits[:, 0].contiguous().to(DEV), rows, out=packed)
    assert _lib.last_kernel("maskpost") == "maskpost_pack"
    out = (guard((n, n), torch.int32), guard((n,), torch.uint8))
    inter, keep = ext.maskpost_nms(bits, area, thr, out=out)
    torch.cuda.synchronize()
    guard.check()
    assert _lib.last_kernel("maskpost") == "maskpost_nms"
    return bits.cpu(), area.cpu(), inter.cpu(), keep.cpu()


def assert_nms(logits, thr, want_keep):
    from uninext_amd.postprocess import mask_nms
    n, _, h, w = logits.shape
    bits, area, inter, keep = run_nms(logits, thr)
    masks = (logits.sigmoid() > 0.5).view(n, -1)
    # the packed words, bit k % 32 of word k / 32, zero past h * w
    padded = torch.zeros(n, bits.shape[1] * 32, dtype=torch.int64)
    padded[:, :h * w] = masks.long()
    words = (padded.view(n, -1, 32) << torch.arange(32)).sum(-1)
    assert torch.equal(bits.long() & 0xFFFFFFFF, words)
    assert torch.equal(area.long(), masks.long().sum(1))
    assert torch.equal(inter.long(), (masks.float() @ masks.float().T).long())      # sums below 2^24: exact, every entry
    assert [bool(k) for k in keep.tolist()] == want_keep
    again = run_nms(logits, thr)
    assert all(torch.equal(a, b) for a, b in zip((bits, area, inter, keep), again))
    assert mask_nms(logits.to(DEV), [0.0] * n, None, nms_thr=thr, fused=True) == want_keep
    return keep


@pytest.mark.parametrize("name", M.NMS_CASES + list(M.NMS_HAND))
def test_mask_nms_kernels_give_the_reference_flags(name):
    c = M.nms_case(name)
    assert torch.equal((c["logits"] > 0).view(len(c["keep"]), -1), c["masks"])
    assert_nms(c["logits"], c["thr"], c["keep"])


def test_mask_nms_at_the_limit_of_1024_masks():
    """The scan kernel's largest matrix (128 KB of LDS, beyond what a launch gets without opting in), against the restatement of
    mask_nms from the matrix of all pairs that tests/test_maskpost_cpu.py holds to the reference on every fixture."""
    from uninext_amd import ext
    n, h, w = 1024, 25, 42
    logits = M.nms_logits(M.nms_params(11, n, h, w), h, w, 11)
    _, _, keep, margin = M.mask_nms_restated(logits, M.NMS_THR)
    assert margin >= M.IOU_MARGIN and 2 <= keep.sum() < n
    assert_nms(logits, M.NMS_THR, [bool(k) for k in keep])
    with pytest.raises(RuntimeError, match=r"code -5"):
        ext.maskpost_nms(torch.zeros(n + 1, 33, dtype=torch.int32, device=DEV), torch.zeros(n + 1, dtype=torch.int32, device=DEV), 0.5)


def test_mask_nms_composition_on_the_gpu_gives_the_same_list():
    from uninext_amd.postprocess import mask_nms
    c = M.nms_case("n37_25x42")
    assert mask_nms(c["logits"].to(DEV), [0.0] * 37, None, nms_thr=c["thr"], fused=False) == c["keep"]


def test_detection_postprocess_with_masks_end_to_end(monkeypatch):
    from uninext_amd import _lib
    from uninext_amd.postprocess import DetectionPostProcess, MaskPostProcess, postprocess_masks
    fx = P.load("thres_few_q300_t64")
    B, Q = fx["box_cls"].shape[:2]
    h, w, stride = 25, 42, 4
    sizes, outs = [(97, 161), (100, 150)], [(60, 100), (100, 150)]
    mask_pred = torch.stack([M.blob_planes(40 + b, Q, h, w) for b in range(B)]).unsqueeze(2)
    args = [fx[k].to(DEV) for k in ("box_cls", "box_pred", "iou_pred")]
    rest = (fx["positive_map"], fx["num_classes"])
    monkeypatch.setattr(MaskPostProcess, "fused", True)
    got = DetectionPostProcess(ota=True, fused=True)(*args, sizes, *rest, score_thres=0.3, mask_pred=mask_pred.to(DEV),
                                                     output_sizes=outs, mask_stride=stride)
    assert _lib.last_kernel("maskpost") == "maskpost_binarize"
    monkeypatch.setattr(MaskPostProcess, "fused", False)
    want = DetectionPostProcess(ota=True, fused=True)(*args, sizes, *rest, score_thres=0.3, mask_pred=mask_pred.to(DEV),
                                                      output_sizes=outs, mask_stride=stride)
    for b, (g, e) in enumerate(zip(got, want)):
        n = len(g["scores"])
        assert 0 < n and torch.equal(g["query_index"], e["query_index"])
        assert g["pred_masks"].dtype == torch.uint8 and tuple(g["pred_masks"].shape) == (n,) + outs[b]
        rows = g["query_index"].cpu()
        _, excluded = M.float64_decision(mask_pred[b, :, 0], rows.tolist(), stride, sizes[b], outs[b], 0.5)
        assert float(excluded.float().mean()) <= M.MAX_EXCLUDED_SHARE
        assert int(((g["pred_masks"] != e["pred_masks"]).cpu() & ~excluded).sum()) == 0
        on_cpu = postprocess_masks(mask_pred[b], rows, sizes[b], outs[b], stride, 0.5, fused=False)
        assert int(((g["pred_masks"].cpu() != on_cpu) & ~excluded).sum()) == 0
        assert 0.02 < float(on_cpu.float().mean()) < 0.98
