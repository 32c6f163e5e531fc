"""The criterion's kernels on the GPU (uninext_amd/csrc/criterion.hip) against the float64 evaluation of the reference's formulas
(tests/criterion_cases.py), the autograd Functions against the composition's autograd, the fused DINOCriterion against the
reference's fixtures, and the kernels' own contracts: guard bands around every output and the workspace, repeatability,
independence of the other images of a batch, error codes.

Tolerance: a fused value passes if its error against float64 is within 1e-4 of the value's own scale, max |value|
(tests/criterion_cases.py: scaled_error; no floor of 1: the gradient of a mask loss is of order 1e-5 and is held to 1e-9).  The fp32
composition's error against the same float64 is computed next to it and printed (tools/criterion_bench.py --errors tabulates
both); nothing is asserted on their ratio."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import criterion_cases as C   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 256                                     # guard elements on either side of an output
SENTINEL = {torch.float32: 12345.0, torch.uint8: 0x5A}


class Guarded:
    """Outputs carved out of larger buffers filled with a sentinel; check() asserts the bands are as they were."""

    def __init__(self):
        self.bufs = []

    def __call__(self, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        buf = torch.full((BAND + n + BAND,), SENTINEL[dtype], dtype=dtype, device=DEV)
        self.bufs.append((buf, n))
        return buf[BAND:BAND + n].view(shape)

    def check(self):
        for buf, n in self.bufs:
            assert bool((buf[:BAND] == SENTINEL[buf.dtype]).all()) and bool((buf[BAND + n:] == SENTINEL[buf.dtype]).all())


scaled = C.scaled_error


def workspace(guard, which, count, per):
    from uninext_amd import _lib
    nbytes = _lib.load().criterion_hip_workspace_bytes(which, count, per)
    assert nbytes > 0 and nbytes % 8 == 0
    return guard((nbytes,), torch.uint8)               # BAND = 256 bytes in front: the carved workspace stays 16-byte aligned


# ---- token focal loss ---------------------------------------------------------------------------------------------------------
def token_composition(logits, mask, row_target, pm):
    """(loss, grad) of the fp32 PyTorch composition on the device."""
    from uninext_amd.criterion import token_sigmoid_binary_focal_loss
    x = logits.to(DEV).requires_grad_(True)
    onehot = torch.zeros_like(x)
    hit = row_target.to(DEV) >= 0
    onehot[hit] = pm.to(DEV)[row_target.to(DEV)[hit].long()]
    loss = token_sigmoid_binary_focal_loss(x, onehot, alpha=C.ALPHA, text_mask=None if mask is None else mask.to(DEV))
    loss.backward()
    return float(loss.detach()), x.grad.cpu()


@pytest.mark.parametrize("variant", C.TOKEN_VARIANTS)
@pytest.mark.parametrize("B,Q,T", C.TOKEN_GEOMETRIES)
def test_token_focal_kernels_equal_float64(B, Q, T, variant):
    from uninext_amd import _lib, ext
    logits, mask, row_target, pm, want_loss, want_grad = C.token_case(B, Q, T, variant)
    x, rt, pmd = logits.to(DEV), row_target.to(DEV), pm.to(DEV)
    m = None if mask is None else mask.to(DEV)
    guard = Guarded()
    out, grad = guard((1,)), guard((B, Q, T))
    ws = workspace(guard, _lib.CRITERION_TOKEN_FOCAL, B * Q, T)
    vec = "<vec4>" if T % 4 == 0 else "<scalar>"
    loss = ext.token_focal_loss_forward(x, m, rt, pmd, C.ALPHA, out=out, workspace=ws)
    assert _lib.last_kernel("criterion") == "token_focal_fwd" + vec
    scale = torch.ones(1, device=DEV)
    ext.token_focal_loss_backward(x, m, rt, pmd, C.ALPHA, scale, out=grad)
    assert _lib.last_kernel("criterion") == "token_focal_bwd" + vec
    torch.cuda.synchronize()
    guard.check()
    ref_loss, ref_grad = token_composition(logits, mask, row_target, pm)
    e_loss, e_grad = scaled(float(loss), want_loss), scaled(grad.cpu(), want_grad)
    print("token %s %s: fused loss %.3e grad %.3e | composition loss %.3e grad %.3e (scaled errors against float64)"
          % ((B, Q, T), variant, e_loss, e_grad, scaled(ref_loss, want_loss), scaled(ref_grad, want_grad)))
    assert bool(torch.isfinite(grad).all()) and np.isfinite(float(loss))
    assert e_loss <= C.MARGIN and e_grad <= C.MARGIN
    if mask is not None:
        dead = ~(mask > 0)
        assert bool((grad.cpu().permute(0, 2, 1)[dead] == 0).all())         # exactly 0.0 at masked tokens
    # a second call gives the same bits
    again = ext.token_focal_loss_forward(x, m, rt, pmd, C.ALPHA)
    assert torch.equal(again, loss)
    assert torch.equal(ext.token_focal_loss_backward(x, m, rt, pmd, C.ALPHA, scale), grad)


def test_more_than_256_tokens_is_an_error_code_and_the_module_takes_the_composition():
    from uninext_amd import _lib, ext
    from uninext_amd.criterion import SetCriterion
    g = torch.Generator().manual_seed(9)
    T = _lib.CRITERION_MAX_TOKENS + 1
    logits = torch.randn(1, 5, T, generator=g).to(DEV)
    rt = torch.full((1, 5), -1, dtype=torch.int32, device=DEV)
    pm = torch.zeros(2, T, device=DEV)
    with pytest.raises(RuntimeError, match=r"code -5"):
        ext.token_focal_loss_forward(logits, None, rt, pm, 0.25)
    with pytest.raises(RuntimeError, match=r"code -5"):
        ext.token_focal_loss_backward(logits, None, rt, pm, 0.25, torch.ones(1, device=DEV))
    assert not ext.token_focal_loss_supported(logits, None) and ext.token_focal_loss_supported(logits[:, :, :256].contiguous(), None)
    assert not ext.token_focal_loss_supported(logits[:, :, :256].contiguous(), None, gamma=1.5)
    ext.token_focal_loss_forward(logits[:, :, :8].contiguous(), None, rt, pm[:, :8].contiguous(), 0.25)
    before = _lib.last_kernel("criterion")
    targets = [{"positive_map": pm.bool()}]
    indices = [(torch.tensor([1, 3]), torch.tensor([0, 1]))]
    crit = SetCriterion(None, {}, ["labelsVL"])
    crit.fused = True
    got = crit.loss_labelsVL({"pred_logits": logits, "text_masks": None}, targets, indices, 2.0)["loss_ce"]
    assert _lib.last_kernel("criterion") == before == "token_focal_fwd<vec4>"           # no kernel ran for the module
    crit.fused = False
    want = crit.loss_labelsVL({"pred_logits": logits, "text_masks": None}, targets, indices, 2.0)["loss_ce"]
    assert torch.equal(got, want)


def test_empty_problems_write_zeros():
    from uninext_amd import ext
    guard = Guarded()
    out = guard((1,))
    ext.token_focal_loss_forward(torch.zeros(2, 0, 8, device=DEV), None, torch.zeros(2, 0, dtype=torch.int32, device=DEV),
                                 torch.zeros(1, 8, device=DEV), 0.25, out=out)
    losses, sums = guard((2,)), guard((0, 4))
    src = torch.zeros(0, 1, 4, 4, device=DEV)
    gt = torch.zeros(1, 1, 16, 16, dtype=torch.bool, device=DEV)
    rows = torch.zeros(0, dtype=torch.int32, device=DEV)
    ext.mask_losses_forward(src, gt, rows, 4, 1.0, out=(losses, sums))
    grad = ext.mask_losses_backward(src, gt, rows, 4, 1.0, sums, torch.ones(1, device=DEV), torch.ones(1, device=DEV))
    torch.cuda.synchronize()
    guard.check()
    assert float(out) == 0.0 and losses.tolist() == [0.0, 0.0] and grad.shape == (0, 1, 4, 4)


# ---- mask losses --------------------------------------------------------------------------------------------------------------
def mask_composition(src, tgt):
    from uninext_amd.criterion import dice_loss, sigmoid_focal_loss
    x = src.to(DEV).requires_grad_(True)
    t = tgt.to(DEV).float().flatten(1)
    lm, ld = sigmoid_focal_loss(x.flatten(1), t, C.MASK_NUM_BOXES), dice_loss(x.flatten(1), t, C.MASK_NUM_BOXES)
    (lm + 2.0 * ld).backward()
    return (float(lm.detach()), float(ld.detach())), x.grad.cpu()


@pytest.mark.parametrize("n,F,h,w,stride", C.MASK_GEOMETRIES)
def test_mask_loss_kernels_equal_float64(n, F, h, w, stride):
    from uninext_amd import _lib, ext
    from uninext_amd.criterion import SetCriterion
    src, gt, gt_row, want, want_grad = C.mask_case(n, F, h, w, stride)
    x, gtd, rows = src.to(DEV), gt.to(DEV), gt_row.to(DEV)
    guard = Guarded()
    losses, sums, grad = guard((2,)), guard((n, 4)), guard((n, F, h, w))
    ws = workspace(guard, _lib.CRITERION_MASK_LOSSES, n, F * h * w)
    vec = "<vec4>" if w % 4 == 0 else "<scalar>"
    ext.mask_losses_forward(x, gtd, rows, stride, C.MASK_NUM_BOXES, out=(losses, sums), workspace=ws)
    assert _lib.last_kernel("criterion") == "mask_losses_fwd" + vec
    ext.mask_losses_backward(x, gtd, rows, stride, C.MASK_NUM_BOXES, sums, torch.ones(1, device=DEV), torch.full((1,), 2.0, device=DEV),
                             out=grad)
    assert _lib.last_kernel("criterion") == "mask_losses_bwd" + vec
    torch.cuda.synchronize()
    guard.check()
    # the target read: sum t per instance, exactly, against get_target_masks(...)[tgt_idx] of the composition
    crit = SetCriterion(None, {}, ["masks"], mask_out_stride=stride)
    targets = [{"masks": gt[b]} for b in range(gt.shape[0])]
    # (get_target_masks pads to multiples of 32: the padding is cropped; at stride 1 it slices nothing)
    dense = crit.get_target_masks(targets, src)[:, :, :h, :w]
    tgt_idx = (torch.div(gt_row.long(), gt.shape[1], rounding_mode="floor"), gt_row.long() % gt.shape[1] // F)
    gathered = dense.reshape(gt.shape[0], -1, F, h, w)[tgt_idx]
    assert torch.equal(gathered, C.target_pixels(gt.view(-1, *gt.shape[-2:]), gt_row, F, h, w, stride).float())
    np.testing.assert_array_equal(sums[:, 3].cpu().numpy(), gathered.flatten(1).sum(1).numpy())
    assert float(sums[0, 3]) == 0.0 and (n < 2 or float(sums[-1, 3]) == F * h * w)
    if n >= 3:
        assert int(gt_row[1]) == int(gt_row[2]) and float(sums[1, 3]) == float(sums[2, 3])
    ref, ref_grad = mask_composition(src, gathered)
    e = [scaled(float(losses[k]), want[k]) for k in range(2)] + [scaled(grad.cpu(), want_grad)]
    r = [scaled(ref[k], want[k]) for k in range(2)] + [scaled(ref_grad, want_grad)]
    print("mask %s: fused mask %.3e dice %.3e grad %.3e | composition mask %.3e dice %.3e grad %.3e (scaled errors against float64)"
          % ((n, F, h, w, stride), *e, *r))
    assert max(e) <= C.MARGIN
    again, sums2 = ext.mask_losses_forward(x, gtd, rows, stride, C.MASK_NUM_BOXES)
    assert torch.equal(again, losses) and torch.equal(sums2, sums)
    assert torch.equal(ext.mask_losses_backward(x, gtd, rows, stride, C.MASK_NUM_BOXES, sums, torch.ones(1, device=DEV),
                                                torch.full((1,), 2.0, device=DEV)), grad)


def test_mask_kernel_refuses_pixels_outside_the_ground_truth():
    from uninext_amd import ext
    src = torch.zeros(1, 1, 5, 4, device=DEV)
    gt = torch.zeros(1, 1, 16, 16, dtype=torch.bool, device=DEV)
    with pytest.raises(RuntimeError, match=r"code -2"):
        ext.mask_losses_forward(src, gt, torch.zeros(1, dtype=torch.int32, device=DEV), 4, 1.0)
    # a row outside the ground truth reads as an all-zero target: nothing is touched out of bounds
    src = torch.zeros(1, 1, 4, 4, device=DEV)
    losses, sums = ext.mask_losses_forward(src, ~gt, torch.full((1,), 7, dtype=torch.int32, device=DEV), 4, 1.0)
    assert float(sums[0, 3]) == 0.0 and float(sums[0, 2]) == 8.0


# ---- the autograd Functions and the module --------------------------------------------------------------------------------------
def test_functions_gradients_equal_the_compositions_autograd():
    from uninext_amd.criterion import MaskLossesFunction, TokenFocalLossFunction
    logits, mask, row_target, pm, _, _ = C.token_case(3, 130, 77, "int64")
    x = logits.to(DEV).requires_grad_(True)
    loss = TokenFocalLossFunction.apply(x, mask.to(DEV), row_target.to(DEV), pm.to(DEV), C.ALPHA, 7.0)
    (loss * 3.0).backward()
    ref_loss, ref_grad = token_composition(logits, mask, row_target, pm)
    C.within(float(loss.detach()), ref_loss / 7.0, "token loss")
    C.within(x.grad.cpu(), ref_grad * (3.0 / 7.0), "token grad")

    src, gt, gt_row, _, _ = C.mask_case(2, 2, 13, 21, 4)
    s = src.to(DEV).requires_grad_(True)
    lm, ld = MaskLossesFunction.apply(s, gt.to(DEV), gt_row.to(DEV), 4, C.MASK_NUM_BOXES)
    (lm + 2.0 * ld).backward()
    tgt = C.target_pixels(gt.view(-1, *gt.shape[-2:]), gt_row, 2, 13, 21, 4)
    ref, ref_grad = mask_composition(src, tgt)
    C.within(float(lm.detach()), ref[0], "loss_mask")
    C.within(float(ld.detach()), ref[1], "loss_dice")
    C.within(s.grad.cpu(), ref_grad, "mask grad")
    # only one of the two losses used: the other's upstream gradient is None
    s2 = src.to(DEV).requires_grad_(True)
    MaskLossesFunction.apply(s2, gt.to(DEV), gt_row.to(DEV), 4, C.MASK_NUM_BOXES)[0].backward()
    assert bool(torch.isfinite(s2.grad).all()) and float(s2.grad.abs().max()) > 0


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_fused_criterion_reproduces_the_reference(name):
    from uninext_amd import _lib
    _, expect = C.load(name)
    got = C.run_fixture(name, fused=True, device=DEV)
    assert set(got) == set(expect)
    for key, want in expect.items():
        C.within(float(got[key]), want, key)            # 1e-4 of the value itself
    # the last loss evaluated: the denoising queries' (or the encoder's) token focal loss, 16 tokens (1 with still_cls and no dn)
    cfg = C.CASES[name]
    assert _lib.last_kernel("criterion") == ("token_focal_fwd<vec4>" if cfg["dn"] or not cfg["still"] else "token_focal_fwd<scalar>")


def test_fused_criterion_gradients_equal_the_compositions():
    from uninext_amd import _lib
    results = []
    for fused in (True, False):
        losses, leaves = C.run_fixture("ota_dn", fused=fused, device=DEV, requires_grad=True)
        sum(v for k, v in losses.items() if v.requires_grad).backward()
        results.append([leaf.grad.cpu() for leaf in leaves])
        if fused:
            assert _lib.last_kernel("criterion") in ("token_focal_bwd<vec4>", "mask_losses_bwd<vec4>")
    assert len(results[0]) == len(results[1]) > 10
    for a, b in zip(*results):
        C.within(a, b, "criterion grad")


def test_fused_is_repeatable_and_an_image_does_not_depend_on_its_batch():
    from uninext_amd.criterion import SetCriterion
    cfg = C.CASES["ota_dn"]
    flat, _ = C.load("ota_dn")
    outputs, targets, indices_list, _ = C.rebuild(flat, cfg, DEV)
    crit = SetCriterion(None, {}, ["labelsVL", "masks"], mask_out_stride=C.STRIDE, ota=False)       # fixed num_boxes
    crit.fused = True
    indices = indices_list[-1]
    run = lambda out, tg, ix: {**crit.loss_labelsVL(out, tg, ix, 4.0), **crit.loss_masks(out, tg, ix, 4.0)}
    first, again = run(outputs, targets, indices), run(outputs, targets, indices)
    for key in first:
        assert torch.equal(first[key], again[key]), key
    alone = []
    for b in range(C.BS):
        out_b = {"pred_logits": outputs["pred_logits"][b:b + 1].contiguous(), "text_masks": outputs["text_masks"][b:b + 1].contiguous(),
                 "pred_masks": outputs["pred_masks"][b:b + 1]}
        alone.append(run(out_b, targets[b:b + 1], indices[b:b + 1]))
    # the sums are linear in the images: the batch's loss is the sum of the images' alone (float64 partial sums: to the last bits)
    for key in first:
        total = sum(float(a[key]) for a in alone)
        assert abs(float(first[key]) - total) <= 1e-6 * abs(total), (key, float(first[key]), total)


def test_a_gradient_does_not_depend_on_its_neighbours():
    """grad_logits of an image and grad_src of an instance, bit for bit, whatever the rest of the batch holds (NaN, huge values)
    and whether or not there is a rest."""
    from uninext_amd import ext
    g = torch.Generator().manual_seed(21)
    logits, mask, row_target, pm, _, _ = C.token_case(3, 130, 77, "int64")
    x, m, rt, pmd = logits.to(DEV), mask.to(DEV), row_target.to(DEV), pm.to(DEV)
    one = torch.ones(1, device=DEV)
    grad = ext.token_focal_loss_backward(x, m, rt, pmd, C.ALPHA, one)
    junk = x.clone()
    junk[0] = float("nan")
    junk[2] = (torch.randn(130, 77, generator=g) * 1e30).to(DEV)
    assert torch.equal(ext.token_focal_loss_backward(junk, m, rt, pmd, C.ALPHA, one)[1], grad[1])
    alone = ext.token_focal_loss_backward(x[1:2].contiguous(), m[1:2].contiguous(), rt[1:2].contiguous(), pmd, C.ALPHA, one)
    assert torch.equal(alone[0], grad[1]) and float(grad[1].abs().max()) > 0
    for geom, keep in (((3, 1, 7, 9, 4), 1), ((26, 1, 50, 84, 4), 11)):            # one slice an instance; several
        src, gt, gt_row, _, _ = C.mask_case(*geom)
        s, gtd, rows = src.to(DEV), gt.to(DEV), gt_row.to(DEV)
        two = torch.full((1,), 2.0, device=DEV)

        def grad_src(s_, rows_):
            _, sums = ext.mask_losses_forward(s_, gtd, rows_, geom[4], C.MASK_NUM_BOXES)
            return ext.mask_losses_backward(s_, gtd, rows_, geom[4], C.MASK_NUM_BOXES, sums, one, two)

        want = grad_src(s, rows)[keep]
        junk = (torch.randn(src.shape, generator=g) * 1e30).to(DEV)
        junk[0] = float("nan")
        junk[keep] = s[keep]
        assert torch.equal(grad_src(junk, rows)[keep], want)
        assert torch.equal(grad_src(s[keep:keep + 1].contiguous(), rows[keep:keep + 1].contiguous())[0], want)
        assert float(want.abs().max()) > 0
