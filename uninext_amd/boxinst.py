"""BoxInst training (`MODEL.BOXINST.ENABLED`): the box-supervised mask losses and the two target tensors they consume.

Mirror of the reference's `loss_masks_boxinst`, `unfold_wo_center`, `compute_project_term`, `compute_pairwise_term`
(projects/UNINEXT/uninext/models/deformable_detr/deformable_detr.py:457-527, :787-851), of the `cfg` block of `SetCriterion.__init__`
(:313-322) and of `prepare_image_targets_boxinst`, `add_bitmasks_from_boxes`, `get_images_color_similarity`
(uninext/uninext_img.py:529-659): the same names, argument orders and dictionary keys (`loss_prj`, `loss_pairwise`).
`BoxInstSetCriterion` / `BoxInstDINOCriterion` are the criterion classes with `"masks_boxinst"` accepted in `losses`; they change
nothing else.  `rgb2lab` restates skimage.color.rgb2lab (skimage is not a dependency): sRGB, D65, observer 2.

`FUSED` (module attribute, for `boxinst_targets(..., fused=)`) and the criterion classes' `fused_boxinst` (a class attribute of its
own: `fused` keeps steering loss_labelsVL and loss_masks), both ON by default since they were measured on an MI355X
(profiles/r26_boxinst.txt, tools/boxinst_bench.py): forward + backward of the loss at batch 2, 64 kept instances of 200 x 336 in
0.95 ms against 6.74 ms (p10-p90 0.92-1.33 against 6.72-7.14), 0 host synchronisations against 129, 86 MiB against 1268 MiB above the
inputs; the targets of two 800 x 1344 images in 0.32 ms against 9.09 ms, 0 host synchronisations against 261.  `boxinst.FUSED = False`,
`fused=False` or `criterion.fused_boxinst = False` turn them off.

  off  a composition of PyTorch operations restating the reference's arithmetic, held to the reference's fixtures
       (tests/golden/boxinst).  The CPU path, and the yardstick of the fused one.
  on   for contiguous fp32 GPU logits [n, 1, h, w] with bool masks and fp32 similarities on the same device and a 3 x 3 window, both
       losses run on the kernels of uninext_amd/csrc/boxinst.hip through `BoxInstLossesFunction`: one pass over the kept instances for
       the losses, one for the gradient.  The two [n, 1, 9, h, w] unfolded copies, the [n, 8, h, w] temporaries, the gathered targets
       and the `random.sample` subset of the logits are never formed, and `_iter` is never read on the host.  `boxinst_targets` builds
       the bitmasks and the colour similarity on the device, without the round trip through the host for Lab and without the four
       host synchronisations per box.  Anything the kernels do not take (autocast / half masks, more than one frame, another window
       size, rows too wide for the LDS tile) falls back silently to the composition.

What differs from the reference on the fused route: the maxima of the projection term are taken of the logits, not of their fp32
sigmoids; they differ only where two logits of a row or a column collide in sigmoid space (where that is at saturation the
gradient is 0 either way).

Randomness: with more than `boxinst_topk` matched pairs the reference draws `random.sample(range(len), topk)`; both routes make that
call with the same arguments, so after `random.seed(s)` they keep the same pairs and leave the generator in the same state.
"""
import random

import numpy as np
import torch
import torch.nn.functional as F

from . import ext
from .criterion import DINOCriterion, SetCriterion, _scalar, dice_coefficient

FUSED = True                # measured: profiles/r26_boxinst.txt (tools/boxinst_bench.py)
# uninext/config.py:41-50
BOTTOM_PIXELS_REMOVED, PAIRWISE_SIZE, PAIRWISE_DILATION, PAIRWISE_COLOR_THRESH, PAIRWISE_WARMUP_ITERS, TOPK = 10, 3, 2, 0.3, 10000, 64

_XYZ_FROM_RGB = ((0.412453, 0.357580, 0.180423), (0.212671, 0.715160, 0.072169), (0.019334, 0.119193, 0.950227))
_WHITE_D65 = (0.95047, 1.0, 1.08883)


# ---- the reference's functions ------------------------------------------------------------------------------------------------
def unfold_wo_center(x, kernel_size, dilation):
    """[N, C, k * k - 1, H, W]: for every pixel of x [N, C, H, W] its window's values without the centre, zeros outside the image."""
    assert x.dim() == 4
    assert kernel_size % 2 == 1
    padding = (kernel_size + (dilation - 1) * (kernel_size - 1)) // 2           # SAME
    windows = F.unfold(x, kernel_size=kernel_size, padding=padding, dilation=dilation)
    windows = windows.reshape(x.size(0), x.size(1), -1, x.size(2), x.size(3))
    centre = kernel_size ** 2 // 2
    return torch.cat((windows[:, :, :centre], windows[:, :, centre + 1:]), dim=2)


def compute_project_term(mask_scores, gt_bitmasks):
    """The mean over the instances of the dice coefficients of the column maxima and of the row maxima ([n, 1, h, w] both)."""
    mask_losses_y = dice_coefficient(mask_scores.max(dim=2, keepdim=True)[0], gt_bitmasks.max(dim=2, keepdim=True)[0])
    mask_losses_x = dice_coefficient(mask_scores.max(dim=3, keepdim=True)[0], gt_bitmasks.max(dim=3, keepdim=True)[0])
    return (mask_losses_x + mask_losses_y).mean()


def compute_pairwise_term(mask_logits, pairwise_size, pairwise_dilation):
    """[n, k * k - 1, h, w]: -log of the probability that a pixel and its neighbour get the same label, in log space."""
    assert mask_logits.dim() == 4
    log_fg_prob = F.logsigmoid(mask_logits)
    log_bg_prob = F.logsigmoid(-mask_logits)
    log_same_fg_prob = log_fg_prob[:, :, None] + unfold_wo_center(log_fg_prob, kernel_size=pairwise_size, dilation=pairwise_dilation)
    log_same_bg_prob = log_bg_prob[:, :, None] + unfold_wo_center(log_bg_prob, kernel_size=pairwise_size, dilation=pairwise_dilation)
    max_ = torch.max(log_same_fg_prob, log_same_bg_prob)
    log_same_prob = torch.log(torch.exp(log_same_fg_prob - max_) + torch.exp(log_same_bg_prob - max_)) + max_
    return -log_same_prob[:, 0]


def get_images_color_similarity(images, image_masks, kernel_size, dilation):
    """[1, k * k - 1, h, w]: exp(-||lab - lab'|| / 2) of every pixel of images [1, 3, h, w] with its neighbours, times the
    neighbour's value of image_masks [h, w]."""
    assert images.dim() == 4
    assert images.size(0) == 1
    diff = images[:, :, None] - unfold_wo_center(images, kernel_size=kernel_size, dilation=dilation)
    similarity = torch.exp(-torch.norm(diff, dim=1) * 0.5)
    weights = unfold_wo_center(image_masks[None, None], kernel_size=kernel_size, dilation=dilation)
    return similarity * torch.max(weights, dim=1)[0]


def rgb2lab(images_u8):
    """skimage.color.rgb2lab (illuminant D65, observer 2) of uint8 RGB [..., 3], restated: float64 [..., 3] = (L, a, b).  A tensor
    gives a tensor, anything else a numpy array."""
    is_tensor = torch.is_tensor(images_u8)
    rgb = (images_u8.cpu().numpy() if is_tensor else np.asarray(images_u8)).astype(np.float64) / 255
    linear = np.where(rgb > 0.04045, ((rgb + 0.055) / 1.055) ** 2.4, rgb / 12.92)
    xyz = linear @ np.asarray(_XYZ_FROM_RGB, dtype=np.float64).T
    xyz = xyz / np.asarray(_WHITE_D65, dtype=np.float64)
    f = np.where(xyz > 0.008856, np.cbrt(xyz), 7.787 * xyz + 16.0 / 116.0)
    lab = np.stack([116.0 * f[..., 1] - 16.0, 500.0 * (f[..., 0] - f[..., 1]), 200.0 * (f[..., 1] - f[..., 2])], axis=-1)
    return torch.from_numpy(lab).to(images_u8.device) if is_tensor else lab


# ---- the targets ----------------------------------------------------------------------------------------------------------------
def _pad_batch(tensors, size_divisibility, value=0):
    """ImageList.from_tensors: [..., H_i, W_i] at the top left of [bs, ..., H, W], the largest sizes rounded up."""
    H, W = (max(t.shape[k] for t in tensors) for k in (-2, -1))
    d = size_divisibility
    if d > 1:
        H, W = (H + d - 1) // d * d, (W + d - 1) // d * d
    out = tensors[0].new_full((len(tensors),) + tuple(tensors[0].shape[:-2]) + (H, W), value)
    for slot, t in zip(out, tensors):
        slot[..., :t.shape[-2], :t.shape[-1]].copy_(t)
    return out


def boxinst_targets(images, heights, boxes, mask_stride=4, bottom_pixels_removed=BOTTOM_PIXELS_REMOVED, pairwise_size=PAIRWISE_SIZE,
                    pairwise_dilation=PAIRWISE_DILATION, size_divisibility=32, fused=None):
    """What `prepare_image_targets_boxinst` adds to the targets: per image {"masks": bool [G_i, H, W], "image_color_similarity":
    fp32 [G_i, 8, H / mask_stride, W / mask_stride]}, to be merged into the criterion's target dictionaries.

    images: list of [3, H_i, W_i] BGR tensors as the data mapper yields them, uint8 or fp32 holding integers (non-integral values
    are not held to the reference where the pooled value is an exact `.byte()` tie); heights: the `batched_inputs[i]["height"]`
    values; boxes: list of [G_i, 4] xyxy in pixels of the (resized) image, coordinates >= 0 (a negative slice start would wrap
    in the reference).  The images are padded to `size_divisibility`; int(bottom_pixels_removed * H_i / height) bottom rows and the
    padding do not count as neighbours; a bitmask is [int(y1):int(y2 + 1), int(x1):int(x2 + 1)].  The similarity is ONE [8, h, w]
    tensor per image handed out as an expanded view (the reference concatenates G_i copies).  fused: None (the module's FUSED),
    True or False."""
    assert len(images) == len(heights) == len(boxes)
    fused = FUSED if fused is None else fused
    stride = mask_stride
    start = int(stride // 2)
    batch = _pad_batch(images, size_divisibility)
    image_masks = []
    for image, im_h in zip(images, heights):
        keep = torch.ones(image.shape[-2:], dtype=torch.bool, device=image.device)
        pixels_removed = int(bottom_pixels_removed * float(image.size(1)) / float(im_h))
        if pixels_removed > 0:
            keep[-pixels_removed:, :] = False
        image_masks.append(keep)
    image_masks = _pad_batch(image_masks, size_divisibility, False)
    H, W = batch.shape[-2:]
    assert H % stride == 0 and W % stride == 0
    on_device = (fused and batch.is_cuda and batch.dtype in (torch.uint8, torch.float32) and pairwise_size == 3
                 and 1 <= pairwise_dilation <= 8
                 and all(b.is_cuda and b.device == batch.device and b.dtype == torch.float32 and b.dim() == 2 and b.shape[1] == 4
                         for b in boxes))
    out = []
    if on_device:
        similarity = ext.color_similarity(batch, image_masks, stride, pairwise_dilation)
        for b, per_im_boxes in enumerate(boxes):
            out.append({"masks": ext.box_bitmasks(per_im_boxes.contiguous(), H, W),
                        "image_color_similarity": similarity[b].expand(len(per_im_boxes), -1, -1, -1)})
        return out
    downsampled = F.avg_pool2d(batch.float(), kernel_size=stride, stride=stride, padding=0)[:, [2, 1, 0]]
    sampled_masks = image_masks[:, start::stride, start::stride].float()
    for b, per_im_boxes in enumerate(boxes):
        lab = rgb2lab(downsampled[b].byte().permute(1, 2, 0).cpu().numpy())
        lab = torch.as_tensor(lab, device=downsampled.device, dtype=torch.float32).permute(2, 0, 1)[None]
        similarity = get_images_color_similarity(lab, sampled_masks[b], pairwise_size, pairwise_dilation)
        masks = torch.zeros((len(per_im_boxes), H, W), dtype=torch.bool, device=batch.device)
        for slot, per_box in zip(masks, per_im_boxes):
            slot[int(per_box[1]):int(per_box[3] + 1), int(per_box[0]):int(per_box[2] + 1)] = True
        out.append({"masks": masks, "image_color_similarity": similarity.expand(len(per_im_boxes), -1, -1, -1)})
    return out


# ---- the fused losses under autograd ------------------------------------------------------------------------------------------
class BoxInstLossesFunction(torch.autograd.Function):
    """(loss_prj, loss_pairwise) of src [N, 1, h, w] fp32 logits: instance i reads row inst[i] of src, its box mask at the strided
    pixels of row gt_row[i] of gt (bool [..., H_im, W_im]) and the similarities sim[img[i]] ([B, 8, h, w]); warmup a [1] fp32 tensor
    on the device.  Gradient to src only."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, src, inst, gt, gt_row, stride, sim, img, thresh, dilation, warmup):
        src = src.contiguous()
        losses, saved = ext.boxinst_losses_forward(src, inst, gt, gt_row, stride, sim, img, thresh, dilation, warmup)
        ctx.save_for_backward(src, inst, gt, gt_row, sim, img, warmup, *saved)
        ctx.stride, ctx.thresh, ctx.dilation = int(stride), float(thresh), int(dilation)
        return losses[0], losses[1]

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_prj, grad_pairwise):
        src, inst, gt, gt_row, sim, img, warmup = ctx.saved_tensors[:7]
        grad = ext.boxinst_losses_backward(src, inst, gt, gt_row, ctx.stride, sim, img, ctx.thresh, ctx.dilation, warmup,
                                           ctx.saved_tensors[7:], _scalar(grad_prj, src), _scalar(grad_pairwise, src))
        return (grad,) + (None,) * 9


# ---- the criterion --------------------------------------------------------------------------------------------------------------
class _BoxInstLosses:
    """`"masks_boxinst"` accepted in `losses` and dispatched to loss_masks_boxinst; nothing else of the criterion changes (its
    `_forward` already skips `masks_boxinst` for the encoder outputs).  `cfg`: any object with the reference's `MODEL.BOXINST.*`
    attributes; None gives the defaults of uninext/config.py:41-50."""
    fused_boxinst = True        # measured: profiles/r26_boxinst.txt (tools/boxinst_bench.py)

    def __init__(self, matcher, weight_dict, losses, focal_alpha=0.25, mask_out_stride=4, ota=False, still_cls_for_encoder=False, cfg=None):
        super().__init__(matcher, weight_dict, [loss for loss in losses if loss != "masks_boxinst"], focal_alpha=focal_alpha,
                         mask_out_stride=mask_out_stride, ota=ota, still_cls_for_encoder=still_cls_for_encoder, cfg=cfg)
        self.losses = losses
        if cfg is not None:
            self.boxinst_enabled = cfg.MODEL.BOXINST.ENABLED
            self.bottom_pixels_removed = cfg.MODEL.BOXINST.BOTTOM_PIXELS_REMOVED
            self.pairwise_size = cfg.MODEL.BOXINST.PAIRWISE.SIZE
            self.pairwise_dilation = cfg.MODEL.BOXINST.PAIRWISE.DILATION
            self.pairwise_color_thresh = cfg.MODEL.BOXINST.PAIRWISE.COLOR_THRESH
            self._warmup_iters = cfg.MODEL.BOXINST.PAIRWISE.WARMUP_ITERS
            self.boxinst_topk = cfg.MODEL.BOXINST.TOPK
        else:
            self.boxinst_enabled = True
            self.bottom_pixels_removed, self.pairwise_size, self.pairwise_dilation = BOTTOM_PIXELS_REMOVED, PAIRWISE_SIZE, PAIRWISE_DILATION
            self.pairwise_color_thresh, self._warmup_iters, self.boxinst_topk = PAIRWISE_COLOR_THRESH, PAIRWISE_WARMUP_ITERS, TOPK
        self.register_buffer("_iter", torch.zeros([1]))

    def loss_masks_boxinst(self, outputs, targets, indices, num_boxes):
        """The projection and the pairwise loss of the instance masks against the box masks and the colour similarities of the
        targets ("masks", "image_color_similarity": boxinst_targets).  `num_boxes` is unused, as in the reference."""
        self._iter += 1
        assert "pred_masks" in outputs
        src_masks = outputs["pred_masks"]
        bs = len(targets)
        if type(src_masks) == list:                                  # bs x [1, num_inst, frames, h, w]
            src_masks = torch.cat(src_masks, dim=1)[0]
        if src_masks.ndim == 0:                                      # box labels only
            return {'loss_prj': src_masks * 0.0, 'loss_pairwise': src_masks * 0.0}
        src_idx = self._get_src_permutation_idx(indices)
        tgt_idx = self._get_tgt_permutation_idx(indices)
        keep_indexs = None
        if len(tgt_idx[0]) > self.boxinst_topk:                      # a part of the pairs: BoxInst takes more memory
            keep_indexs = random.sample(range(len(tgt_idx[0])), self.boxinst_topk)
            src_idx = tuple([src_idx[0][keep_indexs], src_idx[1][keep_indexs]])
            tgt_idx = tuple([tgt_idx[0][keep_indexs], tgt_idx[1][keep_indexs]])
        if self.fused_boxinst:
            losses = self._fused_boxinst(src_masks, targets, tgt_idx, keep_indexs)
            if losses is not None:
                return losses
        if keep_indexs is not None:
            src_masks = src_masks[keep_indexs]
        target_masks = self.get_target_masks(targets, src_masks)
        num_frames = src_masks.shape[1]
        target_masks = target_masks.reshape(bs, -1, num_frames, target_masks.shape[-2], target_masks.shape[-1])[tgt_idx]
        if len(target_masks) == 0:
            return {'loss_prj': src_masks.sum() * 0.0, 'loss_pairwise': src_masks.sum() * 0.0}
        mask_scores = src_masks.sigmoid()
        image_color_similarity = torch.stack([targets[batch_idx]["image_color_similarity"][target_idx]
                                              for batch_idx, target_idx in zip(tgt_idx[0], tgt_idx[1])], dim=0).to(dtype=mask_scores.dtype)
        loss_prj_term = compute_project_term(mask_scores, target_masks)
        pairwise_losses = compute_pairwise_term(src_masks, self.pairwise_size, self.pairwise_dilation)
        weights = (image_color_similarity >= self.pairwise_color_thresh).float() * target_masks.float()
        loss_pairwise = (pairwise_losses * weights).sum() / weights.sum().clamp(min=1.0)
        warmup_factor = min(self._iter.item() / float(self._warmup_iters), 1.0)
        return {"loss_prj": loss_prj_term, "loss_pairwise": loss_pairwise * warmup_factor}

    def _fused_boxinst(self, src_masks, targets, tgt_idx, keep_indexs):
        """{loss_prj, loss_pairwise} on the kernels, or None where they do not take the arguments."""
        if torch.is_autocast_enabled():
            src_masks = src_masks.float()
        masks = [t["masks"] for t in targets]
        sims = [t["image_color_similarity"] for t in targets]
        if not (src_masks.dim() == 4 and src_masks.shape[1] == 1 and src_masks.is_cuda and src_masks.dtype == torch.float32
                and src_masks.is_contiguous() and self.pairwise_size == 3
                and all(m.dtype == torch.bool and m.dim() == 3 and m.device == src_masks.device for m in masks)
                and all(s.dtype == torch.float32 and s.dim() == 4 and s.device == src_masks.device
                        and tuple(s.shape[1:]) == (8,) + tuple(src_masks.shape[2:]) for s in sims)):
            return None
        h, w = src_masks.shape[2:]
        if len(tgt_idx[0]) == 0:
            return {'loss_prj': src_masks.sum() * 0.0, 'loss_pairwise': src_masks.sum() * 0.0}
        gt = self._padded_masks(targets)
        stride = self.mask_out_stride
        if stride != 1:
            assert h * stride == gt.shape[-2] and w * stride == gt.shape[-1]
        # ONE [8, h, w] similarity an image (every target of an image holds the same one); an image without targets has no weight
        sim = self._once(("boxinst_sim",) + tuple(id(s) for s in sims), lambda: torch.stack(
            [s[0] if len(s) else s.new_zeros(s.shape[1:]) for s in sims]).contiguous())
        if not ext.boxinst_losses_supported(src_masks, gt, sim, self.pairwise_dilation) or gt.shape[-2:] != (h * stride, w * stride):
            return None
        dev = src_masks.device
        n = len(tgt_idx[0])
        if keep_indexs is None:
            if n != src_masks.shape[0]:
                return None
            inst = torch.arange(n, dtype=torch.int32, device=dev)
        else:
            inst = torch.tensor(keep_indexs, dtype=torch.int32).to(dev, non_blocking=True)
        img = tgt_idx[0].to(dev)
        gt_row = (img * gt.shape[1] + tgt_idx[1].to(dev)).to(torch.int32)
        warmup = (self._iter.to(device=dev, dtype=torch.float32) / float(self._warmup_iters)).clamp(max=1.0)
        loss_prj, loss_pairwise = BoxInstLossesFunction.apply(src_masks, inst, gt, gt_row, stride, sim, img.to(torch.int32),
                                                              float(self.pairwise_color_thresh), int(self.pairwise_dilation), warmup)
        return {"loss_prj": loss_prj, "loss_pairwise": loss_pairwise}


class BoxInstSetCriterion(_BoxInstLosses, SetCriterion):
    """SetCriterion for the BoxInst configs: `losses` may hold "masks_boxinst"."""


class BoxInstDINOCriterion(_BoxInstLosses, DINOCriterion):
    """DINOCriterion for the BoxInst configs: `losses` may hold "masks_boxinst"."""
