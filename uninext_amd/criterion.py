"""The training criterion: what consumes the matcher's indices and produces the scalars that backward() starts from.

Mirror of the reference's `SetCriterion` / `DINOCriterion` (projects/UNINEXT/uninext/models/deformable_detr/deformable_detr.py:
290-784) and of the loss functions they call (segmentation.py:74-166, deformable_detr.py:853-879): the same names, argument
orders and dictionary keys (`loss_ce`, `loss_bbox`, `loss_giou`, `loss_boxiou`, `loss_mask`, `loss_dice`, `cardinality_error`,
with the `_{i}`, `_enc`, `_dn`, `_dn_{i}` suffixes), the same `num_boxes` handling, OTA renormalisation, zero-loss early exits and
all_reduce.  `giou_loss` restates fvcore.nn.giou_loss (fvcore is not a dependency), with its eps = 1e-7 in both denominators.
Supported losses: labelsVL, boxes, masks, cardinality; `reid` and `masks_boxinst` raise NotImplementedError here
(`masks_boxinst`: the BoxInst* criterion classes of uninext_amd/boxinst.py; `reid`: the Video* classes of uninext_amd/reid.py).

`SetCriterion.fused` (a class attribute, ON by default since it was measured: 14.7 ms against 61.8 ms for forward + backward at the
training shape on an MI355X, profiles/r18_criterion.txt; `SetCriterion.fused = False` or `criterion.fused = False` turns it off):

  off  every loss is the reference's composition of PyTorch operations.  The CPU path, and the yardstick of the fused one.
  on   for contiguous fp32 GPU tensors, T <= 256 tokens and gamma == 2, `loss_labelsVL` and `loss_masks` run on the kernels of
       uninext_amd/csrc/criterion.hip through `TokenFocalLossFunction` and `MaskLossesFunction`: one pass over the logits for
       the loss and one for the gradient.  The [bs, Q, T] one-hot tensor, the repeated text mask, the two masked_select copies,
       the fp32 copy of the padded full-resolution masks and the gathered target masks are never formed; the matched rows are
       scattered without the Python pair loop (one host-to-device copy per call, none when the indices are on the device;
       where a query appears twice the last pair wins, as in the reference's loop, resolved before the scatter).  Anything the
       kernels do not take falls back silently to the composition.  The box losses stay a composition: a few hundred numbers.

What differs from the reference otherwise: no hard-coded `.cuda()` (compute_dn_loss uses the outputs' device), and the encoder's
binary targets are shallow copies of the target dictionaries with the two replaced entries instead of a deep copy of every mask.
"""
import torch
import torch.nn.functional as F
from torch import nn

from . import ext
from .matcher import box_area, box_cxcywh_to_xyxy

SUPPORTED_LOSSES = ("labelsVL", "cardinality", "boxes", "masks")
MASK_SIZE_DIVISIBILITY = 32     # deformable_detr.py:658


# ---- distributed helpers (util/misc.py) ---------------------------------------------------------------------------------------
def is_dist_avail_and_initialized():
    return torch.distributed.is_available() and torch.distributed.is_initialized()


def get_world_size():
    return torch.distributed.get_world_size() if is_dist_avail_and_initialized() else 1


# ---- loss functions -----------------------------------------------------------------------------------------------------------
def dice_loss(inputs, targets, num_boxes):
    """DICE loss of logits [N, ...] against 0 / 1 targets [N, P] (segmentation.py:74-89): +1 smoothing on both sides."""
    prob = inputs.sigmoid().flatten(1)
    numerator = 2 * (prob * targets).sum(1)
    denominator = prob.sum(-1) + targets.sum(-1)
    return (1 - (numerator + 1) / (denominator + 1)).sum() / num_boxes


def _focal_terms(logits, targets, alpha, gamma):
    prob = logits.sigmoid()
    ce = F.binary_cross_entropy_with_logits(logits, targets, reduction="none")
    p_t = prob * targets + (1 - prob) * (1 - targets)
    loss = ce * ((1 - p_t) ** gamma)
    if alpha >= 0:
        loss = (alpha * targets + (1 - alpha) * (1 - targets)) * loss
    return loss


def sigmoid_focal_loss(inputs, targets, num_boxes, alpha: float = 0.25, gamma: float = 2):
    """RetinaNet's focal loss of logits [N, P] (segmentation.py:92-117): the mean over P, summed over N, over num_boxes."""
    return _focal_terms(inputs, targets, alpha, gamma).mean(1).sum() / num_boxes


def token_sigmoid_binary_focal_loss(pred_logits, targets, alpha=0.25, gamma=2.0, text_mask=None, reduction=True):
    """Focal loss of token logits [bs, n, T] against targets of the same shape, over the tokens whose text_mask [bs, T] is > 0
    (segmentation.py:120-166)."""
    assert targets.dim() == 3 and pred_logits.dim() == 3
    if text_mask is not None:
        assert text_mask.dim() == 2
        keep = (text_mask > 0).unsqueeze(1).repeat(1, pred_logits.size(1), 1)
        pred_logits = torch.masked_select(pred_logits, keep)
        targets = torch.masked_select(targets, keep)
    loss = _focal_terms(pred_logits, targets, alpha, gamma)
    return loss.sum() if reduction else loss


def dice_coefficient(x, target):
    """1 - 2 <x, t> / (|x|^2 + |t|^2 + 1e-5) per instance (deformable_detr.py:871-879)."""
    eps = 1e-5
    n_inst = x.size(0)
    x = x.reshape(n_inst, -1)
    target = target.reshape(n_inst, -1)
    intersection = (x * target).sum(dim=1)
    union = (x ** 2.0).sum(dim=1) + (target ** 2.0).sum(dim=1) + eps
    return 1. - (2 * intersection / union)


def compute_box_iou(inputs, targets):
    """IoU of box k of `inputs` with box k of `targets`, both [N, 4] xyxy (deformable_detr.py:853-869)."""
    area1, area2 = box_area(inputs), box_area(targets)
    lt = torch.max(inputs[:, None, :2], targets[:, :2])
    rb = torch.min(inputs[:, None, 2:], targets[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return torch.diag(inter / (area1[:, None] + area2 - inter))


def giou_loss(boxes1, boxes2, reduction="none", eps=1e-7):
    """fvcore.nn.giou_loss: 1 - GIoU of box k of boxes1 with box k of boxes2 ([N, 4] xyxy).  eps is added to the union under
    the intersection and to the hull's area under the excess, nowhere else; an intersection counts only where it has a positive
    width AND height."""
    x1, y1, x2, y2 = boxes1.unbind(dim=-1)
    x1g, y1g, x2g, y2g = boxes2.unbind(dim=-1)
    assert (x2 >= x1).all(), "bad box: x1 larger than x2"
    assert (y2 >= y1).all(), "bad box: y1 larger than y2"
    xk1, yk1 = torch.max(x1, x1g), torch.max(y1, y1g)
    xk2, yk2 = torch.min(x2, x2g), torch.min(y2, y2g)
    inter = torch.where((yk2 > yk1) & (xk2 > xk1), (xk2 - xk1) * (yk2 - yk1), torch.zeros_like(x1))
    union = (x2 - x1) * (y2 - y1) + (x2g - x1g) * (y2g - y1g) - inter
    iou = inter / (union + eps)
    hull = (torch.max(x2, x2g) - torch.min(x1, x1g)) * (torch.max(y2, y2g) - torch.min(y1, y1g))
    loss = 1 - (iou - (hull - union) / (hull + eps))
    if reduction == "mean":
        return loss.mean() if loss.numel() > 0 else 0.0 * loss.sum()
    if reduction == "sum":
        return loss.sum()
    return loss


def pad_masks(masks, size_divisibility=MASK_SIZE_DIVISIBILITY):
    """[bs, G_max, H_im, W_im]: every image's [G_i, H_i, W_i] masks at the top left of a zero tensor whose height and width are
    the batch's largest rounded up to `size_divisibility` (util/misc.py:288-316 with split = False; the tensor only)."""
    assert masks[0].dim() == 3
    G, H, W = (max(m.shape[k] for m in masks) for k in range(3))
    d = size_divisibility
    if d > 1:
        H, W = (H + d - 1) // d * d, (W + d - 1) // d * d
    out = torch.zeros((len(masks), G, H, W), dtype=masks[0].dtype, device=masks[0].device)
    for slot, m in zip(out, masks):
        slot[:m.shape[0], :m.shape[1], :m.shape[2]].copy_(m)
    return out


# ---- the fused losses under autograd ------------------------------------------------------------------------------------------
def _scalar(grad, like):
    """An upstream gradient (or None) as a [1] fp32 tensor on the device."""
    if grad is None:
        return torch.zeros((1,), dtype=torch.float32, device=like.device)
    return grad.detach().to(torch.float32).reshape(1)


class TokenFocalLossFunction(torch.autograd.Function):
    """loss = (sum of the token focal loss over the counted tokens) / num_boxes, gamma 2.  logits [bs, Q, T] fp32; text_mask
    [bs, T] or None; row_target [bs, Q] int32 (a row of positive_map_all [G, T] fp32, or -1).  Gradient to the logits only."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, logits, text_mask, row_target, positive_map_all, alpha, num_boxes):
        logits = logits.contiguous()
        ctx.save_for_backward(logits, text_mask, row_target, positive_map_all)
        ctx.alpha, ctx.num_boxes = float(alpha), float(num_boxes)
        return ext.token_focal_loss_forward(logits, text_mask, row_target, positive_map_all, alpha)[0] / num_boxes

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad):
        logits, text_mask, row_target, positive_map_all = ctx.saved_tensors
        scale = _scalar(grad, logits) / ctx.num_boxes
        return ext.token_focal_loss_backward(logits, text_mask, row_target, positive_map_all, ctx.alpha, scale), None, None, None, None, None


class MaskLossesFunction(torch.autograd.Function):
    """(loss_mask, loss_dice) of src [n, F, h, w] fp32 logits against the strided pixels of the padded ground truth gt (bool
    [bs, G_max, H_im, W_im]); gt_row [n] int32, the first of an instance's F rows of gt.  Gradient to src only."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, src, gt, gt_row, stride, num_boxes):
        src = src.contiguous()
        losses, sums = ext.mask_losses_forward(src, gt, gt_row, stride, num_boxes)
        ctx.save_for_backward(src, gt, gt_row, sums)
        ctx.stride, ctx.num_boxes = int(stride), float(num_boxes)
        return losses[0], losses[1]

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_mask, grad_dice):
        src, gt, gt_row, sums = ctx.saved_tensors
        grad = ext.mask_losses_backward(src, gt, gt_row, ctx.stride, ctx.num_boxes, sums, _scalar(grad_mask, src),
                                        _scalar(grad_dice, src))
        return grad, None, None, None, None


def matched_rows(indices, row_offsets, num_queries, device):
    """[bs, Q] int32: for every query the row of the concatenated positive maps it is matched to, or -1.  `indices` is the
    matcher's [(src, tgt)] per image, row_offsets[b] the first row of image b.  A query listed twice keeps its LAST pair, as in a
    loop that assigns pair after pair; the last position per query is found with a maximum, so the scatter never sees a
    duplicate.  The work is done where the indices live: one copy to `device` for host indices, none for device ones."""
    bs = len(indices)
    where = indices[0][0].device if bs else device
    keys = [src.to(torch.int64).remainder(num_queries) + b * num_queries for b, (src, _) in enumerate(indices)]
    rows = [tgt.to(torch.int64) + row_offsets[b] for b, (_, tgt) in enumerate(indices)]
    keys = torch.cat(keys) if bs else torch.zeros(0, dtype=torch.int64)
    rows = torch.cat(rows + [torch.full((1,), -1, dtype=torch.int64, device=where)])        # position -1: unmatched
    last = torch.full((bs * num_queries,), -1, dtype=torch.int64, device=where)
    last.scatter_reduce_(0, keys, torch.arange(keys.numel(), device=where), "amax", include_self=True)
    return rows[last].to(torch.int32).view(bs, num_queries).to(device)


# ---- the criterion ------------------------------------------------------------------------------------------------------------
class SetCriterion(nn.Module):
    """The losses of one set of matched predictions, of every auxiliary decoder layer and of the encoder's proposals.

    forward(outputs, targets, indices_list): outputs {"pred_logits" [bs, Q, T], "pred_boxes" [bs, Q, 4], "text_masks" [bs, T],
    optionally "pred_boxious", "pred_masks", "aux_outputs", "enc_outputs"}; targets: per image {"labels", "boxes" [G, 4] cxcywh,
    "positive_map" [G, T], "masks" [G * frames, H, W] bool}; indices_list: the matcher's indices per decoder layer, the last
    layer's last."""
    fused = True

    def __init__(self, matcher, weight_dict, losses, focal_alpha=0.25, mask_out_stride=4, ota=False, still_cls_for_encoder=False, cfg=None):
        super().__init__()
        for loss in losses:
            if loss in ("reid", "masks_boxinst"):
                raise NotImplementedError("SetCriterion: the '%s' loss is not implemented" % loss)
        self.matcher = matcher
        self.weight_dict = weight_dict
        self.losses = losses
        self.focal_alpha = focal_alpha
        self.mask_out_stride = mask_out_stride
        self.ota = ota
        self.still_cls_for_encoder = still_cls_for_encoder
        self._shared = None          # during forward(): the concatenated positive maps and the padded masks of the target lists

    def _once(self, key, make):
        """make(), computed once per forward() for the tensors `key` names by identity (they live as long as the call)."""
        if self._shared is None:
            return make()
        if key not in self._shared:
            self._shared[key] = make()
        return self._shared[key]

    # -- classification ----------------------------------------------------------------------------------
    def loss_labelsVL(self, outputs, targets, indices, num_boxes, log=False):
        """Token-level focal loss of the logits against the positive map of each query's matched target."""
        assert 'pred_logits' in outputs
        assert 'text_masks' in outputs
        src_logits = outputs['pred_logits']
        idx = self._get_src_permutation_idx(indices)
        num_boxes = len(idx[0]) if self.ota else num_boxes
        if num_boxes == 0:
            return {'loss_ce': src_logits.sum() * 0.0}
        text_mask = outputs['text_masks']
        loss_ce = self._fused_labels(src_logits, text_mask, targets, indices, num_boxes) if self.fused else None
        if loss_ce is None:
            onehot = torch.zeros(src_logits.size(), dtype=src_logits.dtype, layout=src_logits.layout, device=src_logits.device)
            positive_map = [t["positive_map"] for t in targets]
            for b, (src_idxs, target_idxs) in enumerate(indices):
                for src_idx, target_idx in zip(src_idxs, target_idxs):
                    onehot[b, src_idx] = positive_map[b][target_idx]
            loss_ce = token_sigmoid_binary_focal_loss(src_logits, onehot, alpha=self.focal_alpha, text_mask=text_mask) / num_boxes
        if log:
            raise ValueError("log is not supported.")
        return {'loss_ce': loss_ce}

    def _fused_labels(self, src_logits, text_mask, targets, indices, num_boxes):
        """loss_ce on the kernels, or None where they do not take the arguments."""
        if torch.is_autocast_enabled():
            src_logits = src_logits.float()
        if not ext.token_focal_loss_supported(src_logits, None) or self.focal_alpha < 0:
            return None
        if text_mask is not None and not (text_mask.dim() == 2 and text_mask.device == src_logits.device and text_mask.is_contiguous()
                                          and text_mask.dtype in (torch.int64, torch.bool, torch.uint8)):
            return None
        bs, Q, T = src_logits.shape
        maps = [t["positive_map"] for t in targets]
        if len(indices) != bs or len(maps) != bs or any(m.dim() != 2 or m.shape[1] not in (1, T) for m in maps):
            return None
        positive_map_all = self._once(("positive_map", T) + tuple(id(m) for m in maps), lambda: torch.cat(
            [m.to(device=src_logits.device, dtype=torch.float32).expand(-1, T) for m in maps]).contiguous())
        offsets, total = [], 0
        for m in maps:
            offsets.append(total)
            total += m.shape[0]
        row_target = matched_rows(indices, offsets, Q, src_logits.device)
        return TokenFocalLossFunction.apply(src_logits, text_mask, row_target, positive_map_all, self.focal_alpha, num_boxes)

    @torch.no_grad()
    def loss_cardinality(self, outputs, targets, indices, num_boxes):
        """Absolute error of the number of predictions that are not "no object": logged, not trained on."""
        pred_logits = outputs['pred_logits']
        tgt_lengths = torch.as_tensor([len(v["labels"]) for v in targets], device=pred_logits.device)
        card_pred = (pred_logits.argmax(-1) != pred_logits.shape[-1] - 1).sum(1)
        return {'cardinality_error': F.l1_loss(card_pred.float(), tgt_lengths.float())}

    # -- boxes ---------------------------------------------------------------------------------------------
    def loss_boxes(self, outputs, targets, indices, num_boxes):
        """L1 and GIoU loss of the matched boxes (cxcywh in [0, 1]); BCE of the predicted IoU where the model has that head."""
        assert 'pred_boxes' in outputs
        idx = self._get_src_permutation_idx(indices)
        src_boxes = outputs['pred_boxes'][idx]
        target_boxes = torch.cat([t['boxes'][i] for t, (_, i) in zip(targets, indices)], dim=0)
        if len(target_boxes) == 0:
            return {'loss_bbox': src_boxes.sum() * 0.0, 'loss_giou': src_boxes.sum() * 0.0}
        src_xyxy, target_xyxy = box_cxcywh_to_xyxy(src_boxes), box_cxcywh_to_xyxy(target_boxes)
        if 'pred_boxious' in outputs:
            with torch.no_grad():
                ious = compute_box_iou(src_xyxy, target_xyxy)
            loss_boxiou = F.binary_cross_entropy_with_logits(outputs['pred_boxious'][idx].flatten(0), ious.flatten(0), reduction='mean')
        num_boxes = src_boxes.shape[0] if self.ota else num_boxes
        losses = {'loss_bbox': F.l1_loss(src_boxes, target_boxes, reduction='none').sum() / num_boxes,
                  'loss_giou': giou_loss(src_xyxy, target_xyxy).sum() / num_boxes}
        if 'pred_boxious' in outputs:
            losses['loss_boxiou'] = loss_boxiou
        return losses

    # -- masks ---------------------------------------------------------------------------------------------
    def loss_masks(self, outputs, targets, indices, num_boxes):
        """Focal and dice loss of the instance masks against the ground truth at every mask_out_stride-th pixel."""
        assert "pred_masks" in outputs
        src_masks = outputs["pred_masks"]
        bs = len(targets)
        if type(src_masks) == list:                                  # bs x [1, num_inst, frames, h, w]
            src_masks = torch.cat(src_masks, dim=1)[0]
        if src_masks.ndim == 0:                                      # box labels only
            return {'loss_mask': src_masks * 0.0, 'loss_dice': src_masks * 0.0}
        tgt_idx = self._get_tgt_permutation_idx(indices)
        num_frames = src_masks.shape[1]
        num_boxes = src_masks.shape[0] if self.ota else num_boxes
        if self.fused:
            losses = self._fused_masks(src_masks, targets, tgt_idx, num_boxes)
            if losses is not None:
                return losses
        target_masks = self.get_target_masks(targets, src_masks)
        target_masks = target_masks.reshape(bs, -1, num_frames, target_masks.shape[-2], target_masks.shape[-1])[tgt_idx]
        if len(target_masks) == 0:
            return {'loss_mask': src_masks.sum() * 0.0, 'loss_dice': src_masks.sum() * 0.0}
        src_masks, target_masks = src_masks.flatten(1), target_masks.flatten(1)
        return {"loss_mask": sigmoid_focal_loss(src_masks, target_masks, num_boxes),
                "loss_dice": dice_loss(src_masks, target_masks, num_boxes)}

    def _padded_masks(self, targets):
        masks = [t["masks"] for t in targets]
        return self._once(("masks",) + tuple(id(m) for m in masks), lambda: pad_masks(masks))

    def _fused_masks(self, src_masks, targets, tgt_idx, num_boxes):
        """{loss_mask, loss_dice} on the kernels, or None where they do not take the arguments."""
        if torch.is_autocast_enabled():
            src_masks = src_masks.float()
        masks = [t["masks"] for t in targets]
        if not (src_masks.dim() == 4 and src_masks.is_cuda and src_masks.dtype == torch.float32 and src_masks.is_contiguous()
                and all(m.dtype == torch.bool and m.dim() == 3 and m.device == src_masks.device for m in masks)):
            return None
        n, num_frames, h, w = src_masks.shape
        if len(tgt_idx[0]) == 0:
            return {'loss_mask': src_masks.sum() * 0.0, 'loss_dice': src_masks.sum() * 0.0}
        gt = self._padded_masks(targets)
        stride = self.mask_out_stride
        if stride != 1:
            assert h * stride == gt.shape[-2] and w * stride == gt.shape[-1]
        if not ext.mask_losses_supported(src_masks, gt) or len(tgt_idx[0]) != n or gt.shape[1] % num_frames \
                or gt.shape[-2:] != (h * stride, w * stride) or not num_boxes > 0:
            return None
        dev = src_masks.device
        gt_row = (tgt_idx[0].to(dev) * gt.shape[1] + tgt_idx[1].to(dev) * num_frames).to(torch.int32)
        loss_mask, loss_dice = MaskLossesFunction.apply(src_masks, gt, gt_row, stride, num_boxes)
        return {"loss_mask": loss_mask, "loss_dice": loss_dice}

    def loss_masks_boxinst(self, outputs, targets, indices, num_boxes):
        raise NotImplementedError("SetCriterion: the 'masks_boxinst' loss is not implemented")

    def loss_reid(self, outputs, targets, indices, num_boxes):
        raise NotImplementedError("SetCriterion: the 'reid' loss is not implemented")

    # -- plumbing ------------------------------------------------------------------------------------------
    def _get_src_permutation_idx(self, indices):
        batch_idx = torch.cat([torch.full_like(src, i) for i, (src, _) in enumerate(indices)])
        src_idx = torch.cat([src for (src, _) in indices])
        return batch_idx, src_idx

    def _get_tgt_permutation_idx(self, indices):
        batch_idx = torch.cat([torch.full_like(tgt, i) for i, (_, tgt) in enumerate(indices)])
        tgt_idx = torch.cat([tgt for (_, tgt) in indices])
        return batch_idx, tgt_idx

    def get_loss(self, loss, outputs, targets, indices, num_boxes, **kwargs):
        loss_map = {
            'labelsVL': self.loss_labelsVL,
            'cardinality': self.loss_cardinality,
            'boxes': self.loss_boxes,
            'masks': self.loss_masks,
            'reid': self.loss_reid,
            'masks_boxinst': self.loss_masks_boxinst,
        }
        assert loss in loss_map, f'do you really want to compute {loss} loss?'
        return loss_map[loss](outputs, targets, indices, num_boxes, **kwargs)

    def _num_boxes(self, outputs, targets):
        """Targets of the batch, averaged over the ranks, at least 1: a Python float."""
        num_boxes = sum(len(t["labels"]) for t in targets)
        num_boxes = torch.as_tensor([num_boxes], dtype=torch.float, device=next(iter(outputs.values())).device)
        if is_dist_avail_and_initialized():
            torch.distributed.all_reduce(num_boxes)
        return torch.clamp(num_boxes / get_world_size(), min=1).item()

    def forward(self, outputs, targets, indices_list):
        """{name: scalar} of the last layer (indices_list[-1]), of auxiliary layer i under `name_{i}` and of the encoder's
        proposals, matched here by `matcher.forward` against class-agnostic targets, under `name_enc`."""
        self._shared = {}
        try:
            return self._forward(outputs, targets, indices_list)
        finally:
            self._shared = None          # also after an exception: the keys are ids, meaningless once the call is over

    def _forward(self, outputs, targets, indices_list):
        num_boxes = self._num_boxes(outputs, targets)
        losses = {}
        for loss in self.losses:
            losses.update(self.get_loss(loss, outputs, targets, indices_list[-1], num_boxes))

        if 'aux_outputs' in outputs:
            for i, aux_outputs in enumerate(outputs['aux_outputs']):
                for loss in self.losses:
                    if loss == 'reid':
                        continue
                    l_dict = self.get_loss(loss, aux_outputs, targets, indices_list[i], num_boxes)
                    losses.update({k + f'_{i}': v for k, v in l_dict.items()})

        if 'enc_outputs' in outputs:
            enc_outputs = outputs['enc_outputs']
            bin_targets = []
            for t in targets:
                bt = dict(t)
                bt['labels'] = torch.zeros_like(t['labels'])         # one class: object
                if self.still_cls_for_encoder and "positive_map" in bt:
                    bt["positive_map"] = torch.ones((len(t["positive_map"]), 1), dtype=torch.bool, device=t["positive_map"].device)
                    enc_outputs['text_masks'] = None
                bin_targets.append(bt)
            indices = self.matcher.forward(enc_outputs, bin_targets)      # never OTA for the first stage
            for loss in self.losses:
                if loss in ['masks', 'reid', "masks_boxinst"]:
                    continue
                l_dict = self.get_loss(loss, enc_outputs, bin_targets, indices, num_boxes)
                losses.update({k + f'_enc': v for k, v in l_dict.items()})
        return losses

    def get_target_masks(self, targets, src_masks):
        """[bs, G_max, h, w] in src_masks' dtype: the padded masks at every mask_out_stride-th pixel from stride // 2."""
        target_masks = pad_masks([t["masks"] for t in targets]).to(src_masks)
        if self.mask_out_stride != 1:
            start = int(self.mask_out_stride // 2)
            im_h, im_w = target_masks.shape[-2:]
            target_masks = target_masks[:, :, start::self.mask_out_stride, start::self.mask_out_stride]
            assert target_masks.size(2) * self.mask_out_stride == im_h
            assert target_masks.size(3) * self.mask_out_stride == im_w
        return target_masks


class DINOCriterion(SetCriterion):
    """SetCriterion plus the losses of the denoising queries (`name_dn`, `name_dn_{i}`)."""

    def forward(self, outputs, targets, indices_list, dn_metas=None):
        losses = super(DINOCriterion, self).forward(outputs, targets, indices_list)
        # compute_dn_loss keeps the reference's signature, which has no `outputs`: the device its zeros and indices are created on
        # (where the reference says .cuda()) travels through this attribute; called on its own it takes the dn outputs' device
        self._dn_device = next(iter(outputs.values())).device
        num_boxes = self._num_boxes(outputs, targets)
        aux_num = len(outputs["aux_outputs"]) if "aux_outputs" in outputs else 0
        self._shared = {}
        try:
            losses.update(self.compute_dn_loss(dn_metas, targets, aux_num, num_boxes))
        finally:
            self._shared = None
        return losses

    def compute_dn_loss(self, dn_metas, targets, aux_num, num_boxes):
        """The labelsVL and boxes losses of the denoising queries: group g of an image with n targets holds target j at query
        g * single_padding + j; num_boxes counts every group.  Without dn_metas: zeros under the reference's keys."""
        device = getattr(self, "_dn_device", None)
        with_dn = bool(dn_metas) and "output_known_lbs_bboxes" in dn_metas
        losses = {}

        def zeros():
            return {k: torch.as_tensor(0.0, device=device) for k in ("loss_bbox_dn", "loss_giou_dn", "loss_class_dn")}

        def dn_losses(known):
            l_dict = {}
            for loss in self.losses:
                if loss not in ['labelsVL', 'boxes']:
                    continue
                kwargs = {"log": False} if "labels" in loss else {}
                l_dict.update(self.get_loss(loss, known, targets, dn_idx, num_boxes * dn_num, **kwargs))
            return l_dict

        if with_dn:
            known, dn_num, single_padding = dn_metas["output_known_lbs_bboxes"], dn_metas["dn_num"], dn_metas["single_padding"]
            if device is None:
                device = next(iter(v for v in known.values() if torch.is_tensor(v))).device
            dn_idx = []
            for t in targets:
                n = len(t["labels"])
                if n > 0:
                    tgt = torch.arange(n, dtype=torch.long, device=device).unsqueeze(0).repeat(dn_num, 1)
                    out = (torch.arange(dn_num, dtype=torch.long, device=device) * single_padding).unsqueeze(1) + tgt
                    dn_idx.append((out.flatten(), tgt.flatten()))
                else:
                    empty = torch.zeros(0, dtype=torch.long, device=device)
                    dn_idx.append((empty, empty))
            losses.update({k + "_dn": v for k, v in dn_losses(known).items()})
        else:
            losses.update(zeros())

        for i in range(aux_num):
            if with_dn:
                l_dict = {k + f"_dn_{i}": v for k, v in dn_losses(known["aux_outputs"][i]).items()}
            else:
                l_dict = {k + f"_{i}": v for k, v in zeros().items()}
            losses.update(l_dict)
        return losses
