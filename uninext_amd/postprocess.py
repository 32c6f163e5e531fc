"""Detection post-processing: from the decoder's token logits, boxes and IoU logits to scored, labelled boxes.

Host-side mirror of `UNINEXT_IMG.inference` (projects/UNINEXT/uninext/uninext_img.py:367-485) and of
`convert_grounding_to_od_logits` (:598-613), without the mask lines (:474-480) and without the `Instances` / `Boxes` containers:
a result is a dict of tensors.  `batched_nms` restates `torchvision.ops.batched_nms`, which the reference calls and which is
not a dependency of this package.

`DetectionPostProcess` composes the step.  With `fused` set (the default), on fp32 GPU tensors within the kernels' sizes, it is two
HIP kernels (include/dynmask_hip.h: detpost_scores_hip_f32 scores every (query, class); detpost_nms_hip_f32 runs the class-aware
NMS of every image in one workgroup each), one batched `torch.topk` and ONE host copy of the per-image counts; otherwise it is
the reference's composition of PyTorch ops, image by image.

Conventions pinned here (DESIGN.md "Detection post-processing"): equal scores are visited by increasing query index; a pair
suppresses when inter / (area_i + area_j - inter) > threshold, so 0 / 0 does not; boxes of different classes are kept apart by
the coordinate offset while boxes.numel() <= 4000 and by comparing classes beyond.

The mask lines (:474-480), `segmentation_postprocess` (models/deformable_detr/segmentation.py:25-71) on result dicts and the
tracker's `mask_iou` / `mask_nms` (models/tracker.py:17-46) follow at the end of the file: `MaskPostProcess` and `mask_nms` run
the maskpost_* kernels of include/dynmask_hip.h on fp32 GPU logits (DESIGN.md "Mask post-processing").
"""
import numpy as np
import torch
import torch.nn.functional as F

from . import ext as MSDA

NMS_IOU_THRESHOLD = 0.7            # uninext_img.py:413
COORDINATE_TRICK_MAX_NUMEL = 4000  # torchvision.ops.batched_nms: the offset route up to here, class by class beyond


def _class_tokens(positive_map, num_classes, num_tokens=None):
    """{class: [token, ...]} as the reference's loop leaves it: class = label - 1 (label 0 addresses the last class, as the
    reference's negative index does), a later label of the same class replaces an earlier one."""
    out = {}
    for label, tokens in positive_map.items():
        c = int(label) - 1
        if not -num_classes <= c < num_classes:
            raise IndexError("label %d is out of range for %d classes" % (label, num_classes))
        toks = [int(t) for t in tokens]
        if num_tokens is not None:
            if any(not -num_tokens <= t < num_tokens for t in toks):
                raise IndexError("a token of label %d is out of range for %d tokens" % (label, num_tokens))
            toks = [t % num_tokens for t in toks]
        out[c % num_classes] = toks
    return out


def convert_grounding_to_od_logits(logits, num_classes, positive_map, score_agg="MEAN"):
    """logits [B, Q, T], positive_map {label (1-based): [token, ...]} -> [B, Q, num_classes]: the mean of a class's token
    logits, 0.0 for a class the map does not name.  The classes are taken in groups of equal token count, one gather and one
    mean per group, which gives the values of the reference's loop over the labels."""
    assert logits.ndim == 3
    assert positive_map is not None
    if score_agg != "MEAN":
        raise NotImplementedError
    scores = torch.zeros(logits.shape[0], logits.shape[1], num_classes, dtype=logits.dtype, device=logits.device)
    by_count = {}
    for c, toks in _class_tokens(positive_map, num_classes, logits.shape[2]).items():
        by_count.setdefault(len(toks), []).append((c, toks))
    for n, group in by_count.items():
        cls = torch.tensor([c for c, _ in group], dtype=torch.long, device=logits.device)
        tok = torch.tensor([t for _, toks in group for t in toks], dtype=torch.long, device=logits.device)
        picked = logits.index_select(2, tok).view(logits.shape[0], logits.shape[1], len(group), n)
        scores[:, :, cls] = picked.mean(-1)          # n == 0: NaN, as the mean of an empty selection is in the reference
    return scores


def box_cxcywh_to_xyxy(x):
    x_c, y_c, w, h = x.unbind(-1)
    return torch.stack([(x_c - 0.5 * w), (y_c - 0.5 * h), (x_c + 0.5 * w), (y_c + 0.5 * h)], dim=-1)


def _greedy_nms(boxes, scores, iou_threshold, classes=None):
    """Indices (int64) of the boxes greedy NMS keeps, by decreasing score, equal scores by increasing index.  With `classes`,
    only a pair of one class suppresses."""
    n = boxes.shape[0]
    if n == 0:
        return torch.empty((0,), dtype=torch.int64, device=boxes.device)
    order = torch.sort(scores, descending=True, stable=True)[1]
    b = boxes[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt = torch.max(b[:, None, :2], b[None, :, :2])
    rb = torch.min(b[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    suppress = inter / (area[:, None] + area[None, :] - inter) > iou_threshold
    if classes is not None:
        c = classes[order]
        suppress &= c[:, None] == c[None, :]
    suppress = suppress.cpu().numpy()
    removed = np.zeros(n, dtype=bool)
    kept = []
    for i in range(n):
        if not removed[i]:
            kept.append(i)
            removed[i + 1:] |= suppress[i, i + 1:]
    return order[torch.as_tensor(kept, dtype=torch.int64, device=boxes.device)]


def nms(boxes, scores, iou_threshold):
    """torchvision.ops.nms: boxes [N, 4] xyxy, scores [N] -> kept indices (int64) by decreasing score."""
    return _greedy_nms(boxes, scores, iou_threshold)


def batched_nms(boxes, scores, idxs, iou_threshold):
    """torchvision.ops.batched_nms: NMS among the boxes of one class only.  boxes [N, 4] xyxy, scores [N], idxs [N] the
    classes -> kept indices (int64) by decreasing score."""
    if boxes.numel() == 0:
        return torch.empty((0,), dtype=torch.int64, device=boxes.device)
    if boxes.numel() > COORDINATE_TRICK_MAX_NUMEL:
        return _greedy_nms(boxes, scores, iou_threshold, classes=idxs)
    max_coordinate = boxes.max()
    offsets = idxs.to(boxes) * (max_coordinate + torch.tensor(1).to(boxes))
    return _greedy_nms(boxes + offsets[:, None], scores, iou_threshold)


_csr_cache = {}


def positive_map_csr(positive_map, num_classes, num_tokens, device):
    """(cls_ptr [C + 1], tok_idx [nnz]) int32 on `device` for the detpost kernels, or None when a label of the map has an
    empty token list (the reference's NaN; the composition reproduces it).  Cached per (map object, num_classes, device): a
    map that is edited in place must be passed as a new object."""
    key = (id(positive_map), int(num_classes), str(device))
    e = _csr_cache.get(key)
    if e is None or e[0] is not positive_map:
        tokens = _class_tokens(positive_map, num_classes)
        flat = [t for toks in tokens.values() for t in toks]
        csr = None
        if all(len(toks) > 0 for toks in tokens.values()):
            ptr, idx = [0], []
            for c in range(num_classes):
                idx.extend(tokens.get(c, ()))
                ptr.append(len(idx))
            csr = (torch.tensor(ptr, dtype=torch.int32).to(device), torch.tensor(idx or [0], dtype=torch.int32).to(device)[:len(idx)])
        if len(_csr_cache) > 32:
            _csr_cache.clear()
        e = (positive_map, csr, min(flat, default=0), max(flat, default=0))
        _csr_cache[key] = e
    _, csr, lo, hi = e
    if lo < -num_tokens or hi >= num_tokens:
        raise IndexError("a token of the positive map is out of range for %d tokens" % num_tokens)
    if csr is None or lo < 0:      # negative (wrapping) token indices: left to the composition
        return None
    return csr


_scale_cache = {}


def _image_scales(image_sizes, device):
    """[B, 1, 4] fp32 (width, height, width, height) of every image on `device`, copied there once per list of sizes."""
    key = (tuple((int(s[0]), int(s[1])) for s in image_sizes), str(device))
    if key not in _scale_cache:
        if len(_scale_cache) > 64:
            _scale_cache.clear()
        _scale_cache[key] = torch.tensor([[[w, h, w, h]] for h, w in key[0]], dtype=torch.float32).to(device)
    return _scale_cache[key]


class DetectionPostProcess:
    """results = DetectionPostProcess(ota, fused, demo_only)(box_cls, box_pred, iou_pred, image_sizes,
    positive_map_label_to_token, num_classes, score_thres=0.0, task="detection")

    box_cls [B, Q, T] token logits, box_pred [B, Q, 4] cxcywh in [0, 1], iou_pred [B, Q, 1] (or [B, Q]) IoU logits or None,
    image_sizes one (height, width) per image.  `ota` selects the reference's branch: NMS at 0.7 over the queries' best classes
    and then the top-k of the surviving (query, class) scores, or the top-k alone.  task "detection" returns up to 100 instances
    per image, "grounding" one.  Per image a dict: `scores` [n], `pred_classes` [n] int64, `pred_boxes` [n, 4] xyxy in pixels,
    `query_index` [n] int64 the rows of the original Q the instances come from (the rows of `mask_pred` the reference keeps)."""

    # The HIP route, on by default: 4.7x ahead of the composition on an MI355X with and without a score threshold, 1 host
    # synchronisation per call against 24 (profiles/r15_postprocess.txt, tools/postprocess_bench.py).  Off the GPU, for other
    # dtypes and beyond the kernels' sizes a call takes the composition whatever this says.
    fused = True

    def __init__(self, ota=True, fused=None, demo_only=False):
        self.ota = bool(ota)
        self.demo_only = bool(demo_only)
        if fused is not None:
            self.fused = bool(fused)

    def __call__(self, box_cls, box_pred, iou_pred, image_sizes, positive_map_label_to_token, num_classes, score_thres=0.0,
                 task="detection", mask_pred=None, output_sizes=None, mask_stride=4, mask_thres=0.5):
        results = self._boxes(box_cls, box_pred, iou_pred, image_sizes, positive_map_label_to_token, num_classes, score_thres, task)
        if mask_pred is not None:      # [B, Q, 1, h, w] (or [B, Q, h, w]) mask logits: the reference's mask lines (:474-480)
            assert len(mask_pred) == len(results)
            masks = MaskPostProcess(mask_stride, mask_thres)
            for b, result in enumerate(results):
                result["pred_masks"] = masks(mask_pred[b], result["query_index"], image_sizes[b],
                                             None if output_sizes is None else output_sizes[b])
        return results

    def _boxes(self, box_cls, box_pred, iou_pred, image_sizes, positive_map_label_to_token, num_classes, score_thres, task):
        if task == "detection":
            max_num_inst = 100
        elif task == "grounding":
            max_num_inst = 1
        else:
            raise ValueError("task must be detection or grounding")
        assert len(box_cls) == len(image_sizes)
        if iou_pred is not None and iou_pred.dim() == 3:
            iou_pred = iou_pred[..., 0]
        args = (box_cls, box_pred, iou_pred, image_sizes, positive_map_label_to_token, num_classes, float(score_thres), max_num_inst)
        if self.fused:
            csr = self._fused_csr(box_cls, box_pred, iou_pred, positive_map_label_to_token, num_classes, max_num_inst)
            if csr is not None:
                return self._fused(csr, *args)
        return self._composition(*args)

    def _fused_csr(self, box_cls, box_pred, iou_pred, positive_map, num_classes, max_num_inst):
        """The CSR positive map when the kernels take the call, None when the composition does."""
        tensors = (box_cls, box_pred) + (() if iou_pred is None else (iou_pred,))
        if not all(t.is_cuda and t.dtype == torch.float32 and t.device == box_cls.device for t in tensors):
            return None
        if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
            return None
        if box_cls.dim() != 3 or box_cls.shape[0] == 0 or tuple(box_pred.shape) != tuple(box_cls.shape[:2]) + (4,):
            return None
        B, Q, T = box_cls.shape
        if iou_pred is not None and tuple(iou_pred.shape) != (B, Q):
            return None
        if not MSDA.detpost_supported(Q, num_classes, T):
            return None
        if not self.ota and Q * num_classes < max_num_inst:      # torch.topk refuses it in the composition; let it
            return None
        return positive_map_csr(positive_map, num_classes, T, box_cls.device)

    def _composition(self, box_cls, box_pred, iou_pred, image_sizes, positive_map, num_classes, score_thres, max_num_inst):
        results = []
        for i in range(len(box_cls)):
            logits = convert_grounding_to_od_logits(box_cls[i].unsqueeze(0), num_classes, positive_map)[0]     # [Q, C]
            prob = logits.sigmoid()
            if iou_pred is not None:
                prob = torch.sqrt(prob * iou_pred[i].unsqueeze(-1).sigmoid())
            if score_thres > 0.0:
                valid_mask = prob > score_thres
                num_inst = min(int(torch.sum(valid_mask).item()), max_num_inst)
                prob = prob.masked_fill(~valid_mask, -1.0)
            else:
                num_inst = max_num_inst
            boxes = box_pred[i]
            C = prob.shape[1]
            if self.ota:
                nms_scores, idxs = torch.max(prob, 1)
                keep = batched_nms(box_cxcywh_to_xyxy(boxes), nms_scores, idxs, NMS_IOU_THRESHOLD)
                prob = prob[keep]
                if self.demo_only:
                    scores, labels = nms_scores[keep], idxs[keep]
                    valid = scores > score_thres
                    results.append(self._result(scores[valid], labels[valid], keep[valid], boxes, image_sizes[i]))
                    continue
                num_inst = min(num_inst, prob.numel())
                scores, flat = torch.topk(prob.reshape(-1), num_inst, dim=0)
                query = keep[torch.div(flat, C, rounding_mode="floor")]
            else:
                scores, flat = torch.topk(prob.reshape(-1), num_inst, dim=0)
                query = torch.div(flat, C, rounding_mode="floor")
            results.append(self._result(scores, flat % C, query, boxes, image_sizes[i]))
        return results

    @staticmethod
    def _result(scores, labels, query, boxes, image_size):
        xyxy = box_cxcywh_to_xyxy(boxes[query])
        scale = torch.tensor([image_size[1], image_size[0], image_size[1], image_size[0]], dtype=xyxy.dtype).to(xyxy.device)
        return {"scores": scores, "pred_classes": labels, "pred_boxes": xyxy * scale, "query_index": query}

    def _fused(self, csr, box_cls, box_pred, iou_pred, image_sizes, positive_map, num_classes, score_thres, max_num_inst):
        with torch.no_grad():
            B, Q, _ = box_cls.shape
            C = num_classes
            dev = box_cls.device
            box_pred = box_pred.contiguous()
            prob, row_max, row_arg, row_valid = MSDA.detpost_scores(
                box_cls.contiguous(), None if iou_pred is None else iou_pred.contiguous(), csr[0], csr[1], score_thres)
            counts = [row_valid.sum(1)] if score_thres > 0.0 else []
            if self.ota:
                keep, n_keep, kept_mask = MSDA.detpost_nms(box_pred, row_max, row_arg, NMS_IOU_THRESHOLD,
                                                           per_class=Q * 4 > COORDINATE_TRICK_MAX_NUMEL)
                counts.append(n_keep)
                if self.demo_only:       # kept scores descend, so the ones above the threshold are a prefix of `keep`
                    counts.append(((row_max > score_thres) & (kept_mask != 0)).sum(1))
                else:
                    prob.masked_fill_((kept_mask == 0).unsqueeze(-1), -2.0)       # below the reference's -1.0
            scale = _image_scales(image_sizes, dev)      # [B, 1, 4]
            if self.ota and self.demo_only:
                query = keep.long().clamp_(min=0)
                scores, labels = row_max.gather(1, query), row_arg.long().gather(1, query)
            else:
                scores, flat = torch.topk(prob.view(B, Q * C), min(max_num_inst, Q * C), dim=1)
                query = torch.div(flat, C, rounding_mode="floor")
                labels = flat - query * C
            boxes = box_cxcywh_to_xyxy(box_pred.gather(1, query.unsqueeze(-1).expand(-1, -1, 4))) * scale
            counts = torch.stack([c.long() for c in counts], 1).tolist() if counts else [[] for _ in range(B)]     # the one host copy
            results = []
            for b, c in enumerate(counts):
                num_inst = min(c[0], max_num_inst) if score_thres > 0.0 else max_num_inst
                if self.ota:
                    n_kept = c[-2] if self.demo_only else c[-1]
                    num_inst = c[-1] if self.demo_only else min(num_inst, n_kept * C)
                results.append({"scores": scores[b, :num_inst], "pred_classes": labels[b, :num_inst],
                                "pred_boxes": boxes[b, :num_inst], "query_index": query[b, :num_inst]})
            return results


def postprocess_detections(*args, ota=True, fused=None, demo_only=False, **kwargs):
    """DetectionPostProcess(ota, fused, demo_only)(...) as a function."""
    return DetectionPostProcess(ota=ota, fused=fused, demo_only=demo_only)(*args, **kwargs)


class MaskPostProcess:
    """masks = MaskPostProcess(mask_stride, mask_thres, fused)(mask_pred, query_index, image_size, output_size=None)

    mask_pred [Q, 1, h, w] or [Q, h, w] mask logits of one image, query_index [n] int64 the rows of its instances (what
    DetectionPostProcess returns), image_size (height, width) of the image inside the padded batch, output_size (height, width)
    the masks are wanted at, None for the image size.  Returns [n, H, W] uint8 of 0 / 1: the mask lines of
    `UNINEXT_IMG.inference` (uninext_img.py:474-480: bilinear x mask_stride, sigmoid, > mask_thres, crop to the image) followed,
    with an output size, by the nearest resize of `segmentation_postprocess` (segmentation.py:60-65).  With `fused`, on fp32 GPU
    logits within the kernel's sizes, it is one HIP kernel that forms only the pixels the nearest step picks
    (include/dynmask_hip.h: maskpost_binarize_hip_f32); otherwise the reference's sequence of PyTorch ops.  Conventions:
    DESIGN.md "Mask post-processing"."""

    # The HIP route, on by default: 3.7x / 7.6x ahead of the composition at 100 instances of 200x336 logits to 800x1333 / 480x640 on
    # an MI355X, 1.9x at 10 instances to 720x1280, under 1 MB of temporaries against 0.9 GB (profiles/r19_maskpost.txt,
    # tools/maskpost_bench.py).  Off the GPU, for other dtypes and beyond the kernel's sizes a call takes the composition.
    fused = True

    def __init__(self, mask_stride=4, mask_thres=0.5, fused=None):
        self.mask_stride = int(mask_stride)
        self.mask_thres = float(mask_thres)
        if fused is not None:
            self.fused = bool(fused)

    def __call__(self, mask_pred, query_index, image_size, output_size=None):
        if mask_pred.dim() == 4:
            assert mask_pred.shape[1] == 1
            mask_pred = mask_pred[:, 0]
        assert mask_pred.dim() == 3 and query_index.dim() == 1
        Q, h, w = mask_pred.shape
        s = self.mask_stride
        crop = (min(int(image_size[0]), h * s), min(int(image_size[1]), w * s))      # a slice past the plane ends with it
        out = crop if output_size is None else (int(output_size[0]), int(output_size[1]))
        n = query_index.shape[0]
        if (self.fused and mask_pred.is_cuda and mask_pred.dtype == torch.float32 and query_index.dtype == torch.int64
                and query_index.device == mask_pred.device and not (torch.is_grad_enabled() and mask_pred.requires_grad)
                and MSDA.maskpost_supported(h, w, s, crop, out, self.mask_thres, Q, n)):
            return MSDA.maskpost_binarize(mask_pred.contiguous(), query_index.contiguous(), s, crop, out, self.mask_thres)
        if n == 0:
            return torch.zeros((0,) + out, dtype=torch.uint8, device=mask_pred.device)
        mask = mask_pred[query_index].unsqueeze(1)
        mask = F.interpolate(mask, size=(h * s, w * s), mode="bilinear", align_corners=False)
        mask = mask.sigmoid() > self.mask_thres
        mask = mask[:, :, :crop[0], :crop[1]]
        if output_size is not None:
            mask = F.interpolate(mask.float(), size=out, mode="nearest")
        return mask.squeeze(1).byte()


def postprocess_masks(mask_pred, query_index, image_size, output_size=None, mask_stride=4, mask_thres=0.5, fused=None):
    """MaskPostProcess(mask_stride, mask_thres, fused)(mask_pred, query_index, image_size, output_size) as a function."""
    return MaskPostProcess(mask_stride, mask_thres, fused)(mask_pred, query_index, image_size, output_size)


def segmentation_postprocess(result, output_height, output_width, image_size=None):
    """`segmentation_postprocess` (models/deformable_detr/segmentation.py:25-71) on a result dict of DetectionPostProcess: the
    boxes are scaled from the image size to the output size and clipped to it, instances whose box is empty are dropped, and
    `pred_masks` ([n, H, W] or [n, 1, H, W], if present) are resized with mode='nearest' and returned as [n, output_height,
    output_width] uint8.  `image_size` (height, width) is the size the boxes refer to; without it, the size of `pred_masks`.
    Returns a new dict."""
    if image_size is None:
        assert "pred_masks" in result, "segmentation_postprocess: image_size is needed when the result carries no masks"
        image_size = tuple(result["pred_masks"].shape[-2:])
    scale_x, scale_y = output_width / image_size[1], output_height / image_size[0]
    boxes = result["pred_boxes"].clone()
    boxes[:, 0::2] *= scale_x
    boxes[:, 1::2] *= scale_y
    boxes[:, 0::2] = boxes[:, 0::2].clamp(min=0, max=output_width)
    boxes[:, 1::2] = boxes[:, 1::2].clamp(min=0, max=output_height)
    nonempty = ((boxes[:, 2] - boxes[:, 0]) > 0) & ((boxes[:, 3] - boxes[:, 1]) > 0)
    out = {key: value[nonempty] for key, value in result.items() if key != "pred_boxes"}
    out["pred_boxes"] = boxes[nonempty]
    if "pred_masks" in out:
        mask = out["pred_masks"]
        mask = mask.unsqueeze(1) if mask.dim() == 3 else mask
        mask = F.interpolate(mask.float(), size=(output_height, output_width), mode="nearest")
        out["pred_masks"] = mask.squeeze(1).byte()
    return out


def mask_iou(mask1, mask2):
    """`mask_iou` (models/tracker.py:17-24): masks [k, h, w] -> [k] (intersection + 1e-6) / (union + 1e-6), so two empty masks
    have IoU 1."""
    mask1 = mask1.char()
    mask2 = mask2.char()
    intersection = (mask1 * mask2).sum(-1).sum(-1)
    union = (mask1 + mask2 - mask1 * mask2).sum(-1).sum(-1)
    return (intersection + 1e-6) / (union + 1e-6)


# mask_nms' default route: the kernels, 0.17 / 0.22 ms and 1 host synchronisation at 30 / 100 detections of 200x336 against 15 /
# 68 ms and 153 / 652 for the reference's loop on an MI355X (profiles/r19_maskpost.txt)
MASK_NMS_FUSED = True


def mask_nms(seg_masks, scores, category_ids=None, nms_thr=0.5, fused=None):
    """`mask_nms` (models/tracker.py:26-46): seg_masks [n, 1, h, w] (or [n, h, w]) mask logits, binarised at the low resolution
    with sigmoid > 0.5; greedy in the GIVEN order (`scores` gives the number of masks only, `category_ids` is unused, as in the
    reference): a kept mask suppresses every later one whose mask IoU with it is above nms_thr.  Returns a list of Python
    bools.  With `fused` (None: MASK_NMS_FUSED), on fp32 GPU logits of at most 1024 masks, it is the kernels of
    include/dynmask_hip.h (maskpost_pack_hip_f32, maskpost_nms_hip_u32) and ONE host copy of the keep flags; otherwise the
    reference's double loop with a host synchronisation per visited pair."""
    n_samples = len(scores)
    if n_samples == 0:
        return []
    if seg_masks.dim() == 3:
        seg_masks = seg_masks.unsqueeze(1)
    assert seg_masks.dim() == 4 and seg_masks.shape[1] == 1 and seg_masks.shape[0] >= n_samples
    if ((MASK_NMS_FUSED if fused is None else fused) and seg_masks.is_cuda and seg_masks.dtype == torch.float32
            and n_samples <= MSDA._lib.MASKPOST_MAX_MASKS and seg_masks.shape[2] * seg_masks.shape[3] < 1 << 30
            and seg_masks.numel() < 1 << 31 and not (torch.is_grad_enabled() and seg_masks.requires_grad)):
        rows = torch.arange(n_samples, dtype=torch.int64, device=seg_masks.device)
        bits, area = MSDA.maskpost_pack(seg_masks[:, 0].contiguous(), rows)
        _, keep = MSDA.maskpost_nms(bits, area, nms_thr)
        return [bool(k) for k in keep.tolist()]        # the one host copy
    keep = [True for _ in range(n_samples)]
    seg_masks = seg_masks.sigmoid() > 0.5
    for i in range(n_samples - 1):
        if not keep[i]:
            continue
        mask_i = seg_masks[i]
        for j in range(i + 1, n_samples, 1):
            if not keep[j]:
                continue
            mask_j = seg_masks[j]
            iou = mask_iou(mask_i, mask_j)[0]
            if iou > nms_thr:
                keep[j] = False
    return keep
