"""Re-ID contrastive training of the video configs: positive / negative selection and the re-ID loss.

Mirror of the reference's `select_pos_neg`, `get_pos_idx`, `get_in_boxes_info`, `dynamic_k_matching`
(projects/UNINEXT/uninext/models/pos_neg_select.py) and `SetCriterion.loss_reid` (deformable_detr.py:529-565): the same names,
argument orders, dictionary keys and `embed_head` handling (the `[1]([0](...))` chain of the deformable re-ID head with its two
asserts, `.detach()` under `detach_reid`).  `VideoSetCriterion` / `VideoDINOCriterion` are the criterion classes with `"reid"`
accepted in `losses`; they change nothing else.  torchvision is not a dependency: `box_iou` is uninext_amd.matcher's.

`FUSED` (module attribute) / `select_pos_neg(..., fused=)`, ON by default since it was measured: 3.2 ms against 36.1 ms for forward +
backward at the video training shape on an MI355X, 1 host synchronisation against 254 (profiles/r21_reid.txt; `reid.FUSED = False` or
`fused=False` turns it off):

  off  a composition of PyTorch operations restating the reference's arithmetic (the matcher's cost helpers, one top-k over all
       targets, the loss over the (positive, negative) pairs only), held to the reference's fixtures.  The CPU path, and the
       yardstick of the fused one.
  on   for contiguous fp32 GPU tensors, 100 <= Q <= 8192 and C a multiple of 64 up to 512, the selection of the whole batch runs in
       two kernels (include/ota_hip.h: ota_cost_hip_f32, ota_reid_select_hip) and `select_pos_neg` returns a `PackedContrastItems`,
       which `loss_reid` consumes through `ReidLossFunction` (ota_reid_scores_hip_f32, ota_reid_loss_hip_f32, ota_reid_loss_bwd_hip_f32).
       Anything the kernels do not take falls back silently to the composition (Q < 100 therefore raises what torch.topk raises
       in the reference, on both routes).

Randomness: the reference draws the auxiliary negatives with `random.sample(list(range(0, n_neg)), k)`, once per item in item
order.  The fused route makes the same calls with the same arguments in the same order, so after `random.seed(s)` both routes
pick the same queries and leave the generator in the same state.  That is why the fused route has ONE device-to-host copy per
call: the per-target (n_pos, n_neg) counts come down (`_host_copy`), the drawn ranks go up as one int32 array.  The targets'
`valid` flags are read on the device.
"""
import random

import torch
from torch import nn

from . import _lib, ext
from .criterion import DINOCriterion, SetCriterion
from .matcher import (FOCAL_ALPHA, FOCAL_GAMMA, OTA_BG_PENALTY, OTA_GIOU_WEIGHT, OTA_PRIOR_PENALTY, OTA_STRIDE, HungarianMatcherVL,
                      box_cxcywh_to_xyxy, box_iou, focal_token_cost, generalized_box_iou)

FUSED = True                # measured: profiles/r21_reid.txt (tools/reid_bench.py)
POS_CANDIDATES = 10         # pos_neg_select.py:130
NEG_CANDIDATES = 100        # pos_neg_select.py:131
OTA_TAKEN_PENALTY = 100000.0   # pos_neg_select.py:210


def _host_copy(t):
    """THE device-to-host copy of the fused route."""
    return t.cpu()


def _num_sample_neg(n_pos, n_neg):
    """How many negatives the auxiliary loss samples (pos_neg_select.py:76-81)."""
    if n_pos == 0:
        return 10
    if n_pos * 10 >= n_neg:
        return n_neg
    return n_pos * 10


def _contrast_item(rows, key_row, pos_mask, neg_mask, drawn, one, zero):
    """One contrast item.  rows [Q, C]: the image's reference embeddings; key_row [1, C]; pos_mask: the target's positives; neg_mask:
    the queries that may overlap the target -- every query OUTSIDE it is a negative; drawn: the ranks (among the negatives, in
    query order) of the auxiliary loss's negatives, or None to draw them here, the way the reference draws them."""
    pos, neg = rows[pos_mask], rows[~neg_mask]
    if drawn is None:
        drawn = random.sample(list(range(0, len(neg))), _num_sample_neg(len(pos), len(neg)))
    label = torch.cat([one.repeat(len(pos)), zero.repeat(len(neg))], dim=0)
    contrast = torch.einsum('nc,kc->nk', [torch.cat([pos, neg], dim=0), key_row])
    aux_label = torch.cat([one.repeat(len(pos)), zero.repeat(len(drawn))], dim=0)
    unit_rows = nn.functional.normalize(torch.cat([pos, neg[drawn]], dim=0).float(), dim=1)
    unit_key = nn.functional.normalize(key_row.float(), dim=1)
    return {'contrast': contrast, 'label': label, 'aux_consin': torch.einsum('nc,kc->nk', [unit_rows, unit_key]), 'aux_label': aux_label}


class PackedContrastItems:
    """The fused route's result of `select_pos_neg`: the items of the whole batch as device arrays.  `len()` is the number of
    items; `expand()` gives the reference's list of dicts ('contrast', 'label', 'aux_consin', 'aux_label')."""

    def __init__(self, ref_embeds, key_embeds, sizes, key_index, valid, matching_pos, matching_neg, item_meta, ranks, items, host_ranks):
        self.ref_embeds, self.key_embeds = ref_embeds, key_embeds          # [bs, Q, C], [bs, Qk, C]: where the gradient goes
        self.sizes = sizes                                                 # targets per image
        self.key_index, self.valid = key_index, valid                      # [G_total] int64 / uint8
        self.matching_pos, self.matching_neg = matching_pos, matching_neg  # uint8, the batch layout of include/ota_hip.h
        self.item_meta, self.ranks = item_meta, ranks                      # int32 [n, 5], int32 [max(total, 1)]
        self.items, self.host_ranks = items, host_ranks                    # host: (image, target, first rank, ranks, n_aux) per item
        self.item_counts = [sum(1 for it in items if it[0] == b) for b in range(len(sizes))]

    def __len__(self):
        return len(self.items)

    def expand(self):
        one = torch.tensor(1).to(self.ref_embeds)
        zero = torch.tensor(0).to(self.ref_embeds)
        Q = self.ref_embeds.shape[1]
        offsets = [0]
        for n in self.sizes:
            offsets.append(offsets[-1] + n)
        out = []
        for b, target, first, count, _ in self.items:
            g0, G = offsets[b], self.sizes[b]
            pos = self.matching_pos[Q * g0:Q * (g0 + G)].view(Q, G)[:, target - g0] > 0
            neg = self.matching_neg[Q * g0:Q * (g0 + G)].view(Q, G)[:, target - g0] > 0
            key_embed_i = self.key_embeds[b, self.key_index[target]].unsqueeze(0)
            out.append(_contrast_item(self.ref_embeds[b], key_embed_i, pos, neg, self.host_ranks[first:first + count], one, zero))
        return out


def select_pos_neg(ref_box, all_indices, targets, det_targets, embed_head, hs_key, hs_ref, ref_cls, detach_reid=False,
                   use_deformable_reid_head=False, src_info_key=None, src_info_ref=None, fused=None):
    """The contrast items of a batch of key / reference frame pairs.

    ref_box [bs, Q, 4] cxcywh and ref_cls [bs, Q, T] token probabilities: the reference frames' predictions; targets: the reference
    frames' ground truth per image ("labels", "boxes", "positive_map" [G, T], "valid" [G]); all_indices: per image, for every
    target the key-frame query matched to it; det_targets: the key frames' ground truth (unused, as in the reference); hs_key /
    hs_ref [bs, Q, C]: the decoder states the embedding head is applied to.  fused: None (the module's FUSED), True or False.
    Returns a list of {'contrast', 'label', 'aux_consin', 'aux_label'} per valid target, or a PackedContrastItems (fused route)."""
    if use_deformable_reid_head:
        assert (src_info_key is not None) and (src_info_ref is not None)
        assert detach_reid
        sampler, projection = embed_head[0], embed_head[1]

        def embed(hs, info):
            return projection(sampler(hs.detach(), info["reference_points"], info["src"], info["src_spatial_shapes"],
                                      info["src_level_start_index"], info["src_valid_ratios"], info["src_padding_mask"]))

        ref_embeds, key_embeds = embed(hs_ref, src_info_ref), embed(hs_key, src_info_key)
    elif detach_reid:
        ref_embeds, key_embeds = embed_head(hs_ref.detach()), embed_head(hs_key.detach())
    else:
        ref_embeds, key_embeds = embed_head(hs_ref), embed_head(hs_key)
    assert len(targets) == len(all_indices)
    if (FUSED if fused is None else fused) and _fusable(ref_box, all_indices, targets, ref_embeds, key_embeds, ref_cls):
        return _select_fused(ref_box, all_indices, targets, ref_embeds, key_embeds, ref_cls)
    one = torch.tensor(1).to(ref_embeds)
    zero = torch.tensor(0).to(ref_embeds)
    items = []
    for b, (target, key_queries) in enumerate(zip(targets, all_indices)):
        count = len(target["labels"])
        pos_masks, neg_masks = get_pos_idx(ref_box[b], ref_cls[b], target["boxes"].reshape(count, 4), target["positive_map"], target["valid"])
        for g, (is_valid, key_query) in enumerate(zip(target["valid"], key_queries)):
            if is_valid:
                items.append(_contrast_item(ref_embeds[b], key_embeds[b, key_query].unsqueeze(0), pos_masks[g], neg_masks[g], None, one, zero))
    return items


def get_pos_idx(bz_boxes, bz_out_prob, bz_gtboxs, bz_tgt_ids, valid):
    """(positives, overlapping) of one image: per target a [Q] bool mask, None for a target that is not valid.  The simOTA cost of
    the matcher over the valid targets, then dynamic_k_matching twice ON THE SAME cost tensor, with 10 and with 100 candidates:
    what the first run's repair loop adds to the cost, the second run sees."""
    with torch.no_grad():
        present = valid.reshape(-1).bool()
        slots = present.tolist()
        positives, overlapping = [], []
        if any(slots):
            gt_boxes, gt_maps = bz_gtboxs[present], bz_tgt_ids[present]
            candidate, in_box_and_center = get_in_boxes_info(bz_boxes, gt_boxes, expanded_strides=OTA_STRIDE)
            boxes_xyxy, gt_xyxy = box_cxcywh_to_xyxy(bz_boxes), box_cxcywh_to_xyxy(gt_boxes)
            ious = box_iou(boxes_xyxy, gt_xyxy)
            cost = focal_token_cost(bz_out_prob, gt_maps) + OTA_GIOU_WEIGHT * (-generalized_box_iou(boxes_xyxy, gt_xyxy)) \
                + OTA_PRIOR_PENALTY * (~in_box_and_center)
            cost[~candidate] = cost[~candidate] + OTA_BG_PENALTY
            positives = dynamic_k_matching(cost, ious, len(gt_boxes), POS_CANDIDATES)
            overlapping = dynamic_k_matching(cost, ious, len(gt_boxes), NEG_CANDIDATES)
        found = iter(zip(positives, overlapping))
        spread = [next(found) if slot else (None, None) for slot in slots] or [(None, None)]
    return [p for p, _ in spread], [n for _, n in spread]


def get_in_boxes_info(boxes, target_gts, expanded_strides):
    """(query centre inside ANY target box or ANY target centre square) [Q], (inside box AND centre square) [Q, G]: the matcher's."""
    return HungarianMatcherVL.get_in_boxes_info(None, boxes, target_gts, expanded_strides)


def dynamic_k_matching(cost, pair_wise_ious, num_gt, n_candidate_k):
    """Per target a [Q] bool mask of the queries assigned to it: k_g = max(int(sum of the target's n_candidate_k best IoUs), 1)
    cheapest queries claim target g; a query claimed by several targets keeps its cheapest; a target left without a query takes
    its cheapest query after every taken row was made 100000 dearer.  `cost` is modified in place (the second call of
    get_pos_idx depends on it).  One top-k over all columns and a rank mask stand in for a top-k per target (k_g <= n_candidate_k)."""
    ks = torch.topk(pair_wise_ious, n_candidate_k, dim=0).values.sum(0).int().clamp(min=1)
    cheapest_first = torch.topk(cost, n_candidate_k, dim=0, largest=False).indices            # [n_candidate_k, G]
    within_k = torch.arange(n_candidate_k, device=cost.device)[:, None] < ks[None, :]
    claimed = torch.zeros(cost.shape, dtype=torch.bool, device=cost.device).scatter_(0, cheapest_first, within_k)

    contested = claimed.sum(1) > 1              # decided HERE and not again inside the loop: the reference's quirk, kept

    def settle():
        keep = cost[contested].min(dim=1).indices
        claimed[contested] = False
        claimed[contested.nonzero().squeeze(1), keep] = True

    if contested.any():
        settle()
    while True:
        orphans = (~claimed.any(0)).nonzero().squeeze(1)
        if orphans.numel() == 0:
            break
        cost[claimed.any(1)] += OTA_TAKEN_PENALTY
        for g in orphans.tolist():
            claimed[cost[:, g].argmin(), g] = True
        if (claimed.sum(1) > 1).any():
            settle()
    return [claimed[:, g] for g in range(num_gt)]


# ---- the fused route ----------------------------------------------------------------------------------------------------------
def _plain(t, dtypes, dim=None):
    return torch.is_tensor(t) and t.is_cuda and t.dtype in dtypes and t.is_contiguous() and (dim is None or t.dim() == dim)


def _fusable(ref_box, all_indices, targets, ref_embeds, key_embeds, ref_cls):
    f32 = (torch.float32,)
    if not (_plain(ref_box, f32, 3) and _plain(ref_cls, f32, 3) and _plain(ref_embeds, f32, 3) and _plain(key_embeds, f32, 3)):
        return False
    bs, Q, C = ref_embeds.shape
    dev = ref_embeds.device
    if not (0 < bs <= _lib.OTA_MAX_BATCH and _lib.REID_MIN_QUERIES <= Q <= _lib.REID_MAX_QUERIES and C % 64 == 0 and 0 < C <= _lib.REID_MAX_DIM):
        return False
    T = ref_cls.shape[2]
    if not (tuple(ref_box.shape) == (bs, Q, 4) and tuple(ref_cls.shape) == (bs, Q, T) and key_embeds.shape[0] == bs
            and key_embeds.shape[1] > 0 and key_embeds.shape[2] == C and len(targets) == bs
            and ref_box.device == dev and ref_cls.device == dev and key_embeds.device == dev):
        return False
    total = 0
    for v, indices in zip(targets, all_indices):
        n = len(v["labels"])
        total += n
        if n == 0:
            continue
        pm, tb, valid = v["positive_map"], v["boxes"], v["valid"]
        if not (torch.is_tensor(pm) and pm.device == dev and pm.dtype in (torch.bool, torch.uint8) and tuple(pm.shape) == (n, T) and n <= 4096
                and torch.is_tensor(tb) and tb.device == dev and tb.dtype == torch.float32 and tb.numel() == 4 * n
                and torch.is_tensor(valid) and valid.device == dev and valid.dtype in (torch.bool, torch.uint8) and valid.numel() == n
                and torch.is_tensor(indices) and indices.device == dev and indices.dtype == torch.int64 and indices.numel() == n):
            return False      # (host-side index lists, index-valued positive maps, other dtypes: the composition)
    return total > 0


def _select_device_launch(ref_box, all_indices, targets, ref_cls, num_key_queries):
    """Everything of the selection that runs on the device, WITHOUT the host copy: (sizes, key_index, valid, matching_pos,
    matching_neg, words) -- see uninext_amd.ext.reid_select."""
    with torch.no_grad():
        prob = ref_cls
        neg = (1 - FOCAL_ALPHA) * (prob ** FOCAL_GAMMA) * (-(1 - prob + 1e-8).log())       # pos_neg_select.py:113-114, all images at once
        pos = FOCAL_ALPHA * ((1 - prob) ** FOCAL_GAMMA) * (-(prob + 1e-8).log())
        table = pos - neg
        sizes = [len(v["labels"]) for v in targets]
        have = [(v, idx, n) for v, idx, n in zip(targets, all_indices, sizes) if n > 0]
        gt_boxes = torch.cat([v["boxes"].reshape(n, 4) for v, _, n in have]).contiguous()
        pm = torch.cat([v["positive_map"] for v, _, _ in have]).contiguous()
        valid = torch.cat([v["valid"].reshape(n) for v, _, n in have]).ne(0).to(torch.uint8)
        key_index = torch.cat([idx.reshape(n) for _, idx, n in have]).contiguous()
        _, _, _, mpos, mneg, words = ext.reid_select(table, ref_box, gt_boxes, pm, valid, key_index, sizes, num_key_queries)
    return sizes, key_index, valid, mpos, mneg, words


_STAGING = {}               # device -> [pinned int32 buffer, event behind its last upload]


def _upload(words, dev):
    """`words` (Python ints) as an int32 tensor on `dev` through a cached pinned staging buffer, without blocking: the buffer only
    grows (to the next power of two), so pinned memory is allocated a handful of times in a process, not once per call or size."""
    n = len(words)
    slot = _STAGING.get(dev)
    if slot is None or slot[0].numel() < n:
        slot = _STAGING[dev] = [torch.empty(max(1024, 1 << (n - 1).bit_length()), dtype=torch.int32).pin_memory(), torch.cuda.Event()]
    else:
        slot[1].synchronize()                              # the previous upload has left the buffer (long since: a host copy lies between)
    slot[0][:n] = torch.tensor(words, dtype=torch.int32)
    up = slot[0][:n].to(dev, non_blocking=True)
    slot[1].record(torch.cuda.current_stream(dev))
    return up


def _select_fused(ref_box, all_indices, targets, ref_embeds, key_embeds, ref_cls):
    dev = ref_embeds.device
    sizes, key_index, valid, mpos, mneg, words = _select_device_launch(ref_box, all_indices, targets, ref_cls, key_embeds.shape[1])
    host = _host_copy(words).tolist()                      # THE host synchronisation of the call
    total = sum(sizes)
    stats = host[2 * total:]
    if any(s & 4 for s in stats):
        # generalized_box_iou's asserts (util/box_ops.py:76-77): same exception, raised behind the one host copy
        raise AssertionError("select_pos_neg: degenerate box (x1 < x0, y1 < y0 or NaN) in image(s) %s" % [b for b, s in enumerate(stats) if s & 4])
    if any(s & 2 for s in stats):
        raise RuntimeError("select_pos_neg: the repair loop of dynamic_k_matching did not terminate (the reference would spin)")
    if any(s & 8 for s in stats):
        raise IndexError("select_pos_neg: an index of all_indices is out of range for the key embeddings")
    items, ranks, target = [], [], 0
    for b, n in enumerate(sizes):
        for _ in range(n):
            n_pos, n_neg = host[2 * target], host[2 * target + 1]
            if n_pos >= 0:                                 # (-1: not valid)
                drawn = random.sample(list(range(0, n_neg)), _num_sample_neg(n_pos, n_neg))
                items.append((b, target, len(ranks), len(drawn), n_pos + len(drawn)))
                ranks.extend(drawn)
            target += 1
    flat = [x for it in items for x in it] + (ranks if ranks else [0])
    up = _upload(flat, dev)                                # the drawn ranks go up as one array
    n = len(items)
    return PackedContrastItems(ref_embeds, key_embeds, sizes, key_index, valid, mpos, mneg, up[:n * _lib.REID_META].view(n, _lib.REID_META),
                               up[n * _lib.REID_META:], items, ranks)


class ReidLossFunction(torch.autograd.Function):
    """(loss_reid, loss_reid_aux) of the packed items.  Gradients to ref_embeds [bs, Q, C] and key_embeds [bs, Qk, C]."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, ref_embeds, key_embeds, packed):
        ref_embeds, key_embeds = ref_embeds.contiguous(), key_embeds.contiguous()
        dot, cos, ref_norm, key_norm = ext.reid_scores(ref_embeds, key_embeds, packed.key_index, packed.valid, packed.sizes)
        losses, roles, stats = ext.reid_loss_forward(dot, cos, packed.matching_pos, packed.matching_neg, packed.item_meta, packed.ranks,
                                                     packed.sizes, ref_embeds.shape[1])
        ctx.save_for_backward(ref_embeds, key_embeds, dot, cos, ref_norm, key_norm, roles, stats)
        ctx.packed = packed
        return losses[0], losses[1]

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_loss, grad_aux):
        ref_embeds, key_embeds, dot, cos, ref_norm, key_norm, roles, stats = ctx.saved_tensors
        p = ctx.packed
        grads = torch.stack([torch.zeros((), device=ref_embeds.device) if g is None else g.detach().to(torch.float32).reshape(())
                             for g in (grad_loss, grad_aux)])
        grad_ref, grad_key = ext.reid_loss_backward(ref_embeds, key_embeds, p.key_index, dot, cos, ref_norm, key_norm, roles, stats,
                                                    p.item_meta, p.item_counts, grads, p.sizes)
        return grad_ref, grad_key, None


def loss_reid(outputs, targets, indices, num_boxes):
    """{'loss_reid', 'loss_reid_aux'} of outputs['pred_qd'] (the result of select_pos_neg); without items both are
    outputs['reid_params'] * 0 (deformable_detr.py:529-565)."""
    qd_items = outputs['pred_qd']
    if len(qd_items) == 0:
        return {'loss_reid': outputs['reid_params'] * 0, 'loss_reid_aux': outputs['reid_params'] * 0}
    if isinstance(qd_items, PackedContrastItems):
        loss, aux = ReidLossFunction.apply(qd_items.ref_embeds, qd_items.key_embeds, qd_items)
        return {'loss_reid': loss, 'loss_reid_aux': aux}
    terms, aux_terms = [], []
    for item in qd_items:
        scores, is_pos = item['contrast'][:, 0], item['label'] == 1
        # log(1 + sum over (positive, negative) pairs of e^(neg - pos)): only the pairs, and the 0 of the "1"
        pairs = (scores[~is_pos][None, :] - scores[is_pos][:, None]).reshape(-1)
        terms.append(torch.logsumexp(torch.cat([pairs, pairs.new_zeros(1)]), dim=0))
        aux_terms.append(((item['aux_consin'][:, 0] - item['aux_label']) ** 2).mean())
    return {'loss_reid': torch.stack(terms).sum() / len(qd_items), 'loss_reid_aux': torch.stack(aux_terms).sum() / len(qd_items)}


class _ReidLosses:
    """`"reid"` accepted in `losses` and dispatched to loss_reid; nothing else of the criterion changes (its `_forward` already
    skips `reid` for the auxiliary and the encoder outputs)."""

    def __init__(self, matcher, weight_dict, losses, focal_alpha=0.25, mask_out_stride=4, ota=False, still_cls_for_encoder=False, cfg=None):
        super().__init__(matcher, weight_dict, [loss for loss in losses if loss != "reid"], focal_alpha=focal_alpha,
                         mask_out_stride=mask_out_stride, ota=ota, still_cls_for_encoder=still_cls_for_encoder, cfg=cfg)
        self.losses = losses

    def loss_reid(self, outputs, targets, indices, num_boxes):
        return loss_reid(outputs, targets, indices, num_boxes)


class VideoSetCriterion(_ReidLosses, SetCriterion):
    """SetCriterion for the video configs: `losses` may hold "reid"."""


class VideoDINOCriterion(_ReidLosses, DINOCriterion):
    """DINOCriterion for the video configs: `losses` may hold "reid"."""
