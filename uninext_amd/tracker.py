"""The online trackers of video inference: `IDOL_Tracker` (models/tracker.py:50-298), which `UNINEXT_VID.inference_vis` calls
once per frame (the vis19 / vis21 / ovis routes), and `QuasiDenseEmbedTracker` (:304-503), which `inference_mot` calls on the
bdd_track route (BDD100K MOT and MOTS).

`IDOL_Tracker.fused` selects between two routes.  Off, `match` is the reference's composition: a dict of tracklets in
insertion order and Python loops, on the CPU or the GPU, with this package's `mask_nms` for the pre-NMS.  On, for fp32 GPU
inputs with match_metric 'bisoftmax', at most MASKPOST_HIP_MAX_MASKS detections, an embedding width of at most 256 and a memory
that stays within `capacity` slots, the memory bank lives in two preallocated device buffers (uninext_amd.ext.TrackState) and
a call is the kernels of include/dynmask_hip.h (maskpost_pack / maskpost_nms for the pre-NMS, track_hip_scores,
track_hip_associate, track_hip_update) with ONE host copy: the keep flags, the ids and the two counters in one buffer.
Anything else takes the composition; a live device bank is first written out into the dict, so a video may cross a limit
without losing an identity.  `tracklets`, `backdrops` and `memo` are built from the device state when they are read; nothing
in `match` reads them.  Conventions: DESIGN.md "Online tracker".

`QuasiDenseEmbedTracker.fused` does the same for the QuasiDense tracker: off, the reference's composition with a restated
`bbox_overlaps`; on, under the conditions of `QuasiDenseEmbedTracker._takes_fused`, the tracklets AND the backdrop ring live in
two device buffers (uninext_amd.ext.QDTrackState) and a call is qdtrack_hip_prepare (score order, box IoU, the pre-NMS' flags),
qdtrack_hip_scores, qdtrack_hip_associate and qdtrack_hip_update with one host copy.  Conventions: DESIGN.md "Online tracker",
"The QuasiDense tracker".
"""
import warnings

import torch
import torch.nn.functional as F

from . import ext as MSDA
from .postprocess import mask_iou, mask_nms

MATCH_METRICS = ("bisoftmax", "softmax", "cosine")


def temporal_weights(length):
    """The reference's `torch.range(0.0, 1, 1 / length)[1:]` (tracker.py:183), the deprecation warning aside."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return torch.range(0.0, 1, 1 / length)[1:]


def temporal_table(memory_len):
    """[memory_len + 1, memory_len] fp32, row `length` holding temporal_weights(length), or None when some length does not give
    `length` entries (the reference would fail to broadcast there; such a configuration is left to the composition)."""
    table = torch.zeros(memory_len + 1, memory_len, dtype=torch.float32)
    for length in range(1, memory_len + 1):
        w = temporal_weights(length)
        if w.numel() != length:
            return None
        table[length, :length] = w
    return table


class _Bank:
    """A tracker's device memory bank: two states that a call reads and writes in turn, the host's copy of the live count, and
    the tracker's extras (IDOL: `temporal`, the table on the device or None; QuasiDense: `backdrops`, the host's copy of the
    backdrop frames' rows, newest first)."""

    def __init__(self, make_state, device, D, **extras):
        self.states = [make_state(), make_state()]
        self.count = 0
        self.device, self.D = device, D
        self.__dict__.update(extras)

    def swap(self):
        self.states.reverse()

    def takes(self, n, D, device, capacity):
        return self.device == device and self.D == D and self.count + n <= capacity


def _fused_inputs(tracker, bboxes, labels, embeds, frame_id, indices):
    """What both trackers' `_takes_fused` ask first: `fused` and the bisoftmax metric, an int frame_id, fp32 [n, 5] boxes on a
    GPU with fp32 [n, D] embeddings, int64 [n] labels and n indices on the same device, and no autograd."""
    if not tracker.fused or tracker.match_metric != 'bisoftmax' or not isinstance(frame_id, int) or isinstance(frame_id, bool):
        return False
    if not (bboxes.is_cuda and bboxes.dim() == 2 and bboxes.shape[1] == 5 and embeds.dim() == 2 and labels.dim() == 1):
        return False
    n, dev = embeds.shape[0], bboxes.device
    if not (bboxes.shape[0] == n and labels.shape[0] == n and len(indices) == n
            and bboxes.dtype == embeds.dtype == torch.float32 and labels.dtype == torch.int64
            and embeds.device == dev and labels.device == dev):
        return False
    return not (torch.is_grad_enabled() and (bboxes.requires_grad or embeds.requires_grad))


class IDOL_Tracker(object):
    """IDOL_Tracker(...)(the reference's arguments and defaults, tracker.py:52-70; `capacity` the slots of the device bank,
    `fused` None for the class default).  bboxes, labels, ids, indices = match(bboxes [n, 5], labels [n], masks [n, 1, h, w] mask
    logits, track_feats [n, D], frame_id, indices (a list of n)): the detections the pre-NMS keeps, `ids` int64 on the CPU (>= 0
    a tracklet, -1 a backdrop, -2 neither), `indices` a Python list."""

    # The kernels' route, on by default: 0.25 / 0.42 ms per frame at about 30 / 100 detections of 200x336 logits against 6.4 / 16.1 ms
    # for the composition on an MI355X, 0.26 / 0.47 ms against 9.5 / 29.6 ms with the long-match flags, 1 host synchronisation
    # per frame against 178 - 895 (profiles/r20_tracker.txt, tools/tracker_bench.py).  Off the GPU, for other dtypes or metrics
    # and beyond the kernels' sizes a call takes the composition whatever this says.
    fused = True

    def __init__(self,
                 nms_thr_pre=0.7,
                 nms_thr_post=0.3,
                 init_score_thr=0.2,
                 addnew_score_thr=0.5,
                 obj_score_thr=0.1,
                 match_score_thr=0.5,
                 memo_tracklet_frames=10,
                 memo_backdrop_frames=1,
                 memo_momentum=0.5,
                 nms_conf_thr=0.5,
                 nms_backdrop_iou_thr=0.5,
                 nms_class_iou_thr=0.7,
                 with_cats=True,
                 match_metric='bisoftmax',
                 long_match=False,
                 frame_weight=False,
                 temporal_weight=False,
                 memory_len=10,
                 capacity=1024,
                 fused=None):
        assert 0 <= memo_momentum <= 1.0
        assert memo_tracklet_frames >= 0
        assert memo_backdrop_frames >= 0
        self.memory_len = memory_len
        self.temporal_weight = temporal_weight
        self.long_match = long_match
        self.frame_weight = frame_weight
        self.nms_thr_pre = nms_thr_pre
        self.nms_thr_post = nms_thr_post
        self.init_score_thr = init_score_thr
        self.addnew_score_thr = addnew_score_thr
        self.obj_score_thr = obj_score_thr
        self.match_score_thr = match_score_thr
        self.memo_tracklet_frames = memo_tracklet_frames
        self.memo_backdrop_frames = memo_backdrop_frames
        self.memo_momentum = memo_momentum
        self.nms_conf_thr = nms_conf_thr
        self.nms_backdrop_iou_thr = nms_backdrop_iou_thr
        self.nms_class_iou_thr = nms_class_iou_thr
        self.with_cats = with_cats
        assert match_metric in MATCH_METRICS
        self.match_metric = match_metric
        self.capacity = int(capacity)
        if fused is not None:
            self.fused = bool(fused)

        self.num_tracklets = 0
        self._tracklets = dict()
        self._backdrops = []       # dicts, or (bboxes, embeds, labels, kept rows, ids) of a fused frame until they are read
        self._bank = None
        self._temporal = None      # the table of temporal_table(), False when it cannot be built

    # ------------------------------------------------------------------ state, as the reference names it
    @property
    def empty(self):
        if self._bank is not None:
            return self._bank.count == 0
        return False if self._tracklets else True

    @property
    def tracklets(self):
        """{id: dict(bbox, embed, long_embed, long_score, label, last_frame, velocity, acc_frame, exist_frame)} in insertion
        order; read from the device bank while that is live (a host synchronisation)."""
        return self._bank_tracklets() if self._bank is not None else self._tracklets

    @tracklets.setter
    def tracklets(self, value):
        self._bank = None
        self._tracklets = value

    @property
    def backdrops(self):
        for k, b in enumerate(self._backdrops):
            if not isinstance(b, dict):
                bboxes, embeds, labels, kept, ids = b
                rows = kept[(ids == -1).to(kept.device)]
                self._backdrops[k] = dict(bboxes=bboxes[rows], embeds=embeds[rows], labels=labels[rows])
        return self._backdrops

    @backdrops.setter
    def backdrops(self, value):
        self._backdrops = value

    def _bank_tracklets(self):
        bank = self._bank
        M, s = bank.count, bank.states[0]
        ids, lens = s.id[:M].tolist(), s.long_len[:M].tolist()
        last, acc, exist = s.last_frame[:M].tolist(), s.acc_frame[:M].tolist(), s.exist_frame[:M].tolist()
        bbox, embed, label, velocity = s.bbox[:M].clone(), s.embed[:M].clone(), s.label[:M].clone(), s.velocity[:M].clone()
        long_embed, long_score = s.long_embed[:M].clone(), s.long_score[:M].clone()
        return {ids[m]: dict(bbox=bbox[m], embed=embed[m], long_embed=list(long_embed[m, :lens[m]].unbind(0)),
                             long_score=list(long_score[m, :lens[m]].unbind(0)), label=label[m], last_frame=last[m],
                             velocity=velocity[m], acc_frame=acc[m], exist_frame=exist[m]) for m in range(M)}

    def _materialise(self):
        """Write the device bank out into the dict of tracklets; the composition goes on from there."""
        if self._bank is not None:
            tracklets = self._bank_tracklets()
            self._backdrops = list(self.backdrops)
            self._bank = None
            self._tracklets = tracklets

    # ------------------------------------------------------------------ the reference's composition (tracker.py:102-298)
    def update_memo(self, ids, bboxes, embeds, labels, frame_id):
        self._materialise()
        tracklets = self._tracklets
        tracklet_inds = ids > -1
        for id, bbox, embed, label in zip(ids[tracklet_inds], bboxes[tracklet_inds], embeds[tracklet_inds], labels[tracklet_inds]):
            id = int(id)
            if id in tracklets:
                t = tracklets[id]
                velocity = (bbox - t['bbox']) / (frame_id - t['last_frame'])
                t['bbox'] = bbox
                t['long_score'].append(bbox[-1])
                t['embed'] = (1 - self.memo_momentum) * t['embed'] + self.memo_momentum * embed
                t['long_embed'].append(embed)
                t['last_frame'] = frame_id
                t['label'] = label
                t['velocity'] = (t['velocity'] * t['acc_frame'] + velocity) / (t['acc_frame'] + 1)
                t['acc_frame'] += 1
                t['exist_frame'] += 1
            else:
                tracklets[id] = dict(bbox=bbox, embed=embed, long_embed=[embed], long_score=[bbox[-1]], label=label,
                                     last_frame=frame_id, velocity=torch.zeros_like(bbox), acc_frame=0, exist_frame=1)

        backdrop_inds = torch.nonzero(ids == -1, as_tuple=False).squeeze(1)
        self._backdrops.insert(0, dict(bboxes=bboxes[backdrop_inds], embeds=embeds[backdrop_inds], labels=labels[backdrop_inds]))

        invalid_ids = []
        for k, v in tracklets.items():
            if frame_id - v['last_frame'] >= self.memo_tracklet_frames:
                invalid_ids.append(k)
            if len(v['long_embed']) > self.memory_len:
                v['long_embed'].pop(0)
            if len(v['long_score']) > self.memory_len:
                v['long_score'].pop(0)
        for invalid_id in invalid_ids:
            tracklets.pop(invalid_id)
        if len(self._backdrops) > self.memo_backdrop_frames:
            self._backdrops.pop()

    @property
    def memo(self):
        """(bboxes [M, 5], labels [M], embeds [M, D] the matching embeddings, ids [M] int64 on the CPU, velocities [M, 5], the
        rings' embeddings (a list of [len, D]), their scores (a list of [len]), exist_frame [M] int64 on the CPU)."""
        memo_embeds, memo_ids, memo_bboxes, memo_labels, memo_vs = [], [], [], [], []
        memo_long_embeds, memo_long_score, memo_exist_frame = [], [], []
        for k, v in self.tracklets.items():
            memo_bboxes.append(v['bbox'][None, :])
            if self.long_match:
                weights = torch.stack(v['long_score'])
                if self.temporal_weight:
                    weights = weights + temporal_weights(len(weights)).to(weights)
                memo_embeds.append(((torch.stack(v['long_embed']) * weights.unsqueeze(1)).sum(0) / weights.sum())[None, :])
            else:
                memo_embeds.append(v['embed'][None, :])
            memo_long_embeds.append(torch.stack(v['long_embed']))
            memo_long_score.append(torch.stack(v['long_score']))
            memo_exist_frame.append(v['exist_frame'])
            memo_ids.append(k)
            memo_labels.append(v['label'].view(1, 1))
            memo_vs.append(v['velocity'][None, :])
        memo_ids = torch.tensor(memo_ids, dtype=torch.long).view(1, -1)
        memo_exist_frame = torch.tensor(memo_exist_frame, dtype=torch.long)
        memo_bboxes = torch.cat(memo_bboxes, dim=0)
        memo_embeds = torch.cat(memo_embeds, dim=0)
        memo_labels = torch.cat(memo_labels, dim=0).squeeze(1)
        memo_vs = torch.cat(memo_vs, dim=0)
        return (memo_bboxes, memo_labels, memo_embeds, memo_ids.squeeze(0), memo_vs, memo_long_embeds, memo_long_score,
                memo_exist_frame)

    def _number_new(self, ids, new_inds):
        num_news = int(new_inds.sum())
        ids[new_inds] = torch.arange(self.num_tracklets, self.num_tracklets + num_news, dtype=torch.long)
        self.num_tracklets += num_news

    def _mark_backdrops(self, ids, masks):
        unselected_inds = torch.nonzero(ids == -2, as_tuple=False).squeeze(1)
        mask_ious = mask_iou(masks[unselected_inds].sigmoid() > 0.5, masks.permute(1, 0, 2, 3).sigmoid() > 0.5)
        for i, ind in enumerate(unselected_inds):
            if (mask_ious[i, :ind] < self.nms_thr_post).all():
                ids[ind] = -1

    def _match_composition(self, bboxes, labels, masks, embeds, frame_id, indices):
        valids = mask_nms(masks, bboxes[:, -1], None, self.nms_thr_pre)
        indices = torch.tensor(indices)[valids].tolist()
        bboxes = bboxes[valids, :]
        labels = labels[valids]
        masks = masks[valids]
        embeds = embeds[valids, :]
        ids = torch.full((bboxes.size(0), ), -2, dtype=torch.long)

        if bboxes.size(0) > 0 and not self.empty:
            (memo_bboxes, memo_labels, memo_embeds, memo_ids, memo_vs, memo_long_embeds, memo_long_score,
             memo_exist_frame) = self.memo
            memo_exist_frame = memo_exist_frame.to(memo_embeds)
            memo_ids = memo_ids.to(memo_embeds)
            if self.match_metric == 'bisoftmax':
                feats = torch.mm(embeds, memo_embeds.t())
                scores = (feats.softmax(dim=1) + feats.softmax(dim=0)) / 2
            elif self.match_metric == 'softmax':
                scores = torch.mm(embeds, memo_embeds.t()).softmax(dim=1)
            elif self.match_metric == 'cosine':
                scores = torch.mm(F.normalize(embeds, p=2, dim=1), F.normalize(memo_embeds, p=2, dim=1).t())
            else:
                raise NotImplementedError
            for i in range(bboxes.size(0)):
                row = scores[i, :]
                if self.frame_weight:
                    non_backs = (memo_ids > -1) & (row > 0.5)
                    if (row[non_backs] > 0.5).sum() > 1:
                        weighted = row.clone()
                        frame_weight = memo_exist_frame[row[memo_ids > -1] > 0.5]
                        weighted[non_backs] = weighted[non_backs] * frame_weight
                        weighted[~non_backs] = weighted[~non_backs] * frame_weight.mean()
                        row = weighted
                conf, memo_ind = torch.max(row, dim=0)
                id = memo_ids[memo_ind]
                if conf > self.match_score_thr:
                    if id > -1:
                        ids[i] = id
                        scores[:i, memo_ind] = 0
                        scores[i + 1:, memo_ind] = 0
            self._number_new(ids, (ids == -2) & (bboxes[:, 4] > self.addnew_score_thr).cpu())
            self._mark_backdrops(ids, masks)
            self.update_memo(ids, bboxes, embeds, labels, frame_id)
        elif self.empty:
            self._number_new(ids, (ids == -2) & (bboxes[:, 4] > self.init_score_thr).cpu())
            self._mark_backdrops(ids, masks)
            self.update_memo(ids, bboxes, embeds, labels, frame_id)
        return bboxes, labels, ids, indices

    # ------------------------------------------------------------------ the kernels' route
    def _temporal_table(self):
        if self._temporal is None:
            table = temporal_table(self.memory_len) if 1 <= self.memory_len <= MSDA._lib.TRACK_MAX_MEMORY_LEN else None
            self._temporal = False if table is None else table
        return self._temporal

    def _takes_fused(self, bboxes, labels, masks, embeds, frame_id, indices):
        """True when the kernels take the call (the conditions of the module's docstring)."""
        if not _fused_inputs(self, bboxes, labels, embeds, frame_id, indices):
            return False
        n, D = embeds.shape
        dev = bboxes.device
        if not (masks.dim() == 4 and masks.shape[1] == 1 and masks.shape[0] == n and masks.dtype == torch.float32
                and masks.device == dev and not (torch.is_grad_enabled() and masks.requires_grad)):
            return False
        if not (MSDA.track_supported(n, self.capacity, D, self.memory_len) and masks.shape[2] * masks.shape[3] < 1 << 30
                and masks.numel() < 1 << 31 and 0 <= self.match_score_thr and abs(frame_id) < 1 << 30
                and self.memo_tracklet_frames < 1 << 30):
            return False
        if self.long_match and self.temporal_weight and self._temporal_table() is False:
            return False
        if self._bank is None:
            return not self._tracklets and n <= self.capacity        # a dict that is in use stays the memory
        return self._bank.takes(n, D, dev, self.capacity)

    def _match_fused(self, bboxes, labels, masks, embeds, frame_id, indices):
        n, D = embeds.shape
        dev = bboxes.device
        if n == 0:             # the reference updates nothing, but for the empty backdrop of an empty memory (tracker.py:281-294)
            if self.empty:
                self._push_backdrop(dict(bboxes=bboxes, embeds=embeds, labels=labels))
            return bboxes, labels, torch.full((0,), -2, dtype=torch.long), []
        with torch.no_grad():
            if self._bank is None:
                temporal = self._temporal_table() if self.long_match and self.temporal_weight else None
                self._bank = _Bank(lambda: MSDA.TrackState(self.capacity, D, self.memory_len, dev), dev, D,
                                   temporal=None if temporal is None else temporal.to(dev))
                self._bank.states[0].meta[1:].fill_(self.num_tracklets)
            bank = self._bank
            cur, nxt = bank.states
            M = bank.count
            bboxes, embeds, labels = bboxes.contiguous(), embeds.contiguous(), labels.contiguous()
            bits, area = MSDA.maskpost_pack(masks[:, 0].contiguous(), torch.arange(n, dtype=torch.int64, device=dev))
            inter, keep = MSDA.maskpost_nms(bits, area, self.nms_thr_pre)
            scores = MSDA.track_scores(embeds, keep, cur, M, self.long_match, bank.temporal) if M > 0 else None
            plan, result = MSDA.track_associate(scores, keep, bboxes, inter, area, cur, nxt, M, self.frame_weight,
                                                self.match_score_thr, self.addnew_score_thr if M > 0 else self.init_score_thr,
                                                self.nms_thr_post, frame_id, self.memo_tracklet_frames)
            MSDA.track_update(embeds, bboxes, labels, plan, result, cur, nxt, M, self.memo_momentum, frame_id)
            host = result[:2 * n + 2].tolist()         # the one host copy
            bank.swap()
            bank.count, self.num_tracklets = host[2 * n], host[2 * n + 1]
            kept = [i for i in range(n) if host[i]]
            ids = torch.tensor([host[n + i] for i in kept], dtype=torch.long)
            rows = kept_rows = result[2 * n + 2:2 * n + 2 + len(kept)]      # on the device: no second copy
            out_bboxes, out_labels = bboxes.index_select(0, rows), labels.index_select(0, rows)
            self._push_backdrop((bboxes, embeds, labels, kept_rows, ids))
            return out_bboxes, out_labels, ids, [indices[i] for i in kept]

    def _push_backdrop(self, entry):
        self._backdrops.insert(0, entry)
        if len(self._backdrops) > self.memo_backdrop_frames:
            self._backdrops.pop()

    def match(self, bboxes, labels, masks, track_feats, frame_id, indices):
        if self._takes_fused(bboxes, labels, masks, track_feats, frame_id, indices):
            return self._match_fused(bboxes, labels, masks, track_feats, frame_id, indices)
        self._materialise()
        return self._match_composition(bboxes, labels, masks, track_feats, frame_id, indices)


def bbox_overlaps(bboxes1, bboxes2, eps=1e-6):
    """mmcv's bbox_overlaps(mode='iou', is_aligned=False) (util/mmcv_utils.py:146-191) for [m, 4] and [n, 4] boxes: [m, n]."""
    assert bboxes1.size(-1) == 4 or bboxes1.size(0) == 0
    assert bboxes2.size(-1) == 4 or bboxes2.size(0) == 0
    rows, cols = bboxes1.size(-2), bboxes2.size(-2)
    if rows * cols == 0:
        return bboxes1.new_zeros((rows, cols))
    area1 = (bboxes1[..., 2] - bboxes1[..., 0]) * (bboxes1[..., 3] - bboxes1[..., 1])
    area2 = (bboxes2[..., 2] - bboxes2[..., 0]) * (bboxes2[..., 3] - bboxes2[..., 1])
    lt = torch.max(bboxes1[..., :, None, :2], bboxes2[..., None, :, :2])
    rb = torch.min(bboxes1[..., :, None, 2:], bboxes2[..., None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    overlap = wh[..., 0] * wh[..., 1]
    union = area1[..., None] + area2[..., None, :] - overlap
    union = torch.max(union, union.new_tensor([eps]))
    return overlap / union


class QuasiDenseEmbedTracker(object):
    """QuasiDenseEmbedTracker(...)(the reference's arguments and defaults, tracker.py:306-317; `capacity` the tracklet slots and
    `backdrop_capacity` the rows per backdrop frame of the device bank, `fused` None for the class default).  bboxes, labels, ids,
    indices = match(bboxes [n, 5], labels [n], track_feats [n, D], frame_id, indices (a list or a 1-D tensor of n)): the
    detections the box pre-NMS keeps, by descending score; `ids` int64 on the CPU (>= 0 a tracklet, -1 unmatched, -2 a low-scoring
    duplicate of a tracklet), `indices` a Python list."""

    # The kernels' route, on by default: 0.17 / 0.33 ms per frame at about 30 / 100 detections against 6.0 / 16.6 ms for the
    # composition on an MI355X with the bdd_track arguments, the p10 .. p90 ranges far apart, 1 host synchronisation per frame
    # against 155 / 621, the same ids and indices on every frame (profiles/r22_qdtrack.txt, tools/qdtrack_bench.py).  Off the
    # GPU, for other dtypes or metrics and beyond the kernels' sizes a call takes the composition whatever this says.
    fused = True

    def __init__(self,
                 init_score_thr=0.8,
                 obj_score_thr=0.5,
                 match_score_thr=0.5,
                 memo_tracklet_frames=10,
                 memo_backdrop_frames=1,
                 memo_momentum=0.8,
                 nms_conf_thr=0.5,
                 nms_backdrop_iou_thr=0.3,
                 nms_class_iou_thr=0.7,
                 with_cats=True,
                 match_metric='bisoftmax',
                 capacity=1024,
                 backdrop_capacity=256,
                 fused=None):
        assert 0 <= memo_momentum <= 1.0
        assert memo_tracklet_frames >= 0
        assert memo_backdrop_frames >= 0
        self.init_score_thr = init_score_thr
        self.obj_score_thr = obj_score_thr
        self.match_score_thr = match_score_thr
        self.memo_tracklet_frames = memo_tracklet_frames
        self.memo_backdrop_frames = memo_backdrop_frames
        self.memo_momentum = memo_momentum
        self.nms_conf_thr = nms_conf_thr
        self.nms_backdrop_iou_thr = nms_backdrop_iou_thr
        self.nms_class_iou_thr = nms_class_iou_thr
        self.with_cats = with_cats
        assert match_metric in MATCH_METRICS
        self.match_metric = match_metric
        self.capacity = int(capacity)
        self.backdrop_capacity = int(backdrop_capacity)
        if fused is not None:
            self.fused = bool(fused)

        self.num_tracklets = 0
        self._tracklets = dict()
        self._backdrops = []
        self._bank = None
        self._last_frame = None    # the frame_id of the last call when it was an int

    # ------------------------------------------------------------------ state, as the reference names it
    @property
    def empty(self):
        if self._bank is not None:
            return self._bank.count == 0
        return False if self._tracklets else True

    @property
    def tracklets(self):
        """{id: dict(bbox, embed, label, last_frame, velocity, acc_frame)} in insertion order; read from the device bank while
        that is live (a host synchronisation)."""
        return self._bank_tracklets() if self._bank is not None else self._tracklets

    @tracklets.setter
    def tracklets(self, value):
        self._materialise()
        self._tracklets = value

    @property
    def backdrops(self):
        """[dict(bboxes, embeds, labels)], newest first; read from the device bank while that is live."""
        return self._bank_backdrops() if self._bank is not None else self._backdrops

    @backdrops.setter
    def backdrops(self, value):
        self._materialise()
        self._backdrops = value

    def _bank_tracklets(self):
        bank = self._bank
        M, s = bank.count, bank.states[0]
        ids, last, acc = s.id[:M].tolist(), s.last_frame[:M].tolist(), s.acc_frame[:M].tolist()
        bbox, embed, label, velocity = s.bbox[:M].clone(), s.embed[:M].clone(), s.label[:M].clone(), s.velocity[:M].clone()
        return {ids[m]: dict(bbox=bbox[m], embed=embed[m], label=label[m], last_frame=last[m], velocity=velocity[m],
                             acc_frame=acc[m]) for m in range(M)}

    def _bank_backdrops(self):
        s = self._bank.states[0]
        return [dict(bboxes=s.backdrop_bbox[k, :rows].clone(), embeds=s.backdrop_embed[k, :rows].clone(),
                     labels=s.backdrop_label[k, :rows].clone()) for k, rows in enumerate(self._bank.backdrops)]

    def _materialise(self):
        """Write the device bank out into the dict of tracklets and the list of backdrops; the composition goes on from there."""
        if self._bank is not None:
            tracklets, backdrops = self._bank_tracklets(), self._bank_backdrops()
            self._bank = None
            self._tracklets, self._backdrops = tracklets, backdrops

    # ------------------------------------------------------------------ the reference's composition (tracker.py:338-503)
    def update_memo(self, ids, bboxes, embeds, labels, frame_id):
        self._materialise()
        tracklets = self._tracklets
        tracklet_inds = (ids > -1).to(bboxes.device)
        for id, bbox, embed, label in zip(ids[ids > -1], bboxes[tracklet_inds], embeds[tracklet_inds], labels[tracklet_inds]):
            id = int(id)
            if id in tracklets:
                t = tracklets[id]
                velocity = (bbox - t['bbox']) / (frame_id - t['last_frame'])
                t['bbox'] = bbox
                t['embed'] = (1 - self.memo_momentum) * t['embed'] + self.memo_momentum * embed
                t['last_frame'] = frame_id
                t['label'] = label
                t['velocity'] = (t['velocity'] * t['acc_frame'] + velocity) / (t['acc_frame'] + 1)
                t['acc_frame'] += 1
            else:
                tracklets[id] = dict(bbox=bbox, embed=embed, label=label, last_frame=frame_id, velocity=torch.zeros_like(bbox),
                                     acc_frame=0)

        backdrop_inds = torch.nonzero(ids == -1, as_tuple=False).squeeze(1)
        ious = bbox_overlaps(bboxes[backdrop_inds.to(bboxes.device), :-1], bboxes[:, :-1])
        for i, ind in enumerate(backdrop_inds):
            if (ious[i, :ind] > self.nms_backdrop_iou_thr).any():
                backdrop_inds[i] = -1
        backdrop_inds = backdrop_inds[backdrop_inds > -1].to(bboxes.device)
        self._backdrops.insert(0, dict(bboxes=bboxes[backdrop_inds], embeds=embeds[backdrop_inds], labels=labels[backdrop_inds]))

        invalid_ids = []
        for k, v in tracklets.items():
            if frame_id - v['last_frame'] >= self.memo_tracklet_frames:
                invalid_ids.append(k)
        for invalid_id in invalid_ids:
            tracklets.pop(invalid_id)
        if len(self._backdrops) > self.memo_backdrop_frames:
            self._backdrops.pop()

    @property
    def memo(self):
        """(bboxes [M, 5], labels [M], embeds [M, D], ids [M] int64 on the CPU with -1 for a backdrop, velocities [M, 5]): the
        tracklets in insertion order, then the backdrop frames, newest first."""
        memo_embeds, memo_ids, memo_bboxes, memo_labels, memo_vs = [], [], [], [], []
        for k, v in self.tracklets.items():
            memo_bboxes.append(v['bbox'][None, :])
            memo_embeds.append(v['embed'][None, :])
            memo_ids.append(k)
            memo_labels.append(v['label'].view(1, 1))
            memo_vs.append(v['velocity'][None, :])
        memo_ids = torch.tensor(memo_ids, dtype=torch.long).view(1, -1)
        for backdrop in self.backdrops:
            backdrop_ids = torch.full((1, backdrop['embeds'].size(0)), -1, dtype=torch.long)
            memo_bboxes.append(backdrop['bboxes'])
            memo_embeds.append(backdrop['embeds'])
            memo_ids = torch.cat([memo_ids, backdrop_ids], dim=1)
            memo_labels.append(backdrop['labels'][:, None])
            memo_vs.append(torch.zeros_like(backdrop['bboxes']))
        memo_bboxes = torch.cat(memo_bboxes, dim=0)
        memo_embeds = torch.cat(memo_embeds, dim=0)
        memo_labels = torch.cat(memo_labels, dim=0).squeeze(1)
        memo_vs = torch.cat(memo_vs, dim=0)
        return memo_bboxes, memo_labels, memo_embeds, memo_ids.squeeze(0), memo_vs

    def _match_composition(self, bboxes, labels, track_feats, frame_id, indices):
        _, inds = bboxes[:, -1].sort(descending=True)
        bboxes = bboxes[inds, :]
        labels = labels[inds]
        embeds = track_feats[inds, :]

        valids = bboxes.new_ones((bboxes.size(0)))
        ious = bbox_overlaps(bboxes[:, :-1], bboxes[:, :-1])
        for i in range(1, bboxes.size(0)):
            thr = self.nms_backdrop_iou_thr if bboxes[i, -1] < self.obj_score_thr else self.nms_class_iou_thr
            if (ious[i, :i] > thr).any():
                valids[i] = 0
        valids = valids == 1
        # the reference indexes `indices` in their given order with the flags of the SORTED rows (tracker.py:448)
        indices = torch.as_tensor(indices).cpu()[valids.cpu()].tolist()
        bboxes = bboxes[valids, :]
        labels = labels[valids]
        embeds = embeds[valids, :]
        ids = torch.full((bboxes.size(0), ), -1, dtype=torch.long)

        if bboxes.size(0) > 0 and not self.empty:
            memo_bboxes, memo_labels, memo_embeds, memo_ids, memo_vs = self.memo
            if self.match_metric == 'bisoftmax':
                feats = torch.mm(embeds, memo_embeds.t())
                scores = (feats.softmax(dim=1) + feats.softmax(dim=0)) / 2
            elif self.match_metric == 'softmax':
                scores = torch.mm(embeds, memo_embeds.t()).softmax(dim=1)
            elif self.match_metric == 'cosine':
                scores = torch.mm(F.normalize(embeds, p=2, dim=1), F.normalize(memo_embeds, p=2, dim=1).t())
            else:
                raise NotImplementedError
            if self.with_cats:
                cat_same = labels.view(-1, 1) == memo_labels.view(1, -1)
                scores *= cat_same.float().to(scores.device)
            for i in range(bboxes.size(0)):
                conf, memo_ind = torch.max(scores[i, :], dim=0)
                id = memo_ids[int(memo_ind)]
                if conf > self.match_score_thr:
                    if id > -1:
                        if bboxes[i, -1] > self.obj_score_thr:
                            ids[i] = id
                            scores[:i, memo_ind] = 0
                            scores[i + 1:, memo_ind] = 0
                        else:
                            if conf > self.nms_conf_thr:
                                ids[i] = -2
        new_inds = (ids == -1) & (bboxes[:, 4] > self.init_score_thr).cpu()
        num_news = int(new_inds.sum())
        ids[new_inds] = torch.arange(self.num_tracklets, self.num_tracklets + num_news, dtype=torch.long)
        self.num_tracklets += num_news
        self.update_memo(ids, bboxes, embeds, labels, frame_id)
        return bboxes, labels, ids, indices

    # ------------------------------------------------------------------ the kernels' route
    def _takes_fused(self, bboxes, labels, embeds, frame_id, indices):
        """True when the kernels take the call: fp32 GPU inputs, match_metric 'bisoftmax', sizes within the limits of
        include/dynmask_hip.h, thresholds >= 0, an int frame_id above the last call's, no autograd, and a bank that stays
        within `capacity` tracklets and `backdrop_capacity` backdrops per frame."""
        if not _fused_inputs(self, bboxes, labels, embeds, frame_id, indices):
            return False
        n, D = embeds.shape
        dev = bboxes.device
        if not (MSDA.qdtrack_supported(n, self.capacity, D, self.backdrop_capacity, self.memo_backdrop_frames)
                and 0 <= self.match_score_thr and 0 <= self.nms_conf_thr and abs(frame_id) < 1 << 30
                and self.memo_tracklet_frames < 1 << 30 and n <= self.backdrop_capacity):
            return False
        if self._last_frame is not None and frame_id <= self._last_frame:
            return False
        if self._bank is None:     # a dict or a list that is in use stays the memory
            return not self._tracklets and not self._backdrops and n <= self.capacity
        return self._bank.takes(n, D, dev, self.capacity)

    def _match_fused(self, bboxes, labels, embeds, frame_id, indices):
        n, D = embeds.shape
        dev = bboxes.device
        K = self.memo_backdrop_frames
        with torch.no_grad():
            if self._bank is None:
                self._bank = _Bank(lambda: MSDA.QDTrackState(self.capacity, D, self.backdrop_capacity, K, dev), dev, D, backdrops=[])
                self._bank.states[0].meta[1:2].fill_(self.num_tracklets)
            bank = self._bank
            cur, nxt = bank.states
            M, drops = bank.count, bank.backdrops
            bboxes, embeds, labels = bboxes.contiguous(), embeds.contiguous(), labels.contiguous()
            order, iou, valid = MSDA.qdtrack_prepare(bboxes, self.obj_score_thr, self.nms_backdrop_iou_thr, self.nms_class_iou_thr)
            scores = MSDA.qdtrack_scores(embeds, labels, order, valid, cur, M, drops, self.with_cats) if M > 0 and n > 0 else None
            plan, result = MSDA.qdtrack_associate(scores, valid, order, bboxes, iou, cur, nxt, M, drops, self.match_score_thr,
                                                  self.obj_score_thr, self.nms_conf_thr, self.init_score_thr,
                                                  self.nms_backdrop_iou_thr, frame_id, self.memo_tracklet_frames)
            MSDA.qdtrack_update(embeds, bboxes, labels, order, plan, result, cur, nxt, M, drops, self.memo_momentum, frame_id)
            host = result[:3 * n + 4].tolist()         # the one host copy
            bank.swap()
            kept, bank.count, self.num_tracklets, new_drops = host[3 * n:]
            bank.backdrops = ([new_drops] + drops)[:K]
            rows = result[:kept]                       # on the device: no second copy
            ids = torch.tensor(host[n:n + kept], dtype=torch.long)
            return bboxes.index_select(0, rows), labels.index_select(0, rows), ids, [indices[r] for r in host[2 * n:2 * n + kept]]    # tracker.py:448

    def match(self, bboxes, labels, track_feats, frame_id, indices):
        if torch.is_tensor(indices):
            indices = indices.tolist()
        fused = self._takes_fused(bboxes, labels, track_feats, frame_id, indices)
        self._last_frame = frame_id if isinstance(frame_id, int) and not isinstance(frame_id, bool) else None
        if fused:
            return self._match_fused(bboxes, labels, track_feats, frame_id, indices)
        self._materialise()
        return self._match_composition(bboxes, labels, track_feats, frame_id, indices)
