"""QuasiDenseEmbedTracker.match + update_memo + memo (projects/UNINEXT/uninext/models/tracker.py:304-503, match_metric
'bisoftmax') with mmcv's bbox_overlaps (util/mmcv_utils.py:146-191), restated in float64 on numpy, written from the reference's
text like tests/tracker_ref.py: the yardstick the tracker's two routes are compared with.  Besides the reference's results a call
returns the SMALLEST MARGIN of every decision it took:

    |IoU - threshold| of every pair the pre-NMS reads (the threshold is the row's) and of every pair the backdrop filter reads;
    |score - obj_score_thr| of every row, |score - init_score_thr| of every row still -1 after the walk;
    the gap between adjacent sorted scores;
    |conf - match_score_thr| of every row the walk reaches, |conf - nms_conf_thr| where that is compared, and, when conf is above
    match_score_thr, the gap between the two largest entries of the row at the moment of its max (below the threshold nothing
    depends on WHICH column is the largest: the row stays -1 whichever it is).

A case whose margins stay above tests/tracker_cases.py: MARGIN cannot be decided differently by fp32 arithmetic.  `events` names
what a run reached; `columns` the memory's (tracklets, backdrops) at every walk."""
import numpy as np


def bbox_overlaps(a, b, eps=1e-6):
    area1 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt = np.maximum(a[:, None, :2], b[None, :, :2])
    rb = np.minimum(a[:, None, 2:], b[None, :, 2:])
    wh = np.clip(rb - lt, 0, None)
    overlap = wh[..., 0] * wh[..., 1]
    union = np.maximum(area1[:, None] + area2[None, :] - overlap, eps)
    return overlap / union


def _softmax(x, axis):
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


class RefTracker:
    def __init__(self, init_score_thr=0.8, obj_score_thr=0.5, match_score_thr=0.5, memo_tracklet_frames=10, memo_backdrop_frames=1,
                 memo_momentum=0.8, nms_conf_thr=0.5, nms_backdrop_iou_thr=0.3, nms_class_iou_thr=0.7, with_cats=True, **unused):
        self.__dict__.update(locals())
        self.num_tracklets = 0
        self.tracklets = {}
        self.backdrops = []
        self.events = []
        self.columns = []

    def memo(self):
        t, b = self.tracklets, self.backdrops
        D = next(iter(t.values()))["embed"].shape[0] if t else (b[0]["embeds"].shape[1] if b else 1)
        cat = lambda own, theirs, shape, dtype: np.concatenate(
            [np.asarray(own, dtype=dtype).reshape((-1,) + shape)] + [np.asarray(x, dtype=dtype).reshape((-1,) + shape) for x in theirs])
        return dict(bboxes=cat([v["bbox"] for v in t.values()], [x["bboxes"] for x in b], (5,), np.float64),
                    labels=cat([v["label"] for v in t.values()], [x["labels"] for x in b], (), np.int64),
                    embeds=cat([v["embed"] for v in t.values()], [x["embeds"] for x in b], (D,), np.float64),
                    ids=cat(list(t), [np.full(len(x["labels"]), -1) for x in b], (), np.int64),
                    vs=cat([v["velocity"] for v in t.values()], [np.zeros_like(x["bboxes"]) for x in b], (5,), np.float64),
                    last_frame=np.asarray([v["last_frame"] for v in t.values()], dtype=np.int64),
                    acc_frame=np.asarray([v["acc_frame"] for v in t.values()], dtype=np.int64),
                    backdrop_rows=np.asarray([len(x["labels"]) for x in b], dtype=np.int64))

    def match(self, bboxes, labels, embeds, frame_id, indices):
        """fp32 torch tensors in; (ids, indices, kept count, smallest margin, the sorted IoU matrix) out."""
        bboxes, embeds = bboxes.double().numpy(), embeds.double().numpy()
        labels = labels.numpy()
        margin = [np.inf]
        n = len(bboxes)
        inds = np.argsort(-bboxes[:, 4], kind="stable")
        bboxes, labels, embeds = bboxes[inds], labels[inds], embeds[inds]
        margin.extend(np.abs(np.diff(bboxes[:, 4])))
        margin.extend(np.abs(bboxes[:, 4] - self.obj_score_thr))
        ious = bbox_overlaps(bboxes[:, :4], bboxes[:, :4])
        valid = np.ones(n, dtype=bool)
        for i in range(1, n):
            thr = self.nms_backdrop_iou_thr if bboxes[i, 4] < self.obj_score_thr else self.nms_class_iou_thr
            margin.extend(np.abs(ious[i, :i] - thr))
            hits = ious[i, :i] > thr
            if hits.any():
                valid[i] = False
                if not valid[:i][hits].any():
                    self.events.append("dropped_by_dropped_rows_alone")
        if n > 1 and not valid[1:].any():
            self.events.append("all_but_the_first_dropped")
        indices = [indices[p] for p in range(n) if valid[p]]        # tracker.py:448: the given order, the sorted rows' flags
        bboxes, labels, embeds, iou_valid = bboxes[valid], labels[valid], embeds[valid], ious[valid][:, valid]
        k = len(bboxes)
        ids = [-1] * k
        if k > 0 and self.tracklets:
            slots = list(self.tracklets)
            M = len(slots)
            memo = self.memo()
            self.columns.append((M, len(memo["ids"]) - M))
            feats = embeds @ memo["embeds"].T
            assert np.abs(feats).max() <= 8.0 + 1e-9
            scores = (_softmax(feats, 1) + _softmax(feats, 0)) / 2
            same = labels[:, None] == memo["labels"][None, :]
            if (~same[np.arange(k), scores.argmax(1)] & (scores.max(1) > self.match_score_thr) & (scores.argmax(1) < M)).any():
                self.events.append("cross_class_best_column")
            if self.with_cats:
                scores = scores * same
            for i in range(k):
                row = scores[i]
                best = int(np.argmax(row))
                conf = row[best]
                margin.append(abs(conf - self.match_score_thr))
                if conf > self.match_score_thr:
                    if len(row) > 1:
                        margin.append(conf - np.partition(row, -2)[-2])
                    if best < M:
                        if bboxes[i, 4] > self.obj_score_thr:
                            ids[i] = slots[best]
                            others = np.arange(k) != i
                            if (scores[others, best] > self.match_score_thr).any():
                                self.events.append("column_zeroed_under_a_rival")
                            scores[others, best] = 0
                        else:
                            margin.append(abs(conf - self.nms_conf_thr))
                            if conf > self.nms_conf_thr:
                                ids[i] = -2
                                self.events.append("minus_two")
                    else:
                        self.events.append("best_column_is_a_backdrop")
                        if bboxes[i, 4] > self.init_score_thr:
                            self.events.append("backdrop_best_then_new_tracklet")
        elif k > 0 and any(len(b["labels"]) for b in self.backdrops):
            self.events.append("no_tracklets_while_backdrops_exist")
        started = 0
        for i in range(k):
            if ids[i] == -1:
                margin.append(abs(bboxes[i, 4] - self.init_score_thr))
                if bboxes[i, 4] > self.init_score_thr:
                    ids[i] = self.num_tracklets
                    self.num_tracklets += 1
                    started += 1
        if k > 0 and started == 0 and any(len(b["labels"]) for b in self.backdrops):
            self.events.append("starts_no_tracklet_while_backdrops_exist")
        self.update(ids, bboxes, embeds, labels, frame_id, iou_valid, margin)
        return ids, indices, k, float(min(margin)), ious

    def update(self, ids, bboxes, embeds, labels, frame_id, ious, margin):
        for id, bbox, embed, label in zip(ids, bboxes, embeds, labels):
            if id < 0:
                continue
            if id in self.tracklets:
                t = self.tracklets[id]
                if frame_id - t["last_frame"] > 1:
                    self.events.append("reappeared_after_%d" % (frame_id - t["last_frame"]))
                velocity = (bbox - t["bbox"]) / (frame_id - t["last_frame"])
                t["bbox"] = bbox
                t["embed"] = (1 - self.memo_momentum) * t["embed"] + self.memo_momentum * embed
                t["last_frame"] = frame_id
                t["label"] = label
                t["velocity"] = (t["velocity"] * t["acc_frame"] + velocity) / (t["acc_frame"] + 1)
                t["acc_frame"] += 1
            else:
                self.tracklets[id] = dict(bbox=bbox, embed=embed, label=label, last_frame=frame_id, velocity=np.zeros_like(bbox),
                                          acc_frame=0)
        rows = []
        for i in range(len(ids)):
            if ids[i] == -1:
                margin.extend(np.abs(ious[i, :i] - self.nms_backdrop_iou_thr))
                if (ious[i, :i] > self.nms_backdrop_iou_thr).any():
                    self.events.append("backdrop_filtered")
                else:
                    rows.append(i)
        self.backdrops.insert(0, dict(bboxes=bboxes[rows], embeds=embeds[rows], labels=labels[rows]))
        for key in [k for k, v in self.tracklets.items() if frame_id - v["last_frame"] >= self.memo_tracklet_frames]:
            self.tracklets.pop(key)
            self.events.append("expired")
            if not self.tracklets:
                self.events.append("memory_emptied")
        if len(self.backdrops) > self.memo_backdrop_frames:
            self.backdrops.pop()


def run(name, cases, seed=None):
    """The case on the float64 tracker: dict(frames=[(ids, indices, kept)], margins=[per frame], memo={...}, events=set,
    columns=[(tracklets, backdrops) of every walk], ious=[the sorted IoU matrix of every frame])."""
    ref = RefTracker(**cases.CASES[name][3])
    frames, margins, ious = [], [], []
    for fr in cases.frames(name, seed):
        ids, indices, kept, margin, iou = ref.match(fr["bboxes"], fr["labels"], fr["embeds"], fr["frame_id"], list(fr["indices"]))
        frames.append((ids, indices, kept))
        margins.append(margin)
        ious.append(iou)
    return dict(frames=frames, margins=margins, memo=ref.memo(), events=set(ref.events), columns=ref.columns, ious=ious)
