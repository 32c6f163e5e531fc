"""IDOL_Tracker.match + update_memo + memo (projects/UNINEXT/uninext/models/tracker.py:98-298, match_metric 'bisoftmax')
restated in float64 on numpy, written from the reference's text like tests/decoder_ref.py: the yardstick the tracker's two
routes are compared with.  Besides the reference's results a call returns the SMALLEST MARGIN of every decision it took:

    |conf - match_score_thr| of every row reached;  the gap between the two largest entries of the row at the moment of its max
    (but for a row whose maximum is an exact 0.0 of zeroed columns: that tie is exact in fp32 too);
    |score - 0.5| of every entry of a row under frame_weight;  |detection score - addnew / init threshold| of every detection
    still unassigned there;  |IoU - nms_thr_post| of every pair the backdrop test reads;  |IoU - nms_thr_pre| of every pair the
    pre-NMS visits.

A case whose margins stay above tests/tracker_cases.py: MARGIN cannot be decided differently by fp32 arithmetic."""
import numpy as np


def _iou(a, b):
    inter = float(np.logical_and(a, b).sum())
    union = float(np.logical_or(a, b).sum())
    return (inter + 1e-6) / (union + 1e-6)


def _softmax(x, axis):
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


class RefTracker:
    def __init__(self, nms_thr_pre=0.7, nms_thr_post=0.3, init_score_thr=0.2, addnew_score_thr=0.5, match_score_thr=0.5,
                 memo_tracklet_frames=10, memo_momentum=0.5, long_match=False, frame_weight=False, temporal_weight=False,
                 memory_len=10, **unused):
        self.__dict__.update(locals())
        self.num_tracklets = 0
        self.tracklets = {}
        self.events = []

    def memo_embed(self, v):
        if not self.long_match:
            return v["embed"]
        w = np.asarray(v["long_score"], dtype=np.float64)
        if self.temporal_weight:
            w = w + np.arange(1, len(w) + 1, dtype=np.float64) / len(w)
        return (np.stack(v["long_embed"]) * w[:, None]).sum(0) / w.sum()

    def memo(self):
        t = self.tracklets
        return dict(bboxes=np.stack([v["bbox"] for v in t.values()]), labels=np.asarray([v["label"] for v in t.values()], dtype=np.int64),
                    embeds=np.stack([self.memo_embed(v) for v in t.values()]), ids=np.asarray(list(t), dtype=np.int64),
                    vs=np.stack([v["velocity"] for v in t.values()]),
                    long_embeds=np.concatenate([np.stack(v["long_embed"]) for v in t.values()]),
                    long_score=np.concatenate([np.asarray(v["long_score"])[:, None] for v in t.values()]),
                    long_len=np.asarray([len(v["long_embed"]) for v in t.values()], dtype=np.int64),
                    exist_frame=np.asarray([v["exist_frame"] for v in t.values()], dtype=np.int64))

    def match(self, bboxes, labels, masks, embeds, frame_id, indices):
        """fp32 torch tensors in; (ids, indices, kept count, smallest margin) out."""
        bboxes, embeds = bboxes.double().numpy(), embeds.double().numpy()
        labels = labels.numpy()
        binary = masks.numpy()[:, 0] > 0                # sigmoid(x) > 0.5
        margin = [np.inf]
        n = len(bboxes)
        keep = [True] * n
        for i in range(n - 1):
            if not keep[i]:
                continue
            for j in range(i + 1, n):
                if keep[j]:
                    iou = _iou(binary[i], binary[j])
                    margin.append(abs(iou - self.nms_thr_pre))
                    if iou > self.nms_thr_pre:
                        keep[j] = False
        sel = [i for i in range(n) if keep[i]]
        indices = [indices[i] for i in sel]
        bboxes, labels, binary, embeds = bboxes[sel], labels[sel], binary[sel], embeds[sel]
        k = len(sel)
        ids = [-2] * k
        was_empty = not self.tracklets
        if k > 0 and not was_empty:
            slots = list(self.tracklets)
            memo = np.stack([self.memo_embed(self.tracklets[s]) for s in slots])
            exist = np.asarray([self.tracklets[s]["exist_frame"] for s in slots], dtype=np.float64)
            feats = embeds @ memo.T
            assert np.abs(feats).max() <= 8.0 + 1e-9
            scores = (_softmax(feats, 1) + _softmax(feats, 0)) / 2
            for i in range(k):
                row = scores[i].copy()
                if self.frame_weight:
                    margin.append(np.abs(row - 0.5).min())
                    hits = row > 0.5
                    if hits.sum() > 1:
                        plain = int(np.argmax(row))
                        row = np.where(hits, row * exist, row * exist[hits].mean())
                        self.events.append("frame_weight")
                        if int(np.argmax(row)) != plain:
                            self.events.append("frame_weight_changed_winner")
                best = int(np.argmax(row))
                conf = row[best]
                if len(row) > 1 and conf != 0.0:        # a tie of columns zeroed before is exact in every arithmetic
                    margin.append(conf - np.partition(row, -2)[-2])
                margin.append(abs(conf - self.match_score_thr))
                if conf > self.match_score_thr:
                    ids[i] = slots[best]
                    others = np.arange(k) != i
                    if (scores[others, best] > self.match_score_thr).any():
                        self.events.append("column_zeroed_under_a_rival")
                    scores[others, best] = 0
        if k > 0 or was_empty:
            thr = self.init_score_thr if was_empty else self.addnew_score_thr
            for i in range(k):
                if ids[i] == -2:
                    margin.append(abs(bboxes[i, 4] - thr))
                    if bboxes[i, 4] > thr:
                        ids[i] = self.num_tracklets
                        self.num_tracklets += 1
            for i in range(k):
                if ids[i] == -2:
                    ious = [_iou(binary[i], binary[j]) for j in range(i)]
                    margin.extend(abs(v - self.nms_thr_post) for v in ious)
                    if all(v < self.nms_thr_post for v in ious):
                        ids[i] = -1
                        self.events.append("backdrop_first" if i == 0 else "backdrop")
                    else:
                        self.events.append("left_unselected")
            self.update(ids, bboxes, embeds, labels, frame_id)
        return ids, indices, k, float(min(margin))

    def update(self, ids, bboxes, embeds, labels, frame_id):
        for id, bbox, embed, label in zip(ids, bboxes, embeds, labels):
            if id < 0:
                continue
            if id in self.tracklets:
                t = self.tracklets[id]
                if frame_id - t["last_frame"] > 1:
                    self.events.append("reappeared_after_%d" % (frame_id - t["last_frame"]))
                velocity = (bbox - t["bbox"]) / (frame_id - t["last_frame"])
                t["bbox"] = bbox
                t["long_score"].append(bbox[-1])
                t["embed"] = (1 - self.memo_momentum) * t["embed"] + self.memo_momentum * embed
                t["long_embed"].append(embed)
                t["last_frame"] = frame_id
                t["label"] = label
                t["velocity"] = (t["velocity"] * t["acc_frame"] + velocity) / (t["acc_frame"] + 1)
                t["acc_frame"] += 1
                t["exist_frame"] += 1
            else:
                self.tracklets[id] = dict(bbox=bbox, embed=embed, long_embed=[embed], long_score=[bbox[-1]], label=label,
                                          last_frame=frame_id, velocity=np.zeros_like(bbox), acc_frame=0, exist_frame=1)
        for key in [k for k, v in self.tracklets.items() if frame_id - v["last_frame"] >= self.memo_tracklet_frames]:
            self.tracklets.pop(key)
            self.events.append("expired")
        for v in self.tracklets.values():
            if len(v["long_embed"]) > self.memory_len:
                v["long_embed"].pop(0)
                v["long_score"].pop(0)
                self.events.append("ring_wrapped")
        if not self.tracklets:
            self.events.append("memory_emptied")


def run(name, cases, seed=None):
    """The case on the float64 tracker: dict(frames=[(ids, indices, kept)], margins=[per frame], memo={...}, events=set,
    memos=[the memo after every frame, None while the memory is empty])."""
    ref = RefTracker(**cases.CASES[name][3])
    frames, margins, memos = [], [], []
    for fr in cases.frames(name, seed):
        ids, indices, kept, margin = ref.match(fr["bboxes"], fr["labels"], fr["masks"], fr["embeds"], fr["frame_id"], list(fr["indices"]))
        frames.append((ids, indices, kept))
        margins.append(margin)
        memos.append(ref.memo() if ref.tracklets else None)
    return dict(frames=frames, margins=margins, memo=ref.memo(), events=set(ref.events), memos=memos)
