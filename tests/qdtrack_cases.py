"""What tests/test_qdtrack_cpu.py, tests/test_qdtrack_gpu.py and tests/golden/make_qdtrack_golden.py share: the seeded sequences
the QuasiDense tracker is tested on, and the reference's recorded answers (tests/golden/qdtrack/<case>.npz).

A sequence is a script: per frame a list of detections (key, score, cell, shift[, label]).  `key` picks one vector of an
orthonormal basis (an object, or clutter); the detection's embedding is that vector plus seeded noise, scaled to norm
0.98 sqrt(8) as in tests/tracker_cases.py, so that |embeds . memo^T| <= 8 whatever the memory has averaged.  The box is the 9 x 6
rectangle of `cell` (six cells to a row of the grid, 10 x 8 apart) moved `shift` pixels to the right and drifting with the frame:
two boxes of one cell `s` pixels apart have IoU 1, 0.8, 0.636, 0.5, 0.385, 0.286 for s = 0 .. 5, boxes of different cells 0.  The
label is key % 5 unless given.  Scores: OBJECT is above init_score_thr, MID between obj_score_thr and init_score_thr (never
starts a tracklet), LOW below obj_score_thr; a frame's scores are then lowered by 0.002 x a seeded permutation of the rows, so
that no two are equal and the rows do NOT arrive in score order.

Every case must keep a float64 margin of MARGIN (tests/tracker_cases.py) on every decision of every frame (tests/qdtrack_ref.py
measures it, tests/test_qdtrack_cpu.py asserts it): a condition on the inputs, met by choosing the seed, not a tolerance on the
kernels."""
import functools
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from tracker_cases import CELLS_PER_ROW, EMBED_NORM, MARGIN, NOISE, _basis, assert_memo_close  # noqa: E402,F401

GOLDEN = os.path.join(HERE, "golden", "qdtrack")
OBJECT, MID, LOW = 0.95, 0.65, 0.4
SCORE_STEP = 0.002


def _objects(keys, score=OBJECT):
    return [(k, score, k, 0) for k in keys]


def _clutter(first, count, score=MID, cell=70):
    """`count` detections of keys nobody has seen, each in a cell of its own"""
    return [(first + j, score, cell + j, 0) for j in range(count)]


def _waves():
    """n = 63, 64, 65, 65, 1 valid rows; the memory grows 63 -> 64 -> 65 tracklets (its only columns: every row starts or feeds
    a tracklet, the backdrop frames are empty), so rows and tracklet columns cross a wave of 64."""
    return [_objects(range(63)), _objects(range(64)), _objects(range(65)), _objects(range(65)), _objects([7]),
            _objects(reversed(range(65))), _objects(range(63)), _objects(range(65))]


def _waves_backdrops():
    """60 tracklets and a backdrop frame of 3, 4, 5, 4 rows: the memory has 63, 64, 65, 64 columns, the 64 | 65 boundary among the
    backdrops."""
    objs = _objects(range(60))
    return [objs, objs + _clutter(100, 3), objs + _clutter(110, 4), objs + _clutter(120, 5), objs + _clutter(130, 4), objs,
            objs + _clutter(140, 5), objs + _clutter(150, 1)]


def _bookkeeping():
    """memo_tracklet_frames = 3.  Object 1 is away for one frame (back with a velocity divisor of 2), 2 for two (3), 3 for three
    (expired: a new identity); three frames of clutter empty the memory, a fourth meets an empty memory that still has
    backdrops, and objects 0 and 1 start afresh."""
    return [_objects([0, 1, 2, 3]), _objects([0]), _objects([0, 1]), _objects([0, 2]), _objects([0, 3]), _clutter(10, 3), _clutter(20, 3),
            _clutter(30, 2), _clutter(40, 3), _objects([0, 1]), _objects([1, 0])]


def _decisions():
    """Frame 2: object 6's MID detection finds no tracklet and becomes a backdrop; frame 3: it is back with a score above
    init_score_thr, its best column is that backdrop, and it starts a tracklet.  Frame 4: object 2 is seen only by a LOW detection
    (-2).  Frame 5: two detections of object 0 compete; the loser finds the column zeroed and starts a tracklet.  Frame 6: cell
    4 holds four boxes: the second is dropped by the first, the third by the dropped second alone, the LOW fourth by the
    backdrop threshold; object 0's cell holds a MID stranger 3 pixels off, which the pre-NMS keeps and the backdrop filter drops.
    Frame 7: one cell, every row but the first dropped."""
    return [_objects([0, 2, 4]), _objects([0, 2, 4]),
            _objects([0, 2, 4]) + [(6, MID, 6, 0)],
            _objects([0, 2, 4, 6]),
            [(0, OBJECT, 0, 0), (4, OBJECT, 4, 0), (6, OBJECT, 6, 0), (2, LOW, 2, 0)],
            [(0, OBJECT, 0, 0), (0, OBJECT - 0.03, 20, 0), (2, OBJECT, 2, 0), (4, OBJECT, 4, 0)],
            [(0, OBJECT, 0, 0), (21, MID, 0, 3), (4, OBJECT, 4, 0), (4, OBJECT - 0.03, 4, 1), (4, OBJECT - 0.06, 4, 2), (22, LOW, 4, 4),
             (2, OBJECT, 2, 0)],
            [(2, OBJECT, 2, 0), (2, OBJECT - 0.03, 2, 1), (23, MID, 2, 0), (24, LOW, 2, 4)],
            _objects([0, 2, 4, 6])]


def _cats():
    """Frame 3: object 1 arrives under another label.  with_cats: its column is gated to 0 and it starts a tracklet; without:
    it keeps its identity."""
    return [_objects([0, 1, 2]), _objects([0, 1, 2]), _objects([2, 1, 0]), [(0, OBJECT, 0, 0), (1, OBJECT, 1, 0, 4), (2, OBJECT, 2, 0)],
            _objects([0, 1, 2]), _objects([0, 2]), _objects([0, 1, 2]), _objects([1, 2, 0])]


def _ring():
    """Objects and a changing number of MID strangers, for the backdrop ring at memo_backdrop_frames 0, 1 and 2"""
    return [_objects([0, 1]) + _clutter(3, 1), _objects([0, 1, 2]) + _clutter(4, 2), _objects([0, 1, 2]), _objects([2, 1]) + _clutter(3, 1),
            _objects([0, 1, 2]) + [(3, OBJECT, 70, 0)], _objects([0, 3]) + _clutter(5, 1), _objects([0, 1, 2, 3]) + [(5, OBJECT, 70, 0)],
            _objects([0, 1, 2, 3, 5])]


def _grow():
    """Two, two, then three and more detections: with capacity = 4 the third frame no longer fits the device bank, with
    backdrop_capacity = 2 it does not either."""
    return [_objects([0, 1]), _objects([0, 1]), _objects([0, 1, 2]), _objects([0, 1, 2, 3, 4]), _objects([4, 3, 2, 1, 0]),
            _objects([0, 2, 4, 5]), _objects([0, 1, 2, 3, 4, 5]), _objects([5, 0])]


BDD = dict(memo_momentum=1.0)       # the bdd_track route's setting (uninext_vid.py:330); the class default is 0.8
# name: (script, embedding width, seed, constructor arguments)
CASES = {
    "waves": (_waves, 256, 2, {}),
    "waves_backdrops": (_waves_backdrops, 256, 1, BDD),
    "bookkeeping": (_bookkeeping, 256, 1, dict(memo_tracklet_frames=3, **BDD)),
    "decisions": (_decisions, 256, 1, {}),
    "decisions_bdd": (_decisions, 256, 1, BDD),
    "cats_on": (_cats, 8, 1, BDD),
    "cats_off": (_cats, 8, 1, dict(with_cats=False, **BDD)),
    "ring0": (_ring, 6, 1, dict(memo_backdrop_frames=0)),
    "ring1": (_ring, 6, 1, dict(memo_backdrop_frames=1)),
    "ring2": (_ring, 6, 1, dict(memo_backdrop_frames=2, **BDD)),
    "grow": (_grow, 8, 1, {}),
    "grow_backdrops": (_grow, 8, 1, BDD),
}
IOU_FRAMES = (2, 6, 7)     # the frames whose sorted box IoU matrix the fixtures carry
OVERFLOW = {"grow": dict(capacity=4), "grow_backdrops": dict(backdrop_capacity=2)}      # the frames fit up to the third


def _key_count(script):
    return 1 + max(d[0] for frame in script for d in frame)


@functools.lru_cache(maxsize=None)
def frames(name, seed=None):
    """The case's frames: a list of dict(bboxes [n, 5], labels [n] int64, embeds [n, D], frame_id, indices) of fp32 CPU tensors.
    Shared: callers must not write into them."""
    script, D, case_seed, _ = CASES[name]
    script = script()
    seed = case_seed if seed is None else seed
    basis = _basis(seed, D, _key_count(script))
    g = torch.Generator().manual_seed(seed + 7919)
    out = []
    for f, frame in enumerate(script):
        n = len(frame)
        lower = torch.randperm(n, generator=g).tolist()
        bboxes, labels, embeds = [], [], []
        for j, det in enumerate(frame):
            key, score, cell, shift = det[:4]
            noise = torch.randn(D, generator=g, dtype=torch.float64) / D ** 0.5
            e = basis[key] / basis[key].norm() + NOISE * noise
            embeds.append(EMBED_NORM * e / e.norm())
            x, y = 10.0 * (cell % CELLS_PER_ROW) + 0.5 * f + shift, 8.0 * (cell // CELLS_PER_ROW) + 0.25 * f
            bboxes.append([x, y, x + 9.0, y + 6.0, score - SCORE_STEP * lower[j]])
            labels.append(det[4] if len(det) > 4 else key % 5)
        out.append(dict(bboxes=torch.tensor(bboxes, dtype=torch.float64).float().view(n, 5), labels=torch.tensor(labels, dtype=torch.int64),
                        embeds=torch.stack(embeds).float().view(n, D), frame_id=f, indices=[7 * i + 3 for i in range(n)]))
    return out


def run(tracker, name, device="cpu", upto=None, frames_=None, outputs=None):
    """Drive `tracker` through the case; returns per frame (ids list, indices, kept count).  `outputs`, a list, receives the
    returned (bboxes, labels) of every frame."""
    out = []
    for fr in (frames_ or frames(name))[:upto]:
        b, l, ids, ind = tracker.match(fr["bboxes"].to(device), fr["labels"].to(device), fr["embeds"].to(device), fr["frame_id"],
                                       list(fr["indices"]))
        assert b.shape[0] == l.shape[0] == ids.shape[0] == len(ind) and ids.dtype == torch.int64 and not ids.is_cuda
        assert isinstance(ind, list)
        out.append((ids.tolist(), ind, len(ind)))
        if outputs is not None:
            outputs.append((b, l))
    return out


MEMO_NAMES = ("bboxes", "labels", "embeds", "ids", "vs")


def memo_arrays(tracker):
    """The 5-tuple of `tracker.memo` as {name: float64 / int64 numpy array} (empty arrays for an empty memory), with the
    tracklets' last_frame and acc_frame and the backdrop frames' rows added."""
    tracklets, backdrops = tracker.tracklets, tracker.backdrops
    out = {}
    if tracklets or any(len(b["labels"]) for b in backdrops):
        for name, t in zip(MEMO_NAMES, tracker.memo):
            t = t.detach().cpu()
            out[name] = t.numpy().astype(np.float64 if t.is_floating_point() else np.int64)
    else:
        D = backdrops[0]["embeds"].shape[1] if backdrops else 1
        out = dict(bboxes=np.zeros((0, 5)), labels=np.zeros(0, dtype=np.int64), embeds=np.zeros((0, D)), ids=np.zeros(0, dtype=np.int64),
                   vs=np.zeros((0, 5)))
    out["last_frame"] = np.asarray([int(v["last_frame"]) for v in tracklets.values()], dtype=np.int64)
    out["acc_frame"] = np.asarray([int(v["acc_frame"]) for v in tracklets.values()], dtype=np.int64)
    out["backdrop_rows"] = np.asarray([len(b["labels"]) for b in backdrops], dtype=np.int64)
    return out


def with_rowsums(memo):
    """`memo` with its embeddings replaced by their row sums, as the fixtures store them"""
    memo = dict(memo)
    memo["embeds_rowsum"] = memo.pop("embeds").sum(1)
    return memo


@functools.lru_cache(maxsize=None)
def golden(name):
    """The reference's record of the case: dict(frames=[(ids, indices, kept)], memo={...}, seed, ious=[the first frames' sorted
    box IoU matrices])."""
    with np.load(os.path.join(GOLDEN, "%s.npz" % name)) as z:
        count = int(z["frames"])
        fr = [([int(v) for v in z["%d.ids" % t]], [int(v) for v in z["%d.indices" % t]], int(z["kept"][t])) for t in range(count)]
        memo = {k[5:]: z[k] for k in z.files if k.startswith("memo.")}
        ious = {int(k[4:]): z[k] for k in z.files if k.startswith("iou.")}
        return dict(frames=fr, memo=memo, seed=int(z["seed"]), ious=ious)
