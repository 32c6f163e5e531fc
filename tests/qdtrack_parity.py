"""Per-entry parity of the QuasiDense tracker's kernels (uninext_amd/csrc/qdtrack.hip: rank, iou_valid, feats_rows, cols_final,
associate, update) at their wave and workgroup edges: the cases and the restatements.  No GPU is needed to import this;
tests/test_qdtrack_parity_gpu.py holds the four entry points to it through uninext_amd.ext.

Floats are multiples of 2^-10 (tests/tracker_parity.py: dy), so float64 sees exactly what fp32 holds.  Banks are built directly,
field by field.

  prepare  random boxes that overlap a lot, scores with one planted tie: `order` against a stable descending sort, the IoU matrix
           BITWISE against torch's on the same inputs (the package's restated bbox_overlaps on the CPU, which
           tests/test_qdtrack_cpu.py pins to the reference's bits) and `valid` against the flags that matrix gives.
  scores   against tests/tracker_parity.py: scores64 on the memory's columns laid out as one bank (tracklets, then backdrops),
           with that module's error measure and bound (SUM_DEPTH u s and the project's 1e-4 max(1, max|ref|)); the class gate
           multiplies both sides by the same exact 0 / 1.
  step     (STEPS) one whole call (prepare, scores, associate, update) against tests/qdtrack_ref.py in float64 started from the same
           bank: ids and integers equal, the next state's floats within 1e-4 of each tensor's magnitude (assert_memo_close),
           on inputs whose float64 margin is at least MARGIN."""
import functools
import os
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qdtrack_ref                                                            # noqa: E402
import tracker_parity as TP                                                   # noqa: E402
from tracker_cases import MARGIN                                              # noqa: E402

F32, F64 = np.float32, np.float64
OBJ_THR, BACKDROP_THR, CLASS_THR = 0.5, 0.3, 0.7

PREPARE_NS = (1, 2, 63, 64, 65, 257)


@functools.lru_cache(maxsize=None)
def prepare_inputs(n):
    """bboxes [n, 5] fp32: corners on a grid of 1/8 inside 48 x 48 (plenty of overlaps), scores k / 1024 all different but for
    rows 0 and n - 1 (when n > 2), which tie"""
    g = TP._rng("qdtrack_prepare_%d" % n)
    xy = g.randint(0, 256, (n, 2)) / 8.0
    wh = g.randint(32, 160, (n, 2)) / 8.0
    score = (1 + g.permutation(1000)[:n]) / 1024.0 if n <= 1000 else None
    if n > 2:
        score[n - 1] = score[0]
    return np.concatenate([xy, xy + wh, score[:, None]], 1).astype(F32)


def prepare_expected(bboxes):
    """(order, iou [n, n] fp32 by torch on the CPU, valid)"""
    from uninext_amd.tracker import bbox_overlaps
    order = np.argsort(-bboxes[:, 4].astype(F64), kind="stable").astype(np.int32)
    boxes = torch.from_numpy(bboxes[order, :4].copy())
    iou = bbox_overlaps(boxes, boxes).numpy()
    n = len(order)
    valid = np.ones(n, dtype=np.uint8)
    for i in range(1, n):
        thr = F32(BACKDROP_THR) if bboxes[order[i], 4] < F32(OBJ_THR) else F32(CLASS_THR)
        valid[i] = 0 if (iou[i, :i] > thr).any() else 1
    return order, iou, valid


# name: n, M tracklets, backdrop rows, D
BANKS = {"n1_M1_b0_D6": (1, 1, 0, 6), "n63_M65_b0_D8": (63, 65, 0, 8), "n64_M63_b1_D256": (64, 63, 1, 256), "n65_M64_b1_D6": (65, 64, 1, 6),
         "n65_M1_b64_D8": (65, 1, 64, 8), "n1_M65_b0_D256": (1, 65, 0, 256), "n64_M64_b65_D8": (64, 64, 65, 8), "n63_M1_b63_D256": (63, 1, 63, 256)}
# the whole step needs objects that can be told apart with a margin: every size at D = 256, few objects at D = 6 and 8; the
# last entry is the seed that gives the float64 margin
STEPS = {"step_n1_M1_b0_D6": (1, 1, 0, 6, 0), "step_n5_M3_b1_D6": (5, 3, 1, 6, 0), "step_n6_M4_b2_D8": (6, 4, 2, 8, 0),
         "step_n63_M65_b0_D256": (63, 65, 0, 256, 0), "step_n64_M63_b1_D256": (64, 63, 1, 256, 0), "step_n65_M64_b1_D256": (65, 64, 1, 256, 0),
         "step_n65_M1_b64_D256": (65, 1, 64, 256, 0), "step_n64_M64_b65_D256": (64, 64, 65, 256, 0)}
# (n, M, D) at which the two trackers' score entry points must give the same bits for the same bank of tracklets alone (no
# backdrops): the wave (63 | 65), workgroup (257 columns) and 16-byte-load (D 255 | 256, 6, 8) edges
SAME_BITS = {"same_n%d_M%d_D%d" % (n, M, D): (n, M, 0, D) for n, M, D in ((1, 1, 6), (63, 65, 8), (65, 64, 256), (64, 257, 255))}
FRAME = 20


@functools.lru_cache(maxsize=None)
def bank_inputs(name, seed=0):
    """One frame against a bank of M tracklets and one backdrop frame: detection i sees object i % (M + b + 2) -- tracklets,
    backdrops, two strangers -- from a cell of its own, so the pre-NMS keeps every row; a third of the tracklets carry another
    label than their object's detections (the class gate)."""
    n, M, b, D = (BANKS.get(name) or SAME_BITS.get(name) or STEPS[name])[:4]
    seed = STEPS[name][4] if name in STEPS else seed
    g = np.random.RandomState(zlib.crc32(name.encode()) + seed)
    K = M + b + 2
    keys = g.standard_normal((K, D))
    if K <= D:
        keys = np.linalg.qr(keys.T)[0].T
    keys /= np.linalg.norm(keys, axis=1, keepdims=True)
    radius = 0.98 * np.sqrt(8.0)
    memo = TP._rows(g, keys[:M + b], 0.3, radius)
    obj = np.arange(n) % K
    embeds = TP._rows(g, keys[obj], 0.3, radius)
    cell = g.permutation(4 * max(n, M + b) + 8)
    box = lambda c, f: np.stack([10.0 * (c % 6) + 0.5 * f, 8.0 * (c // 6) + 0.25 * f, 10.0 * (c % 6) + 0.5 * f + 9.0, 8.0 * (c // 6) + 0.25 * f + 6.0], 1)
    score = np.where(np.arange(n) % 7 == 3, 0.4, np.where(np.arange(n) % 5 == 1, 0.65, 0.95)) - g.permutation(n) / 512.0
    bboxes = TP.dy(np.concatenate([box(cell[:n], FRAME), score[:, None]], 1))
    labels = (obj % 5).astype(np.int64)
    ms = np.arange(M)
    state = dict(id=(100 + 3 * ms).astype(np.int64), label=np.where(ms % 3 == 2, (ms + 1) % 5, ms % 5).astype(np.int64),
                 bbox=TP.dy(np.concatenate([box(cell[:M] if M <= n else cell[:M], FRAME - 2), np.full((M, 1), 0.9)], 1)),
                 velocity=TP.dy(g.standard_normal((M, 5))), last_frame=(FRAME - 1 - ms % 3).astype(np.int32),
                 acc_frame=(ms % 4).astype(np.int32), embed=memo[:M],
                 backdrop_label=((M + np.arange(b)) % 5).astype(np.int64),
                 backdrop_bbox=TP.dy(np.concatenate([box(cell[M:M + b], FRAME - 1), np.full((b, 1), 0.6)], 1)).reshape(b, 5),
                 backdrop_embed=memo[M:].reshape(b, D))
    return dict(n=n, M=M, b=b, D=D, C=M + n + 3, B=max(n, b) + 3, bboxes=bboxes, labels=labels, embeds=embeds, state=state,
                num_tracklets=5000, frame_id=FRAME, momentum=0.8125)


def reference_tracker(x, **kwargs):
    """tests/qdtrack_ref.py's tracker holding the bank of `x` in float64"""
    ref = qdtrack_ref.RefTracker(memo_momentum=x["momentum"], memo_tracklet_frames=3, **kwargs)
    st = x["state"]
    for m in range(x["M"]):
        ref.tracklets[int(st["id"][m])] = dict(bbox=st["bbox"][m].astype(F64), embed=st["embed"][m].astype(F64), label=int(st["label"][m]),
                                               last_frame=int(st["last_frame"][m]), velocity=st["velocity"][m].astype(F64),
                                               acc_frame=int(st["acc_frame"][m]))
    ref.backdrops = [dict(bboxes=st["backdrop_bbox"].astype(F64), embeds=st["backdrop_embed"].astype(F64), labels=st["backdrop_label"])]
    ref.num_tracklets = x["num_tracklets"]
    return ref


def as_score_bank(x):
    """The memory's columns as ONE bank of tests/tracker_parity.py (tracklets, then the backdrop frame), for scores64"""
    Mt, D = x["M"] + x["b"], x["D"]
    state = TP.blank_state(Mt + 1, D, 1, Mt, 0)
    state["embed"][:Mt] = np.concatenate([x["state"]["embed"], x["state"]["backdrop_embed"]])
    return state
