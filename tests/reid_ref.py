"""A float32 numpy restatement of the re-ID positive / negative selection (pos_neg_select.py: get_pos_idx :99-153 with
dynamic_k_matching :187-226), built on oracle/ota_oracle.py by import: the cost terms and the dynamic-k assignment are the
oracle's; what is added here is the candidate count (10, then 100), the cost matrix CARRIED OVER from the first run to the second
(the reference passes the same tensor twice: the repair loop's + 100000 rows stay), the background penalty applied once, and
the `valid` filter.  The exact yardstick of the integers of include/ota_hip.h: ota_reid_select_hip.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import ota_oracle as O  # noqa: E402

F = np.float32
ALPHA, GAMMA = F(0.25), F(2.0)


def _dynamic_k(cost, iou, flags, candidates):
    """oracle.dynamic_k with `candidates` in place of its 10.  -> (matching uint8 [Q, G], status, repaired: the repair loop ran)."""
    before = cost.copy()
    _, _, _, M, status = O.dynamic_k(cost, iou, flags, candidates=candidates)
    fg = (flags & 1).any(1)
    with np.errstate(invalid="ignore"):
        after_bg = np.where(fg[:, None], before, before + O.BG_PENALTY)
    return M, status, not np.array_equal(after_bg, cost, equal_nan=True)


def select(class_table, boxes, tgt_boxes, positive_map, valid, carry=True):
    """One image.  class_table [Q, T] float32 (the focal table, formed by the caller), boxes [Q, 4], tgt_boxes [G, 4], positive_map
    [G, T], valid [G].  -> None without a valid target, else a dict: pos, neg uint8 [Q, G] (columns of invalid targets zero; `neg` is
    the 100-candidate matching: a target's negatives are the queries OUTSIDE it), n_pos, n_neg [G] (-1 for invalid targets), status,
    repaired (the first run's repair loop ran).  carry=False: the second run on a fresh cost matrix instead -- NOT what the
    reference does; the tests use it to show that a case depends on the carried-over rows."""
    valid = np.asarray(valid).astype(bool)
    Q, G = boxes.shape[0], len(valid)
    if not valid.any():
        return None
    assert Q >= 100, "torch.topk(ious, 100) raises in the reference"
    cost, iou, flags = O.cost_terms(class_table, boxes, tgt_boxes[valid], positive_map[valid])
    m_pos, st1, repaired = _dynamic_k(cost, iou, flags, 10)
    if carry:
        m_neg, st2, _ = _dynamic_k(cost, iou, flags | 1, 100)          # (every row foreground: the penalty is not added again)
    else:
        fresh, _, _ = O.cost_terms(class_table, boxes, tgt_boxes[valid], positive_map[valid])
        m_neg, st2, _ = _dynamic_k(fresh, iou, flags, 100)
    pos, neg = np.zeros((Q, G), np.uint8), np.zeros((Q, G), np.uint8)
    pos[:, valid], neg[:, valid] = m_pos, m_neg
    n_pos, n_neg = np.full(G, -1, np.int64), np.full(G, -1, np.int64)
    n_pos[valid], n_neg[valid] = m_pos.sum(0), Q - m_neg.sum(0)
    return {"pos": pos, "neg": neg, "n_pos": n_pos, "n_neg": n_neg, "status": st1 | st2, "repaired": repaired}


def num_sample_neg(n_pos, n_neg):
    """pos_neg_select.py:76-81."""
    if n_pos == 0:
        return 10
    if n_pos * 10 >= n_neg:
        return n_neg
    return n_pos * 10


def focal_table(prob):
    """pos - neg of pos_neg_select.py:113-114 by PyTorch's own elementwise operations (the caller of the kernels forms it so)."""
    import torch
    p = torch.as_tensor(prob)
    neg = (1 - 0.25) * (p ** 2.0) * (-(1 - p + 1e-8).log())
    pos = 0.25 * ((1 - p) ** 2.0) * (-(p + 1e-8).log())
    return (pos - neg).numpy()
