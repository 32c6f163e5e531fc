"""What tests/test_reid_cpu.py, tests/test_reid_gpu.py, tests/golden/make_reid_golden.py and tools/reid_bench.py share: the seeded
inputs of the re-ID selection / loss cases (tests/golden/reid/*.npz hold the fixture cases' inputs together with what the
reference's select_pos_neg and loss_reid made of them) and the scaled error of tests/criterion_cases.py.

A case: `Q` reference queries, `Qk` key queries, `C` channels, `T` tokens and per image a dict: `n` targets, `valid` flags, `keys`
(the key query matched to each target), `near` (queries scattered closely around each target: what drives the dynamic k), `dup`
(target 1 is a copy of target 0: after the conflict resolution one of the two is left without a query, so the repair loop runs).
Cases with "fixture" are minted from the reference (Q <= 160, at most 6 targets per image); the others are held to the numpy
restatement (tests/reid_ref.py) and to the composition only.
"""
import os

import numpy as np
import torch

from criterion_cases import scaled_error  # noqa: F401  (the project's tolerance: <= 1e-4 of the value's own scale)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "reid")
TOLERANCE = 1e-4
SEED = 20240611                 # random.seed of every case


def _img(n, valid=None, keys=None, near=12, dup=False):
    return {"n": n, "valid": [1] * n if valid is None else valid, "keys": keys, "near": near, "dup": dup}


CASES = {
    # every query is a candidate of the 100-candidate run
    "reid_q100_c64": {"seed": 1, "Q": 100, "Qk": 16, "C": 64, "T": 8, "images": [_img(3), _img(2)], "fixture": True},
    "reid_q101_g1_c256": {"seed": 2, "Q": 101, "Qk": 16, "C": 256, "T": 8, "images": [_img(1)], "fixture": True},
    # Q no multiple of 64; an image without targets, one whose targets are all invalid, one with an invalid target first, in the
    # middle and last; two targets sharing a key row
    "reid_q130_mixed_c64": {"seed": 13, "Q": 130, "Qk": 16, "C": 64, "T": 8, "fixture": True,
                            "images": [_img(0), _img(6, valid=[0, 1, 0, 1, 1, 0], keys=[5, 3, 7, 3, 9, 1]), _img(2, valid=[0, 0]), _img(2)]},
    # the first run's repair loop fires: its + 100000 rows change what the second run selects
    "reid_q160_repair_c64": {"seed": 24, "Q": 160, "Qk": 16, "C": 64, "T": 8, "images": [_img(3, dup=True), _img(4, dup=True, valid=[1, 1, 0, 1])],
                             "fixture": True},
    # 100 of 130 queries lie on the target: the 100-candidate k is large, 10 * n_pos >= n_neg, every negative is sampled
    "reid_q130_allneg_c64": {"seed": 5, "Q": 130, "Qk": 16, "C": 64, "T": 8, "images": [_img(1, near=100), _img(2, near=45)], "fixture": True},
    # more than one pass of the 1024-thread workgroup
    "reid_q1030_c64": {"seed": 16, "Q": 1030, "Qk": 1030, "C": 64, "T": 8, "images": [_img(4, valid=[1, 0, 1, 1]), _img(3)], "fixture": False},
}
FIXTURES = [name for name, cfg in CASES.items() if cfg["fixture"]]


def make_inputs(cfg):
    """{name: numpy array}: ref_box [bs, Q, 4], ref_cls [bs, Q, T] (probabilities), hs_ref [bs, Q, C], hs_key [bs, Qk, C], all float32,
    and per image b: boxes_b [n, 4], pm_b [n, T] bool, valid_b [n] bool, idx_b [n] int64."""
    rng = np.random.RandomState(cfg["seed"])
    Q, Qk, C, T, images = cfg["Q"], cfg["Qk"], cfg["C"], cfg["T"], cfg["images"]
    bs = len(images)
    out = {}
    ref_box = np.empty((bs, Q, 4), np.float32)
    for b, im in enumerate(images):
        n = im["n"]
        gt = np.concatenate([rng.uniform(0.25, 0.75, (n, 2)), rng.uniform(0.15, 0.4, (n, 2))], 1).astype(np.float32)
        pm = np.zeros((n, T), bool)
        for g in range(n):
            pm[g, rng.choice(T, size=rng.randint(1, 4), replace=False)] = True
        if im["dup"]:
            gt[1], pm[1] = gt[0], pm[0]
        boxes = np.concatenate([rng.uniform(0.05, 0.95, (Q, 2)), rng.uniform(0.05, 0.5, (Q, 2))], 1).astype(np.float32)
        row = 0
        for g in range(n):                    # the queries near target g: its box with a few per cent of jitter
            m = min(im["near"], Q - row)
            boxes[row:row + m] = gt[g] * (1 + rng.uniform(-0.06, 0.06, (m, 4))).astype(np.float32)
            row += m
        ref_box[b] = boxes[rng.permutation(Q)]
        out["boxes_%d" % b], out["pm_%d" % b] = gt, pm
        out["valid_%d" % b] = np.asarray(im["valid"], bool).reshape(n)
        keys = im["keys"] if im["keys"] is not None else rng.randint(0, Qk, n).tolist()
        out["idx_%d" % b] = np.asarray(keys, np.int64).reshape(n)
    out["ref_box"] = ref_box
    out["ref_cls"] = rng.uniform(0.02, 0.98, (bs, Q, T)).astype(np.float32)
    out["hs_ref"] = (0.5 * rng.standard_normal((bs, Q, C))).astype(np.float32)
    out["hs_key"] = (0.5 * rng.standard_normal((bs, Qk, C))).astype(np.float32)
    return out


def rebuild(flat, bs, device="cpu", embed_dtype=torch.float32):
    """The arguments of select_pos_neg from make_inputs' arrays: (ref_box, all_indices, targets, det_targets, hs_key, hs_ref, ref_cls)."""
    def t(a, dtype=None):
        return torch.as_tensor(np.asarray(a), dtype=dtype).to(device)
    targets, all_indices = [], []
    for b in range(bs):
        n = len(flat["valid_%d" % b])
        targets.append({"labels": t(np.zeros(n, np.int64)), "boxes": t(flat["boxes_%d" % b]), "positive_map": t(flat["pm_%d" % b]),
                        "valid": t(flat["valid_%d" % b])})
        all_indices.append(t(flat["idx_%d" % b]))
    return (t(flat["ref_box"]), all_indices, targets, targets, t(flat["hs_key"], embed_dtype), t(flat["hs_ref"], embed_dtype), t(flat["ref_cls"]))


def load_fixture(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def candidate_sum_margin(flat, bs):
    """The smallest distance from an integer of the float64 sum of a valid target's 10 and 100 largest IoUs: the fixtures keep it
    above 1e-3, so the order in which an implementation adds the IoUs cannot move a dynamic k."""
    from uninext_amd.matcher import box_cxcywh_to_xyxy, box_iou
    worst = 1.0
    for b in range(bs):
        valid = flat["valid_%d" % b]
        if not valid.any():
            continue
        iou = box_iou(box_cxcywh_to_xyxy(torch.as_tensor(flat["ref_box"][b])), box_cxcywh_to_xyxy(torch.as_tensor(flat["boxes_%d" % b][valid])))
        top = torch.sort(iou.double(), dim=0, descending=True)[0]
        for k in (10, 100):
            s = top[:k].sum(0).numpy()
            worst = min(worst, float(np.min(np.abs(s - np.round(s)))))
    return worst
