"""Mint known-answer detections with the REFERENCE post-processing (build container only).

    python tests/golden/make_postprocess_golden.py

Takes the bodies of `UNINEXT_IMG.inference` (projects/UNINEXT/uninext/uninext_img.py:367-485) and of
`convert_grounding_to_od_logits` (:598-613) out of the reference checkout with `ast` at generation time (the module itself
imports detectron2 and friends) and executes them on seeded CPU inputs, with stand-ins for what they call from outside:
`ops.batched_nms` (torchvision is not installed: uninext_amd.postprocess.batched_nms, the restatement the tests pin by hand),
`Boxes`, `Instances` and `box_cxcywh_to_xyxy`.  `mask_pred` carries a one-hot row per query, so the reference's own selection
of the mask rows comes back as `query_index`.  Nothing of the reference's text is stored: a fixture
(tests/golden/postprocess/*.npz) holds the inputs and, per run (a configuration of ota / demo_only / score_thres / task), the
reference's scores, classes, boxes and query rows.

Every query has one dominant class and a score on a jittered grid, so the generator can ASSERT the margins that let a test
demand exact indices (and reseeds until they hold): every IoU at least 1e-4 away from 0.7, all NMS scores at least 1e-4
apart, every row's best class at least 1e-4 ahead of its second, the scores of the returned instances and the first one
dropped at least 1e-4 apart, and every entry at least 1e-4 away from the score threshold.
"""
import ast
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from uninext_amd import postprocess as pp  # noqa: E402

REF = os.environ.get("UNINEXT_REFERENCE", "/root/reference")
SRC = os.path.join(REF, "projects/UNINEXT/uninext/uninext_img.py")
OUT = os.path.join(HERE, "postprocess")
MARGIN = 1e-4


class Boxes:
    def __init__(self, tensor):
        self.tensor = tensor.clone()

    def scale(self, scale_x, scale_y):
        self.tensor[:, 0::2] *= scale_x
        self.tensor[:, 1::2] *= scale_y


class Instances:
    def __init__(self, image_size):
        self.image_size = image_size


def load_reference():
    """(inference(self, ...), convert_grounding_to_od_logits) executed from the reference's source."""
    tree = ast.parse(open(SRC).read())
    picked = []
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name in ("inference", "convert_grounding_to_od_logits"):
            picked.append(node)
    assert sorted(n.name for n in picked) == ["convert_grounding_to_od_logits", "inference"]
    ns = {"torch": torch, "F": F, "ops": types.SimpleNamespace(batched_nms=pp.batched_nms), "Boxes": Boxes,
          "Instances": Instances, "box_cxcywh_to_xyxy": pp.box_cxcywh_to_xyxy}
    exec(compile(ast.Module(body=picked, type_ignores=[]), SRC, "exec"), ns)
    return ns["inference"], ns["convert_grounding_to_od_logits"]


def make_inputs(seed, B, Q, T, C, max_tokens=4, empty=(), iou=True, lo=0.06, hi=0.98, spread_top=0):
    """box_cls [B, Q, T], box_pred [B, Q, 4], iou_pred [B, Q, 1] or None, positive_map {label: tokens}."""
    g = torch.Generator().manual_seed(seed)
    positive_map, t = {}, 1
    for c in range(C):
        if c in empty:
            continue
        n = T - 1 if C == 1 else int(torch.randint(1, max_tokens + 1, (1,), generator=g))
        positive_map[c + 1] = list(range(t, t + n))
        t += n
    assert t <= T, (t, T)
    named = torch.tensor([c for c in range(C) if c not in empty])
    logits = torch.randn(B, Q, T, generator=g) * 0.5 - 6.0
    iou_pred = torch.zeros(B, Q, 1) if iou else None
    cxcy, wh = torch.empty(B, Q, 2), torch.empty(B, Q, 2)
    for b in range(B):
        centres = 0.15 + 0.7 * torch.rand(12, 2, generator=g)
        cluster = torch.randint(0, 12, (Q,), generator=g)
        cxcy[b] = centres[cluster] + 0.03 * torch.randn(Q, 2, generator=g)
        wh[b] = 0.02 + 0.38 * torch.rand(Q, 2, generator=g) ** 2
        palette = named[torch.randint(0, len(named), (12, 3), generator=g)]          # three classes per cluster
        dominant = palette[cluster, torch.randint(0, 3, (Q,), generator=g)]
        twin = torch.randint(0, Q, (Q,), generator=g)
        for q in range(Q // 3, Q):               # near-duplicates of an earlier query, same class: what NMS is for
            if twin[q] < Q // 3:
                cxcy[b, q] = cxcy[b, twin[q]] + 0.004 * torch.randn(2, generator=g)
                wh[b, q] = wh[b, twin[q]] * (1 + 0.03 * torch.randn(2, generator=g))
                dominant[q] = dominant[twin[q]]
        grid = (torch.randperm(Q, generator=g).float() + 0.3 * torch.rand(Q, generator=g)) / Q
        s = lo + (hi - lo) * grid
        z = torch.log(s / (1 - s))
        for q in range(Q):
            logits[b, q, positive_map[int(dominant[q]) + 1]] = z[q]
        if iou:
            iou_pred[b, :, 0] = z
        if spread_top:        # the best queries sit apart on a lattice: NMS removes none of them
            top = torch.argsort(s, descending=True)[:spread_top]
            k = torch.arange(spread_top)
            side = int(np.ceil(np.sqrt(spread_top)))
            cxcy[b, top, 0] = (k % side + 0.5) / side
            cxcy[b, top, 1] = (k // side + 0.5) / side
            wh[b, top] = 0.3 / side
    return logits, torch.cat([cxcy, wh], -1), iou_pred, positive_map


def gaps_ok(values, margin=MARGIN):
    v = np.sort(np.asarray(values, dtype=np.float64))
    return len(v) < 2 or float(np.min(np.diff(v))) >= margin


def margins_hold(convert, logits, boxes, iou_pred, positive_map, C, run):
    """The assertions of the module docstring for one run on these inputs."""
    max_inst = 1 if run.get("task", "detection") == "grounding" else 100
    thres = run.get("score_thres", 0.0)
    for b in range(logits.shape[0]):
        prob = convert(logits[b:b + 1], C, positive_map)[0].sigmoid()
        if iou_pred is not None:
            prob = torch.sqrt(prob * iou_pred[b].sigmoid())
        if thres > 0:
            if float((prob - thres).abs().min()) < MARGIN:
                return False
            num_inst = min(int((prob > thres).sum()), max_inst)
            prob[prob <= thres] = -1.0
        else:
            num_inst = max_inst
        if C > 1:
            top2 = prob.topk(2, dim=1)[0]
            tied = top2[:, 0] == top2[:, 1]       # exactly equal (classes without tokens, or all -1.0): the first index wins
            if bool((~tied).any()) and float((top2[:, 0] - top2[:, 1])[~tied].min()) < MARGIN:
                return False
        if run["ota"]:
            s, idx = prob.max(1)
            if thres <= 0 and not gaps_ok(s):
                return False
            xyxy = pp.box_cxcywh_to_xyxy(boxes[b])
            off = xyxy + (idx.float() * (xyxy.max() + 1))[:, None]
            area = (off[:, 2] - off[:, 0]) * (off[:, 3] - off[:, 1])
            wh = (torch.min(off[:, None, 2:], off[None, :, 2:]) - torch.max(off[:, None, :2], off[None, :, :2])).clamp(min=0)
            inter = wh[..., 0] * wh[..., 1]
            iou = inter / (area[:, None] + area[None, :] - inter)
            if float((iou - pp.NMS_IOU_THRESHOLD).abs().min()) < MARGIN:
                return False
            if thres > 0:       # scores of -1.0 tie on purpose; what has to be apart is every pair that can suppress
                i, j = torch.nonzero(iou > pp.NMS_IOU_THRESHOLD, as_tuple=True)
                far = (s[i] - s[j]).abs() >= MARGIN
                if not bool((far | (i == j) | ((s[i] == -1) & (s[j] == -1))).all()):
                    return False
            keep = pp.batched_nms(xyxy, s, idx, pp.NMS_IOU_THRESHOLD)
            prob = prob[keep]
            if run.get("demo_only"):
                continue
        flat = prob.reshape(-1)
        num_inst = min(num_inst, flat.numel())
        top = flat.topk(min(num_inst + 1, flat.numel()))[0]
        top = top[top > 0]                        # the -1.0 entries a high threshold reaches are compared by count only
        if not gaps_ok(top):
            return False
    return True


CASES = {
    # name: (inputs, image sizes, runs)
    "coco_q300_t256": (dict(B=2, Q=300, T=256, C=80, empty=(7, 41), lo=0.5), [(800, 1200), (750, 1333)], {
        "ota": dict(ota=True),
        "topk_only": dict(ota=False),
        "demo_only": dict(ota=True, demo_only=True, score_thres=0.75),
        "thres_reaches_invalid": dict(ota=True, score_thres=0.9, prefix_only=True),
    }),
    "coco_q900_t64": (dict(B=1, Q=900, T=64, C=24, max_tokens=2, empty=(3,)), [(1000, 1333)], {
        "ota": dict(ota=True),
        "topk_only": dict(ota=False),
    }),
    "thres_few_q300_t64": (dict(B=2, Q=300, T=64, C=20, max_tokens=3, lo=0.02, hi=0.34, spread_top=40),
                           [(480, 640), (600, 900)], {
        "ota": dict(ota=True, score_thres=0.3),
        "topk_only": dict(ota=False, score_thres=0.3),
    }),
    "grounding_q300_t64": (dict(B=2, Q=300, T=64, C=1), [(480, 640), (333, 500)], {
        "ota": dict(ota=True, task="grounding"),
        "topk_only": dict(ota=False, task="grounding"),
    }),
    "noiou_q300_t64": (dict(B=2, Q=300, T=64, C=20, max_tokens=3, iou=False), [(480, 640), (640, 480)], {
        "ota": dict(ota=True),
        "demo_only": dict(ota=True, demo_only=True),
    }),
}


def main():
    inference, convert = load_reference()
    os.makedirs(OUT, exist_ok=True)
    for name, (kw, sizes, runs) in CASES.items():
        for seed in range(1, 400):
            logits, boxes, iou_pred, positive_map = make_inputs(seed, **kw)
            if all(margins_hold(convert, logits, boxes, iou_pred, positive_map, kw["C"], run) for run in runs.values()):
                break
        else:
            raise SystemExit("%s: no seed satisfies the margins" % name)
        B, Q = logits.shape[:2]
        assert all(w >= Q for _, w in sizes)      # the one-hot mask rows survive the crop to the image
        mask_pred = (torch.eye(Q) * 20 - 10).view(1, Q, 1, 1, Q).repeat(B, 1, 1, 1, 1)
        labels = sorted(positive_map)
        save = {"box_cls": logits.numpy(), "box_pred": boxes.numpy(), "image_sizes": np.asarray(sizes, dtype=np.int64),
                "num_classes": np.int64(kw["C"]), "seed": np.int64(seed), "pm_labels": np.asarray(labels, dtype=np.int64),
                "pm_ptr": np.cumsum([0] + [len(positive_map[l]) for l in labels]).astype(np.int64),
                "pm_tokens": np.asarray([t for l in labels for t in positive_map[l]], dtype=np.int64),
                "runs": np.asarray(sorted(runs))}
        if iou_pred is not None:
            save["iou_pred"] = iou_pred.numpy()
        for run, cfg in runs.items():
            me = types.SimpleNamespace(ota=cfg["ota"], demo_only=cfg.get("demo_only", False), mask_on=True, mask_stride=1,
                                       mask_thres=0.5)
            res = inference(me, logits.clone(), boxes.clone(), mask_pred, sizes, positive_map, kw["C"],
                            score_thres=cfg.get("score_thres", 0.0), task=cfg.get("task", "detection"),
                            iou_pred=iou_pred.clone() if iou_pred is not None else [None] * B)
            save[run + ".ota"] = np.bool_(cfg["ota"])
            save[run + ".demo_only"] = np.bool_(cfg.get("demo_only", False))
            save[run + ".score_thres"] = np.float64(cfg.get("score_thres", 0.0))
            save[run + ".task"] = np.asarray(cfg.get("task", "detection"))
            save[run + ".prefix_only"] = np.bool_(cfg.get("prefix_only", False))
            counts = []
            for b, r in enumerate(res):
                assert r.pred_masks.sum() == len(r.scores) and len(r.scores) > 0
                save["%s.scores_%d" % (run, b)] = r.scores.numpy()
                save["%s.classes_%d" % (run, b)] = r.pred_classes.numpy()
                save["%s.boxes_%d" % (run, b)] = r.pred_boxes.tensor.numpy()
                save["%s.query_%d" % (run, b)] = r.pred_masks[:, 0, 0, :].float().argmax(-1).numpy()
                counts.append((len(r.scores), int((r.scores > 0).sum())))
            if cfg.get("prefix_only"):
                assert all(v < n for n, v in counts), counts        # top-k did reach the -1.0 entries
            elif cfg.get("score_thres", 0.0) > 0 and not cfg.get("demo_only"):
                assert all(v == n < 100 for n, v in counts), counts
            print(name, run, "seed", seed, counts)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **save)
        print(path, os.path.getsize(path) // 1024, "KB")
        assert os.path.getsize(path) <= 640 * 1024


if __name__ == "__main__":
    main()
