"""What tests/test_postprocess_cpu.py and tests/test_postprocess_gpu.py share: the reference's fixtures
(tests/golden/postprocess/*.npz, minted by tests/golden/make_postprocess_golden.py), seeded inputs for the two kernels with
the margins that allow exact comparisons, and the hand-built NMS cases."""
import functools
import glob
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "postprocess")
FIXTURES = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
EXPECTED_FIXTURES = ["coco_q300_t256", "coco_q900_t64", "grounding_q300_t64", "noiou_q300_t64", "thres_few_q300_t64"]
MARGIN = 1e-4        # the project's fp32 tolerance; what the generators keep every decision away from its threshold


@functools.lru_cache(maxsize=None)
def load(name):
    """The fixture as a dict: tensors of the inputs, the positive map, and {run: (config, [expected per image])}."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    positive_map = {int(l): [int(t) for t in z["pm_tokens"][a:b]]
                    for l, a, b in zip(z["pm_labels"], z["pm_ptr"][:-1], z["pm_ptr"][1:])}
    B = z["box_cls"].shape[0]
    runs = {}
    for run in (str(r) for r in z["runs"]):
        cfg = dict(ota=bool(z[run + ".ota"]), demo_only=bool(z[run + ".demo_only"]), score_thres=float(z[run + ".score_thres"]),
                   task=str(z[run + ".task"]), prefix_only=bool(z[run + ".prefix_only"]))
        expect = [dict(scores=z["%s.scores_%d" % (run, b)], classes=z["%s.classes_%d" % (run, b)],
                       boxes=z["%s.boxes_%d" % (run, b)], query=z["%s.query_%d" % (run, b)]) for b in range(B)]
        runs[run] = (cfg, expect)
    return dict(box_cls=torch.from_numpy(z["box_cls"]), box_pred=torch.from_numpy(z["box_pred"]),
                iou_pred=torch.from_numpy(z["iou_pred"]) if "iou_pred" in z else None,
                image_sizes=[tuple(int(v) for v in s) for s in z["image_sizes"]], num_classes=int(z["num_classes"]),
                positive_map=positive_map, runs=runs)


RUNS = [(name, run) for name in EXPECTED_FIXTURES for run in
        {"coco_q300_t256": ("ota", "topk_only", "demo_only", "thres_reaches_invalid"), "coco_q900_t64": ("ota", "topk_only"),
         "thres_few_q300_t64": ("ota", "topk_only"), "grounding_q300_t64": ("ota", "topk_only"),
         "noiou_q300_t64": ("ota", "demo_only")}[name]]


def check_against_fixture(post, name, run, device="cpu"):
    """post: a DetectionPostProcess factory (ota, demo_only) -> object.  Indices and labels exact, scores and boxes within
    MARGIN; a run whose top-k reaches the -1.0 entries is compared on its count and its valid prefix."""
    fx = load(name)
    cfg, expect = fx["runs"][run]
    to = lambda t: None if t is None else t.to(device)
    got = post(cfg["ota"], cfg["demo_only"])(to(fx["box_cls"]), to(fx["box_pred"]), to(fx["iou_pred"]), fx["image_sizes"],
                                             fx["positive_map"], fx["num_classes"], score_thres=cfg["score_thres"],
                                             task=cfg["task"])
    assert len(got) == len(expect)
    for g, e, size in zip(got, expect, fx["image_sizes"]):
        n = len(e["scores"])
        assert len(g["scores"]) == len(g["pred_classes"]) == len(g["pred_boxes"]) == len(g["query_index"]) == n
        m = int((e["scores"] > 0).sum()) if cfg["prefix_only"] else n
        assert cfg["prefix_only"] == (m < n)
        assert g["query_index"].dtype == torch.int64 and g["pred_classes"].dtype == torch.int64
        np.testing.assert_array_equal(g["query_index"][:m].cpu().numpy(), e["query"][:m])
        np.testing.assert_array_equal(g["pred_classes"][:m].cpu().numpy(), e["classes"][:m])
        np.testing.assert_allclose(g["scores"][:m].cpu().numpy(), e["scores"][:m], rtol=0, atol=MARGIN)
        np.testing.assert_array_equal(g["scores"][m:].cpu().numpy(), e["scores"][m:])          # exactly -1.0
        # boxes are in pixels: the tolerance of a [0, 1] coordinate times the image's larger side
        np.testing.assert_allclose(g["pred_boxes"][:m].cpu().numpy(), e["boxes"][:m], rtol=0, atol=MARGIN * max(size))
    return got


def literal_convert(logits, num_classes, positive_map):
    """convert_grounding_to_od_logits as a literal loop over the labels."""
    scores = torch.zeros(logits.shape[0], logits.shape[1], num_classes)
    for label, tokens in positive_map.items():
        scores[:, :, label - 1] = logits[:, :, torch.LongTensor(tokens)].mean(-1)
    return scores


def random_positive_map(g, C, T, empty=(), long_class=None):
    """{label: tokens}: 1 to 4 tokens a class drawn from [0, T), none for `empty`, six for `long_class`."""
    pm = {}
    for c in range(C):
        if c in empty:
            continue
        n = 6 if c == long_class else int(torch.randint(1, 5, (1,), generator=g))
        pm[c + 1] = [int(t) for t in torch.randint(0, T, (min(n, T),), generator=g)]
    return pm


SCORE_CONFIGS = [(False, 0.0), (False, 0.3), (True, 0.0), (True, 0.3)]      # (with IoU logits, score threshold)


def _score_tables(logits, iou, pm, C):
    """{config: (prob before the threshold, prob, valid)} by the composition."""
    from uninext_amd.postprocess import convert_grounding_to_od_logits
    out = {}
    for with_iou, thres in SCORE_CONFIGS:
        raw = convert_grounding_to_od_logits(logits, C, pm).sigmoid()
        if with_iou:
            raw = torch.sqrt(raw * iou.unsqueeze(-1).sigmoid())
        valid = raw > thres
        out[(with_iou, thres)] = (raw, raw.masked_fill(~valid, -1.0) if thres > 0 else raw, valid)
    return out


def _too_close(tables, C, band):
    """[(b, q, best class, second class or -1)] of the decisions that lie within `band` of their threshold."""
    bad = set()
    for (with_iou, thres), (raw, prob, _) in tables.items():
        if thres > 0:
            for b, q, c in torch.nonzero((raw - thres).abs() < band).tolist():
                bad.add((b, q, c, -1))
        if C > 1:
            vals, idx = prob.topk(2, dim=-1)
            # exactly equal entries (a row of -1.0, two classes of the same tokens) are decided by the first-index rule
            close = (vals[..., 0] - vals[..., 1] < band) & (vals[..., 0] != vals[..., 1])
            for b, q in torch.nonzero(close).tolist():
                bad.add((b, q, int(idx[b, q, 0]), int(idx[b, q, 1])))
    return bad


@functools.lru_cache(maxsize=None)
def scores_case(Q, C, T, B=2):
    """Seeded inputs of detpost_scores, nudged until every row's best class is MARGIN ahead of the second and every entry MARGIN
    away from the threshold 0.3 (asserted); (logits, iou, positive_map, {(with_iou, thres): (prob, max, arg, valid counts) by
    the composition})."""
    g = torch.Generator().manual_seed(1000 + Q + C + T)
    pm = random_positive_map(g, C, T, empty=(1,) if C > 2 else (), long_class=2 if C > 2 and T >= 6 else None)
    logits = torch.randn(B, Q, T, generator=g) * 2.0 - 1.0
    iou = torch.randn(B, Q, generator=g) * 2.0
    for _ in range(100):
        bad = _too_close(_score_tables(logits, iou, pm, C), C, 2 * MARGIN)
        if not bad:
            break
        for b, q, c, second in bad:
            if c + 1 in pm:
                logits[b, q, pm[c + 1][0]] += 0.05
            elif second >= 0 and second + 1 in pm:
                logits[b, q, pm[second + 1][0]] -= 0.05
            else:
                iou[b, q] += 0.05
    tables = _score_tables(logits, iou, pm, C)
    assert not _too_close(tables, C, MARGIN)
    expect = {}
    for cfg, (raw, prob, valid) in tables.items():
        mx, arg = prob.max(-1)
        expect[cfg] = (prob, mx, arg, valid.sum(-1) if cfg[1] > 0 else torch.zeros(B, Q, dtype=torch.long))
    return logits, iou, pm, expect


def iou_matrix(xyxy):
    area = (xyxy[:, 2] - xyxy[:, 0]) * (xyxy[:, 3] - xyxy[:, 1])
    wh = (torch.min(xyxy[:, None, 2:], xyxy[None, :, 2:]) - torch.max(xyxy[:, None, :2], xyxy[None, :, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (area[:, None] + area[None, :] - inter)


@functools.lru_cache(maxsize=None)
def nms_case(Q, B, iou_threshold=0.7):
    """Seeded (boxes [B, Q, 4] cxcywh, scores [B, Q], classes [B, Q] int32) with heavy overlap (clustered centres, sizes 0.02 to
    0.4, near-duplicates, a few classes) and DISTINCT scores, and per mode the CPU restatement's (keep, n_keep, kept_mask).
    Asserted on the CPU: no IoU, of the offset boxes or of the plain ones, lies within MARGIN of the threshold."""
    from uninext_amd.postprocess import _greedy_nms, box_cxcywh_to_xyxy
    for seed in range(200):
        g = torch.Generator().manual_seed(7000 + 31 * Q + B + 1000 * seed)
        centres = 0.2 + 0.6 * torch.rand(B, 6, 2, generator=g)
        cluster = torch.randint(0, 6, (B, Q), generator=g)
        cxcy = torch.gather(centres, 1, cluster.unsqueeze(-1).expand(-1, -1, 2)) + 0.03 * torch.randn(B, Q, 2, generator=g)
        wh = 0.02 + 0.38 * torch.rand(B, Q, 2, generator=g)
        cls = torch.randint(0, 4, (B, Q), generator=g).int()
        for b in range(B):
            for q in range(Q // 2, Q):          # near-duplicates of the first half
                t = int(torch.randint(0, max(Q // 2, 1), (1,), generator=g))
                cxcy[b, q] = cxcy[b, t] + 0.004 * torch.randn(2, generator=g)
                wh[b, q] = wh[b, t] * (1 + 0.03 * torch.randn(2, generator=g))
                if q % 3:
                    cls[b, q] = cls[b, t]
        boxes = torch.cat([cxcy, wh], -1)
        scores = torch.stack([(torch.randperm(Q, generator=g).float() + 0.5) / Q for _ in range(B)])
        expect, ok = {0: [], 1: []}, True
        for b in range(B):
            xyxy = box_cxcywh_to_xyxy(boxes[b])
            off = xyxy + (cls[b].float() * (xyxy.max() + 1))[:, None]
            same = cls[b][:, None] == cls[b][None, :]
            ok &= float((iou_matrix(off) - iou_threshold).abs().min()) >= MARGIN
            ok &= float((iou_matrix(xyxy) - iou_threshold).abs()[same].min()) >= MARGIN
            expect[0].append(_greedy_nms(off, scores[b], iou_threshold))
            expect[1].append(_greedy_nms(xyxy, scores[b], iou_threshold, classes=cls[b]))
        if ok:
            return boxes, scores, cls, expect
    raise AssertionError("no seed gives the IoU margin for Q=%d B=%d" % (Q, B))


def hand_cases():
    """{name: (boxes xyxy [N, 4], scores [N], classes [N], expected keep)} at threshold 0.5."""
    f = lambda rows: torch.tensor(rows, dtype=torch.float32)
    return {
        # A (0..10) and B (3..13): IoU 7/13 > 0.5; B and C (6..16): the same; A and C: 4/16: A removes B, C stays
        "chain": (f([[0, 0, 10, 10], [3, 0, 13, 10], [6, 0, 16, 10]]), f([0.9, 0.8, 0.7]), [0, 0, 0], [0, 2]),
        "identical_two_classes": (f([[1, 1, 5, 5], [1, 1, 5, 5]]), f([0.6, 0.9]), [0, 1], [1, 0]),
        "identical_one_class": (f([[1, 1, 5, 5], [1, 1, 5, 5]]), f([0.6, 0.9]), [2, 2], [1]),
        # zero area: 0 / 0 is NaN and NaN > threshold is false
        "zero_area": (f([[2, 2, 2, 2], [2, 2, 2, 2], [0, 0, 0, 0]]), f([0.5, 0.4, 0.3]), [0, 0, 0], [0, 1, 2]),
        "equal_scores": (f([[0, 0, 4, 4], [10, 10, 14, 14], [0, 0, 4, 4.1], [20, 20, 24, 24]]), f([0.5, 0.5, 0.5, 0.5]),
                         [0, 0, 0, 0], [0, 1, 3]),
    }


def xyxy_to_cxcywh(b):
    return torch.stack([(b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], -1)
