"""Per-entry parity of the QuasiDense tracker's kernels on the GPU, each entry point called on its own through uninext_amd.ext
(tests/qdtrack_parity.py has the cases, the restatements and what each comparison means)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qdtrack_cases as C  # noqa: E402
import qdtrack_parity as P  # noqa: E402
import tracker_parity as TP  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def device_bank(x, frames=1):
    from uninext_amd import ext
    s = ext.QDTrackState(x["C"], x["D"], x["B"], frames, DEV)
    M, b = x["M"], x["b"]
    for field in ("id", "label", "bbox", "velocity", "last_frame", "acc_frame", "embed"):
        getattr(s, field)[:M] = torch.from_numpy(x["state"][field]).to(DEV)
    for field in ("label", "bbox", "embed"):
        getattr(s, "backdrop_" + field)[0, :b] = torch.from_numpy(x["state"]["backdrop_" + field]).to(DEV)
    s.meta[:3] = torch.tensor([M, x["num_tracklets"], b], device=DEV)
    return s, ext.QDTrackState(x["C"], x["D"], x["B"], frames, DEV)


@pytest.mark.parametrize("n", P.PREPARE_NS)
def test_prepare_order_iou_bits_and_valid_flags(n):
    from uninext_amd import _lib, ext
    bboxes = P.prepare_inputs(n)
    want_order, want_iou, want_valid = P.prepare_expected(bboxes)
    order, iou, valid = ext.qdtrack_prepare(torch.from_numpy(bboxes).to(DEV), P.OBJ_THR, P.BACKDROP_THR, P.CLASS_THR)
    assert _lib.last_kernel("qdtrack") == "qdtrack_prepare"
    assert np.array_equal(order.cpu().numpy(), want_order)
    if n > 2:
        at = want_order.tolist()
        assert at.index(0) + 1 == at.index(n - 1)          # the planted tie: the lower index first
    assert np.array_equal(iou.cpu().numpy().view(np.int32), want_iou.view(np.int32))
    assert np.array_equal(valid.cpu().numpy(), want_valid)
    print("n %d: %d of %d rows valid" % (n, int(want_valid.sum()), n))
    assert n < 60 or 1 < int(want_valid.sum()) < n


@pytest.mark.parametrize("with_cats", [False, True])
@pytest.mark.parametrize("name", list(P.BANKS))
def test_scores_against_float64(name, with_cats):
    from uninext_amd import ext
    x = P.bank_inputs(name)
    n, M, b = x["n"], x["M"], x["b"]
    cur, _ = device_bank(x)
    g = np.random.RandomState(n + M)
    order = g.permutation(n).astype(np.int32)
    valid = TP.keep_pattern("alt" if n > 1 else "all", n)
    sorted_embeds, sorted_labels = x["embeds"][order], x["labels"][order]
    ref = TP.scores64(P.as_score_bank(x), sorted_embeds, valid, False, None)
    gate = sorted_labels[:, None] == np.concatenate([x["state"]["label"], x["state"]["backdrop_label"]])[None, :]
    want, mag = ref["scores"], ref["mag_scores"]
    kept = np.flatnonzero(valid)
    memo = torch.from_numpy(np.concatenate([x["state"]["embed"], x["state"]["backdrop_embed"]]))
    feats = torch.mm(torch.from_numpy(sorted_embeds[kept]), memo.t())
    comp = np.full(want.shape, np.nan)
    comp[kept] = ((feats.softmax(dim=1) + feats.softmax(dim=0)) / 2).double().numpy()
    if with_cats:
        want, mag, comp = want * gate, mag * gate, comp * gate
    got = ext.qdtrack_scores(torch.from_numpy(x["embeds"]).to(DEV), torch.from_numpy(x["labels"]).to(DEV), torch.from_numpy(order).to(DEV),
                             torch.from_numpy(valid).to(DEV), cur, M, [b], with_cats).cpu().double().numpy()
    got[valid == 0] = np.nan                    # rows the pre-NMS dropped are not written
    worst = TP.measure("%s%s" % (name, "_cats" if with_cats else ""), "scores", "plain", got, want, mag, comp)
    print(TP.TABLE[-1] if TP.TABLE else "", "worst error / bound %.3f" % worst)
    if with_cats:
        assert (got[kept][~gate[kept]] == 0).all()


@pytest.mark.parametrize("name", list(P.SAME_BITS))
def test_both_trackers_score_the_same_bank_to_the_same_bits(name):
    """track_scores and qdtrack_scores run one score core (csrc/track_bank.hpp): M tracklets and no backdrops, no class gate,
    the identity order and the same flags give the same int32 views in the kept rows."""
    from uninext_amd import ext
    x = P.bank_inputs(name)
    n, M, D = x["n"], x["M"], x["D"]
    assert x["b"] == 0
    flags = torch.from_numpy(TP.keep_pattern("alt", n)).to(DEV)
    embeds, labels = torch.from_numpy(x["embeds"]).to(DEV), torch.from_numpy(x["labels"]).to(DEV)
    qd, _ = device_bank(x)
    order = torch.arange(n, dtype=torch.int32, device=DEV)
    got_qd = ext.qdtrack_scores(embeds, labels, order, flags, qd, M, [0], False)
    idol = ext.TrackState(x["C"], D, 1, DEV)
    idol.embed[:M] = torch.from_numpy(P.as_score_bank(x)["embed"][:M]).to(DEV)
    got_idol = ext.track_scores(embeds, flags, idol, M, False)
    kept = flags.bool()
    assert got_qd.shape == got_idol.shape == (n, M) and int(kept.sum()) == (n + 1) // 2
    assert not torch.isnan(got_qd[kept]).any()
    assert torch.equal(got_qd[kept].view(torch.int32), got_idol[kept].view(torch.int32))


@pytest.mark.parametrize("name", list(P.STEPS))
def test_a_whole_step_against_float64(name):
    from uninext_amd import ext
    x = P.bank_inputs(name)
    n, M, b = x["n"], x["M"], x["b"]
    ref = P.reference_tracker(x)
    t = lambda a: torch.from_numpy(a)
    ids64, ind64, kept64, margin, _ = ref.match(t(x["bboxes"]), t(x["labels"]), t(x["embeds"]), x["frame_id"], list(range(n)))
    print(name, "float64 margin %.2e, %d rows kept, events %s" % (margin, kept64, sorted(set(ref.events))))
    assert margin >= C.MARGIN                    # a condition on the inputs
    cur, nxt = device_bank(x)
    bboxes, labels, embeds = t(x["bboxes"]).to(DEV), t(x["labels"]).to(DEV), t(x["embeds"]).to(DEV)
    order, iou, valid = ext.qdtrack_prepare(bboxes, ref.obj_score_thr, ref.nms_backdrop_iou_thr, ref.nms_class_iou_thr)
    scores = ext.qdtrack_scores(embeds, labels, order, valid, cur, M, [b], True)
    plan, result = ext.qdtrack_associate(scores, valid, order, bboxes, iou, cur, nxt, M, [b], ref.match_score_thr, ref.obj_score_thr,
                                         ref.nms_conf_thr, ref.init_score_thr, ref.nms_backdrop_iou_thr, x["frame_id"], 3)
    ext.qdtrack_update(embeds, bboxes, labels, order, plan, result, cur, nxt, M, [b], x["momentum"], x["frame_id"])
    host = result.cpu().tolist()
    kept, count, num, drops = host[3 * n:3 * n + 4]
    assert kept == kept64 and host[n:n + kept] == ids64 and host[2 * n:2 * n + kept] == ind64
    want = ref.memo()
    assert count == len(want["last_frame"]) and num == ref.num_tracklets and [drops] == want["backdrop_rows"].tolist()
    assert nxt.meta.tolist()[:3] == [count, num, drops]
    f = lambda a: a.cpu().numpy().astype(np.float64 if a.is_floating_point() else np.int64)
    got = dict(bboxes=np.concatenate([f(nxt.bbox[:count]), f(nxt.backdrop_bbox[0, :drops])]),
               labels=np.concatenate([f(nxt.label[:count]), f(nxt.backdrop_label[0, :drops])]),
               embeds=np.concatenate([f(nxt.embed[:count]), f(nxt.backdrop_embed[0, :drops])]),
               ids=np.concatenate([f(nxt.id[:count]), np.full(drops, -1, dtype=np.int64)]),
               vs=np.concatenate([f(nxt.velocity[:count]), np.zeros((drops, 5))]),
               last_frame=f(nxt.last_frame[:count]), acc_frame=f(nxt.acc_frame[:count]), backdrop_rows=np.asarray([drops], dtype=np.int64))
    C.assert_memo_close(got, want, name)
