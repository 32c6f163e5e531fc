"""The online tracker without a GPU: uninext_amd.tracker.IDOL_Tracker's composition route (the reference's composition, which is
also what the fused route is compared with) against the reference's recorded frames (tests/golden/tracker/*.npz, minted by
tests/golden/make_tracker_golden.py) and against the float64 restatement (tests/tracker_ref.py); the conditions the cases must
meet (the float64 margin of every decision, the edges each case is there for); the table of torch.range the kernels' temporal
weights rest on; and the public surface against the reference's recorded signature."""
import functools
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tracker_cases as C  # noqa: E402
import tracker_ref  # noqa: E402

from uninext_amd.tracker import IDOL_Tracker, temporal_table, temporal_weights  # noqa: E402


@functools.lru_cache(maxsize=None)
def ref64(name):
    return tracker_ref.run(name, C)


@functools.lru_cache(maxsize=None)
def composition(name):
    tracker = IDOL_Tracker(fused=False, **C.CASES[name][3])
    return C.run(tracker, name), tracker


@pytest.mark.parametrize("name", list(C.CASES))
def test_every_decision_of_every_frame_keeps_the_float64_margin(name):
    """A condition on the INPUTS (a case that misses it is re-seeded), not a tolerance: an fp32 dot product of 256 terms with
    |feats| <= 8 is off by at most about 256 * 2^-24 * 8 = 1.2e-4 and a softmax's derivative is at most 1/4."""
    margins = ref64(name)["margins"]
    print(name, ["%.2e" % m for m in margins])
    assert len(margins) == len(C.frames(name)) and min(margins) >= C.MARGIN
    assert 8 <= len(margins) <= 14
    assert all(fr["masks"].shape[1:] == (1, 12, 20) for fr in C.frames(name))
    assert max(float((fr["embeds"].double().norm(dim=1) ** 2).max()) for fr in C.frames(name)) <= 8.0


def test_the_cases_reach_the_edges_they_are_there_for():
    n = [len(fr["indices"]) for fr in C.frames("waves")]
    assert {1, 63, 64, 65} <= set(n)
    live = [len([i for i in ids if i >= 0]) for ids, _, _ in ref64("waves")["frames"]]
    assert live[1] == 64 and live[2] == 65 and n[3] == 65                  # 65 rows against 64, then 65 live columns
    events = ref64("bookkeeping")["events"]
    assert {"reappeared_after_2", "reappeared_after_3", "expired", "ring_wrapped", "memory_emptied"} <= events
    assert C.CASES["bookkeeping"][3] == dict(memo_tracklet_frames=3, memory_len=3)
    frames = ref64("bookkeeping")["frames"]
    assert frames[4][0][3] == 4 and frames[9][0] == [5, 6]                 # object 3 came back as a new identity; a fresh start
    assert {"column_zeroed_under_a_rival", "backdrop", "backdrop_first", "left_unselected"} <= ref64("decisions")["events"]
    assert ref64("decisions")["frames"][2][2] == 6                          # the pre-NMS dropped the duplicate
    assert {"frame_weight", "frame_weight_changed_winner"} <= ref64("frame_weight")["events"]
    assert C.CASES["d8"][1] == 8 and C.CASES["bookkeeping_long"][3]["long_match"]
    assert C.CASES["bookkeeping_long_temporal"][3]["temporal_weight"]
    grow = [len(fr["indices"]) for fr in C.frames(C.OVERFLOW_CASE)]
    assert grow[0] <= C.OVERFLOW_CAPACITY and 2 + grow[1] <= C.OVERFLOW_CAPACITY < 2 + grow[2]


@pytest.mark.parametrize("name", list(C.CASES))
def test_composition_reproduces_every_golden_frame_and_the_float64_integers(name):
    got, _ = composition(name)
    gold = C.golden(name)
    assert gold["seed"] == C.CASES[name][2] and len(gold["frames"]) == len(got)
    for t, (frame, want, want64) in enumerate(zip(got, gold["frames"], ref64(name)["frames"])):
        assert frame == want, (name, t)
        assert frame == want64, (name, t)


@pytest.mark.parametrize("name", list(C.CASES))
def test_composition_final_memo_against_float64_and_the_golden(name):
    _, tracker = composition(name)
    memo = C.memo_arrays(tracker.memo)
    C.assert_memo_close(memo, ref64(name)["memo"], name)
    for key in ("embeds", "long_embeds"):
        memo[key + "_rowsum"] = memo.pop(key).sum(1)
    C.assert_memo_close(memo, C.golden(name)["memo"], name + " (golden)")
    assert tracker.num_tracklets == 1 + max(max(ids, default=-1) for ids, _, _ in C.golden(name)["frames"])
    assert not tracker.empty and list(tracker.tracklets) == [int(i) for i in memo["ids"]]


def test_torch_range_gives_length_entries_k_over_length():
    """tracker.py:183: torch.range(0.0, 1, 1 / length)[1:] has `length` entries, float32(k / length) for k = 1 .. length, for
    every length up to the largest memory_len the tests use (and the default 10); the kernels read this table."""
    top = max([10] + [kw.get("memory_len", 10) for _, _, _, kw in C.CASES.values()])
    for length in range(1, top + 1):
        w = temporal_weights(length)
        assert w.dtype == torch.float32 and w.numel() == length
        assert np.array_equal(w.numpy(), (np.arange(1, length + 1, dtype=np.float64) / length).astype(np.float32)), length
    table = temporal_table(top)
    assert tuple(table.shape) == (top + 1, top) and float(table[3, 2]) == 1.0 and float(table[3, 3:].abs().sum()) == 0.0


def test_public_surface_is_the_references():
    with open(os.path.join(C.GOLDEN, "signature.json")) as f:
        want = json.load(f)
    init = [[k, v.default] for k, v in inspect.signature(IDOL_Tracker.__init__).parameters.items() if k != "self"]
    assert init[:len(want["init"])] == want["init"]
    assert [k for k, _ in init[len(want["init"]):]] == ["capacity", "fused"] and init[len(want["init"])][1] == 1024
    assert [k for k in inspect.signature(IDOL_Tracker.match).parameters if k != "self"] == want["match"]
    for member in ("match", "update_memo", "memo", "empty", "tracklets", "backdrops"):
        assert hasattr(IDOL_Tracker, member)
    import uninext_amd
    assert uninext_amd.IDOL_Tracker is IDOL_Tracker
    tracker = IDOL_Tracker()
    assert tracker.empty and tracker.num_tracklets == 0 and tracker.tracklets == {} and tracker.backdrops == []
    from uninext_amd import postprocess, tracker as module
    assert module.mask_nms is postprocess.mask_nms and module.mask_iou is postprocess.mask_iou


def test_cpu_inputs_take_the_composition_whatever_fused_says():
    tracker = IDOL_Tracker(fused=True, **C.CASES["decisions"][3])
    assert C.run(tracker, "decisions") == C.golden("decisions")["frames"]
    assert tracker._bank is None and len(tracker.backdrops) == 1
    frames = ref64("decisions")["frames"]
    assert tracker.backdrops[0]["bboxes"].shape[0] == sum(i == -1 for i in frames[-1][0])
