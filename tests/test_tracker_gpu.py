"""The online tracker's kernels on the GPU (include/dynmask_hip.h: track_hip_*; uninext_amd.tracker.IDOL_Tracker with fused =
True) on the sequences of tests/tracker_cases.py: every frame's ids, indices and kept count against the reference's record
(tests/golden/tracker/*.npz), the final memo against the float64 restatement (tests/tracker_ref.py), repeatability, the one host
copy per call, the lazily built tracklets / backdrops against the composition's, and the fallback after a capacity overflow."""
import functools
import os
import sys
import warnings

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tracker_cases as C  # noqa: E402
import tracker_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def ref64(name):
    return tracker_ref.run(name, C)


@functools.lru_cache(maxsize=None)
def fused(name):
    from uninext_amd.tracker import IDOL_Tracker
    tracker = IDOL_Tracker(fused=True, **C.CASES[name][3])
    return C.run(tracker, name, DEV), tracker


@pytest.mark.parametrize("name", list(C.CASES))
def test_fused_reproduces_every_golden_frame(name):
    from uninext_amd import _lib
    got, tracker = fused(name)
    assert tracker._bank is not None and _lib.last_kernel("track") == "track_update"      # the kernels ran, to the last frame
    gold = C.golden(name)["frames"]
    assert len(got) == len(gold)
    for t, (frame, want) in enumerate(zip(got, gold)):
        assert frame == want, (name, t, frame, want)
    assert tracker.num_tracklets == 1 + max(max(ids, default=-1) for ids, _, _ in gold)
    assert tracker._bank.count == len(ref64(name)["memo"]["ids"]) and not tracker.empty


@pytest.mark.parametrize("name", list(C.CASES))
def test_fused_final_memo_against_float64(name):
    _, tracker = fused(name)
    C.assert_memo_close(C.memo_arrays(tracker.memo), ref64(name)["memo"], name)


@pytest.mark.parametrize("name", ["waves", "bookkeeping_long_temporal", "frame_weight"])
def test_two_runs_give_the_same_bits(name):
    from uninext_amd.tracker import IDOL_Tracker
    _, first = fused(name)
    second = IDOL_Tracker(fused=True, **C.CASES[name][3])
    assert C.run(second, name, DEV) == fused(name)[0]
    for a, b in zip(first._bank.states, second._bank.states):
        assert torch.equal(a.buffer, b.buffer)


def test_one_host_copy_per_match():
    from uninext_amd.tracker import IDOL_Tracker
    frames = [{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in fr.items()} for fr in C.frames("decisions")]
    tracker = IDOL_Tracker(fused=True, **C.CASES["decisions"][3])
    counts = []
    for t, fr in enumerate(frames):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                tracker.match(fr["bboxes"], fr["labels"], fr["masks"], fr["embeds"], fr["frame_id"], list(fr["indices"]))
        finally:
            torch.cuda.set_sync_debug_mode("default")
        counts.append(sum("synchroniz" in str(w.message).lower() for w in seen))
    print("synchronising calls per frame:", counts)
    assert tracker._bank is not None
    assert counts == [1] * len(frames)


@pytest.mark.parametrize("name", ["decisions", "bookkeeping_long"])
def test_lazy_tracklets_and_backdrops_agree_with_the_composition(name):
    from uninext_amd.tracker import IDOL_Tracker
    _, tracker = fused(name)
    plain = IDOL_Tracker(fused=False, **C.CASES[name][3])
    assert C.run(plain, name, DEV) == fused(name)[0] and plain._bank is None
    a, b = tracker.tracklets, plain.tracklets
    assert list(a) == list(b)
    for key in a:
        for field in ("last_frame", "acc_frame", "exist_frame"):
            assert a[key][field] == b[key][field], (key, field)
        assert int(a[key]["label"]) == int(b[key]["label"]) and len(a[key]["long_embed"]) == len(b[key]["long_embed"])
        for field in ("bbox", "embed", "velocity"):
            torch.testing.assert_close(a[key][field], b[key][field], rtol=0, atol=1e-4 * max(float(b[key][field].abs().max()), 1e-30))
        torch.testing.assert_close(torch.stack(a[key]["long_embed"]), torch.stack(b[key]["long_embed"]), rtol=0, atol=0)
        torch.testing.assert_close(torch.stack(a[key]["long_score"]), torch.stack(b[key]["long_score"]), rtol=0, atol=0)
    assert len(tracker.backdrops) == len(plain.backdrops) == 1
    for field in ("bboxes", "embeds", "labels"):
        assert torch.equal(tracker.backdrops[0][field], plain.backdrops[0][field]), field


def test_capacity_overflow_falls_back_and_keeps_the_identities():
    from uninext_amd.tracker import IDOL_Tracker
    name = C.OVERFLOW_CASE
    tracker = IDOL_Tracker(fused=True, capacity=C.OVERFLOW_CAPACITY, **C.CASES[name][3])
    assert C.run(tracker, name, DEV, upto=2) == C.golden(name)["frames"][:2]
    assert tracker._bank is not None and tracker._bank.count == 2
    rest = C.run(tracker, name, DEV, frames_=C.frames(name)[2:])
    assert rest == C.golden(name)["frames"][2:]
    assert tracker._bank is None and len(tracker.tracklets) == len(ref64(name)["memo"]["ids"])
    C.assert_memo_close(C.memo_arrays(tracker.memo), ref64(name)["memo"], name)
