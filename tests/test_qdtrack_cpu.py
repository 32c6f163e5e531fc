"""The QuasiDense tracker without a GPU: uninext_amd.tracker.QuasiDenseEmbedTracker's composition route (the reference's
composition, which is also what the fused route is compared with) against the reference's recorded frames
(tests/golden/qdtrack/*.npz, minted by tests/golden/make_qdtrack_golden.py) and against the float64 restatement
(tests/qdtrack_ref.py); the conditions the cases must meet (the float64 margin of every decision, the edges each case is there
for); the restated bbox_overlaps against the reference's bits; the public surface against the reference's recorded signature;
and the new exports and the kernels' resources."""
import ctypes
import functools
import inspect
import json
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import qdtrack_cases as C  # noqa: E402
import qdtrack_ref  # noqa: E402

from uninext_amd.tracker import QuasiDenseEmbedTracker, bbox_overlaps  # noqa: E402

EXPORTS = ("qdtrack_hip_state_offset", "qdtrack_hip_prepare_f32", "qdtrack_hip_scores_f32", "qdtrack_hip_associate_f32",
           "qdtrack_hip_update_f32", "qdtrack_hip_last_kernel")
KERNELS = ("rank", "iou_valid", "feats_rows", "cols_final", "associate", "update")


@functools.lru_cache(maxsize=None)
def ref64(name):
    return qdtrack_ref.run(name, C)


@functools.lru_cache(maxsize=None)
def composition(name):
    tracker = QuasiDenseEmbedTracker(fused=False, **C.CASES[name][3])
    return C.run(tracker, name), tracker


@pytest.mark.parametrize("name", list(C.CASES))
def test_every_decision_of_every_frame_keeps_the_float64_margin(name):
    """A condition on the INPUTS (a case that misses it is re-seeded), not a tolerance: an fp32 dot product of 256 terms with
    |feats| <= 8 is off by at most about 256 * 2^-24 * 8 = 1.2e-4 and a softmax's derivative is at most 1/4; a box IoU of
    coordinates below 2^8 is off by a few 2^-24."""
    margins = ref64(name)["margins"]
    print(name, ["%.2e" % m for m in margins])
    assert len(margins) == len(C.frames(name)) and min(margins) >= C.MARGIN
    assert 8 <= len(margins) <= 14
    assert max(float((fr["embeds"].double().norm(dim=1) ** 2).max()) for fr in C.frames(name)) <= 8.0
    shuffled = [fr["bboxes"][:, 4].argsort(descending=True).tolist() != list(range(len(fr["indices"]))) for fr in C.frames(name)]
    assert sum(shuffled) >= len(shuffled) // 2      # the rows do not arrive in score order, or the sort would go untested


def test_the_cases_reach_the_edges_they_are_there_for():
    kept = lambda name: [k for _, _, k in ref64(name)["frames"]]
    assert {1, 63, 64, 65} <= set(kept("waves"))
    assert {(63, 0), (64, 0), (65, 0)} <= set(ref64("waves")["columns"])               # 64 | 65 among the tracklets
    assert {(60, 3), (60, 4), (60, 5)} <= set(ref64("waves_backdrops")["columns"])     # 64 | 65 among the backdrops
    assert {C.CASES[n][1] for n in C.CASES} == {6, 8, 256}
    events = ref64("bookkeeping")["events"]
    assert {"reappeared_after_2", "reappeared_after_3", "expired", "memory_emptied", "no_tracklets_while_backdrops_exist",
            "starts_no_tracklet_while_backdrops_exist"} <= events
    frames = ref64("bookkeeping")["frames"]
    assert frames[4][0] == [0, 4] and frames[9][0] == [5, 6]           # object 3 came back as a new identity; a fresh start
    events = ref64("decisions")["events"]
    assert {"backdrop_best_then_new_tracklet", "minus_two", "column_zeroed_under_a_rival", "all_but_the_first_dropped",
            "dropped_by_dropped_rows_alone", "backdrop_filtered"} <= events
    assert -2 in ref64("decisions")["frames"][4][0] and ref64("decisions")["frames"][7][2] == 1
    assert "cross_class_best_column" in ref64("cats_on")["events"] and "cross_class_best_column" in ref64("cats_off")["events"]
    assert ref64("cats_on")["frames"][3][0] != ref64("cats_off")["frames"][3][0]
    assert [C.CASES[n][3]["memo_backdrop_frames"] for n in ("ring0", "ring1", "ring2")] == [0, 1, 2]
    assert "best_column_is_a_backdrop" in ref64("ring2")["events"] and "best_column_is_a_backdrop" not in ref64("ring0")["events"]
    assert max(b for _, b in ref64("ring2")["columns"]) == 3            # two frames' backdrops are columns at once
    assert {C.CASES[n][3].get("memo_momentum", 0.8) for n in C.CASES} == {0.8, 1.0}
    for name, limits in C.OVERFLOW.items():
        n = [len(fr["indices"]) for fr in C.frames(name)]
        live = [0] + [len([i for i in ids if i >= 0]) for ids, _, _ in ref64(name)["frames"]]
        fits = lambda t: live[t] + n[t] <= limits.get("capacity", 1024) and n[t] <= limits.get("backdrop_capacity", 256)
        assert fits(0) and fits(1) and not fits(2), name


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
    memo = C.memo_arrays(tracker)
    C.assert_memo_close(memo, ref64(name)["memo"], name)
    C.assert_memo_close(C.with_rowsums(memo), C.golden(name)["memo"], name + " (golden)")
    assert tracker.num_tracklets == 1 + max(max(ids, default=-1) for ids, _, _ in C.golden(name)["frames"])
    assert not tracker.empty and list(tracker.tracklets) == [int(i) for i in memo["ids"] if i >= 0]
    assert len(tracker.backdrops) == C.CASES[name][3].get("memo_backdrop_frames", 1)


@pytest.mark.parametrize("name", list(C.CASES))
def test_restated_bbox_overlaps_equals_the_references_bits(name):
    gold = C.golden(name)["ious"]
    assert gold
    for t, want in gold.items():
        fr = C.frames(name)[t]
        boxes = fr["bboxes"][fr["bboxes"][:, -1].sort(descending=True)[1], :-1]
        got = bbox_overlaps(boxes, boxes).numpy()
        assert got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32)), (name, t)
    assert tuple(bbox_overlaps(torch.zeros(0, 4), torch.zeros(3, 4)).shape) == (0, 3)


def test_public_surface_is_the_references():
    with open(os.path.join(C.GOLDEN, "signature.json")) as f:
        want = json.load(f)
    init = [[k, v.default] for k, v in inspect.signature(QuasiDenseEmbedTracker.__init__).parameters.items() if k != "self"]
    assert init[:len(want["init"])] == want["init"]
    assert init[len(want["init"]):] == [["capacity", 1024], ["backdrop_capacity", 256], ["fused", None]]
    assert [k for k in inspect.signature(QuasiDenseEmbedTracker.match).parameters if k != "self"] == want["match"]
    for member in ("match", "update_memo", "memo", "empty", "tracklets", "backdrops", "fused"):
        assert hasattr(QuasiDenseEmbedTracker, member)
    assert isinstance(QuasiDenseEmbedTracker.fused, bool)
    import uninext_amd
    assert uninext_amd.QuasiDenseEmbedTracker is QuasiDenseEmbedTracker
    tracker = QuasiDenseEmbedTracker()
    assert tracker.empty and tracker.num_tracklets == 0 and tracker.tracklets == {} and tracker.backdrops == []


def test_cpu_inputs_take_the_composition_whatever_fused_says():
    tracker = QuasiDenseEmbedTracker(fused=True, **C.CASES["decisions"][3])
    assert C.run(tracker, "decisions") == C.golden("decisions")["frames"]
    assert tracker._bank is None and len(tracker.backdrops) == 1
    again = QuasiDenseEmbedTracker(fused=True, **C.CASES["ring1"][3])      # `indices` as a tensor come back as a list
    fr = C.frames("ring1")[0]
    out = again.match(fr["bboxes"], fr["labels"], fr["embeds"], fr["frame_id"], torch.tensor(fr["indices"]))
    assert isinstance(out[3], list) and out[3] == C.golden("ring1")["frames"][0][1]


def test_an_empty_frame_runs_the_expiry_and_pushes_an_empty_backdrop_frame():
    """tracker.py:432-503 with n = 0: nothing is matched or started, update_memo still runs."""
    tracker = QuasiDenseEmbedTracker(fused=False, memo_tracklet_frames=2)
    for fr in C.frames("ring1")[:2]:
        tracker.match(fr["bboxes"], fr["labels"], fr["embeds"], fr["frame_id"], list(fr["indices"]))
    assert len(tracker.tracklets) == 3 and tracker.backdrops[0]["labels"].numel() == 2
    D = C.CASES["ring1"][1]
    empty = (torch.zeros(0, 5), torch.zeros(0, dtype=torch.int64), torch.zeros(0, D))
    b, l, ids, ind = tracker.match(*empty, 2, [])
    assert b.shape == (0, 5) and ids.numel() == 0 and ind == []
    assert len(tracker.tracklets) == 3 and tracker.backdrops[0]["labels"].numel() == 0
    tracker.match(*empty, 3, [])
    assert tracker.empty


def test_the_exports_are_in_the_header_the_table_and_the_library():
    from uninext_amd import _lib
    header = open(os.path.join(ROOT, "include", "dynmask_hip.h")).read()
    for name in EXPORTS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.DYNMASK_EXPORTS and name in _lib._SIGNATURES["dynmask_hip.h"]
        assert getattr(_lib.load(), name).argtypes is not None
    assert [n for n in _lib.DYNMASK_EXPORTS if n.startswith("qdtrack_")] == list(EXPORTS)
    for macro, value in (("QDTRACK_HIP_MAX_BACKDROPS", _lib.QDTRACK_MAX_BACKDROPS),
                         ("QDTRACK_HIP_MAX_BACKDROP_FRAMES", _lib.QDTRACK_MAX_BACKDROP_FRAMES),
                         ("QDTRACK_HIP_STATE_FIELDS", _lib.QDTRACK_STATE_FIELDS)):
        assert re.search(r"#define %s %d\b" % (macro, value), header), macro
    lib = _lib.load()
    assert lib.qdtrack_hip_last_kernel() is not None and lib.qdtrack_hip_state_offset(0, 4, 8, 2, 1) == 0
    offsets = [lib.qdtrack_hip_state_offset(k, 4, 6, 2, 0) for k in range(_lib.QDTRACK_STATE_FIELDS + 1)]
    assert all(o % 16 == 0 for o in offsets) and offsets == sorted(set(offsets))
    assert offsets == [lib.qdtrack_hip_state_offset(k, 4, 6, 2, 1) for k in range(_lib.QDTRACK_STATE_FIELDS + 1)]   # a ring of one
    assert lib.qdtrack_hip_state_offset(_lib.QDTRACK_STATE_FIELDS + 1, 4, 6, 2, 1) == 0 and lib.qdtrack_hip_state_offset(1, 0, 6, 2, 1) == 0
    null = ctypes.c_void_p(None)
    assert lib.qdtrack_hip_prepare_f32(null, 2000, 0.5, 0.3, 0.7, null, null, null, null) == -5      # beyond the sizes: no launch
    assert lib.qdtrack_hip_prepare_f32(null, 0, 0.5, 0.3, 0.7, null, null, null, null) == 0
    assert lib.qdtrack_hip_prepare_f32(null, 3, 0.5, 0.3, 0.7, null, null, null, null) == -1


def test_the_kernels_compile_for_gfx950_without_scratch():
    if shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None:
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    got = kernel_resources.resources(os.path.join(ROOT, "uninext_amd", "csrc", "qdtrack.hip"))
    for kernel in KERNELS:
        found = [k for k in got if k.split("(")[0] == "qdtrack::" + kernel]
        assert len(found) == 1, (kernel, sorted(got))
        r = got[found[0]]
        print("%-24s vgprs %d scratch %d B/lane lds %d occupancy %d" % (kernel, r["vgprs"], r["scratch"], r.get("lds", -1), r["occupancy"]))
        assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0, (kernel, r)
