"""GPU: the tracker's three entry points through the C ABI (track_hip_scores_f32, track_hip_associate_f32, track_hip_update_f32)
against the restatements of tests/tracker_parity.py on banks built directly, at the wave, workgroup and ring edges its
docstring lists; and IDOL_Tracker(fused=True).memo against the float64 tracker after EVERY frame of tests/tracker_cases.py.

Every buffer is the test's own.  Float outputs are handed over filled with NaN, integer outputs with a sentinel, and every
output (the next bank included) is followed by a sentinel tail that must come back bitwise untouched.
  scores     memo_embed, row_stats (maximum, sum) and every score of a kept row within max(8 x the fp32 PyTorch composition's
             error of the same entry, 16 x 2^-24 x s) and the project's 1e-4 bound; rows the pre-NMS dropped keep their bits,
             with no row kept neither is written (memo_embed still is under long_match: it does not depend on the
             detections, and D4_M4_n2_none/long3 holds it to its bound); the bank's NaN (slots >= M, unused ring entries,
             unused fields) reaches no output; track_hip_last_kernel names the variant.
  associate  plan over [0, M), [capacity, capacity + M), [2 capacity, 2 capacity + n), all 3 n + 2 entries of result and
             next_state.meta equal associate_exact; the rest of plan keeps its sentinel; the rest of next_state and all of
             state are bitwise unchanged.
  update     every live field of the next bank (slots [0, count), of each ring [0, long_len)) is bitwise update_exact; the
             source bank is bitwise unchanged; n == 0 returns 0 and writes nothing.
With TRACKER_PARITY_TABLE set the tables are appended to that file.

Largest kernel error / bound seen on an MI355X, per stress and output over every case of this file (stress, output, case, the
entry's kernel error, the composition's error and the bound relative to the entry's own magnitude, error / bound):
    equal memo D256_M257_n2_all/equal 0.00e+00 0.00e+00 0.00e+00 0.000
    long memo D63_M255_n2_all/long10t 1.45e-07 1.45e-07 8.58e-06 0.017
    plain memo D1_M1_n1_all/plain 0.00e+00 0.00e+00 0.00e+00 0.000
    wide memo D256_M257_n65_alt/wide 0.00e+00 0.00e+00 0.00e+00 0.000
    equal rstat D256_M257_n2_all/equal 0.00e+00 0.00e+00 2.47e-04 0.000
    long rstat D12_M257_n63_alt/long3 9.18e-08 2.39e-08 2.23e-05 0.004
    plain rstat D8off_M5_n65_all/plain 1.09e-07 1.87e-08 1.25e-04 0.001
    wide rstat D3_M5_n63_all/wide 8.43e-08 8.43e-08 4.92e-06 0.017
    equal scores D63_M4_n65_alt/equal 1.34e-07 1.34e-07 9.51e-04 0.000
    long scores D8off_M5_n65_alt/long10t 8.87e-07 1.49e-09 2.76e-04 0.003
    plain scores D8off_M5_n65_all/plain 1.86e-07 1.86e-07 8.62e-05 0.002
    wide scores D3_M5_n63_all/wide 5.44e-06 5.37e-06 4.41e-04 0.012
Every entry of every case met its bound with the magnitude as derived: no term had to be added.  All 16 associations and all
8 updates were bitwise the restatements, every sentinel came back untouched, and the fused memo met 1e-4 after every frame of
the eight sequences: the sweep found no kernel bug.  The worst-case dot-product term (D + 2) makes the bound at D = 256 about a
thousand times the rounding actually seen: the measure rejects structural mistakes, not 1e-4-relative ones (tracker_parity's
docstring); the sweep's sharpest instruments are the bitwise halves and the small-D cases.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracker_cases as C       # noqa: E402
import tracker_parity as P      # noqa: E402
import tracker_ref              # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAIL = 64
TAIL_BYTE = 0xA5
INT_SENTINEL, LONG_SENTINEL = -0x12345678, -0x123456789ABCDEF


# ---------------------------------------------------------------------------------------------------------------- the C ABI

def lib():
    from uninext_amd import _lib
    return _lib.load()


def last():
    from uninext_amd import _lib
    return _lib.last_kernel("track")


def guarded(n, dtype, fill):
    """n entries of `fill` followed by TAIL bytes of TAIL_BYTE; (the whole byte buffer, the view of the n entries)"""
    size = torch.empty((), dtype=dtype).element_size()
    raw = torch.full((n * size + TAIL,), TAIL_BYTE, dtype=torch.uint8, device=DEV)
    assert raw.data_ptr() % 16 == 0
    view = raw[:n * size].view(dtype)
    view.fill_(fill)
    return raw, view


def tail_untouched(raw, what):
    assert bool((raw[-TAIL:] == TAIL_BYTE).all()), what + ": written past the end"


class Bank:
    """A memory bank in the test's own buffer, laid out by track_hip_state_offset, with a sentinel tail."""

    def __init__(self, state, C_, D, L):
        at = [lib().track_hip_state_offset(k, C_, D, L) for k in range(len(P.FIELDS) + 1)]
        assert all(a % 16 == 0 for a in at) and at[-1] > 0
        self.raw = torch.full((at[-1] + TAIL,), TAIL_BYTE, dtype=torch.uint8, device=DEV)
        assert self.raw.data_ptr() % 16 == 0
        self.views = {}
        for k, (name, dtype, shape) in enumerate(P.FIELDS):
            t = torch.from_numpy(np.ascontiguousarray(state[name]))
            assert at[k] + t.numel() * t.element_size() <= at[k + 1]
            view = self.raw[at[k]:at[k] + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
            view.copy_(t)
            self.views[name] = view
        self.before = self.raw.clone()

    def ptr(self):
        return self.raw.data_ptr()

    def unchanged(self, what, but=()):
        if but:
            now = self.raw.clone()
            for name in but:
                self.views[name].copy_(torch.from_numpy(self.host_before(name)))
        assert torch.equal(self.raw, self.before), what + ": the bank was written"
        if but:
            self.raw.copy_(now)

    def host_before(self, name):
        k = [f[0] for f in P.FIELDS].index(name)
        dtype, shape = P.FIELDS[k][1], self.views[name].shape
        off = self.views[name].data_ptr() - self.raw.data_ptr()
        return self.before[off:off + self.views[name].numel() * self.views[name].element_size()].cpu().numpy().view(dtype).reshape(shape)

    def host(self):
        return {name: v.cpu().numpy() for name, v in self.views.items()}


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    assert t.data_ptr() % 16 == 0
    return t


def nan_bits(t):
    return t.view(torch.int32)


# --------------------------------------------------------------------------------------------------------------------- scores

def run_scores(name):
    from uninext_amd import _lib
    c, x = P.SCORES[name], P.score_inputs(name)
    M, n, D, L, C_ = x["M"], c["n"], x["D"], x["L"], x["C"]
    bank = Bank(x["state"], C_, D, L)
    if c["offset"]:                                       # the base one float past a 16-byte boundary: the scalar path at D % 4 == 0
        room = torch.zeros(n * D + 1, dtype=torch.float32, device=DEV)
        embeds = room[1:]
        embeds.copy_(torch.from_numpy(x["embeds"]).view(-1))
        assert embeds.data_ptr() % 16 == 4
    else:
        embeds = dev(x["embeds"])
    keep = dev(x["keep"])
    temporal = None if x["temporal"] is None else dev(x["temporal"])
    nan = float("nan")
    memo_raw, memo = guarded(M * D, torch.float32, nan)
    stat_raw, stat = guarded(2 * n, torch.float32, nan)
    sc_raw, sc = guarded(n * M, torch.float32, nan)
    handed = [t.clone() for t in (memo, stat, sc)]
    rc = lib().track_hip_scores_f32(embeds.data_ptr(), keep.data_ptr(), bank.ptr(), None if temporal is None else temporal.data_ptr(),
                                    1 if x["long"] else 0, n, M, C_, D, L, memo_raw.data_ptr(), stat_raw.data_ptr(), sc_raw.data_ptr(), None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert last() == ("track_scores<long>" if x["long"] else "track_scores"), (name, last())
    for raw, what in ((memo_raw, "memo_embed"), (stat_raw, "row_stats"), (sc_raw, "scores")):
        tail_untouched(raw, name + " " + what)
    bank.unchanged(name)
    kept = x["keep"].astype(bool)
    dropped = torch.from_numpy(~kept).to(DEV)
    sc2, stat2 = sc.view(n, M), stat.view(n, 2)
    assert torch.equal(nan_bits(sc2[dropped]), nan_bits(handed[2].view(n, M)[dropped])), name + ": a dropped row's scores were written"
    assert torch.equal(nan_bits(stat2[dropped]), nan_bits(handed[1].view(n, 2)[dropped])), name + ": a dropped row's statistics"
    if not x["long"]:
        assert torch.equal(nan_bits(memo), nan_bits(handed[0])), name + ": memo_embed written without long_match"
    if not kept.any():
        assert torch.equal(nan_bits(sc), nan_bits(handed[2])) and torch.equal(nan_bits(stat), nan_bits(handed[1]))
    got = dict(memo=memo.view(M, D).cpu().double().numpy(), rstat=stat2.cpu().double().numpy(), scores=sc2.cpu().double().numpy())
    if not x["long"]:
        got["memo"] = P.score_reference(name)["memo"]     # `embed` itself: nothing of the kernels' to compare
    assert not np.isnan(got["memo"]).any() and not np.isnan(got["scores"][kept]).any() and not np.isnan(got["rstat"][kept]).any(), \
        name + ": NaN in an output (an entry left unwritten, or the bank's NaN read)"
    return got


@pytest.mark.parametrize("name", list(P.SCORES))
def test_scores(name):
    since = len(P.TABLE)
    P.measure_scores(name, run_scores(name), P.score_composition(name, DEV))
    report(since)


# ------------------------------------------------------------------------------------------------------------------ associate

def run_associate(x):
    from uninext_amd import _lib
    M, n, C_, a = x["M"], x["n"], x["C"], x["args"]
    bank, nxt = Bank(x["state"], C_, x["D"], x["L"]), Bank(P.blank_state(C_, x["D"], x["L"], -77, -78), C_, x["D"], x["L"])
    plan_raw, plan = guarded(2 * C_ + n, torch.int32, INT_SENTINEL)
    res_raw, res = guarded(3 * n + 2, torch.int64, LONG_SENTINEL)
    scores = dev(x["scores"]) if M else None
    ins = [dev(x[k]) for k in ("keep", "bboxes", "inter", "area")]
    rc = lib().track_hip_associate_f32(None if scores is None else scores.data_ptr(), *[t.data_ptr() for t in ins], bank.ptr(), nxt.ptr(),
                                       n, M, C_, x["D"], x["L"], 1 if a["frame_weight"] else 0, a["match_thr"], a["new_thr"], a["nms_thr"],
                                       a["frame_id"], a["tracklet_frames"], plan_raw.data_ptr(), res_raw.data_ptr(), None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert last() == "track_associate"
    tail_untouched(plan_raw, "plan")
    tail_untouched(res_raw, "result")
    bank.unchanged("state")
    nxt.unchanged("next_state", but=("meta",))
    return plan.cpu().numpy(), res.cpu().numpy(), nxt.views["meta"].cpu().numpy()


@pytest.mark.parametrize("name", list(P.ASSOC))
def test_associate(name):
    x = P.assoc_inputs(name)
    want_plan, want_res, want_meta, events = P.assoc_expected(name)
    plan, res, meta = run_associate(x)
    want_plan = np.where(want_plan == P.INT_GARBAGE, INT_SENTINEL, want_plan)      # what the kernel does not write keeps the sentinel
    M, C_ = x["M"], x["C"]
    assert (want_plan[M:C_] == INT_SENTINEL).all() and (want_plan[C_ + M:2 * C_] == INT_SENTINEL).all()
    bad = np.flatnonzero(plan != want_plan)
    assert bad.size == 0, (name, "plan", bad[:8].tolist(), plan[bad[:8]].tolist(), want_plan[bad[:8]].tolist())
    bad = np.flatnonzero(res != want_res)
    assert bad.size == 0, (name, "result", bad[:8].tolist(), res[bad[:8]].tolist(), want_res[bad[:8]].tolist())
    assert np.array_equal(meta, want_meta), (name, meta, want_meta)
    print(name, "bitwise; events:", " ".join(sorted(events)))


# --------------------------------------------------------------------------------------------------------------------- update

def run_update(x, n=None):
    from uninext_amd import _lib
    M, C_, D, L = x["M"], x["C"], x["D"], x["L"]
    n = x["n"] if n is None else n
    bank = Bank(x["state"], C_, D, L)
    blank = P.blank_state(C_, D, L, int(x["result"][2 * x["n"]]), int(x["result"][2 * x["n"] + 1]))     # meta is the association's
    nxt = Bank(blank, C_, D, L)
    ins = [dev(x[k]) for k in ("embeds", "bboxes", "labels", "plan", "result")]
    rc = lib().track_hip_update_f32(*[t.data_ptr() for t in ins], bank.ptr(), nxt.ptr(), n, M, C_, D, L, x["keep_weight"], x["momentum"],
                                    x["frame_id"], None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    tail_untouched(nxt.raw, "next_state")
    bank.unchanged("state")
    return nxt


@pytest.mark.parametrize("name", list(P.UPDATES))
def test_update(name):
    x = P.update_inputs(name)
    want, events = P.update_expected(name)
    nxt = run_update(x)
    assert last() == "track_update"
    P.assert_banks_bitwise(nxt.host(), want, name)
    print(name, "bitwise; count", int(want["meta"][0]), "events:", " ".join(sorted(events)))


def test_update_without_detections_writes_nothing():
    x = P.update_inputs("D8_L2")
    run_update(x, n=0).unchanged("next_state")


# ------------------------------------------------------------------------------------- the memo after every frame, end to end

@functools.lru_cache(maxsize=None)
def ref64(name):
    return tracker_ref.run(name, C)


@pytest.mark.parametrize("name", list(C.CASES))
def test_fused_memo_after_every_frame(name):
    from uninext_amd.tracker import IDOL_Tracker
    tracker = IDOL_Tracker(fused=True, **C.CASES[name][3])
    memos = ref64(name)["memos"]
    frames = C.frames(name)
    assert len(memos) == len(frames)
    for t, fr in enumerate(frames):
        tracker.match(fr["bboxes"].to(DEV), fr["labels"].to(DEV), fr["masks"].to(DEV), fr["embeds"].to(DEV), fr["frame_id"], list(fr["indices"]))
        assert tracker._bank is not None
        if memos[t] is None:
            assert tracker.empty, (name, t)
        else:
            C.assert_memo_close(C.memo_arrays(tracker.memo), memos[t], "%s frame %d" % (name, t))


# ------------------------------------------------------------------------------------------------------------------ reporting

report = P.report


def test_print_worst_ratio_per_output_and_stress():
    """Reporting only: prints what the tests above measured in this process (nothing, when it is run alone).  It asserts
    nothing; every entry is held to its bound inside P.measure."""
    print(P.worst_table())
    path = os.environ.get("TRACKER_PARITY_TABLE")
    if path:
        with open(path, "a") as f:
            f.write("WORST\n" + P.worst_table() + "\n")
