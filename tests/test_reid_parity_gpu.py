"""GPU: the re-ID kernels (uninext_amd/csrc/reid.hip) against the restatements of tests/reid_parity.py at the block, wave and rank
edges its docstring and case tables list.

  selection  ota_reid_select_hip through the C ABI on hand-built cost / iou / flags (nothing depends on the cost kernel):
             matching_pos, matching_neg, counts and status bitwise the exact restatement; the cost matrix's valid columns bitwise
             as the two runs leave them.
  scores     ext.reid_scores: dot, cos, ref_norm, key_norm per entry.
  loss       ext.reid_loss_forward on hand-built dot / cos / matchings / items / ranks: roles bitwise, the six item_stats
             columns and the two losses per entry (the NaN of n_aux = 0 and the -inf maxima of empty sets as such).
  backward   ext.reid_loss_backward on the kernels' own forward: coef, key_item_grad, grad_ref, grad_key per entry; grad_key
             bitwise the float32 sum of the kernel's item rows in ascending item order.
Per entry: |got - ref64| <= max(8 x the fp32 PyTorch composition's error at the entry on this GPU, 16 x 2^-24 x s) with s as
derived in tests/reid_parity.py, and the project's 1e-4 max(1, max|ref|) on top; where the composition is not finite at a
finite reference entry its term is dropped and the derived term stands alone.  Every output and workspace is carved out of a
sentinel-filled buffer whose guard bands must come back untouched; entries the contract leaves unwritten (ref_norm of an image
without a valid target, key_norm of an invalid target) are excluded by name and must still hold the sentinel.  Every test
prints the worst |error| / bound per output.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import reid_parity as P     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 256
SENTINEL = {torch.float32: 12345.0, torch.uint8: 0x5A, torch.int32: 0x5A5A5A5A, torch.float64: 12345.0}


class Guarded:
    """Outputs carved out of larger buffers filled with a sentinel; check() asserts the bands are as they were."""

    def __init__(self):
        self.bufs = []

    def __call__(self, shape, dtype=torch.float32, init=None):
        n = int(np.prod(shape))
        buf = torch.full((BAND + n + BAND,), SENTINEL[dtype], dtype=dtype, device=DEV)
        self.bufs.append((buf, n))
        view = buf[BAND:BAND + n].view(shape)
        if init is not None:
            view.copy_(torch.from_numpy(np.ascontiguousarray(init)).view(shape))
        return view

    def check(self):
        for buf, n in self.bufs:
            assert bool((buf[:BAND] == SENTINEL[buf.dtype]).all()) and bool((buf[BAND + n:] == SENTINEL[buf.dtype]).all())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


report = P.report


# ------------------------------------------------------------------------------------------------------------------- selection

@pytest.mark.parametrize("name", list(P.SELECT))
def test_selection_bitwise(name):
    from uninext_amd import _lib
    x, want = P.select_inputs(name), P.select_expected(name)
    Q, off, bs = x["Q"], x["off"], len(x["images"])
    G = int(off[-1])
    guard = Guarded()
    cost = guard((Q * G,), init=P.pack([im["cost"] for im in x["images"]], np.float32))
    iou = dev(P.pack([im["iou"] for im in x["images"]], np.float32))
    flags = dev(P.pack([im["flags"] for im in x["images"]], np.uint8))
    valid = dev(P.pack([im["valid"] for im in x["images"]], np.uint8))
    keys = dev(P.pack([im["keys"] for im in x["images"]], np.int64))
    mpos, mneg = guard((Q * G,), torch.uint8), guard((Q * G,), torch.uint8)
    counts, status = guard((G, 2), torch.int32), guard((bs,), torch.int32)
    gt_off = (ctypes.c_int32 * (bs + 1))(*[int(v) for v in off])
    with torch.cuda.device(DEV):
        rc = _lib.load().ota_reid_select_hip(cost.data_ptr(), iou.data_ptr(), flags.data_ptr(), valid.data_ptr(), keys.data_ptr(), gt_off, bs, Q,
                                             x["Qk"], x["max_rounds"], mpos.data_ptr(), mneg.data_ptr(), counts.data_ptr(), status.data_ptr(),
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    guard.check()
    assert host(status).tolist() == want["status"].tolist()
    got_pos, got_neg, got_counts, got_cost = host(mpos), host(mneg), host(counts), host(cost)
    for b, im in enumerate(x["images"]):
        if off[b + 1] == off[b]:
            continue
        for what, got, ref in (("matching_pos", got_pos, want["pos"]), ("matching_neg", got_neg, want["neg"])):
            bad = np.argwhere(P.block(got, off, Q, b) != P.block(ref, off, Q, b))
            assert not len(bad), (name, what, "image", b, "first (query, target)", bad[:4].tolist())
        assert np.array_equal(got_counts[off[b]:off[b + 1]], want["counts"][off[b]:off[b + 1]]), (name, "counts", b)
        if want["cost"][b] is not None:
            v = np.asarray(im["valid"]).astype(bool)
            after = P.block(got_cost, off, Q, b)[:, v]
            assert np.array_equal(after.view(np.int32), want["cost"][b].view(np.int32)) or np.array_equal(after, want["cost"][b], equal_nan=True), \
                (name, "cost after both runs", b)
    print("%s: %d images, %d targets, status %s: bitwise" % (name, bs, G, sorted(set(want["status"].tolist()))))


# ---------------------------------------------------------------------------------------------------------------------- floats

def run_scores(p, guard):
    from uninext_amd import ext
    Q, G, bs = p["Q"], int(p["off"][-1]), len(p["sizes"])
    out = (guard((Q * G,)), guard((Q * G,)), guard((bs, Q)), guard((G,)))
    return ext.reid_scores(dev(p["ref"]), dev(p["key"]), dev(p["keys"]), dev(p["valid"]), list(p["sizes"]), out=out)


def check_unwritten(p, ref_norm, key_norm):
    ex_r, ex_k = P.unwritten(p)
    assert (host(ref_norm)[ex_r] == np.float32(SENTINEL[torch.float32])).all() and (host(key_norm)[ex_k] == np.float32(SENTINEL[torch.float32])).all()


@pytest.mark.parametrize("name", list(P.SCORES))
def test_scores_per_entry(name):
    p, ref = P.problem("scores", name), P.reference("scores", name)
    guard = Guarded()
    dot, cos, ref_norm, key_norm = run_scores(p, guard)
    torch.cuda.synchronize()
    guard.check()
    check_unwritten(p, ref_norm, key_norm)
    comp = P.composition(p, ref["ls"]["roles"], device=DEV, grads=False)
    since = len(P.TABLE)
    got = dict(dot=host(dot), cos=host(cos), ref_norm=host(ref_norm), key_norm=host(key_norm))
    worst = P.measure_scores(name, p, got, ref["sc"], comp)
    report(since)
    invalid = np.repeat(p["valid"] == 0, 1)
    for b in range(len(p["sizes"])):                       # an invalid target's column is exact zeros
        cols = invalid[p["off"][b]:p["off"][b + 1]]
        assert not P.block(got["dot"], p["off"], p["Q"], b)[:, cols].any() and not P.block(got["cos"], p["off"], p["Q"], b)[:, cols].any()
    assert worst <= 1.0


@pytest.mark.parametrize("name", list(P.LOSS))
def test_loss_forward_per_entry(name):
    from uninext_amd import _lib, ext
    p, ref = P.problem("loss", name), P.reference("loss", name)["ls"]
    Q, n = p["Q"], len(p["meta"])
    guard = Guarded()
    out = (guard((2,)), guard((n, Q), torch.uint8), guard((n, _lib.REID_STATS), torch.float64))
    losses, roles, stats = ext.reid_loss_forward(dev(p["dot"]), dev(p["cos"]), dev(p["mpos"]), dev(p["mneg"]), dev(p["meta"]), dev(p["ranks"]),
                                                 list(p["sizes"]), Q, out=out)
    torch.cuda.synchronize()
    guard.check()
    bad = np.argwhere(host(roles) != ref["roles"])
    assert not len(bad), (name, "roles: first (item, query)", bad[:4].tolist())
    comp = P.composition(p, ref["roles"], device=DEV)
    since = len(P.TABLE)
    worst = P.measure_loss(name, dict(stats=host(stats), losses=host(losses)), ref, comp)
    report(since)
    assert worst <= 1.0


@pytest.mark.parametrize("name", list(P.BACKWARD))
def test_backward_per_entry(name):
    from uninext_amd import _lib, ext
    p, ref = P.problem("backward", name), P.reference("backward", name)
    Q, Qk, C, n, bs = p["Q"], p["Qk"], p["C"], len(p["meta"]), len(p["sizes"])
    guard = Guarded()
    ref_t, key_t, keys, meta = dev(p["ref"]), dev(p["key"]), dev(p["keys"]), dev(p["meta"])
    dot, cos, ref_norm, key_norm = run_scores(p, guard)
    losses, roles, stats = ext.reid_loss_forward(dot, cos, dev(p["mpos"]), dev(p["mneg"]), meta, dev(p["ranks"]), list(p["sizes"]), Q,
                                                 out=(guard((2,)), guard((n, Q), torch.uint8), guard((n, _lib.REID_STATS), torch.float64)))
    ws = (guard((2, n, Q)), guard((n, C)))
    grad_ref, grad_key = ext.reid_loss_backward(ref_t, key_t, keys, dot, cos, ref_norm, key_norm, roles, stats, meta, list(p["item_counts"]),
                                                dev(p["grads"]), list(p["sizes"]), out=(guard((bs, Q, C)), guard((bs, Qk, C))), workspace=ws)
    torch.cuda.synchronize()
    guard.check()
    check_unwritten(p, ref_norm, key_norm)
    assert np.array_equal(host(roles), ref["ls"]["roles"])
    comp = P.composition(p, ref["ls"]["roles"], device=DEV)
    since = len(P.TABLE)
    got = dict(dot=host(dot), cos=host(cos), ref_norm=host(ref_norm), key_norm=host(key_norm), stats=host(stats), losses=host(losses),
               coef=host(ws[0]), key_item_grad=host(ws[1]), grad_ref=host(grad_ref), grad_key=host(grad_key))
    worst = max(P.measure_scores(name, p, got, ref["sc"], comp), P.measure_loss(name, got, ref["ls"], comp), P.measure_backward(name, got, ref["bw"], comp))
    report(since)
    # the one sum whose order is contract: the item rows of a key row in ascending item order, in float32, bitwise
    want = P.key_sum32(got["key_item_grad"], p, ref["bw"]["rows"])
    assert np.array_equal(got["grad_key"].view(np.int32), want.view(np.int32)), (name, "grad_key is not the ascending float32 sum of its item rows")
    # exact zeros: reference rows of the image without items, key rows no item points at
    assert not got["grad_ref"][1].any() and not got["grad_key"][1].any()
    used = {r for r in ref["bw"]["rows"] if r is not None}
    for b in range(bs):
        for k in range(Qk):
            if (b, k) not in used:
                assert not got["grad_key"][b, k].any(), (name, b, k)
    assert worst <= 1.0


def test_print_the_worst_ratios():
    """Prints the largest |error| / bound per output over the tests of this file that ran before it in the same process; it
    asserts nothing (every test above asserts its own)."""
    print(P.HEAD + "\n" + P.worst_table())
