"""The fused re-ID route on the GPU (uninext_amd/csrc/reid.hip through uninext_amd/reid.py, fused=True): its integers against the
numpy restatement (tests/reid_ref.py) and the reference-minted fixtures, its scores entry by entry against float64, its losses and
gradients against the fixtures' float64, and the kernels' own contracts: guard bands around every output and workspace,
repeatability, one host copy, refusals.

Tolerance of losses and gradients: scaled_error <= 1e-4 (tests/criterion_cases.py); the composition's error on the same GPU is
printed beside the fused one."""
import functools
import os
import random
import sys

import numpy as np
import pytest
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import reid_cases as C  # noqa: E402
import reid_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 256
SENTINEL = {torch.float32: 12345.0, torch.uint8: 0x5A, torch.int32: 0x5A5A5A5A, torch.float64: 12345.0}
U = 2.0 ** -24
KEYS = ("loss_reid", "loss_reid_aux")


class Guarded:
    """Outputs carved out of larger buffers filled with a sentinel; check() asserts the bands are as they were."""

    def __init__(self):
        self.bufs = []

    def __call__(self, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        buf = torch.full((BAND + n + BAND,), SENTINEL[dtype], dtype=dtype, device=DEV)
        self.bufs.append((buf, n))
        return buf[BAND:BAND + n].view(shape)

    def check(self):
        for buf, n in self.bufs:
            assert bool((buf[:BAND] == SENTINEL[buf.dtype]).all()) and bool((buf[BAND + n:] == SENTINEL[buf.dtype]).all())


def device_table(prob):
    """The focal table pos - neg of pos_neg_select.py:113-114 as the fused route forms it: PyTorch's elementwise operations on the GPU."""
    prob = torch.as_tensor(prob).to(DEV)
    neg = (1 - 0.25) * (prob ** 2.0) * (-(1 - prob + 1e-8).log())
    pos = 0.25 * ((1 - prob) ** 2.0) * (-(prob + 1e-8).log())
    return pos - neg


def run(name, fused, device=DEV, dtype=torch.float32, head=None, **kwargs):
    """select_pos_neg + loss_reid + both gradients of a case: {packed / items, losses, grads: {key: (grad_ref, grad_key)}, state}."""
    from uninext_amd import reid
    cfg = C.CASES[name]
    flat = C.make_inputs(cfg)
    ref_box, all_indices, targets, det_targets, hs_key, hs_ref, ref_cls = C.rebuild(flat, len(cfg["images"]), device=device, embed_dtype=dtype)
    hs_key.requires_grad_(True)
    hs_ref.requires_grad_(True)
    random.seed(C.SEED)
    items = reid.select_pos_neg(ref_box, all_indices, targets, det_targets, head or nn.Identity(), hs_key, hs_ref, ref_cls, fused=fused, **kwargs)
    state = random.getstate()
    losses = reid.loss_reid({"pred_qd": items, "reid_params": hs_ref.sum()}, None, None, 1.0)
    grads = {k: torch.autograd.grad(losses[k], [hs_ref, hs_key], retain_graph=True, allow_unused=True) for k in KEYS}
    return {"flat": flat, "items": items, "losses": losses, "grads": grads, "state": state, "hs": (hs_ref, hs_key)}


@functools.lru_cache(maxsize=None)
def fused_run(name):
    return run(name, True)


@functools.lru_cache(maxsize=None)
def float64_run(name):
    """The composition in float64 on the CPU (held to the fixtures by tests/test_reid_cpu.py): the yardstick where no fixture is."""
    return run(name, False, device="cpu", dtype=torch.float64)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_integers_equal_the_restatement_and_the_fixture(name):
    from uninext_amd import reid
    got = fused_run(name)
    packed, flat, cfg = got["items"], got["flat"], C.CASES[name]
    assert isinstance(packed, reid.PackedContrastItems)
    Q, off, i = cfg["Q"], 0, 0
    fixture = C.load_fixture(name) if cfg["fixture"] else None
    want64 = float64_run(name)
    assert got["state"] == want64["state"]                                    # the generator is where the composition leaves it
    assert len(packed) == len(want64["items"])
    for b, im in enumerate(cfg["images"]):
        n, valid = im["n"], flat["valid_%d" % b]
        # (the table is PyTorch's on the GPU, copied to the host for the restatement, as in tests/test_matcher_gpu.py)
        want = R.select(device_table(flat["ref_cls"][b]).cpu().numpy(), flat["ref_box"][b], flat["boxes_%d" % b], flat["pm_%d" % b], valid) if n else None
        pos = packed.matching_pos[Q * off:Q * (off + n)].view(Q, n).cpu().numpy()
        neg = packed.matching_neg[Q * off:Q * (off + n)].view(Q, n).cpu().numpy()
        if want is None:
            assert not pos.any() and not neg.any()
        else:
            assert np.array_equal(pos, want["pos"]) and np.array_equal(neg, want["neg"])
            for t in np.nonzero(valid)[0]:
                image, target, first, count, n_aux = packed.items[i]
                assert (image, target) == (b, off + t) and n_aux == want["n_pos"][t] + count
                assert count == R.num_sample_neg(int(want["n_pos"][t]), int(want["n_neg"][t]))
                if fixture is not None:                                       # the reference's integers, index for index: no case excused
                    assert (int(fixture["item_image"][i]), int(fixture["item_target"][i])) == (b, t)
                    assert np.array_equal(pos[:, t], fixture["pos"][i]) and np.array_equal(1 - neg[:, t], fixture["neg"][i])
                    assert packed.host_ranks[first:first + count] == fixture["ranks"][fixture["rank_off"][i]:fixture["rank_off"][i + 1]].tolist()
                i += 1
        off += n
    assert i == len(packed) and (fixture is None or i == len(fixture["item_image"]))
    assert packed.ranks.cpu().tolist()[:len(packed.host_ranks)] == packed.host_ranks
    expanded = packed.expand()
    for mine, theirs in zip(expanded, want64["items"]):
        assert sorted(mine) == ["aux_consin", "aux_label", "contrast", "label"]
        assert mine["label"].tolist() == theirs["label"].tolist() and mine["aux_label"].tolist() == theirs["aux_label"].tolist()
        assert C.scaled_error(mine["contrast"].detach().cpu().numpy(), theirs["contrast"].detach().numpy()) <= C.TOLERANCE


@pytest.mark.parametrize("name", ["reid_q100_c64", "reid_q101_g1_c256", "reid_q130_mixed_c64", "reid_q1030_c64"])
def test_scores_entry_by_entry_against_float64(name):
    """dot is one fp32 FMA chain of C terms: |dot - dot64| <= (C + 2) u S with S = sum |a_c| |b_c| and u = 2^-24 (gamma_C of a
    sequential sum, two units of slack).  cos = dot / (max(|r|, eps) max(|k|, eps)): |r|^2 and |k|^2 are sums of C non-negative terms,
    each within (C + 2) u relatively; the square root halves that and rounds once; the product of the two norms rounds once, the
    division once.  To first order |cos - cos64| <= (C + 2) u S / (|r| |k|) + |cos64| ((C + 2) u + 4 u): asserted with (C + 8) u
    for the second factor."""
    from uninext_amd import ext
    packed = fused_run(name)["items"]
    ref, key = packed.ref_embeds.detach(), packed.key_embeds.detach()
    bs, Q, Cd = ref.shape
    G = sum(packed.sizes)
    guard = Guarded()
    out = (guard((Q * G,)), guard((Q * G,)), guard((bs, Q)), guard((G,)))
    dot, cos, ref_norm, key_norm = ext.reid_scores(ref, key, packed.key_index, packed.valid, packed.sizes, out=out)
    torch.cuda.synchronize()
    guard.check()
    ref64, key64 = ref.double().cpu(), key.double().cpu()
    index, valid, off, worst = packed.key_index.cpu(), packed.valid.cpu(), 0, [0.0, 0.0]
    for b, n in enumerate(packed.sizes):
        d = dot[Q * off:Q * (off + n)].view(Q, n).cpu().double()
        c = cos[Q * off:Q * (off + n)].view(Q, n).cpu().double()
        for t in range(n):
            if not valid[off + t]:
                assert not d[:, t].any() and not c[:, t].any()
                continue
            k = key64[b, index[off + t]]
            d64, S = ref64[b] @ k, ref64[b].abs() @ k.abs()
            nr, nk = ref64[b].norm(dim=1), k.norm()
            c64 = d64 / (nr * nk)
            bound_d = (Cd + 2) * U * S
            bound_c = (Cd + 2) * U * S / (nr * nk) + c64.abs() * (Cd + 8) * U
            assert bool(((d[:, t] - d64).abs() <= bound_d).all()) and bool(((c[:, t] - c64).abs() <= bound_c).all())
            worst = [max(worst[0], float(((d[:, t] - d64).abs() / bound_d).max())), max(worst[1], float(((c[:, t] - c64).abs() / bound_c).max()))]
            assert C.scaled_error(key_norm[off + t].cpu().numpy(), nk.numpy()) <= 1e-6
        if valid[off:off + n].any():
            assert C.scaled_error(ref_norm[b].cpu().numpy(), ref64[b].norm(dim=1).numpy()) <= 1e-6
        off += n
    print("%s: worst |error| / bound: dot %.3f cos %.3f" % (name, worst[0], worst[1]))


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_losses_and_gradients(name):
    got, comp = fused_run(name), run(name, False)
    if C.CASES[name]["fixture"]:
        g = C.load_fixture(name)
        want = {k: (g[k], g["grad_ref." + k], g["grad_key." + k]) for k in KEYS}
    else:
        w = float64_run(name)
        want = {k: (float(w["losses"][k]), w["grads"][k][0].numpy(), w["grads"][k][1].numpy()) for k in KEYS}
    for k in KEYS:
        errs = []
        for r in (got, comp):
            errs.append((C.scaled_error(float(r["losses"][k]), want[k][0]), C.scaled_error(r["grads"][k][0].cpu().numpy(), want[k][1]),
                         C.scaled_error(r["grads"][k][1].cpu().numpy(), want[k][2])))
        print("%s %s: fused loss %.3e grad_ref %.3e grad_key %.3e | composition loss %.3e grad_ref %.3e grad_key %.3e (scaled errors against float64)"
              % ((name, k) + errs[0] + errs[1]))
        assert max(errs[0]) <= C.TOLERANCE, errs[0]


def test_gradients_reach_the_embed_head_and_detach_reid_cuts_the_inputs():
    torch.manual_seed(0)
    head = nn.Linear(64, 64).to(DEV)
    head64 = nn.Linear(64, 64).double()
    head64.load_state_dict({k: v.double().cpu() for k, v in head.state_dict().items()})
    name = "reid_q130_mixed_c64"
    for detach in (False, True):
        got = run(name, True, head=head, detach_reid=detach)
        want = run(name, False, device="cpu", dtype=torch.float64, head=head64, detach_reid=detach)
        total, total64 = sum(got["losses"].values()), sum(want["losses"].values())
        mine = torch.autograd.grad(total, list(head.parameters()) + list(got["hs"]), allow_unused=True)
        theirs = torch.autograd.grad(total64, list(head64.parameters()) + list(want["hs"]), allow_unused=True)
        for a, b in zip(mine[:2], theirs[:2]):
            assert C.scaled_error(a.cpu().numpy(), b.numpy()) <= C.TOLERANCE
        if detach:
            assert mine[2] is None and mine[3] is None and theirs[2] is None
        else:
            assert C.scaled_error(mine[2].cpu().numpy(), theirs[2].numpy()) <= C.TOLERANCE
            assert C.scaled_error(mine[3].cpu().numpy(), theirs[3].numpy()) <= C.TOLERANCE


def test_guard_bands_and_bitwise_repeatability():
    """Every kernel writes inside its outputs and workspaces, and two runs give the same bits."""
    from uninext_amd import _lib, ext, reid
    name = "reid_q130_mixed_c64"
    cfg = C.CASES[name]
    packed = fused_run(name)["items"]
    ref_box, all_indices, targets, _, _, _, ref_cls = C.rebuild(got_flat(name), len(cfg["images"]), device=DEV)
    ref, key = packed.ref_embeds.detach(), packed.key_embeds.detach()
    bs, Q, Cd = ref.shape
    G, n = sum(packed.sizes), len(packed)
    runs = []
    for _ in range(2):
        guard = Guarded()
        table = device_table(ref_cls)
        have = [t for t in targets if len(t["labels"])]
        out = (guard((Q * G,)), guard((Q * G,)), guard((Q * G,), torch.uint8), guard((Q * G,), torch.uint8), guard((Q * G,), torch.uint8),
               guard((2 * G + bs,), torch.int32))
        sel = ext.reid_select(table, ref_box, torch.cat([t["boxes"] for t in have]), torch.cat([t["positive_map"] for t in have]), packed.valid,
                              packed.key_index, packed.sizes, key.shape[1], out=out)
        scores = ext.reid_scores(ref, key, packed.key_index, packed.valid, packed.sizes,
                                 out=(guard((Q * G,)), guard((Q * G,)), guard((bs, Q)), guard((G,))))
        fwd = ext.reid_loss_forward(scores[0], scores[1], sel[3], sel[4], packed.item_meta, packed.ranks, packed.sizes, Q,
                                    out=(guard((2,)), guard((n, Q), torch.uint8), guard((n, _lib.REID_STATS), torch.float64)))
        ws = (guard((2, n, Q)), guard((n, Cd)))
        bwd = ext.reid_loss_backward(ref, key, packed.key_index, scores[0], scores[1], scores[2], scores[3], fwd[1], fwd[2], packed.item_meta,
                                     packed.item_counts, torch.tensor([1.0, 2.0], device=DEV), packed.sizes,
                                     out=(guard((bs, Q, Cd)), guard((bs, key.shape[1], Cd))), workspace=ws)
        torch.cuda.synchronize()
        guard.check()
        # (ref_norm of an image without valid targets is not written: compared where it is defined, through what consumes it)
        runs.append([t.clone() for t in sel[3:] + scores[:2] + (scores[3][packed.valid.bool()],) + fwd + bwd])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert torch.equal(runs[0][0], packed.matching_pos) and torch.equal(runs[0][1], packed.matching_neg)
    again = run(name, True)
    first = fused_run(name)
    for k in KEYS:
        assert torch.equal(again["losses"][k], first["losses"][k])
        assert all(torch.equal(a, b) for a, b in zip(again["grads"][k], first["grads"][k]))


def got_flat(name):
    return fused_run(name)["flat"]


def test_one_host_copy_and_nothing_else_synchronises(monkeypatch):
    """Everything of the fused call but `_host_copy` runs under torch.cuda.set_sync_debug_mode("error"): any other synchronising
    PyTorch call (nonzero, .item(), boolean-mask indexing, .cpu(), a blocking upload) raises there; the composition does raise."""
    from uninext_amd import reid
    name = "reid_q130_mixed_c64"
    cfg = C.CASES[name]
    args = C.rebuild(C.make_inputs(cfg), len(cfg["images"]), device=DEV)
    ref_box, all_indices, targets, det_targets, hs_key, hs_ref, ref_cls = args
    hs_ref.requires_grad_(True)
    fused_run(name)                                                  # warm-up: library load, allocator, pinned staging buffer
    copies = []
    real = reid._host_copy

    def counted(t):
        copies.append(t.numel())
        torch.cuda.set_sync_debug_mode("default")
        try:
            return real(t)
        finally:
            torch.cuda.set_sync_debug_mode("error")

    monkeypatch.setattr(reid, "_host_copy", counted)
    params = torch.ones((), device=DEV, requires_grad=True)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        random.seed(C.SEED)
        packed = reid.select_pos_neg(ref_box, all_indices, targets, det_targets, nn.Identity(), hs_key, hs_ref, ref_cls, fused=True)
        losses = reid.loss_reid({"pred_qd": packed, "reid_params": params}, None, None, 1.0)
        (losses["loss_reid"] + losses["loss_reid_aux"]).backward()
        with pytest.raises(RuntimeError):
            reid.select_pos_neg(ref_box, all_indices, targets, det_targets, nn.Identity(), hs_key, hs_ref, ref_cls, fused=False)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert len(copies) == 1 and isinstance(packed, reid.PackedContrastItems)
    assert torch.equal(losses["loss_reid"], fused_run(name)["losses"]["loss_reid"]) and hs_ref.grad is not None


def test_refusals_fall_back_or_raise():
    from uninext_amd import reid

    def call(cfg, change=None, **kwargs):
        a = list(C.rebuild(C.make_inputs(cfg), len(cfg["images"]), device=DEV))
        if change:
            change(a)
        random.seed(C.SEED)
        return reid.select_pos_neg(a[0], a[1], a[2], a[3], nn.Identity(), a[4], a[5], a[6], fused=True, **kwargs)

    base = {"seed": 9, "Q": 100, "Qk": 8, "C": 64, "T": 8, "images": [C._img(2)]}
    assert isinstance(call(base), reid.PackedContrastItems)
    with pytest.raises(RuntimeError):                              # what torch.topk raises in the reference
        call(dict(base, Q=99))
    assert isinstance(call(dict(base, C=96)), list)                # C no multiple of 64: the composition

    def half(a):
        a[4], a[5] = a[4].half(), a[5].half()

    def strided(a):
        a[0] = torch.cat([a[0], a[0]], dim=2)[:, :, :4]

    def host_indices(a):
        a[1] = [i.cpu() for i in a[1]]

    for change in (half, strided, host_indices):
        assert isinstance(call(base, change), list), change.__name__
    def key_out_of_range(a):
        a[1][0][1] = 8                                             # Qk = 8: one past the key embeddings

    with pytest.raises(IndexError):                                # behind the one host copy; the kernels clamp what they read
        call(base, key_out_of_range)
    zero = call({"seed": 9, "Q": 100, "Qk": 8, "C": 64, "T": 8, "images": [C._img(0), C._img(2, valid=[0, 0])]})
    assert len(zero) == 0
    params = torch.ones((), device=DEV, requires_grad=True)
    losses = reid.loss_reid({"pred_qd": zero, "reid_params": params}, None, None, 1.0)
    assert float(losses["loss_reid"]) == 0.0 and float(losses["loss_reid_aux"]) == 0.0
