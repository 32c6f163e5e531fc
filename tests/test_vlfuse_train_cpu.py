"""The training route of the bi-directional attention core without a GPU: the float64 restatement of
tests/vlfuse_train_cases.py against autograd of BiMultiHeadAttention._core_torch, the inputs of the GPU sweep (the fp32 composition
alone stays inside the bound), wrong variants that must leave it, the C ABI's table rows, and the module flag on the CPU."""
import os
import types

import numpy as np
import pytest
import torch

import parity_measure as PM
import vlfuse_train_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg():
    fuse = types.SimpleNamespace(STABLE_SOFTMAX_2D=False, CLAMP_MIN_FOR_UNDERFLOW=True, CLAMP_MAX_FOR_OVERFLOW=True)
    return types.SimpleNamespace(MODEL=types.SimpleNamespace(DYHEAD=types.SimpleNamespace(FUSE_CONFIG=fuse)))


def _autograd(x):
    """Gradients in float64: of BiMultiHeadAttention._core_torch ITSELF without a mask (and in
    test_restatement_is_autograd_of_core_torch_with_an_int64_mask_that_masks_nothing); with a mask that masks something, of
    _core_torch's sequence RE-TYPED here with one change, because float64 does not show the fp32 fact by itself: a masked score
    is exactly -9e15 (the fp32 add absorbs the score) and still passes the gradient, restated as s + (-9e15 - s.detach())."""
    from uninext_amd.modules.vl_fusion import BiMultiHeadAttention
    H, E = x["H"], x["H"] * VC.D
    attn = BiMultiHeadAttention(v_dim=8, l_dim=8, embed_dim=E, num_heads=H, dropout=0.0, cfg=_cfg()).double()
    scale = np.float32(x["scale"])
    qs = torch.tensor((x["q"] * scale).astype(np.float32).astype(np.float64), requires_grad=True)
    k, vv, vl = (torch.tensor(x[n].astype(np.float64), requires_grad=True) for n in ("k", "vv", "vl"))
    if x["mask"] is None:
        out_v, out_l = attn._core_torch(qs, k, vv, vl, None)
    else:                                                           # _core_torch's own sequence, the absorbing add restated
        B, S, T = x["B"], x["S"], x["T"]
        heads = lambda t: attn._shape(t, -1, B).view(B * H, -1, VC.D)
        w = attn._clamp(torch.bmm(heads(qs), heads(k).transpose(1, 2)))
        w_t = w.transpose(1, 2)
        w_l = attn._clamp(w_t - torch.max(w_t, dim=-1, keepdim=True)[0]).softmax(dim=-1)
        m = torch.tensor(x["mask"]).double()[:, None, None, :].expand(B, H, S, T)
        w4 = w.view(B, H, S, T)
        w4 = torch.where(m == 0, w4 + (VC.MASKED - w4.detach()), w4 + m)
        w_v = w4.reshape(B * H, S, T).softmax(dim=-1)
        merge = lambda t, n: t.view(B, H, n, VC.D).transpose(1, 2).reshape(B, n, E)
        out_v, out_l = merge(torch.bmm(w_v, heads(vl)), S), merge(torch.bmm(w_l, heads(vv)), T)
    loss = (out_v * torch.tensor(x["gv"].astype(np.float64))).sum() + (out_l * torch.tensor(x["gl"].astype(np.float64))).sum()
    loss.backward()
    return dict(out_v=out_v.detach().numpy(), out_l=out_l.detach().numpy(), dq=qs.grad.numpy() * float(scale), dk=k.grad.numpy(),
                dvv=vv.grad.numpy(), dvl=vl.grad.numpy())


@pytest.mark.parametrize("mask,special", [("none", None), ("i64", None), ("allmasked", None), ("f32", None), ("none", "equal"),
                                          ("none", "inner"), ("none", "beyond"), ("allmasked", "equal")])
def test_restatement_is_autograd_of_the_composition_or_its_retyped_masked_sequence_in_float64(mask, special):
    x = VC.make(2, 2, 7, 5, mask, special)
    want, auto = VC.core(x), _autograd(x)
    for n in VC.GRADS + ("out_v", "out_l"):
        scale = max(np.abs(want[n]).max(), 1e-300)
        assert np.abs(auto[n] - want[n]).max() <= 1e-11 * scale, (n, np.abs(auto[n] - want[n]).max() / scale)
    if mask == "allmasked":                                         # uniform over T, and its ds_v is not zero
        a = VC.core(x)
        assert np.abs(a["dr"][-1]).max() > 0


def test_restatement_is_autograd_of_core_torch_with_an_int64_mask_that_masks_nothing():
    """_core_torch itself with an int64 mask of ones: every score gets + 1, nothing is set to -9e15, float64 needs no help."""
    from uninext_amd.modules.vl_fusion import BiMultiHeadAttention
    x = VC.make(2, 2, 7, 5, "none")
    x["mask"] = np.ones((2, 5), dtype=np.int64)
    attn = BiMultiHeadAttention(v_dim=8, l_dim=8, embed_dim=2 * VC.D, num_heads=2, dropout=0.0, cfg=_cfg()).double()
    qs = torch.tensor((x["q"] * np.float32(x["scale"])).astype(np.float32).astype(np.float64), requires_grad=True)
    k, vv, vl = (torch.tensor(x[n].astype(np.float64), requires_grad=True) for n in ("k", "vv", "vl"))
    out_v, out_l = attn._core_torch(qs, k, vv, vl, torch.tensor(x["mask"]))
    ((out_v * torch.tensor(x["gv"].astype(np.float64))).sum() + (out_l * torch.tensor(x["gl"].astype(np.float64))).sum()).backward()
    want = VC.core(x)
    auto = dict(out_v=out_v.detach().numpy(), out_l=out_l.detach().numpy(), dq=qs.grad.numpy() * x["scale"], dk=k.grad.numpy(),
                dvv=vv.grad.numpy(), dvl=vl.grad.numpy())
    for n in auto:
        assert np.abs(auto[n] - want[n]).max() <= 1e-11 * np.abs(want[n]).max(), n


def test_special_cases_are_what_they_say():
    eq, be, inn = (VC.core(VC.make(1, 1, 33, 33, "none", s)) for s in ("equal", "beyond", "inner"))
    assert eq["r"][0, 0, 0, 0] == VC.CLAMP and eq["dr"][0, 0, 0, 0] != 0.0
    assert be["r"][0, 0, 0, 0] > VC.CLAMP and be["r"][0, 0, -1, -1] < -VC.CLAMP and be["dr"][0, 0, 0, 0] == 0.0
    assert (inn["e"][0, 0, :, 0] == -VC.CLAMP).all()


SWEEP = [(S, T, bh, VC.MASKS[(si + ti + bi) % len(VC.MASKS)])
         for si, S in enumerate(VC.SS) for ti, T in enumerate(VC.TS) for bi, bh in enumerate(VC.BHS)]


def test_composition_alone_stays_inside_the_bound_on_the_sweeps_cases():
    """The condition that the inputs were chosen well: the fp32 composition, measured as a kernel would be with the composition
    term dropped (comp = nan), stays inside SUM_DEPTH u s alone on a spread of the sweep's cases and on every special one."""
    cases = [VC.make(bh[0], bh[1], S, T, m) for S, T, bh, m in SWEEP[::9]]
    cases += [VC.make(1, 1, 33, 33, "none", s) for s in VC.SPECIALS] + [VC.make(2, 3, 129, 65, m) for m in VC.MASKS]
    for x in cases:
        want, comp = VC.core(x), VC.core(x, np.float32)
        for n in VC.GRADS + ("out_v", "out_l"):
            nan = np.full(want[n].shape, np.nan)
            PM.errors(comp[n].astype(np.float64), want[n], want["mag_" + n], nan).check(x["name"], n)


@pytest.mark.parametrize("variant,mask,special", [("gate_dropped", "none", "beyond"), ("gate_exclusive", "none", "equal"),
                                                  ("dk_without_ds_l", "i64", None), ("mask_on_text", "i64", None),
                                                  ("delta_swapped", "i64", None), ("dq_unscaled", "i64", None)])
def test_wrong_variants_leave_the_bound(variant, mask, special):
    x = VC.make(1, 1, 33, 33, mask, special)
    want, comp, bad = VC.core(x), VC.core(x, np.float32), VC.core(x, np.float32, variant=variant)
    worst = max(PM.errors(bad[n].astype(np.float64), want[n], want["mag_" + n], comp[n].astype(np.float64)).worst
                for n in VC.GRADS + ("out_v", "out_l"))
    assert worst > 1.0, (variant, worst)


def test_header_and_signature_table_agree_on_the_training_entry_points():
    import test_binding_signatures_cpu as SIG
    from uninext_amd import _lib
    declared = SIG.prototypes(os.path.join(ROOT, "include", "biattn_hip.h"))
    for name in ("biattn_hip_train_f32", "biattn_hip_backward_f32", "biattn_hip_backward_workspace_bytes",
                 "biattn_hip_backward_last_kernel"):
        restype, argtypes = _lib._SIGNATURES["biattn_hip.h"][name]
        row = (SIG.ctypes_kind(restype, name), [SIG.ctypes_kind(t, name) for t in argtypes])
        assert row == declared[name], (name, row, declared[name])
    assert len(declared["biattn_hip_train_f32"][1]) == len(declared["biattn_hip_forward_f32"][1]) + 2
    assert len(declared["biattn_hip_backward_f32"][1]) == 25


def test_module_with_the_flag_on_is_the_composition_bitwise_on_the_cpu():
    from uninext_amd.modules.vl_fusion import BiAttentionBlockForCheckpoint, BiMultiHeadAttention
    assert BiMultiHeadAttention.own_training is False
    torch.manual_seed(3)
    block = BiAttentionBlockForCheckpoint(v_dim=32, l_dim=24, embed_dim=512, num_heads=2, dropout=0.0, init_values=0.25, cfg=_cfg())
    mask = (torch.arange(6)[None, :] < torch.tensor([6, 4])[:, None]).long()
    results = []
    for flag in (False, True):
        block.attn.own_training = flag
        block.zero_grad(set_to_none=True)
        g = torch.Generator().manual_seed(1)
        v = torch.randn(2, 19, 32, generator=g, requires_grad=True)
        l = torch.randn(2, 6, 24, generator=g, requires_grad=True)
        ov, ol = block(v, l, mask)
        (ov.sum() + (ol * ol).sum()).backward()
        results.append([ov.detach(), ol.detach(), v.grad, l.grad] + [p.grad for p in block.parameters()])
    for a, b in zip(*results):
        assert torch.equal(a, b)
