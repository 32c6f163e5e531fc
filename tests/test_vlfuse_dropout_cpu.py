"""The attention dropout inside the bi-directional attention core without a GPU: Philox4x32-10's known answers, the properties
of the keep masks, the float64 restatement of tests/vlfuse_dropout_cases.py against torch's float64 autograd, wrong variants
that must leave the bound, the C ABI's rows and the Python surface, and the registers of the new kernel instantiations."""
import inspect
import os
import shutil
import sys
import types

import numpy as np
import pytest
import torch

import parity_measure as PM
import vlfuse_dropout_cases as DC
import vlfuse_train_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("biattn_hip_train_dropout_f32", "biattn_hip_backward_dropout_f32", "biattn_hip_dropout_keep_u8")


# ------------------------------------------------------------------------------------------------------------- the generator

@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    got = DC.philox4x32_10(counter, key)
    assert " ".join("%08x" % int(w) for w in got) == want


def _plain_philox(counter, key):
    """Philox4x32-10 in plain Python integers, written apart from the numpy one."""
    c, k = list(counter), list(key)
    for _ in range(10):
        a, b = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(b >> 32) ^ c[1] ^ k[0], b & 0xFFFFFFFF, (a >> 32) ^ c[3] ^ k[1], a & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def test_numpy_philox_is_the_plain_python_one_and_the_masks_follow_the_headers_layout():
    seed = DC.seed_of("layout")
    sd, off = (int(v) for v in seed.view(np.uint64))
    p, BH, S, T = 0.5, 3, 5, 7
    kv, kl = DC.keep_masks(seed, p, BH, S, T)
    assert kv.shape == (BH, S, T) and kl.shape == (BH, T, S)
    thr = DC.threshold_of(p)
    assert thr == 1 << 31
    for side, bh, i, j in ((0, 0, 0, 0), (1, 0, 0, 0), (0, 2, 4, 6), (1, 2, 4, 6), (0, 1, 3, 5), (1, 1, 2, 4)):
        w = _plain_philox((off & 0xFFFFFFFF, off >> 32, i, side << 31 | bh << 8 | j // 4), (sd & 0xFFFFFFFF, sd >> 32))
        assert (kv[bh, i, j] if side == 0 else kl[bh, j, i]) == (w[j % 4] >= thr), (side, bh, i, j)


def test_mask_properties():
    seed = DC.seed_of("properties")
    kv0, kl0 = DC.keep_masks(seed, 0.0, 2, 9, 5)
    assert kv0.all() and kl0.all() and DC.threshold_of(0.0) == 0 and DC.scale_of(0.0) == np.float32(1.0)
    kv, kl = DC.keep_masks(seed, 0.5, 2, 33, 32)
    assert not np.array_equal(kv, kl.transpose(0, 2, 1))                      # the two sides are independent
    kv2, _ = DC.keep_masks(DC.seed_of("another"), 0.5, 2, 33, 32)
    assert not np.array_equal(kv, kv2)
    assert not np.array_equal(kv[0], kv[1])                                   # and so are the (batch, head) pairs
    # a change of the offset alone is another mask
    moved = seed.copy()
    moved[1] += 1
    assert not np.array_equal(kv, DC.keep_masks(moved, 0.5, 2, 33, 32)[0])


def test_kept_share():
    """(B * H, S, T) = (6, 257, 256), p = 0.1, a fixed seed: the kept share within 5 sigma of 0.9, sigma = sqrt(0.09 / N).  The
    outcome is deterministic."""
    kv, kl = DC.keep_masks(DC.seed_of("share"), 0.1, 6, 257, 256)
    n = kv.size
    for name, m in (("v", kv), ("l", kl)):
        share = m.mean()
        print("kept share", name, share)
        assert abs(share - 0.9) <= 5.0 * np.sqrt(0.09 / n), (name, share)


# ----------------------------------------------------------------------------------------------------------- the restatement

def test_restatement_without_dropout_is_the_training_restatement_exactly():
    for shape, mask in (((2, 3, 33, 9), "i64"), ((1, 1, 5, 1), "none"), ((2, 2, 7, 5), "allmasked")):
        x = VC.make(*shape, mask)
        kv, kl = DC.case_masks(x, 0.0, DC.seed_of(x["name"]))
        for dt in (np.float64, np.float32):
            a, b = DC.core(x, kv, kl, 0.0, dt), VC.core(x, dt)
            for n in DC.OUTPUTS + (tuple("mag_" + m for m in DC.OUTPUTS) if dt is np.float64 else ()):
                assert np.array_equal(a[n], b[n]), (shape, dt, n)


def _cfg():
    fuse = types.SimpleNamespace(STABLE_SOFTMAX_2D=False, CLAMP_MIN_FOR_UNDERFLOW=True, CLAMP_MAX_FOR_OVERFLOW=True)
    return types.SimpleNamespace(MODEL=types.SimpleNamespace(DYHEAD=types.SimpleNamespace(FUSE_CONFIG=fuse)))


def _autograd(x, keep_v, keep_l, p):
    """torch float64 autograd through BiMultiHeadAttention._core_torch's op sequence, re-typed with the two dropout lines
    replaced by `w * keep * c` (and the absorbing fp32 add of a masked score restated as in tests/test_vlfuse_train_cpu.py)."""
    from uninext_amd.modules.vl_fusion import BiMultiHeadAttention
    B, H, S, T = x["B"], x["H"], x["S"], x["T"]
    E = H * VC.D
    attn = BiMultiHeadAttention(v_dim=8, l_dim=8, embed_dim=E, num_heads=H, dropout=p, cfg=_cfg()).double()
    scale = np.float32(x["scale"])
    c = float(DC.scale_of(p))
    qs = torch.tensor((x["q"] * scale).astype(np.float32).astype(np.float64), requires_grad=True)
    k, vv, vl = (torch.tensor(x[n].astype(np.float64), requires_grad=True) for n in ("k", "vv", "vl"))
    heads = lambda t: attn._shape(t, -1, B).view(B * H, -1, VC.D)
    w = attn._clamp(torch.bmm(heads(qs), heads(k).transpose(1, 2)))
    w_t = w.transpose(1, 2)
    w_l = attn._clamp(w_t - torch.max(w_t, dim=-1, keepdim=True)[0]).softmax(dim=-1)
    if x["mask"] is not None:
        m = torch.tensor(x["mask"]).double()[:, None, None, :].expand(B, H, S, T)
        w4 = w.view(B, H, S, T)
        w = torch.where(m == 0, w4 + (VC.MASKED - w4.detach()), w4 + m).reshape(B * H, S, T)
    w_v = w.softmax(dim=-1)
    p_v = w_v * torch.tensor(keep_v).double() * c
    p_l = w_l * torch.tensor(keep_l).double() * c
    merge = lambda t, n: t.view(B, H, n, VC.D).transpose(1, 2).reshape(B, n, E)
    out_v, out_l = merge(torch.bmm(p_v, heads(vl)), S), merge(torch.bmm(p_l, heads(vv)), T)
    ((out_v * torch.tensor(x["gv"].astype(np.float64))).sum() + (out_l * torch.tensor(x["gl"].astype(np.float64))).sum()).backward()
    return dict(out_v=out_v.detach().numpy(), out_l=out_l.detach().numpy(), dq=qs.grad.numpy() * float(scale), dk=k.grad.numpy(),
                dvv=vv.grad.numpy(), dvl=vl.grad.numpy())


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("shape,mask", [((2, 3, 33, 9), "none"), ((2, 3, 33, 9), "i64"), ((1, 1, 5, 1), "none"), ((1, 1, 5, 1), "f32")])
def test_restatement_is_float64_autograd_of_the_composition_with_the_masks(shape, mask, p):
    x = VC.make(*shape, mask)
    kv, kl = DC.case_masks(x, p, DC.seed_of(x["name"]))
    want, auto = DC.core(x, kv, kl, p), _autograd(x, kv, kl, p)
    for n in DC.OUTPUTS:
        scale = max(np.abs(want[n]).max(), 1e-300)
        assert np.abs(auto[n] - want[n]).max() <= 1e-11 * scale, (n, np.abs(auto[n] - want[n]).max() / scale)


def test_composition_alone_stays_inside_the_bound():
    """The condition that magnitudes and inputs fit: the fp32 composition under the masks, with the composition term dropped,
    stays inside SUM_DEPTH u s alone."""
    for shape, mask, p in (((2, 3, 129, 65), "i64", 0.1), ((2, 3, 129, 65), "allmasked", 0.5), ((1, 1, 33, 33), "none", 0.5)):
        x = VC.make(*shape, mask)
        kv, kl = DC.case_masks(x, p, DC.seed_of(x["name"]))
        want, comp = DC.core(x, kv, kl, p), DC.core(x, kv, kl, p, np.float32)
        for n in DC.OUTPUTS:
            PM.errors(comp[n].astype(np.float64), want[n], want["mag_" + n], np.full(want[n].shape, np.nan)).check(x["name"], n)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("variant", DC.VARIANTS)
def test_wrong_variants_leave_the_bound(variant, p):
    x = VC.make(2, 3, 129, 65, "i64")
    kv, kl = DC.case_masks(x, p, DC.seed_of(x["name"]))
    want, comp = DC.core(x, kv, kl, p), DC.core(x, kv, kl, p, np.float32)
    bad = DC.core(x, kv, kl, p, np.float32, variant=variant)
    worst = max(PM.errors(bad[n].astype(np.float64), want[n], want["mag_" + n], comp[n].astype(np.float64)).worst for n in DC.OUTPUTS)
    assert worst > 1.0, (variant, worst)


# ------------------------------------------------------------------------------------------------------- the ABI and the binding

def test_header_declares_and_the_table_binds_the_three_entry_points():
    import test_binding_signatures_cpu as SIG
    from uninext_amd import _lib
    declared = SIG.prototypes(os.path.join(ROOT, "include", "biattn_hip.h"))
    for name in NEW:
        assert name in declared and name in _lib.BIATTN_EXPORTS, name
        restype, argtypes = _lib._SIGNATURES["biattn_hip.h"][name]
        row = (SIG.ctypes_kind(restype, name), [SIG.ctypes_kind(t, name) for t in argtypes])
        assert row == declared[name], (name, row, declared[name])
    # the arguments of the entry points without dropout plus (float dropout_p, const unsigned long long* seed), the stream last
    for new, old in (("biattn_hip_train_dropout_f32", "biattn_hip_train_f32"), ("biattn_hip_backward_dropout_f32", "biattn_hip_backward_f32")):
        assert declared[new][1] == declared[old][1][:-1] + ["float", "pointer", "pointer"], new
    assert declared["biattn_hip_dropout_keep_u8"] == ("int", ["pointer", "float", "int", "int", "int", "int", "pointer", "pointer", "pointer"])


def test_python_surface():
    from uninext_amd import ext
    from uninext_amd.modules.vl_fusion import BiMultiHeadAttention, VLFuse
    for fn in (ext.bi_attention_train, ext.bi_attention_backward):
        params = inspect.signature(fn).parameters
        assert params["dropout_p"].default == 0.0 and params["seed"].default is None
    assert callable(ext.bi_attention_dropout_keep) and callable(ext.bi_attention_seed)
    assert BiMultiHeadAttention.own_dropout is False and BiMultiHeadAttention.own_training is False
    assert inspect.signature(VLFuse.set_own_training).parameters["dropout"].default is False


def test_module_with_both_flags_on_is_the_composition_bitwise_on_the_cpu():
    """No GPU tensors: the flags change nothing, and F.dropout's stream is the one that is used."""
    from uninext_amd.modules.vl_fusion import BiAttentionBlockForCheckpoint
    torch.manual_seed(3)
    block = BiAttentionBlockForCheckpoint(v_dim=32, l_dim=24, embed_dim=512, num_heads=2, dropout=0.1, init_values=0.25, cfg=_cfg())
    block.train()
    results = []
    for flags in ((False, False), (True, True)):
        block.attn.own_training, block.attn.own_dropout = flags
        block.zero_grad(set_to_none=True)
        g = torch.Generator().manual_seed(1)
        v = torch.randn(2, 19, 32, generator=g, requires_grad=True)
        l = torch.randn(2, 6, 24, generator=g, requires_grad=True)
        torch.manual_seed(9)
        ov, ol = block(v, l, None)
        (ov.sum() + (ol * ol).sum()).backward()
        results.append([ov.detach(), ol.detach(), v.grad, l.grad] + [p.grad for p in block.parameters()])
    for a, b in zip(*results):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ the registers

# (VGPRs at most, scratch bytes per lane) of the instantiations with dropout: what they compiled to when they were written
PINNED = {
    "biattn_bwd.hip": {
        "biattn_bwd::image_train_dropout<1>": (186, 0), "biattn_bwd::image_train_dropout<2>": (204, 0),
        "biattn_bwd::image_train_dropout<4>": (237, 0), "biattn_bwd::image_train_dropout<8>": (256, 0),
        "biattn_bwd::bwd_image_dropout<false>": (256, 0), "biattn_bwd::bwd_image_dropout<true>": (211, 0),
        "biattn_bwd::bwd_text_dropout<0>": (256, 0), "biattn_bwd::bwd_text_dropout<1>": (256, 0),
        "biattn_bwd::bwd_text_dropout<2>": (256, 0), "biattn_bwd::dropout_keep": (20, 0)},
    "biattn.hip": {"biattn::biattn_text_dropout": (256, 0)},
}


@pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None, reason="needs hipcc")
@pytest.mark.parametrize("name", sorted(PINNED))
def test_dropout_kernels_keep_their_registers_and_no_kernel_of_the_file_uses_scratch(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    got = kernel_resources.resources(os.path.join(ROOT, "uninext_amd", "csrc", name))
    assert set(PINNED[name]) <= set(got), sorted(set(PINNED[name]) - set(got))
    for kernel, r in got.items():
        assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0, (kernel, r)
    for kernel, (vgprs, scratch) in PINNED[name].items():
        assert got[kernel]["vgprs"] <= vgprs and got[kernel]["scratch"] == scratch, (kernel, got[kernel])
