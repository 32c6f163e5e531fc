"""The decoder self-attention core's training route (DeformableTransformerDecoderLayer.own_training, biattn_hip_self_train_f32 /
biattn_hip_self_backward_f32 in include/biattn_hip.h): everything that needs no GPU."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import decoder_cases as C          # noqa: E402
import decoder_train_cases as T    # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = [n for n in T.EXPECTED if n.startswith("layer_")]


def build(name, cfg, state, dtype, device="cpu", **args):
    if cfg["kind"] == "decoder":
        args.setdefault("look_forward_twice", True)      # as the fixture's reference run: every box head has a gradient
    return C.build(name, cfg, state, dtype, device, **args)


@pytest.mark.parametrize("name", LAYERS)
def test_reference_helper_agrees_with_float64_multihead_attention(name):
    """core64's gradients against float64 autograd of nn.MultiheadAttention's core on the layer cases' own projections.  The
    only difference is the fp32 rounding of the scaled q (relative 6e-8 per element), so the two agree to 1e-6."""
    cfg, state, x = C.make_case(name)
    E, heads = cfg["d_model"], cfg["heads"]
    w, b = state["self_attn.in_proj_weight"], state["self_attn.in_proj_bias"]
    xin = x["tgt"] + x["query_pos"]
    qk = (xin @ w[:2 * E].t() + b[:2 * E]).float()
    v = (x["tgt"] @ w[2 * E:].t() + b[2 * E:]).float()
    mask = x.get("attn_mask")
    mask = mask if mask is None or mask.dtype == torch.bool else mask.float()
    G = T.upstream(cfg["seed"], 2, cfg["lq"], E)
    got, out = T.reference_grads(qk, v, heads, mask, G)

    mha = torch.nn.MultiheadAttention(E, heads).double()
    with torch.no_grad():      # identity projections: the module's core alone
        mha.in_proj_weight.copy_(torch.eye(E).repeat(3, 1))
        mha.in_proj_bias.zero_()
        mha.out_proj.weight.copy_(torch.eye(E))
        mha.out_proj.bias.zero_()
    q, k, vv = (t.double().clone().requires_grad_(True) for t in (qk[..., :E], qk[..., E:], v))
    ref = mha(q.transpose(0, 1), k.transpose(0, 1), vv.transpose(0, 1),
              attn_mask=mask if mask is None or mask.dtype == torch.bool else mask.double())[0].transpose(0, 1)
    (ref * G.double()).sum().backward()
    assert C.rel_err(out, ref.detach()) < 1e-6
    errs = T.group_err(got, {"dq": q.grad, "dk": k.grad, "dv": vv.grad})
    print(name, errs)
    assert max(errs.values()) < 1e-6


def test_error_codes_without_a_device():
    from uninext_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(1 << 20)      # never dereferenced: every check runs before the device is touched
    off = ctypes.c_void_p((1 << 20) + 4)
    odd = ctypes.c_void_p((1 << 20) + 2)
    big = 1 << 40

    def train(q=fake, k=fake, v=fake, strides=(128, 128, 64), mask=None, kind=0, dims=(2, 2, 40, 32), out=fake, lse=fake):
        return lib.biattn_hip_self_train_f32(q, k, v, *strides, mask, kind, *dims, 0.25, out, lse, None)

    def back(q=fake, k=fake, v=fake, strides=(128, 128, 64), mask=None, kind=0, out=fake, lse=fake, g=fake, dims=(2, 2, 40, 32),
             dq=fake, dk=fake, dv=fake, gstrides=(128, 128, 64), ws=fake, ws_bytes=big):
        return lib.biattn_hip_self_backward_f32(q, k, v, *strides, mask, kind, out, lse, g, *dims, 0.25, dq, dk, dv, *gstrides, ws,
                                                ws_bytes, None)

    for call in (train, back):
        assert call(q=None) == -1 and "null" in _lib.last_error()
        assert call(k=None) == -1 and call(v=None) == -1 and call(out=None) == -1 and call(lse=None) == -1
        assert call(kind=_lib.BIATTN_MASK_BOOL) == -1 and call(kind=_lib.BIATTN_MASK_F32) == -1          # a kind without a mask
        assert call(dims=(2, 2, 0, 32)) == -2 and "dimensions" in _lib.last_error()
        assert call(dims=(2, 0, 40, 32)) == -2 and call(dims=(-1, 2, 40, 32)) == -2
        assert call(dims=(2, 2, 65536, 32)) == -2 and "65535" in _lib.last_error()
        assert call(dims=(2, 2, 40, 64)) == -5 and "head_dim" in _lib.last_error()
        assert call(kind=_lib.BIATTN_MASK_INT64, mask=fake) == -5 and "mask kind" in _lib.last_error()
        assert call(strides=(60, 128, 64)) == -2 and "stride" in _lib.last_error()
        assert call(strides=(128, 130, 64)) == -5 and "multiples of 4" in _lib.last_error()
        assert call(strides=(128, 128, 1 << 31)) == -2 and "large" in _lib.last_error()
        assert call(q=off) == -5 and "aligned" in _lib.last_error()
        assert call(lse=off) == -5 and call(out=off) == -5
        assert call(mask=odd, kind=_lib.BIATTN_MASK_F32) == -5 and "4-byte" in _lib.last_error()
        assert call(dims=(0, 2, 40, 32)) == 0                    # an empty batch enqueues nothing
        assert call(dims=(0, 2, 40, 48)) == -5                   # the geometry is still checked
    assert back(g=None) == -1 and back(dq=None) == -1 and back(dk=None) == -1 and back(dv=None) == -1 and back(ws=None) == -1
    assert back(g=off) == -5 and back(dq=off) == -5 and back(dv=off) == -5 and back(ws=off) == -5
    assert back(gstrides=(128, 128, 60)) == -2 and back(gstrides=(126, 128, 64)) == -5
    need = lib.biattn_hip_self_backward_workspace_bytes(2, 2, 40, 32)
    assert need >= 2 * 2 * 64 * 4 and need < 2 * 2 * 40 * 40 * 4
    assert back(ws_bytes=need - 1) == -6 and "workspace" in _lib.last_error()
    assert lib.biattn_hip_self_backward_workspace_bytes(2, 2, 40, 64) == 0 and lib.biattn_hip_self_backward_workspace_bytes(2, 2, 0, 32) == 0
    assert lib.biattn_hip_self_backward_workspace_bytes(2, 2, 65536, 32) == 0
    assert back(q=None, k=None, v=None, out=None, lse=None, g=None, dims=(0, 2, 40, 32), dq=None, dk=None, dv=None, ws=None,
                ws_bytes=0) == 0                                  # and needs no buffer
    assert _lib.last_kernel("dec_attn_bwd") == "" or _lib.last_kernel("dec_attn_bwd").startswith("dec_bwd_q<")
    for n in ("biattn_hip_self_train_f32", "biattn_hip_self_backward_workspace_bytes", "biattn_hip_self_backward_f32",
              "biattn_hip_self_backward_last_kernel"):
        assert n in _lib._SIGNATURES["biattn_hip.h"] and hasattr(lib, n)


def test_new_kernels_have_no_scratch():
    import kernel_resources
    got = kernel_resources.resources(os.path.join(ROOT, "uninext_amd", "csrc", "dec_attn_bwd.hip"))
    names = ["dec_attn_bwd::%s<%d>" % (k, m) for k in ("attn_lse", "bwd_q", "bwd_kv") for m in (0, 2, 3)]
    assert sorted(got) == sorted(names)
    for n in names:
        print(n, got[n])
        assert got[n]["scratch"] == 0 and got[n].get("vgpr_spill", 0) == 0 and got[n].get("sgpr_spill", 0) == 0, n
        assert got[n]["lds"] <= 64 * 1024


def test_own_training_defaults_to_false_and_setters():
    from uninext_amd import modules as M
    assert M.DeformableTransformerDecoderLayer.own_training is False
    cfg, state, _ = C.make_case("decoder_2layers")
    dec = build("decoder_2layers", cfg, state, torch.float32)
    assert not any(layer.own_training for layer in dec.layers)
    assert dec.set_own_training(True) is dec and all(layer.own_training for layer in dec.layers)
    assert all("own_training" in vars(layer) for layer in dec.layers) and M.DeformableTransformerDecoderLayer.own_training is False
    dec.set_own_training(False)
    assert not any(layer.own_training for layer in dec.layers)
    cfg, state, _ = C.make_case("reid_head")
    head = C.build("reid_head", cfg, state, torch.float32)
    assert head.set_own_training() is head and all(layer.own_training for layer in head.layers)


def test_own_training_on_cpu_tensors_is_the_composition_bitwise():
    """CPU tensors: with the flag on the layer never enters the Function, and its gradients are the flag-off ones."""
    from uninext_amd.modules import decoder_layer as D
    cfg, state, x = C.make_case("layer_dn_mask")
    G = T.fixture_upstream("layer_dn_mask")
    m = C.build("layer_dn_mask", cfg, state, torch.float32)
    off, out_off = T.gradients(cfg, m, x, G, torch.float32)
    off = {k: v.clone() for k, v in off.items()}
    entered = []
    old = D.DecoderSelfAttentionFunction.apply
    D.DecoderSelfAttentionFunction.apply = lambda *a: entered.append(1) or old(*a)
    try:
        m.own_training = True
        on, out_on = T.gradients(cfg, m, x, G, torch.float32)
    finally:
        D.DecoderSelfAttentionFunction.apply = old
    assert not entered and torch.equal(out_off[0], out_on[0])
    assert sorted(on) == sorted(off) and all(torch.equal(on[k], off[k]) for k in off)


def test_fixtures_exist_and_their_digests_match():
    for name in T.EXPECTED:
        path = os.path.join(T.HERE, name + "_grad.npz")
        assert os.path.isfile(path) and os.path.getsize(path) < 500 * 1024, name
        cfg, state, x = C.make_case(name)
        fx = T.load(name)
        assert float(fx["digest"]) == C.digest(state) and float(fx["fp32_err"]) < 3e-5
        assert sorted(fx["grad"]) == sorted(list(T.INPUT_KEYS[cfg["kind"]]) + list(state))
        for k in T.INPUT_KEYS[cfg["kind"]]:
            assert torch.equal(torch.from_numpy(fx[k]).double(), x[k]), (name, k)
        if "attn_mask" in x:
            assert torch.equal(torch.from_numpy(fx["attn_mask"]).to(x["attn_mask"].dtype), x["attn_mask"])
        for g, want in zip(fx["G"], T.fixture_upstream(name)):
            assert torch.equal(g, want)
        rows = [k[len("rows."):] for k in fx if k.startswith("rows.")]
        assert bool(rows) == (cfg["d_model"] == 256) and all(k in state for k in rows)
        for k in rows:
            n = state[k].reshape(-1, state[k].shape[-1]).shape[0]
            assert torch.equal(torch.from_numpy(fx["rows." + k]), T.stored_rows(name, k, n, len(fx["rows." + k])))


@pytest.mark.parametrize("name", T.EXPECTED)
def test_float64_composition_reproduces_the_fixtures(name):
    cfg, state, x = C.make_case(name)
    fx = T.load(name)
    m = build(name, cfg, state, torch.float64)
    got, _ = T.gradients(cfg, m, x, fx["G"], torch.float64)
    for k, want in fx["grad"].items():
        view = T.stored_view(fx, k, got[k]).double()
        # the fixtures store the float32 roundings of the float64 gradients: every entry is within 1e-9 of the group's scale of a
        # number that rounds to the stored one, i.e. within that plus half a float32 step at the stored value
        half_step = (torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs()).double() / 2
        excess = ((view - want.double()).abs() - half_step).clamp(min=0).max() / want.double().abs().max()
        assert float(excess) < 1e-9, (k, float(excess))
