"""ConvNeXt training route (include/patch_embed_hip.h: the backward entry points of the block's head, tail and the channels-first
LayerNorm; uninext_amd/backbone.py: own_training): everything that needs no GPU."""
import ctypes
import os
import shutil
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnext_cases as C         # noqa: E402
import convnext_ref as R           # noqa: E402
import convnext_train_cases as T   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20


# ---- the C ABI without a device --------------------------------------------------------------------------------------------------
def test_argument_errors_need_no_gpu():
    from uninext_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(1 << 20)      # never dereferenced: every check runs before the device is touched
    big = 1 << 40

    def head(x=fake, w=fake, b=fake, lw=fake, go=fake, ws=fake, nbytes=big, B=1, c=32, H=5, W=5):
        return lib.patch_embed_hip_convnext_dwconv_ln_backward_f32(x, w, b, lw, 1e-6, go, B, c, H, W, fake, fake, fake, fake, fake, ws, nbytes, None)
    assert head(x=None) == -1 and "null" in _lib.last_error()
    assert head(w=None) == -1 and head(lw=None) == -1 and head(go=None) == -1
    assert head(H=0) == -2 and "dimensions" in _lib.last_error()
    assert head(W=-1) == -2 and head(c=0) == -2 and head(B=-1) == -2
    for c in (16, 48, 1568, 2048):
        assert head(c=c) == -5, c
    assert "multiple of 32" in _lib.last_error()
    assert head(go=ctypes.c_void_p((1 << 20) + 4)) == -5 and "aligned" in _lib.last_error()
    assert head(B=1 << 20, c=1536, H=64, W=64) == -2 and "large" in _lib.last_error()
    assert head(B=1, c=32, H=1, W=(1 << 26) - 4) == -2
    need = lib.patch_embed_hip_convnext_dwconv_ln_backward_workspace_bytes(1, 32, 5, 5)
    assert need > 0 and head(nbytes=need - 1) == -6 and "workspace" in _lib.last_error()
    assert head(ws=None) == -6

    def tail(go=fake, y=fake, g=fake, s=fake, gy=fake, gg=fake, ws=fake, nbytes=big, B=1, c=3, H=5, W=5):
        return lib.patch_embed_hip_convnext_scale_residual_backward_f32(go, y, g, s, B, c, H, W, gy, gg, ws, nbytes, None)
    assert tail(go=None) == -1 and tail(y=None) == -1 and tail(g=None) == -1       # y and gamma: required for grad_gamma
    assert tail(c=0) == -2 and tail(H=0) == -2 and tail(W=0) == -2 and tail(B=-1) == -2 and tail(B=1 << 16) == -2
    need = lib.patch_embed_hip_convnext_scale_residual_backward_workspace_bytes(1, 3, 5, 5)
    assert need > 0 and tail(nbytes=need - 1) == -6 and tail(ws=None) == -6

    def drop(y=fake, g=fake, s=fake, inp=fake, out=fake, B=1, c=3, H=5, W=5):
        return lib.patch_embed_hip_convnext_scale_residual_drop_f32(y, g, s, inp, B, c, H, W, out, None)
    assert drop(y=None) == -1 and drop(inp=None) == -1 and drop(out=None) == -1 and drop(y=None, s=None) == -1
    assert drop(c=0) == -2 and drop(H=0) == -2 and drop(W=0) == -2 and drop(B=-1) == -2 and drop(B=1 << 16) == -2
    assert drop(B=0) == 0 and drop(B=0, g=None) == 0

    def ln(x=fake, w=fake, go=fake, ws=fake, nbytes=big, B=1, c=3, H=5, W=5):
        return lib.patch_embed_hip_layernorm_cf_backward_f32(x, w, 1e-6, go, B, c, H, W, fake, fake, fake, ws, nbytes, None)
    assert ln(x=None) == -1 and ln(w=None) == -1 and ln(go=None) == -1
    assert ln(c=0) == -2 and ln(H=0) == -2 and ln(W=0) == -2 and ln(B=-1) == -2 and ln(B=4, c=1 << 15, H=1 << 7, W=1 << 7) == -2
    need = lib.patch_embed_hip_layernorm_cf_backward_workspace_bytes(1, 3, 5, 5)
    assert need > 0 and ln(nbytes=need - 1) == -6 and ln(ws=None) == -6


def test_workspace_bytes_follow_the_shape_and_the_header():
    from uninext_amd import _lib
    lib = _lib.load()
    head = lib.patch_embed_hip_convnext_dwconv_ln_backward_workspace_bytes
    tail = lib.patch_embed_hip_convnext_scale_residual_backward_workspace_bytes
    ln = lib.patch_embed_hip_layernorm_cf_backward_workspace_bytes
    for fn in (head, tail, ln):
        assert fn(2, 64, 9, 13) == fn(2, 64, 9, 13) > 0
        for bad in ((0, 64, 9, 13), (-1, 64, 9, 13), (2, 0, 9, 13), (2, 64, 0, 13), (2, 64, 9, -3), (1 << 16, 64, 9, 13), (64, 1024, 1024, 1024)):
            assert fn(*bad) == 0, bad
    assert head(2, 48, 9, 13) == 0 and head(2, 2048, 9, 13) == 0             # C the head does not take
    assert tail(2, 48, 9, 13) > 0 and ln(2, 2100, 3, 5) > 0
    # include/patch_embed_hip.h: at most 1.6 x the bytes of x + 4 MiB for any shape, 1.15 x + 4 MiB at the ConvNeXt-L stage shapes
    for c, H, W in C.LARGE_STAGES:
        xb = 2 * c * H * W * 4
        print("C %d %dx%d: x %.1f MiB, head %.1f MiB, tail %.2f MiB, ln %.2f MiB" % (c, H, W, xb / MIB, head(2, c, H, W) / MIB,
                                                                                 tail(2, c, H, W) / MIB, ln(2, c, H, W) / MIB))
        assert xb <= head(2, c, H, W) <= 1.15 * xb + 4 * MIB
        assert tail(2, c, H, W) == (2 * ((H * W + 63) // 64) * c * 4 + 255) // 256 * 256
        assert ln(2, c, H, W) == (2 * ((H * W + 63) // 64) * 2 * c * 4 + 255) // 256 * 256
    for shape in ((1, 32, 1, 1), (3, 32, 1, 4001), (1, 1536, 1, 9), (2, 32, 71, 116), (1, 64, 4000, 4000), (5, 96, 3, 20)):
        b, c, H, W = shape
        xb = b * c * H * W * 4
        assert xb <= head(*shape) <= 1.6 * xb + 4 * MIB, shape


def test_band_cases_sum_several_tiles_a_band():
    """The cases that tests/test_convnext_train_gpu.py has for pass two's loop over a band: more than one tile a band, a shorter
    last band, and the shape at the cap of 64 tiles -- read off the library's own workspace size, whose header formula has the bands in it."""
    from uninext_amd import _lib
    head = _lib.load().patch_embed_hip_convnext_dwconv_ln_backward_workspace_bytes
    a256 = lambda n: (n + 255) // 256 * 256
    for case in T.HEAD_CASES + [T.WIDE_HEAD_CASE]:
        assert T.head_bands(case[1], case[0], case[2], case[3])[1] == 1, case       # what the band cases are there for
    c, B, H, W = T.BAND_CAP_SHAPE
    assert T.head_bands(B, c, H, W)[1] == 64 < -(-T.head_bands(B, c, H, W)[0] // (512 // (c // 32)))
    for c, B, H, W in [case[:4] for case in T.BAND_HEAD_CASES] + [T.BAND_CAP_SHAPE]:
        tiles, per, bands = T.head_bands(B, c, H, W)
        print("C %d B %d %dx%d: %d tiles, %d a band, %d bands, %d in the last" % (c, B, H, W, tiles, per, bands, tiles - (bands - 1) * per))
        assert per > 1 and tiles > bands > 1 and tiles % per != 0
        # 4 * (B C H W + 2 C tiles_of_the_forward + 50 C bands), each part rounded up to 256: what is left for the forward's tiles
        # must be a whole number of them, and one that a th x tw tiling of the map gives
        rest = head(B, c, H, W) - a256(4 * B * c * H * W) - a256(4 * 49 * c * bands) - a256(4 * c * bands)
        assert rest > 0 and rest % (8 * c) == 0, (c, B, H, W, rest)
        assert rest // (8 * c) in {B * (-(-H // th)) * (-(-W // tw)) for th in range(1, 9) for tw in (4, 7, 8)}, (c, B, H, W, rest)


# ---- the modules on the CPU: the flag changes nothing there ---------------------------------------------------------------------
def _grads(module, x, seed):
    module.zero_grad()
    xa = x.clone().requires_grad_(True)
    torch.manual_seed(seed)
    out = module(xa)
    outs = list(out.values()) if isinstance(out, dict) else [out]
    g = torch.Generator().manual_seed(seed + 1)
    torch.autograd.backward(outs, [torch.randn(o.shape, generator=g) for o in outs])
    return outs, [xa.grad] + [p.grad for p in module.parameters()]


def _same(a, b):
    return all((s is None and t is None) or torch.equal(s, t) for s, t in zip(a, b)) and len(a) == len(b)


def test_own_training_on_cpu_tensors_is_the_flag_off_module():
    from uninext_amd.backbone import Block, ConvNeXt, LayerNorm
    assert Block.own_training is False and LayerNorm.own_training is False and ConvNeXt.own_training is False
    blk = Block(32, drop_path=0.5).train()
    C.randomise(blk, torch.Generator().manual_seed(1))
    x = torch.randn(4, 32, 6, 7, generator=torch.Generator().manual_seed(2))
    off = _grads(blk, x, 5)
    blk.own_training = True
    assert not blk._use_hip_training(x)
    on = _grads(blk, x, 5)
    assert _same(off[0], on[0]) and _same(off[1], on[1]) and "own_training" in vars(blk) and Block.own_training is False

    ln = LayerNorm(24, data_format="channels_first").train()
    C.randomise(ln, torch.Generator().manual_seed(3))
    x = torch.randn(2, 24, 5, 7, generator=torch.Generator().manual_seed(4))
    off = _grads(ln, x, 6)
    ln.own_training = True
    assert not ln._use_hip_training(x)
    on = _grads(ln, x, 6)
    assert _same(off[0], on[0]) and _same(off[1], on[1])

    net = ConvNeXt(depths=(1, 1, 1, 1), dims=(32, 32, 32, 64), drop_path_rate=0.5, layer_scale_init_value=1.0).train()
    C.randomise(net, torch.Generator().manual_seed(7))
    x = torch.randn(2, 3, 48, 64, generator=torch.Generator().manual_seed(8))
    off = _grads(net, x, 9)
    assert net.set_own_training(True) is net and net.own_training
    flagged = [m for m in net.modules() if getattr(m, "own_training", False) and m is not net]
    assert sum(isinstance(m, Block) for m in flagged) == 4 and sum(isinstance(m, LayerNorm) for m in flagged) == 7
    assert not any(b.norm.own_training for s in net.stages for b in s)         # channels_last: F.layer_norm
    on = _grads(net, x, 9)
    assert _same(off[0], on[0]) and _same(off[1], on[1])
    net.set_own_training(False)
    assert not net.own_training and not any(getattr(m, "own_training", False) for m in net.modules())


def test_launchers_refuse_cpu_tensors():
    from uninext_amd import ext
    x, dw_w, dw_b, ln_w, ln_b = C.head_case(1, 1, 32, 4, 4)
    with pytest.raises(RuntimeError, match="unsupported"):
        ext.convnext_dwconv_ln_backward(x, dw_w, dw_b, ln_w, 1e-6, torch.zeros(1, 4, 4, 32))
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.convnext_scale_residual_drop(torch.zeros(1, 4, 4, 32), None, torch.ones(1), x)
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.convnext_scale_residual_backward(x, torch.zeros(1, 4, 4, 32), ln_w, None)
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.layernorm_channels_first_backward(x, ln_w, 1e-6, x)


# ---- the fixtures pin the restatement's gradients to the reference's -----------------------------------------------------------------
def test_gradient_fixtures_load():
    names = sorted(f[:-len("_grad.npz")] for f in os.listdir(T.HERE) if f.endswith(".npz"))
    assert names == T.GRAD_NAMES
    for name in names:
        assert os.path.getsize(os.path.join(T.HERE, name + "_grad.npz")) < 1 << 20
    assert len([k for k in T.load_grads("block_c32") if k.startswith("grad.")]) == 10
    assert len([k for k in T.load_grads("block_c96_noscale") if k.startswith("grad.")]) == 9


@pytest.mark.parametrize("name", ["block_c32", "block_c96_noscale"])
def test_restatement_gradients_match_the_block_fixtures(name):
    fx, g = C.load(name), T.load_grads(name)
    got = T.restatement_block_grads(fx, g["grad_out"])
    assert set(got) == {k for k in g if k.startswith("grad.")}
    for k, v in got.items():
        assert v.shape == g[k].shape and C.max_err(v, g[k]) < 1e-12, (k, C.max_err(v, g[k]))


def test_restatement_gradients_match_the_network_fixture():
    fx, g = C.load("net_small"), T.load_grads("net_small")
    got = T.restatement_net_grads(fx, {k[len("grad_out."):]: v for k, v in g.items() if k.startswith("grad_out.")})
    assert set(got) == {k for k in g if k.startswith("grad.")}
    for k, v in got.items():
        assert v.shape == g[k].shape and C.max_err(v, g[k]) < 1e-12 * max(1.0, float(g[k].abs().max())), (k, C.max_err(v, g[k]))


def test_seeded_cases_clear_the_variance_floor():
    """Every pixel of every case of tests/test_convnext_train_gpu.py (which asserts it again): no case drops pixels."""
    for case in T.HEAD_CASES + [T.WIDE_HEAD_CASE] + T.BAND_HEAD_CASES:
        c, B, H, W, bias = case
        x, dw_w, dw_b, _, _ = C.head_case(T.head_seed(case), B, c, H, W, bias)
        assert float(R.channel_variance(R.dwconv7(x, dw_w, dw_b), 1).min()) > C.VARIANCE_FLOOR, case
    for c, B, H, W in T.CF_CASES:
        if c > 1:
            x = C.cf_case(200 + C.CF_CASES.index((c, B, H, W)), B, c, H, W)[0]
            assert float(R.channel_variance(x, 1).min()) > C.VARIANCE_FLOOR, (c, B, H, W)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_kernels_compile_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    got = kernel_resources.resources(os.path.join(ROOT, "uninext_amd", "csrc", "convnext_bwd.hip"))
    want = ["convnext::head_bwd_gu<4>", "convnext::head_bwd_gu<7>", "convnext::head_bwd_gu<8>", "convnext::head_bwd_xw<true, true>",
            "convnext::head_bwd_xw<true, false>", "convnext::head_bwd_xw<false, true>", "convnext::reduce_partials", "convnext::tail_bwd",
            "convnext::layernorm_cf_bwd<true>", "convnext::layernorm_cf_bwd<false>"]
    for kernel in want:
        assert kernel in got, (kernel, sorted(got))
        r = got[kernel]
        print("%-40s vgprs %d scratch %d B/lane occupancy %d" % (kernel, r["vgprs"], r["scratch"], r["occupancy"]))
        assert r["scratch"] == 0, (kernel, r)
