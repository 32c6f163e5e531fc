"""ConvNeXt backbone (uninext_amd/backbone.py: LayerNorm, Block, DropPath, ConvNeXt; include/patch_embed_hip.h: the three
convnext kernels): everything that needs no GPU."""
import ctypes
import os
import shutil
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnext_cases as C   # noqa: E402
import convnext_ref as R     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not C.reference_available(), reason="needs a checkout of the reference (UNINEXT_REFERENCE)")


def test_fixtures_load():
    assert C.NAMES == C.EXPECTED
    for name in C.NAMES:
        assert os.path.getsize(os.path.join(C.HERE, name + ".npz")) < 1 << 20
    fx = C.load("block_c32")
    assert fx["x"].shape == (2, 32, 9, 13) and fx["normed"].shape == (2, 9, 13, 32) and fx["out"].shape == fx["x"].shape
    assert "gamma.weight" in fx["state"] and "gamma.weight" not in C.load("block_c96_noscale")["state"]
    assert set(C.load("net_small")) >= {"x", "res2", "res3", "res4", "res5", "state"}


# ---- the fixtures against the float64 restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["block_c32", "block_c96_noscale"])
def test_restatement_matches_the_block_fixtures(name):
    fx = C.load(name)
    s = fx["state"]
    conv = R.dwconv7(fx["x"], s["dwconv.weight"], s["dwconv.bias"])
    assert float(R.channel_variance(conv, 1).min()) > C.VARIANCE_FLOOR
    normed = R.dwconv_ln(fx["x"], s["dwconv.weight"], s["dwconv.bias"], s["norm.weight.weight"][0], s["norm.bias.weight"][0], C.EPS)
    assert C.max_err(normed, fx["normed"]) < 1e-10
    assert C.max_err(R.block(fx["x"], s), fx["out"]) < 1e-10


def test_restatement_matches_the_layernorm_fixture():
    fx = C.load("ln_cf_c48")
    assert float(R.channel_variance(fx["x"], 1).min()) > C.VARIANCE_FLOOR
    out = R.layernorm_cf(fx["x"], fx["state"]["weight.weight"][0], fx["state"]["bias.weight"][0], C.EPS)
    assert C.max_err(out, fx["out"]) < 1e-10


def test_restatement_matches_the_network_fixture():
    fx = C.load("net_small")
    out = R.convnext(fx["x"], fx["state"], C.NET_DEPTHS)
    assert sorted(out) == ["res2", "res3", "res4", "res5"]
    for k, v in out.items():
        assert v.shape == fx[k].shape and C.max_err(v, fx[k]) < 1e-9, k


# ---- the modules on the CPU ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["block_c32", "block_c96_noscale"])
def test_block_float64_matches_the_fixture(name):
    fx = C.load(name)
    blk = C.our_block(fx, torch.float64)
    with torch.no_grad():
        out = blk(fx["x"])
        normed = blk.norm(blk.dwconv(fx["x"]).permute(0, 2, 3, 1))
    assert C.max_err(out, fx["out"]) < 1e-10 and C.max_err(normed, fx["normed"]) < 1e-10
    with torch.no_grad():
        out32 = C.our_block(fx, torch.float32)(fx["x"].float())
    assert C.max_err(out32, fx["out"]) < C.tol(fx["out"])


def test_network_matches_the_fixture():
    fx = C.load("net_small")
    with torch.no_grad():
        out = C.our_net(fx, torch.float64)(fx["x"])
        out32 = C.our_net(fx, torch.float32)(fx["x"].float())
    assert list(out) == ["res2", "res3", "res4", "res5"]
    for k in out:
        assert C.max_err(out[k], fx[k]) < 1e-9, k
        assert C.max_err(out32[k], fx[k]) < C.tol(fx[k]), k


def test_state_dict_keys():
    from uninext_amd.backbone import Block, ConvNeXt, LayerNorm
    assert set(LayerNorm(8).state_dict()) == {"weight.weight", "bias.weight"}
    want = {"dwconv.weight", "dwconv.bias", "norm.weight.weight", "norm.bias.weight", "pwconv1.weight", "pwconv1.bias",
            "pwconv2.weight", "pwconv2.bias", "gamma.weight"}
    assert set(Block(32).state_dict()) == want
    blk = Block(32, layer_scale_init_value=0)
    assert blk.gamma is None and set(blk.state_dict()) == want - {"gamma.weight"}
    assert torch.equal(Block(32, layer_scale_init_value=0.5).gamma.weight, torch.full((1, 32), 0.5))
    net = ConvNeXt(depths=(1, 1, 2, 1), dims=(32, 32, 64, 64), drop_path_rate=0.3)
    keys = set(net.state_dict())
    assert {"downsample_layers.0.0.weight", "downsample_layers.0.1.weight.weight", "downsample_layers.3.0.bias.weight",
            "downsample_layers.3.1.bias", "stages.2.1.gamma.weight", "norm1.weight.weight", "norm3.bias.weight"} <= keys
    assert not any(k.startswith("norm0") for k in keys)
    lin = net.stages[0][0].pwconv1
    assert float(lin.bias.detach().abs().max()) == 0 and 0.015 < float(lin.weight.detach().std()) < 0.025    # trunc_normal_(std=.02)
    rates = [getattr(b.drop_path, "drop_prob", 0.0) for s in net.stages for b in s]
    assert rates[0] == 0.0 and abs(rates[-1] - 0.3) < 1e-6 and rates == sorted(rates)
    with pytest.raises(NotImplementedError):
        LayerNorm(8, data_format="channels_middle")


@needs_reference
def test_modules_agree_with_the_reference_classes():
    """Both directions of load_state_dict(strict=True), and fp32 outputs within 1e-6 of the reference's classes."""
    from uninext_amd.backbone import Block, ConvNeXt, LayerNorm
    ref = C.load_reference()
    gen = torch.Generator().manual_seed(5)
    for dim, scale in ((32, 1.0), (48, 0.0)):
        theirs, ours = ref.Block(dim, layer_scale_init_value=scale).eval(), Block(dim, layer_scale_init_value=scale).eval()
        C.randomise(theirs, gen)
        ours.load_state_dict(theirs.state_dict(), strict=True)
        theirs.load_state_dict(ours.state_dict(), strict=True)
        x = torch.randn(2, dim, 9, 13, generator=gen)
        with torch.no_grad():
            assert C.max_err(ours(x), theirs(x)) <= 1e-6
    for fmt, shape in (("channels_first", (2, 24, 5, 7)), ("channels_last", (2, 5, 7, 24))):
        theirs, ours = ref.LayerNorm(24, eps=1e-6, data_format=fmt).eval(), LayerNorm(24, eps=1e-6, data_format=fmt).eval()
        C.randomise(theirs, gen)
        ours.load_state_dict(theirs.state_dict(), strict=True)
        theirs.load_state_dict(ours.state_dict(), strict=True)
        x = torch.randn(shape, generator=gen)
        with torch.no_grad():
            assert C.max_err(ours(x), theirs(x)) <= 1e-6
    kw = dict(in_chans=3, depths=[1, 2, 1, 1], dims=[32, 32, 64, 64], drop_path_rate=0.0, layer_scale_init_value=1.0, out_indices=[0, 2, 3])
    theirs, ours = ref.ConvNeXt(**kw).eval(), ConvNeXt(**kw).eval()
    C.randomise(theirs, gen)
    ours.load_state_dict(theirs.state_dict(), strict=True)
    theirs.load_state_dict(ours.state_dict(), strict=True)
    x = torch.randn(1, 3, 64, 96, generator=gen)
    with torch.no_grad():
        a, b = ours(x), theirs(x)
    assert list(a) == list(b) == ["res2", "res3", "res4"]
    for k in a:
        assert C.max_err(a[k], b[k]) <= 1e-6, k


def test_drop_path():
    from uninext_amd.backbone import Block, DropPath
    d = DropPath(0.5)
    x = torch.ones(64, 3, 2, 2)
    assert d.eval()(x) is x
    torch.manual_seed(0)
    y = d.train()(x)
    per_sample = y.flatten(1)
    assert bool(((per_sample == 0).all(1) | (per_sample == 2).all(1)).all()) and 0 < int((per_sample[:, 0] == 0).sum()) < 64
    blk = Block(32, drop_path=0.25)
    assert isinstance(blk.drop_path, DropPath) and isinstance(Block(32).drop_path, torch.nn.Identity)
    blk.train()
    blk(torch.randn(4, 32, 5, 5)).sum().backward()           # the PyTorch route, with drop_path in it
    assert blk.dwconv.weight.grad is not None and blk.gamma.weight.grad is not None


def test_routing_predicates_and_supported_table():
    """What must go to PyTorch does (the GPU side is exercised in tests/test_convnext_gpu.py)."""
    from uninext_amd import ext
    from uninext_amd.backbone import Block, LayerNorm
    blk = Block(32).eval()
    ln = LayerNorm(32, data_format="channels_first").eval()
    x = torch.zeros(1, 32, 5, 5)
    with torch.no_grad():
        assert not blk._use_hip(x) and not ln._use_hip(x)                      # CPU tensors
    assert not ext.convnext_dwconv_ln_supported(x, blk.dwconv.weight)

    class OnGpu:   # a tensor stand-in that says it is on the GPU
        def __init__(self, *shape, dtype=torch.float32, contiguous=True):
            self.is_cuda, self.dtype, self.shape, self.requires_grad, self.c = True, dtype, torch.Size(shape), False, contiguous
            self.device = torch.device("cpu")                                  # where the parameters of this test live
        def is_contiguous(self):
            return self.c
        def dim(self):
            return len(self.shape)
    w = lambda c, dtype=torch.float32: OnGpu(c, 1, 7, 7, dtype=dtype)
    ok = ext.convnext_dwconv_ln_supported
    for c in (32, 64, 96, 128, 192, 256, 384, 512, 768, 1024, 1536):           # every dim of tiny / base / large
        assert ok(OnGpu(2, c, 9, 13), w(c)), c
    assert ok(OnGpu(1, 32, 1, 1), w(32)) and ok(OnGpu(0, 32, 3, 20), w(32))
    for c in (1, 16, 48, 100, 1568, 2048):
        assert not ok(OnGpu(2, c, 9, 13), w(c)), c
    assert not ok(OnGpu(2, 32, 9, 13, dtype=torch.float64), w(32)) and not ok(OnGpu(2, 32, 9, 13), w(32, torch.float16))
    assert not ok(OnGpu(2, 32, 9, 13, contiguous=False), w(32)) and not ok(OnGpu(32, 9, 13), w(32))
    assert not ok(OnGpu(2, 32, 9, 13), OnGpu(32, 1, 3, 3)) and not ok(OnGpu(2, 32, 9, 13), w(64))

    g = OnGpu(1, 32, 5, 5)
    old = Block.fused, LayerNorm.fused
    assert old == (True, True)                                                 # on by default: profiles/r10_convnext.txt
    try:
        with torch.no_grad():
            assert blk._use_hip(g) and ln._use_hip(g)
            assert not blk._use_hip(OnGpu(1, 32, 5, 5, dtype=torch.float64)) and not blk._use_hip(OnGpu(1, 32, 5, 5, contiguous=False))
            assert not ln._use_hip(OnGpu(1, 16, 5, 5)) and not ln._use_hip(OnGpu(1, 32, 5, 5, dtype=torch.float16))
            assert not Block(48).eval()._use_hip(OnGpu(1, 48, 5, 5))             # C = 48: no kernel
            assert not Block(32).double().eval()._use_hip(g)                    # parameters of another dtype
            noisy = Block(32, drop_path=0.5)
            assert not noisy.train()._use_hip(g) and noisy.eval()._use_hip(g)   # stochastic depth only ever on the PyTorch route
            Block.fused = LayerNorm.fused = False
            assert not blk._use_hip(g) and not ln._use_hip(g)
            Block.fused = LayerNorm.fused = True
        assert not blk._use_hip(g) and not ln._use_hip(g)                       # autograd records (parameters)
    finally:
        Block.fused, LayerNorm.fused = old


def test_seeded_cases_clear_the_variance_floor():
    """The seeded cases of tests/test_convnext_gpu.py (which asserts it again on what it feeds the kernels).  One channel has no
    variance at all: there the answer is the bias exactly, and the test says so."""
    for seed, (c, B, H, W, bias) in enumerate(C.HEAD_CASES):
        x, dw_w, dw_b, _, _ = C.head_case(100 + seed, B, c, H, W, bias)
        assert float(R.channel_variance(R.dwconv7(x, dw_w, dw_b), 1).min()) > C.VARIANCE_FLOOR, (c, B, H, W)
    for seed, (c, B, H, W, bias, _) in enumerate(C.WIDE_HEAD_CASES):
        x, dw_w, dw_b, _, _ = C.head_case(300 + seed, B, c, H, W, bias)
        assert float(R.channel_variance(R.dwconv7(x, dw_w, dw_b), 1).min()) > C.VARIANCE_FLOOR, (c, B, H, W)
    for seed, (c, B, H, W) in enumerate(C.CF_CASES):
        if c > 1:
            assert float(R.channel_variance(C.cf_case(200 + seed, B, c, H, W)[0], 1).min()) > C.VARIANCE_FLOOR, (c, B, H, W)


# ---- the C ABI without a device --------------------------------------------------------------------------------------------------
def test_error_codes_without_a_device():
    from uninext_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(1 << 20)      # never dereferenced: every check runs before the device is touched
    head = lambda x=fake, w=fake, b=fake, lw=fake, lb=fake, out=fake, B=1, c=32, H=5, W=5: lib.patch_embed_hip_convnext_dwconv_ln_f32(
        x, w, b, lw, lb, 1e-6, B, c, H, W, out, None)
    assert head(x=None) == -1 and "null" in _lib.last_error()
    assert head(w=None) == -1 and head(lw=None) == -1 and head(lb=None) == -1 and head(out=None) == -1
    assert head(H=0) == -2 and "dimensions" in _lib.last_error()
    assert head(W=-1) == -2 and head(c=0) == -2 and head(B=-1) == -2
    for c in (16, 48, 1568, 2048):
        assert head(c=c) == -5, c
    assert "multiple of 32" in _lib.last_error()
    assert head(out=ctypes.c_void_p((1 << 20) + 4)) == -5 and "aligned" in _lib.last_error()
    assert head(B=1 << 20, c=1536, H=64, W=64) == -2 and "large" in _lib.last_error()
    assert head(B=1, c=32, H=1, W=(1 << 26) - 4) == -2 and "large" in _lib.last_error()     # a map side past 65535
    assert head(B=0) == 0 and head(B=0, b=None) == 0                         # an empty batch enqueues nothing

    tail = lambda y=fake, g=fake, inp=fake, out=fake, B=1, c=3, H=5, W=5: lib.patch_embed_hip_convnext_scale_residual_f32(
        y, g, inp, B, c, H, W, out, None)
    assert tail(y=None) == -1 and tail(inp=None) == -1 and tail(out=None) == -1
    assert tail(c=0) == -2 and tail(H=0) == -2 and tail(W=0) == -2 and tail(B=-1) == -2
    assert tail(B=1 << 16) == -2
    assert tail(B=0) == 0 and tail(B=0, g=None) == 0

    ln = lambda x=fake, w=fake, b=fake, out=fake, B=1, c=3, H=5, W=5: lib.patch_embed_hip_layernorm_cf_f32(x, w, b, 1e-6, B, c, H, W, out, None)
    assert ln(x=None) == -1 and ln(w=None) == -1 and ln(b=None) == -1 and ln(out=None) == -1
    assert ln(c=0) == -2 and ln(H=0) == -2 and ln(W=0) == -2 and ln(B=-1) == -2
    assert ln(B=4, c=1 << 15, H=1 << 7, W=1 << 7) == -2
    assert ln(B=0) == 0
    assert isinstance(_lib.last_kernel("convnext"), str)                     # refused calls leave the record alone


def test_launchers_refuse_cpu_tensors():
    from uninext_amd import ext
    x, dw_w, dw_b, ln_w, ln_b = C.head_case(1, 1, 32, 4, 4)
    with pytest.raises(RuntimeError, match="unsupported"):
        ext.convnext_dwconv_ln(x, dw_w, dw_b, ln_w, ln_b, 1e-6)
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.convnext_scale_residual(torch.zeros(1, 4, 4, 32), None, x)
    with pytest.raises(RuntimeError, match="CUDA"):
        ext.layernorm_channels_first(x, ln_w, ln_b, 1e-6)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_kernels_compile_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    got = kernel_resources.resources(os.path.join(ROOT, "uninext_amd", "csrc", "convnext.hip"))
    want = ["convnext::dwconv_ln<4>", "convnext::dwconv_ln<7>", "convnext::dwconv_ln<8>", "convnext::scale_residual",
            "convnext::layernorm_cf<true>", "convnext::layernorm_cf<false>"]
    for kernel in want:
        assert kernel in got, (kernel, sorted(got))
        r = got[kernel]
        print("%-32s vgprs %d scratch %d B/lane lds %d occupancy %d" % (kernel, r["vgprs"], r["scratch"], r.get("lds", -1), r["occupancy"]))
        assert r["scratch"] == 0, (kernel, r)
        assert r.get("lds", 0) == 0, (kernel, r)         # no static LDS in front of the dynamic region: its base stays 16-byte aligned
