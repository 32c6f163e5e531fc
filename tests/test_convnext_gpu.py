"""MI355X tests of the ConvNeXt kernels (include/patch_embed_hip.h: patch_embed_hip_convnext_dwconv_ln_f32, patch_embed_hip_convnext_scale_residual_f32,
patch_embed_hip_layernorm_cf_f32) and of the modules on top of them (uninext_amd/backbone.py).  Reference: the float64 restatement of
tests/convnext_ref.py and the reference-minted fixtures of tests/golden/convnext/.  Tolerance: the project's 1e-4 * max(1, max|ref|)
(tests/test_conv3x3_gpu.py); every compared LayerNorm runs on pixels whose channel variance is above 1e-2 (asserted)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnext_cases as C   # noqa: E402
import convnext_ref as R     # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def fused_routes():
    """This file is about the kernel routes of the modules (Block.fused, LayerNorm.fused), whatever the defaults are."""
    from uninext_amd.backbone import Block, LayerNorm
    old = Block.fused, LayerNorm.fused
    Block.fused = LayerNorm.fused = True
    try:
        yield
    finally:
        Block.fused, LayerNorm.fused = old


def to(dev, *ts):
    return [None if t is None else t.to(device=dev, dtype=torch.float32).contiguous() for t in ts]


def last():
    from uninext_amd import _lib
    return _lib.last_kernel("convnext")


def check(got, ref, what):
    err, bound = C.max_err(got, ref), C.tol(ref)
    print("%s: max abs err %.3g, bound %.3g (scale %.3g)" % (what, err, bound, float(ref.abs().max())))
    assert got.shape == ref.shape and err < bound, (what, err, bound)


# ---- the block's head -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["block_c32", "block_c96_noscale"])
def test_dwconv_ln_fixture(name, dev):
    from uninext_amd import ext
    fx = C.load(name)
    s = fx["state"]
    out = ext.convnext_dwconv_ln(*to(dev, fx["x"], s["dwconv.weight"], s["dwconv.bias"], s["norm.weight.weight"][0], s["norm.bias.weight"][0]), C.EPS)
    assert last().startswith("convnext_dwconv_ln<")
    check(out, fx["normed"], name)


@pytest.mark.parametrize("case", range(len(C.HEAD_CASES)))
def test_dwconv_ln_vs_float64(case, dev):
    from uninext_amd import ext
    c, B, H, W, bias = C.HEAD_CASES[case]
    x, dw_w, dw_b, ln_w, ln_b = C.head_case(100 + case, B, c, H, W, bias)
    assert float(R.channel_variance(R.dwconv7(x, dw_w, dw_b), 1).min()) > C.VARIANCE_FLOOR
    ref = R.dwconv_ln(x, dw_w, dw_b, ln_w, ln_b, C.EPS)
    args = to(dev, x, dw_w, dw_b, ln_w, ln_b)
    assert ext.convnext_dwconv_ln_supported(args[0], args[1])
    out = ext.convnext_dwconv_ln(*args, C.EPS)
    assert out.shape == (B, H, W, c) and out.is_contiguous()
    check(out, ref, "C %d B %d %dx%d bias %s [%s]" % (c, B, H, W, bias, last()))


@pytest.mark.parametrize("case", range(len(C.WIDE_HEAD_CASES)))
def test_dwconv_ln_wide_tiles_vs_float64(case, dev):
    """The <7> and <8> instantiations, named: a change of the tile rule cannot silently take them out of the tests."""
    from uninext_amd import ext
    c, B, H, W, bias, kernel = C.WIDE_HEAD_CASES[case]
    x, dw_w, dw_b, ln_w, ln_b = C.head_case(300 + case, B, c, H, W, bias)
    assert float(R.channel_variance(R.dwconv7(x, dw_w, dw_b), 1).min()) > C.VARIANCE_FLOOR
    out = ext.convnext_dwconv_ln(*to(dev, x, dw_w, dw_b, ln_w, ln_b), C.EPS)
    assert last() == kernel
    check(out, R.dwconv_ln(x, dw_w, dw_b, ln_w, ln_b, C.EPS), "C %d B %d %dx%d [%s]" % (c, B, H, W, kernel))


def test_small_cases_take_the_narrow_tile(dev):
    from uninext_amd import ext
    ext.convnext_dwconv_ln(*to(dev, *C.head_case(100, 3, 96, 11, 23)), C.EPS)
    assert last() == "convnext_dwconv_ln<4>"


def test_dwconv_ln_constant_pixels_are_exact(dev):
    """Zero taps and a bias of 0.5 in all 64 channels: every sum is exact in fp32 in any order, the deviations are zero and the
    result is ln_bias broadcast, bitwise."""
    from uninext_amd import ext
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 64, 10, 15, generator=g)
    ln_w, ln_b = 1.0 + torch.randn(64, generator=g), torch.randn(64, generator=g)
    out = ext.convnext_dwconv_ln(*to(dev, x, torch.zeros(64, 1, 7, 7), torch.full((64,), 0.5), ln_w, ln_b), C.EPS)
    want = ln_b.to(dev).expand(2, 10, 15, 64).contiguous()
    assert torch.equal(out, want) and out.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()


def test_dwconv_ln_refusals(dev):
    from uninext_amd import ext
    x, dw_w, dw_b, ln_w, ln_b = to(dev, *C.head_case(1, 1, 48, 5, 5))
    assert not ext.convnext_dwconv_ln_supported(x, dw_w)
    with pytest.raises(RuntimeError, match="unsupported"):
        ext.convnext_dwconv_ln(x, dw_w, dw_b, ln_w, ln_b, C.EPS)
    x, dw_w, dw_b, ln_w, ln_b = to(dev, *C.head_case(1, 1, 32, 5, 5))
    with pytest.raises(RuntimeError, match="ln_weight"):
        ext.convnext_dwconv_ln(x, dw_w, dw_b, ln_w[:16].contiguous(), ln_b, C.EPS)
    assert ext.convnext_dwconv_ln(x[:0].contiguous(), dw_w, dw_b, ln_w, ln_b, C.EPS).shape == (0, 5, 5, 32)


# ---- the block's tail -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,B,H,W", C.TAIL_CASES)
@pytest.mark.parametrize("scaled", [True, False])
def test_scale_residual_is_bitwise_pytorch(c, B, H, W, scaled, dev):
    from uninext_amd import ext
    g = torch.Generator().manual_seed(c * 7 + H)
    y, inp, gamma = to(dev, torch.randn(B, H, W, c, generator=g), torch.randn(B, c, H, W, generator=g), torch.randn(c, generator=g) if scaled else None)
    out = ext.convnext_scale_residual(y, gamma, inp)
    assert last() == "convnext_scale_residual"
    want = inp + ((gamma * y) if scaled else y).permute(0, 3, 1, 2)
    assert out.shape == inp.shape and out.is_contiguous() and torch.equal(out, want)
    check(out, R.scale_residual(y, gamma, inp), "tail C %d" % c)


# ---- channels-first LayerNorm -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(C.CF_CASES)))
def test_layernorm_cf_vs_float64(case, dev):
    from uninext_amd import ext
    c, B, H, W = C.CF_CASES[case]
    x, w, b = C.cf_case(200 + case, B, c, H, W)
    out = ext.layernorm_channels_first(*to(dev, x, w, b), C.EPS)
    assert last() == ("layernorm_cf<cached>" if c <= 2048 else "layernorm_cf<streamed>")
    if c == 1:      # no variance to speak of: x - u is zero and the answer is the bias, exactly
        assert torch.equal(out.cpu(), b.view(1, 1, 1, 1).expand(B, 1, H, W))
        return
    assert float(R.channel_variance(x, 1).min()) > C.VARIANCE_FLOOR
    check(out, R.layernorm_cf(x, w, b, C.EPS), "layernorm_cf C %d [%s]" % (c, last()))


def test_layernorm_cf_fixture_and_module(dev):
    from uninext_amd.backbone import LayerNorm
    fx = C.load("ln_cf_c48")
    ln = LayerNorm(48, eps=C.EPS, data_format="channels_first")
    ln.load_state_dict(fx["state"], strict=True)
    ln = ln.to(dev).eval()
    x = fx["x"].float().to(dev)
    with torch.no_grad():
        out = ln(x)
        assert last() == "layernorm_cf<cached>"
        check(out, fx["out"], "ln_cf_c48 (kernel)")
        LayerNorm.fused = False
        try:
            check(ln(x), fx["out"], "ln_cf_c48 (PyTorch)")
        finally:
            LayerNorm.fused = True
        last_layout = LayerNorm(48).to(dev).eval()
        y = torch.randn(2, 5, 7, 48, device=dev)
        assert torch.equal(last_layout(y), torch.nn.functional.layer_norm(y, (48,), last_layout.weight.weight[0], last_layout.bias.weight[0], 1e-6))


# ---- the modules -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["block_c32", "block_c96_noscale"])
def test_block_fixture_on_the_fused_route(name, dev):
    fx = C.load(name)
    blk = C.our_block(fx, torch.float32, dev)
    with torch.no_grad():
        out = blk(fx["x"].float().to(dev))
    assert last() == "convnext_scale_residual"
    check(out, fx["out"], name)


def test_small_network_fixture(dev):
    from uninext_amd import ext
    fx = C.load("net_small")
    net = C.our_net(fx, torch.float32, dev)
    seen = []
    real = ext.convnext_dwconv_ln, ext.layernorm_channels_first
    ext.convnext_dwconv_ln = lambda *a: (seen.append("head"), real[0](*a))[1]
    ext.layernorm_channels_first = lambda *a: (seen.append("ln"), real[1](*a))[1]
    try:
        with torch.no_grad():
            out = net(fx["x"].float().to(dev))
    finally:
        ext.convnext_dwconv_ln, ext.layernorm_channels_first = real
    assert seen.count("head") == sum(C.NET_DEPTHS) and seen.count("ln") == 7
    assert list(out) == ["res2", "res3", "res4", "res5"]
    for k in out:
        check(out[k], fx[k], "net_small " + k)


@pytest.mark.parametrize("dim,H,W", C.LARGE_STAGES)
def test_block_at_convnext_large_stage_shapes(dim, H, W, dev):
    """One Block.forward at bs 2 on the fused route against the PyTorch route of the same module on the GPU."""
    from uninext_amd.backbone import Block
    blk = Block(dim, layer_scale_init_value=1.0).eval()
    C.randomise(blk, torch.Generator().manual_seed(dim))
    blk = blk.to(dev)
    x = torch.randn(2, dim, H, W, generator=torch.Generator().manual_seed(dim + 1)).to(dev)
    from uninext_amd import ext
    calls = []
    real = ext.convnext_dwconv_ln, ext.convnext_scale_residual
    ext.convnext_dwconv_ln = lambda *a: (calls.append("head"), real[0](*a))[1]
    ext.convnext_scale_residual = lambda *a: (calls.append("tail"), real[1](*a))[1]
    try:
        with torch.no_grad():
            out = blk(x)
            assert calls == ["head", "tail"] and last() == "convnext_scale_residual"
            Block.fused = False
            ref = blk(x)
            assert calls == ["head", "tail"]
    finally:
        Block.fused = True
        ext.convnext_dwconv_ln, ext.convnext_scale_residual = real
    torch.cuda.synchronize()
    scale = float(ref.abs().max())
    err = float((out - ref).abs().max())
    print("C %d %dx%d: max abs diff %.3g, scale %.3g" % (dim, H, W, err, scale))
    assert err < 1e-4 * max(1.0, scale)


def test_bitwise_repeatable_across_runs_and_streams(dev):
    from uninext_amd import ext
    head = to(dev, *C.head_case(3, 2, 192, 23, 31))
    g = torch.Generator().manual_seed(4)
    y, inp, gamma = to(dev, torch.randn(2, 23, 31, 192, generator=g), torch.randn(2, 192, 23, 31, generator=g), torch.randn(192, generator=g))
    cf = to(dev, *C.cf_case(5, 2, 192, 23, 31))
    runs = {"head": lambda: ext.convnext_dwconv_ln(*head, C.EPS), "tail": lambda: ext.convnext_scale_residual(y, gamma, inp),
            "ln": lambda: ext.layernorm_channels_first(*cf, C.EPS)}
    for name, run in runs.items():
        a, b = run(), run()
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            c = run()
        side.synchronize()
        assert torch.equal(a, b) and torch.equal(a, c), name
        assert a.cpu().numpy().tobytes() == c.cpu().numpy().tobytes(), name


def test_autograd_takes_the_pytorch_route(dev):
    """Under autograd the block runs PyTorch's operations (no kernel of this file is enqueued); its output and all ten gradients
    are bitwise those of the composition written out here."""
    import torch.nn.functional as F
    from uninext_amd import ext
    fx = C.load("block_c32")
    blk = C.our_block(fx, torch.float32, dev)
    twin = C.our_block(fx, torch.float32, dev)
    x = fx["x"].float().to(dev)
    ext.layernorm_channels_first(*to(dev, *C.cf_case(1, 1, 3, 4, 4)), C.EPS)
    before = last()
    xa = x.clone().requires_grad_(True)
    out = blk(xa)
    assert last() == before == "layernorm_cf<cached>"
    grad = torch.randn(out.shape, generator=torch.Generator().manual_seed(8)).to(dev)
    out.backward(grad)

    xb = x.clone().requires_grad_(True)
    t = F.conv2d(xb, twin.dwconv.weight, twin.dwconv.bias, padding=3, groups=32).permute(0, 2, 3, 1)
    t = F.layer_norm(t, (32,), twin.norm.weight.weight[0], twin.norm.bias.weight[0], 1e-6)
    t = F.linear(F.gelu(F.linear(t, twin.pwconv1.weight, twin.pwconv1.bias)), twin.pwconv2.weight, twin.pwconv2.bias)
    ref = xb + (twin.gamma.weight[0] * t).permute(0, 3, 1, 2)
    ref.backward(grad)
    assert torch.equal(out, ref)
    names = ["x"] + [n for n, _ in blk.named_parameters()]
    pairs = [(xa.grad, xb.grad)] + [(p.grad, q.grad) for p, q in zip(blk.parameters(), twin.parameters())]
    assert len(pairs) == 10
    for name, (got, want) in zip(names, pairs):
        assert got is not None and want is not None
        assert torch.equal(got, want), name
