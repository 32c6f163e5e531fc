"""MI355X tests of the patch-embedding training route: patch_embed_hip_backward_f32 (include/patch_embed_hip.h) through
PatchEmbedFunction / PatchEmbed.own_exact_training / patch_conv2d(..., own_training=True) (uninext_amd/backbone.py).

Checker: PyTorch's own autograd of the convolution in float64.  The bound per gradient tensor is
max(1e-4 * max|ref|, 2 * the error of the fp32 PyTorch route) -- the own route is no further from float64 than twice the library's."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = os.path.join(ROOT, "tests", "golden", "patch_bwd")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _err(a, ref):
    return float((a.detach().double() - ref.detach().double()).abs().max()) if ref.numel() else 0.0


def _bound(ref, err_torch32):
    return max(1e-4 * (float(ref.abs().max()) if ref.numel() else 0.0), 2.0 * err_torch32)


def _run(x, w, b, grad_out, channels_last, own, dtype=torch.float32, need=(True, True, True)):
    """(out, grad_x, grad_weight, grad_bias) of the patch convolution in `dtype`; own: through PatchEmbedFunction.  `need` says
    which of x, weight, bias require grad (None where not)."""
    from uninext_amd.backbone import PatchEmbedFunction
    xx = x.detach().to(dtype).requires_grad_(need[0])
    ww = w.detach().to(dtype).requires_grad_(need[1])
    bb = b.detach().to(dtype).requires_grad_(need[2]) if b is not None else None
    if own:
        out = PatchEmbedFunction.apply(xx, ww, bb, channels_last)
        assert type(out.grad_fn).__name__ == "PatchEmbedFunctionBackward"
    else:
        out = F.conv2d(xx, ww, bb, stride=w.shape[2])
        out = out.permute(0, 2, 3, 1) if channels_last else out
    out.backward(grad_out.to(dtype))
    return out, xx.grad, ww.grad, (bb.grad if bb is not None else None)


def _check(x, w, b, grad_out, channels_last, need=(True, True, True)):
    want = _run(x, w, b, grad_out, channels_last, False, torch.float64, need)
    torch32 = _run(x, w, b, grad_out, channels_last, False, torch.float32, need)
    got = _run(x, w, b, grad_out, channels_last, True, torch.float32, need)
    for name, g, t, r in zip(("out", "grad_x", "grad_weight", "grad_bias"), got, torch32, want):
        if r is None:
            assert g is None, name
            continue
        e, bound = _err(g, r), _bound(r, _err(t, r))
        print("%-12s err %.3e  torch fp32 %.3e  bound %.3e" % (name, e, _err(t, r), bound))
        assert g.dtype == torch.float32 and g.shape == r.shape, name
        assert e <= bound, (name, e, bound)
    return got


def _inputs(B, C, H, W, E, k, channels_last, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=gen).to(dev)
    w = (torch.randn(E, C, k, k, generator=gen) / (C * k * k) ** 0.5).to(dev)
    b = (0.1 * torch.randn(E, generator=gen)).to(dev)
    Hp, Wp = H // k, W // k
    grad_out = torch.randn((B, Hp, Wp, E) if channels_last else (B, E, Hp, Wp), generator=gen).to(dev)
    return x, w, b, grad_out


@pytest.mark.parametrize("name", ["vit_remainder", "vit_tiles", "convnext_stem", "convnext_down"])
def test_fixture_parity(name, dev):
    with np.load(os.path.join(FIXTURES, name + ".npz")) as z:
        g = {k: z[k] for k in z.files}
    t = lambda key: torch.from_numpy(g[key]).to(dev)
    cl = bool(int(g["channels_last"]))
    torch32 = _run(t("x"), t("weight"), t("bias"), t("grad_out"), cl, False)
    got = _run(t("x"), t("weight"), t("bias"), t("grad_out"), cl, True)
    for i, key in enumerate(("out", "gx", "gw", "gb")):
        ref = t(key).double()
        e, bound = _err(got[i], ref), _bound(ref, _err(torch32[i], ref))
        print("%-4s err %.3e bound %.3e" % (key, e, bound))
        assert e <= bound, (key, e, bound)


# k, C, E, B, H, W: every patch size; M and E off the tile multiples; remainder rows / columns; both tile configurations
SEEDED = [
    (2, 12, 40, 2, 27, 35),
    (2, 64, 136, 1, 50, 61),
    (4, 3, 24, 2, 22, 35),
    (4, 8, 200, 1, 45, 70),
    (8, 3, 72, 2, 41, 53),
    (8, 4, 130, 1, 40, 72),
    (16, 3, 136, 2, 37, 50),
    (16, 3, 1280, 1, 64, 96),
]


@pytest.mark.parametrize("channels_last", [True, False])
@pytest.mark.parametrize("k,C,E,B,H,W", SEEDED)
def test_seeded_parity(k, C, E, B, H, W, channels_last, dev):
    x, w, b, grad_out = _inputs(B, C, H, W, E, k, channels_last, dev, seed=k * 1000 + E + H)
    _check(x, w, b, grad_out, channels_last)


@pytest.mark.parametrize("channels_last", [True, False])
def test_empty_batch_and_no_patch(channels_last, dev):
    for B, H, W in ((0, 37, 50), (2, 8, 50)):          # no image; images smaller than one patch
        x, w, b, grad_out = _inputs(B, 3, H, W, 40, 16, channels_last, dev, seed=3)
        got = _run(x, w, b, grad_out, channels_last, True)
        assert got[1].shape == x.shape and got[2].shape == w.shape and got[3].shape == b.shape
        assert float(got[2].abs().max()) == 0.0 and float(got[3].abs().max()) == 0.0
        if x.numel():
            assert float(got[1].abs().max()) == 0.0


@pytest.mark.parametrize("channels_last", [True, False])
@pytest.mark.parametrize("k,C,H,W", [(16, 3, 37, 50), (2, 12, 13, 19), (4, 8, 45, 70), (8, 4, 41, 40)])
def test_remainder_pixels_are_exact_zeros(k, C, H, W, channels_last, dev):
    from uninext_amd import ext
    x, w, b, grad_out = _inputs(2, C, H, W, 48, k, channels_last, dev, seed=5)
    junk = torch.full_like(x, float("nan"))           # leave NaNs in the block the caching allocator hands out next
    del junk
    gx, _, _ = ext.patch_embed_backward(x, w, grad_out, channels_last, need_input=True, need_weight=False, need_bias=False)
    Hc, Wc = (H // k) * k, (W // k) * k
    assert torch.isfinite(gx).all()
    assert (gx[:, :, Hc:, :] == 0).all() and (gx[:, :, :, Wc:] == 0).all()
    assert float(gx[:, :, :Hc, :Wc].abs().max()) > 0


@pytest.mark.parametrize("channels_last", [True, False])
def test_needs_input_grad_combinations(channels_last, dev):
    x, w, b, grad_out = _inputs(2, 12, 27, 35, 40, 2, channels_last, dev, seed=9)
    full = _check(x, w, b, grad_out, channels_last)
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, False, True), (False, True, True)):
        got = _check(x, w, b, grad_out, channels_last, need)
        for i in range(3):                                # a part computed alone is the same bits as with the others
            if need[i] and not (i == 2 and not need[1]):  # grad-bias alone runs the column-sum kernel
                assert torch.equal(got[i + 1], full[i + 1]), (need, i)
    _check(x, w, None, grad_out, channels_last)        # bias None


def test_frozen_weight_trainable_bias_takes_the_training_route(dev):
    from uninext_amd.backbone import PatchEmbed
    pe = PatchEmbed(embed_dim=40).to(dev)
    pe.own_exact_training = True
    pe.proj.weight.requires_grad_(False)
    x, _, _, grad_out = _inputs(2, 3, 37, 50, 40, 16, True, dev, seed=10)
    out = pe(x)
    assert type(out.grad_fn).__name__ == "PatchEmbedFunctionBackward"
    out.backward(grad_out)
    assert pe.proj.weight.grad is None
    want = grad_out.double().sum((0, 1, 2))
    assert _err(pe.proj.bias.grad, want) <= 1e-4 * float(want.abs().max())


def _bench_shapes():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import patch_embed_bench
    return patch_embed_bench.SHAPES


@pytest.mark.parametrize("shape", _bench_shapes(), ids=lambda s: s[0].split(" (")[0].replace(" ", "_"))
def test_full_size_vs_pytorch(shape, dev):
    """The bench shapes at full size against the fp32 PyTorch route: within 1e-4 of the scale."""
    _, B, C, H, W, E, k, cl = shape
    x, w, b, grad_out = _inputs(B, C, H, W, E, k, cl, dev, seed=11)
    need = (C > 3, True, True)                        # the image itself needs no gradient
    got = _run(x, w, b, grad_out, cl, True, need=need)
    want = _run(x, w, b, grad_out, cl, False, need=need)
    for name, g, r in zip(("out", "grad_x", "grad_weight", "grad_bias"), got, want):
        if r is None:
            continue
        e = _err(g, r)
        print("%-12s err vs PyTorch %.3e (scale %.3e)" % (name, e, float(r.abs().max())))
        assert e <= 1e-4 * float(r.abs().max()), name


@pytest.mark.parametrize("channels_last", [True, False])
def test_bitwise_repeatable_across_streams(channels_last, dev):
    x, w, b, grad_out = _inputs(2, 64, 100, 166, 128, 2, channels_last, dev, seed=12)
    a = _run(x, w, b, grad_out, channels_last, True)
    c = _run(x, w, b, grad_out, channels_last, True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d = _run(x, w, b, grad_out, channels_last, True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for u, v, z in zip(a[1:], c[1:], d[1:]):
        assert torch.equal(u, v) and torch.equal(u, z)


def test_route_opt_in_and_default(dev):
    from uninext_amd.backbone import PatchEmbed, patch_conv2d
    x = torch.randn(1, 3, 64, 80, device=dev, requires_grad=True)
    pe = PatchEmbed(embed_dim=64).to(dev)
    out = pe(x)                                       # default: the reference's conv + permute
    assert type(out.grad_fn.next_functions[0][0]).__name__ == "ConvolutionBackward0"
    pe.own_exact_training = True
    assert type(pe(x).grad_fn).__name__ == "PatchEmbedFunctionBackward"
    pe.exact_fp32 = False                             # the training route is exact whatever exact_fp32 says
    assert type(pe(x).grad_fn).__name__ == "PatchEmbedFunctionBackward"
    conv = torch.nn.Conv2d(8, 16, kernel_size=2, stride=2).to(dev)
    y = torch.randn(2, 8, 20, 30, device=dev, requires_grad=True)
    assert type(patch_conv2d(y, conv).grad_fn).__name__ == "ConvolutionBackward0"
    assert type(patch_conv2d(y, conv, own_training=True).grad_fn).__name__ == "PatchEmbedFunctionBackward"
    with torch.no_grad():                             # inference keeps its own route either way
        assert patch_conv2d(y, conv, own_training=True).grad_fn is None


def test_autocast_falls_back(dev):
    from uninext_amd.backbone import PatchEmbed, patch_conv2d
    conv = torch.nn.Conv2d(8, 16, kernel_size=2, stride=2).to(dev)
    x = torch.randn(2, 8, 20, 30, device=dev, requires_grad=True)
    pe = PatchEmbed(embed_dim=32).to(dev)
    pe.own_exact_training = True
    img = torch.randn(1, 3, 64, 80, device=dev)
    with torch.autocast("cuda", dtype=torch.float16):
        want = conv(x)
        got = patch_conv2d(x, conv, own_training=True)
        vit = pe(img)
    assert got.dtype == want.dtype == torch.float16
    assert type(got.grad_fn).__name__ == "ConvolutionBackward0"
    assert torch.equal(got, want)
    assert vit.dtype == torch.float16 and type(vit.grad_fn).__name__ == "PermuteBackward0"


def test_training_steps_track_pytorch(dev):
    """Three SGD steps from the same start on both routes (ViT PatchEmbed and a ConvNeXt downsample conv in sequence): the
    parameters stay within the bound after every step."""
    from uninext_amd.backbone import PatchEmbed, patch_conv2d

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.pe = PatchEmbed(kernel_size=(4, 4), stride=(4, 4), in_chans=3, embed_dim=32)
            self.down = torch.nn.Conv2d(32, 64, kernel_size=2, stride=2)

        def forward(self, x, own):
            self.pe.own_exact_training = own
            y = self.pe(x).permute(0, 3, 1, 2)
            return patch_conv2d(y, self.down, own_training=own)

    torch.manual_seed(13)
    ref = Net().to(dev)
    own = Net().to(dev)
    own.load_state_dict(ref.state_dict())
    f64 = Net().to(dev).double()
    f64.load_state_dict(ref.state_dict())
    gen = torch.Generator().manual_seed(14)
    x = torch.randn(2, 3, 70, 90, generator=gen).to(dev)
    nets = ((own, True), (ref, False), (f64, False))
    opts = [torch.optim.SGD(n.parameters(), lr=0.05) for n, _ in nets]
    for step in range(3):
        for (n, o), opt in zip(nets, opts):
            opt.zero_grad()
            (n(x.to(next(n.parameters()).dtype), o) ** 2).mean().backward()
            opt.step()
        for (k, p_own), p_ref, p64 in zip(own.named_parameters(), ref.parameters(), f64.parameters()):
            e, bound = _err(p_own, p64), _bound(p64.detach(), _err(p_ref, p64))
            assert e <= bound, (step, k, e, bound)
