"""MI355X tests of the static mask head's own training route: conv3x3_hip_backward_exact_f32 (include/conv3x3_hip.h) through
Conv3x3ReluFunction / MaskHeadSmallConv.own_exact_training (uninext_amd/mask_head.py).

Checker: PyTorch's own autograd of relu(conv2d) in float64.  The bound per gradient tensor is
max(1e-4 * max|ref|, 2 * the error of the fp32 PyTorch route) -- the own route is no further from float64 than twice the library's."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maskhead_bwd")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _conv(cin, cout, dev, gen, bias=True, bias_shift=0.0, padding_mode="zeros"):
    conv = torch.nn.Conv2d(cin, cout, 3, padding=1, bias=bias, padding_mode=padding_mode)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(cout, cin, 3, 3, generator=gen) / (9 * cin) ** 0.5)
        if bias:
            conv.bias.copy_(0.1 * torch.randn(cout, generator=gen) + bias_shift)
    return conv.to(dev)


def _err(a, ref):
    return float((a.detach().double() - ref.detach()).abs().max()) if ref.numel() else 0.0


def _bound(ref, err_torch32):
    return max(1e-4 * (float(ref.abs().max()) if ref.numel() else 0.0), 2.0 * err_torch32)


def _run(conv, x, grad_out, own, dtype=torch.float32):
    """(out, grad_x, grad_weight, grad_bias) of relu(conv(x)) in `dtype`; own: through Conv3x3ReluFunction."""
    from uninext_amd.mask_head import conv3x3_relu
    xx = x.detach().to(dtype).requires_grad_(True)
    if dtype == torch.float32:
        c = conv
    else:
        c = torch.nn.Conv2d(conv.in_channels, conv.out_channels, 3, padding=1, bias=conv.bias is not None).to(x.device, dtype)
        c.load_state_dict({k: v.to(dtype) for k, v in conv.state_dict().items()})
    for p in c.parameters():
        p.grad = None
    out = conv3x3_relu(xx, c, own_training=True) if own else F.relu(c(xx))
    out.backward(grad_out.to(dtype))
    return out, xx.grad, c.weight.grad, (c.bias.grad if c.bias is not None else None)


def _check_layer(conv, x, grad_out):
    from uninext_amd.mask_head import Conv3x3ReluFunction
    want = _run(conv, x, grad_out, own=False, dtype=torch.float64)
    torch32 = _run(conv, x, grad_out, own=False)
    got = _run(conv, x, grad_out, own=True)
    assert type(got[0].grad_fn).__name__ == Conv3x3ReluFunction.__name__ + "Backward"
    for name, g, t, w in zip(("out", "grad_x", "grad_weight", "grad_bias"), got, torch32, want):
        if w is None:
            continue
        e, bound = _err(g, w), _bound(w, _err(t, w))
        print("%-12s err %.3e  torch fp32 %.3e  bound %.3e" % (name, e, _err(t, w), bound))
        assert g.dtype == torch.float32 and g.shape == w.shape
        assert e <= bound, (name, e, bound)


@pytest.mark.parametrize("B,cin,cout,H,W", [
    (1, 16, 8, 5, 7),          # tile tails, every width residue mod 4 across the set
    (2, 16, 24, 6, 5),
    (2, 32, 40, 17, 18),
    (1, 16, 16, 1, 1),         # a single pixel
    (2, 16, 2, 13, 18),        # cout < 16: grad-input of 16 padded channels, grad-weight masked
    (3, 48, 130, 9, 31),       # partial channel tiles on both sides
    (2, 256, 256, 25, 42),     # lay3 at the training shapes
    (2, 64, 8, 100, 168),      # lay2 at the training shapes
])
def test_layer_parity(B, cin, cout, H, W, dev):
    gen = torch.Generator().manual_seed(B * 1000 + cin + cout)
    conv = _conv(cin, cout, dev, gen)
    x = torch.randn(B, cin, H, W, generator=gen).to(dev)
    grad_out = torch.randn(B, cout, H, W, generator=gen).to(dev)
    _check_layer(conv, x, grad_out)


def test_negative_bias_mostly_clamped(dev):
    gen = torch.Generator().manual_seed(5)
    conv = _conv(32, 48, dev, gen, bias_shift=-1.5)
    x = torch.randn(2, 32, 11, 23, generator=gen).to(dev)
    with torch.no_grad():
        assert float((F.relu(conv(x)) == 0).float().mean()) > 0.8
    _check_layer(conv, x, torch.randn(2, 48, 11, 23, generator=gen).to(dev))


def test_jia_dcn_full_size_vs_miopen(dev):
    """256 -> 256 at 100 x 168, bs 2 (the largest layer of a training step): against the fp32 MIOpen route, bound 1e-4 of the scale."""
    gen = torch.Generator().manual_seed(7)
    conv = _conv(256, 256, dev, gen)
    x = torch.randn(2, 256, 100, 168, generator=gen).to(dev)
    grad_out = torch.randn(2, 256, 100, 168, generator=gen).to(dev)
    got = _run(conv, x, grad_out, own=True)
    want = _run(conv, x, grad_out, own=False)
    for name, g, w in zip(("out", "grad_x", "grad_weight", "grad_bias"), got, want):
        e = _err(g, w.double())
        print("%-12s err vs MIOpen %.3e (scale %.3e)" % (name, e, float(w.abs().max())))
        assert e <= 1e-4 * float(w.abs().max()), name


def test_needs_input_grad_combinations(dev):
    from uninext_amd import ext
    from uninext_amd.mask_head import conv3x3_relu
    gen = torch.Generator().manual_seed(9)
    conv = _conv(16, 24, dev, gen)
    x = torch.randn(2, 16, 9, 10, generator=gen).to(dev)
    grad_out = torch.randn(2, 24, 9, 10, generator=gen).to(dev)
    full = _run(conv, x, grad_out, own=True)

    conv.weight.requires_grad_(False)                      # frozen weight: no grad-weight, the rest unchanged
    conv.weight.grad, conv.bias.grad = None, None
    xx = x.clone().requires_grad_(True)
    conv3x3_relu(xx, conv, own_training=True).backward(grad_out)
    assert conv.weight.grad is None and torch.equal(xx.grad, full[1]) and torch.equal(conv.bias.grad, full[3])
    conv.weight.requires_grad_(True)

    conv.bias.grad = None                                  # input without grad: no grad-input
    out = conv3x3_relu(x, conv, own_training=True)
    assert out.requires_grad
    out.backward(grad_out)
    assert torch.equal(conv.weight.grad, full[2]) and torch.equal(conv.bias.grad, full[3])

    nob = _conv(16, 24, dev, torch.Generator().manual_seed(9), bias=False)   # bias None
    got = _run(nob, x, grad_out, own=True)
    ref = _run(nob, x, grad_out, own=False, dtype=torch.float64)
    assert got[3] is None
    for g, w in zip(got[1:3], ref[1:3]):
        assert _err(g, w) <= 1e-4 * float(w.abs().max())

    empty = torch.zeros(0, 16, 9, 10, device=dev)            # empty batch: zero parameter gradients, empty input gradient
    got = _run(conv, empty, torch.zeros(0, 24, 9, 10, device=dev), own=True)
    assert got[1].shape == empty.shape
    assert float(got[2].abs().max()) == 0.0 and float(got[3].abs().max()) == 0.0
    g_x, g_w, g_b = ext.conv3x3_backward(x, None, None, grad_out, 24, relu=False, need_input=False, need_weight=False)
    assert g_x is None and g_w is None
    assert _err(g_b, grad_out.double().sum((0, 2, 3))) <= 1e-4 * float(grad_out.abs().sum((0, 2, 3)).max())


def test_bitwise_repeatable_across_streams(dev):
    gen = torch.Generator().manual_seed(11)
    conv = _conv(64, 64, dev, gen)
    x = torch.randn(2, 64, 50, 84, generator=gen).to(dev)
    grad_out = torch.randn(2, 64, 50, 84, generator=gen).to(dev)
    a = _run(conv, x, grad_out, own=True)
    b = _run(conv, x, grad_out, own=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = _run(conv, x, grad_out, own=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for u, v, w in zip(a[1:], b[1:], c[1:]):
        assert torch.equal(u, v) and torch.equal(u, w)


def _head_from_fixture(g, dev, own):
    from uninext_amd.mask_head import MaskHeadSmallConv
    fpn_dims = [g["fpn%d" % i].shape[1] for i in range(3)] if "fpn0" in g else None
    dim = g["x0"].shape[1]
    head = MaskHeadSmallConv(dim, fpn_dims, dim)
    head.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p:")})
    head = head.to(dev)
    head.own_exact_training = own
    return head, fpn_dims


def _head_grads(g, dev, own):
    head, fpn_dims = _head_from_fixture(g, dev, own)
    x = [torch.from_numpy(g["x%d" % i]).to(dev).requires_grad_(True) for i in range(3)]
    fpns = [torch.from_numpy(g["fpn%d" % i]).to(dev).requires_grad_(True) for i in range(3)] if fpn_dims else None
    out = head(x, fpns)
    out.backward(torch.from_numpy(g["grad_out"]).to(dev))
    grads = {"gx%d" % i: t.grad for i, t in enumerate(x)}
    if fpns:
        grads.update({"gfpn%d" % i: t.grad for i, t in enumerate(fpns)})
    grads.update({"g:" + k: p.grad for k, p in head.named_parameters()})
    return out, grads


@pytest.mark.parametrize("name", ["nofpn", "fpn"])
def test_module_matches_reference_gradients(name, dev):
    with np.load(os.path.join(FIXTURES, name + ".npz")) as z:
        g = {k: z[k] for k in z.files}
    out, own = _head_grads(g, dev, True)
    _, lib = _head_grads(g, dev, False)
    assert _err(out, torch.from_numpy(g["out"]).to(dev).double()) <= 1e-4 * float(np.abs(g["out"]).max())
    keys = [k for k in g if k.startswith(("gx", "gfpn", "g:"))]
    assert len(keys) == len(own)
    for k in keys:
        ref = torch.from_numpy(g[k]).to(dev).double()
        e, bound = _err(own[k], ref), _bound(ref, _err(lib[k], ref))
        print("%-20s err %.3e bound %.3e" % (k, e, bound))
        assert e <= bound, (k, e, bound)


def _layer_grad_fns(head, x, monkeypatch):
    from uninext_amd import mask_head
    seen = []
    orig = mask_head.conv3x3_relu

    def spy(*args, **kwargs):
        out = orig(*args, **kwargs)
        seen.append(type(out.grad_fn).__name__)
        return out

    monkeypatch.setattr(mask_head, "conv3x3_relu", spy)
    head(x, None).sum().backward()
    return seen


def test_route_opt_in_uses_own_backward(dev, monkeypatch):
    from uninext_amd.mask_head import Conv3x3ReluFunction, MaskHeadSmallConv
    head = MaskHeadSmallConv(64, None, 64).to(dev)
    head.own_exact_training = True
    x = [torch.randn(2, 64, h, w, device=dev, requires_grad=True) for h, w in ((13, 18), (7, 9), (4, 5))]
    assert _layer_grad_fns(head, x, monkeypatch) == [Conv3x3ReluFunction.__name__ + "Backward"] * 5
    assert all(p.grad is not None for p in head.parameters())


def test_route_default_is_pytorch(dev, monkeypatch):
    from uninext_amd.mask_head import MaskHeadSmallConv
    assert MaskHeadSmallConv.own_exact_training is False
    head = MaskHeadSmallConv(64, None, 64).to(dev)
    x = [torch.randn(2, 64, h, w, device=dev, requires_grad=True) for h, w in ((13, 18), (7, 9), (4, 5))]
    assert _layer_grad_fns(head, x, monkeypatch) == ["ReluBackward0"] * 5


@pytest.mark.parametrize("grad", [True, False])
def test_autocast_falls_back(grad, dev):
    from uninext_amd.mask_head import conv3x3_relu
    conv = _conv(16, 24, dev, torch.Generator().manual_seed(3))
    x = torch.randn(1, 16, 8, 9, device=dev, requires_grad=grad)
    with torch.set_grad_enabled(grad), torch.autocast("cuda", dtype=torch.float16):
        want = F.relu(conv(x))
        got = conv3x3_relu(x, conv, own_training=True)
    assert got.dtype == want.dtype == torch.float16
    assert torch.equal(got, want)


@pytest.mark.parametrize("grad", [True, False])
def test_reflect_padding_falls_back(grad, dev):
    from uninext_amd.mask_head import conv3x3_relu
    conv = _conv(16, 24, dev, torch.Generator().manual_seed(4), padding_mode="reflect")
    x = torch.randn(1, 16, 8, 9, device=dev, requires_grad=grad)
    with torch.set_grad_enabled(grad):
        want = F.relu(conv(x))
        got = conv3x3_relu(x, conv, own_training=True)
    assert torch.equal(got, want)
    if grad:
        assert type(got.grad_fn).__name__ == "ReluBackward0"


def test_training_steps_track_pytorch(dev):
    """Three SGD steps from the same start on both routes: the parameters stay within the bound after every step (a stale packed
    weight after optimizer.step() would not)."""
    from uninext_amd.mask_head import MaskHeadSmallConv
    torch.manual_seed(13)
    ref = MaskHeadSmallConv(64, None, 64).to(dev)
    own = MaskHeadSmallConv(64, None, 64).to(dev)
    own.load_state_dict(ref.state_dict())
    own.own_exact_training = True
    f64 = MaskHeadSmallConv(64, None, 64).to(dev).double()
    f64.load_state_dict(ref.state_dict())
    gen = torch.Generator().manual_seed(14)
    x = [torch.randn(2, 64, h, w, generator=gen).to(dev) for h, w in ((13, 18), (7, 9), (4, 5))]
    heads = (own, ref, f64)
    opts = [torch.optim.SGD(h.parameters(), lr=0.05) for h in heads]
    for step in range(3):
        for h, opt in zip(heads, opts):
            opt.zero_grad()
            xs = [t.to(next(h.parameters()).dtype) for t in x]
            (h(xs, None) ** 2).mean().backward()
            opt.step()
        for (k, p_own), p_ref, p64 in zip(own.named_parameters(), ref.parameters(), f64.parameters()):
            e, bound = _err(p_own, p64.detach()), _bound(p64.detach(), _err(p_ref, p64.detach()))
            assert e <= bound, (step, k, e, bound)
