"""MI355X tests of the ConvNeXt training route: the backward kernels of include/patch_embed_hip.h (block head, tail with stochastic
depth, channels-first LayerNorm) and the modules with own_training on (uninext_amd/backbone.py).  Reference: float64 autograd
through the restatement of tests/convnext_ref.py and the reference-minted gradients of tests/golden/convnext_train/.  Tolerance: the
project's 1e-4 * max(1, max|ref|) per gradient tensor; every compared LayerNorm runs on pixels whose channel variance is above 1e-2
(asserted).  The error of PyTorch's own fp32 composition is printed beside ours, for the record only."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnext_cases as C         # noqa: E402
import convnext_ref as R           # noqa: E402
import convnext_train_cases as T   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def to(dev, *ts):
    return [None if t is None else t.to(device=dev, dtype=torch.float32).contiguous() for t in ts]


def last():
    from uninext_amd import _lib
    return _lib.last_kernel("convnext")


def check(got, ref, what, composition=None):
    err, bound = C.max_err(got, ref), C.tol(ref)
    comp = "" if composition is None else ", fp32 PyTorch composition %.3g" % C.max_err(composition, ref)
    print("%s: max abs err %.3g, bound %.3g (scale %.3g)%s" % (what, err, bound, float(ref.abs().max()), comp))
    assert tuple(got.shape) == tuple(ref.shape) and err < bound, (what, err, bound)


def bits(t):
    return None if t is None else t.detach().cpu().numpy().tobytes()


# ---- the block's head -------------------------------------------------------------------------------------------------------------
HEAD_NAMES = ("x", "dw_weight", "dw_bias", "ln_weight", "ln_bias")


@pytest.mark.parametrize("case", T.HEAD_CASES + [T.WIDE_HEAD_CASE] + T.BAND_HEAD_CASES, ids=lambda c: "C%d_B%d_%dx%d" % c[:4])
def test_head_backward_vs_float64(case, dev):
    from uninext_amd import ext
    inputs, grad_out, ref = T.head_reference(tuple(case))        # asserts the variance floor
    x, dw_w, dw_b, ln_w, ln_b = to(dev, *inputs)
    got = ext.convnext_dwconv_ln_backward(x, dw_w, dw_b, ln_w, C.EPS, grad_out.to(dev))
    assert last().startswith("convnext_dwconv_ln_backward<")
    comp = T.head_grads([t for t in (x, dw_w, dw_b, ln_w, ln_b)], grad_out.to(dev), torch.float32)
    assert (got[2] is None) == (dw_b is None)
    for name, g in zip(HEAD_NAMES, got):
        if g is not None:
            check(g, ref[name], "head %s grad_%s" % (case, name), comp[name])


def test_head_backward_skips_leave_the_rest_bitwise(dev):
    from uninext_amd import ext
    inputs, grad_out, _ = T.head_reference((96, 3, 11, 23, True))
    x, dw_w, dw_b, ln_w, ln_b = to(dev, *inputs)
    go = grad_out.to(dev)
    flags = ("need_input", "need_dw_weight", "need_dw_bias", "need_ln_weight", "need_ln_bias")
    full = [bits(g) for g in ext.convnext_dwconv_ln_backward(x, dw_w, dw_b, ln_w, C.EPS, go)]
    subsets = [{f: False} for f in flags] + [{f: f == keep for f in flags} for keep in flags]
    for kw in subsets:
        got = ext.convnext_dwconv_ln_backward(x, dw_w, dw_b, ln_w, C.EPS, go, **kw)
        for f, g, want in zip(flags, got, full):
            if kw.get(f, True):
                assert bits(g) == want, (kw, f)
            else:
                assert g is None, (kw, f)
    empty = ext.convnext_dwconv_ln_backward(x[:0].contiguous(), dw_w, dw_b, ln_w, C.EPS, go[:0].contiguous())
    assert empty[0].shape == (0, 96, 11, 23) and all(float(g.abs().max()) == 0.0 for g in empty[1:])


def test_empty_batch_at_the_c_entry_points(dev):
    """B = 0 handed to the library itself (uninext_amd.ext answers an empty batch without calling it): no kernel, and zeros in the
    parameter gradients that were asked for, in those alone."""
    from uninext_amd import _lib, ext
    lib = _lib.load()
    c = 96
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
    p = torch.zeros(64, device=dev).data_ptr()                    # an address for operands that an empty batch never reads
    ext.layernorm_channels_first(*to(dev, *C.cf_case(1, 1, 3, 2, 2)), C.EPS)
    before = last()
    g_w, g_b, g_lw, g_lb = nan(c, 1, 7, 7), nan(c), nan(c), nan(c)
    ext._launch(dev, lib.patch_embed_hip_convnext_dwconv_ln_backward_f32, p, p, p, p, C.EPS, p, 0, c, 11, 23, None, g_w.data_ptr(), None,
                g_lw.data_ptr(), g_lb.data_ptr(), None, 0)
    assert all(float(g.abs().max()) == 0.0 for g in (g_w, g_lw, g_lb)) and bool(torch.isnan(g_b).all())
    g_w, g_b = nan(c, 1, 7, 7), nan(c)
    ext._launch(dev, lib.patch_embed_hip_convnext_dwconv_ln_backward_f32, p, p, None, p, C.EPS, p, 0, c, 11, 23, None, None, g_b.data_ptr(),
                None, None, None, 0)
    assert float(g_b.abs().max()) == 0.0 and bool(torch.isnan(g_w).all())
    g_g = nan(c)
    ext._launch(dev, lib.patch_embed_hip_convnext_scale_residual_backward_f32, p, p, p, None, 0, c, 11, 23, None, g_g.data_ptr(), None, 0)
    assert float(g_g.abs().max()) == 0.0
    g_w, g_b = nan(c), nan(c)
    ext._launch(dev, lib.patch_embed_hip_layernorm_cf_backward_f32, p, p, C.EPS, p, 0, c, 11, 23, None, g_w.data_ptr(), None, None, 0)
    ext._launch(dev, lib.patch_embed_hip_layernorm_cf_backward_f32, p, p, C.EPS, p, 0, c, 11, 23, None, None, None, None, 0)
    assert float(g_w.abs().max()) == 0.0 and bool(torch.isnan(g_b).all())
    assert last() == before == "layernorm_cf<cached>"


def test_head_backward_takes_a_grad_out_at_any_address(dev):
    """The kernel reads grad_out 16 bytes at once; a contiguous view that starts 4 bytes into its storage, as autograd may hand
    over, is staged by uninext_amd.ext: the gradients are bitwise those of the aligned tensor, through the Function too."""
    from uninext_amd import ext
    from uninext_amd.backbone import ConvNeXtHeadFunction
    inputs, grad_out, _ = T.head_reference((96, 3, 11, 23, True))
    x, dw_w, dw_b, ln_w, ln_b = to(dev, *inputs)
    go = grad_out.to(dev)
    odd = torch.empty(go.numel() + 1, device=dev)[1:].view_as(go).copy_(go)
    assert go.data_ptr() % 16 == 0 and odd.data_ptr() % 16 == 4 and odd.is_contiguous()
    full = [bits(g) for g in ext.convnext_dwconv_ln_backward(x, dw_w, dw_b, ln_w, C.EPS, go)]
    assert [bits(g) for g in ext.convnext_dwconv_ln_backward(x, dw_w, dw_b, ln_w, C.EPS, odd)] == full
    leaves = [t.clone().requires_grad_(True) for t in (x, dw_w, dw_b, ln_w, ln_b)]
    got = torch.autograd.grad(ConvNeXtHeadFunction.apply(*leaves, C.EPS), leaves, odd)
    assert [bits(g) for g in got] == full


# ---- the block's tail -------------------------------------------------------------------------------------------------------------
def _tail_case(c, hw, scaled, dev):
    g = torch.Generator().manual_seed(c * 131 + hw)
    B = 3
    y, inp, go = torch.randn(B, 1, hw, c, generator=g), torch.randn(B, c, 1, hw, generator=g), torch.randn(B, c, 1, hw, generator=g)
    gamma = torch.randn(c, generator=g) if scaled else None
    s = torch.tensor([1.0 / 0.3, 0.0, 1.0 / 0.3])               # keep = 0.3; the middle sample is dropped
    return to(dev, y, inp, go, gamma, s)


@pytest.mark.parametrize("scaled", [True, False])
def test_tail_forward_with_sample_scale_is_bitwise_pytorch(scaled, dev):
    from uninext_amd import ext
    for c in T.TAIL_SIZES:
        for hw in T.TAIL_SIZES:
            y, inp, _, gamma, s = _tail_case(c, hw, scaled, dev)
            out = ext.convnext_scale_residual_drop(y, gamma, s, inp)
            assert last() == "convnext_scale_residual_drop"
            branch = ((gamma * y) if scaled else y).permute(0, 3, 1, 2)
            want = inp + branch * s.view(-1, 1, 1, 1)
            assert out.is_contiguous() and bits(out) == bits(want.contiguous()), (c, hw)
            assert torch.equal(out[1], inp[1])
            assert bits(ext.convnext_scale_residual_drop(y, gamma, None, inp)) == bits(ext.convnext_scale_residual(y, gamma, inp))


@pytest.mark.parametrize("scaled", [True, False])
def test_tail_backward(scaled, dev):
    from uninext_amd import ext
    from uninext_amd.backbone import ConvNeXtTailFunction
    for c in T.TAIL_SIZES:
        for hw in T.TAIL_SIZES:
            y, inp, go, gamma, s = _tail_case(c, hw, scaled, dev)
            for scale in (s, None):
                g_y, g_g = ext.convnext_scale_residual_backward(go, y, gamma, scale)
                assert last() == "convnext_scale_residual_backward"
                t = go if scale is None else go * scale.view(-1, 1, 1, 1)
                want = ((t * gamma.view(1, -1, 1, 1)) if scaled else t).permute(0, 2, 3, 1).contiguous()
                assert bits(g_y) == bits(want), (c, hw)
                assert (g_g is None) == (not scaled)
                if scaled:
                    ref = (t.double() * y.double().permute(0, 3, 1, 2)).sum((0, 2, 3)).cpu()
                    err, bound = C.max_err(g_g, ref), C.tol(ref)
                    assert err < bound, (c, hw, err, bound)
                    only = ext.convnext_scale_residual_backward(go, y, gamma, scale, need_y=False)
                    assert only[0] is None and bits(only[1]) == bits(g_g)
                    assert bits(ext.convnext_scale_residual_backward(go, None, gamma, scale, need_gamma=False)[0]) == bits(g_y)
    # the Function hands grad_out itself to `input`
    y, inp, go, gamma, s = _tail_case(65, 129, True, dev)
    ya, ga, ia = y.clone().requires_grad_(True), gamma.clone().requires_grad_(True), inp.clone().requires_grad_(True)
    g_y, g_in = torch.autograd.grad(ConvNeXtTailFunction.apply(ya, ga, s, ia), (ya, ia), go)
    assert g_in.data_ptr() == go.data_ptr()
    assert float(g_y[1].abs().max()) == 0.0                 # the dropped sample


# ---- channels-first LayerNorm -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(T.CF_CASES)))
def test_layernorm_cf_backward_vs_float64(case, dev):
    from uninext_amd import ext
    c = T.CF_CASES[case][0]
    inputs, grad_out, ref = T.cf_reference(case)                  # asserts the variance floor
    x, w, b = to(dev, *inputs)
    go = grad_out.to(dev)
    got = ext.layernorm_channels_first_backward(x, w, C.EPS, go)
    assert last() == ("layernorm_cf_backward<cached>" if c <= 512 else "layernorm_cf_backward<streamed>")
    comp = T.cf_grads([x, w, b], go, torch.float32)
    for name, g in zip(("x", "weight", "bias"), got):
        check(g, ref[name], "layernorm_cf %s grad_%s" % (T.CF_CASES[case], name), comp[name])
    if c == 1:
        assert float(got[0].abs().max()) == 0.0 and float(got[1].abs().max()) == 0.0
    full = [bits(g) for g in got]
    for skip in range(3):
        need = [i != skip for i in range(3)]
        part = ext.layernorm_channels_first_backward(x, w, C.EPS, go, need_input=need[0], need_weight=need[1], need_bias=need[2])
        assert [bits(g) for g in part] == [f if n else None for f, n in zip(full, need)]


# ---- the modules -----------------------------------------------------------------------------------------------------------------
def _recorded(names):
    """Wraps the named launchers of uninext_amd.ext so that their calls are listed; returns (calls, restore)."""
    from uninext_amd import ext
    calls, real = [], {n: getattr(ext, n) for n in names}
    for n, fn in real.items():
        setattr(ext, n, lambda *a, _n=n, _fn=fn, **kw: (calls.append(_n), _fn(*a, **kw))[1])
    return calls, lambda: [setattr(ext, n, fn) for n, fn in real.items()]


@pytest.mark.parametrize("name", ["block_c32", "block_c96_noscale"])
def test_block_under_autograd_on_the_kernels(name, dev):
    fx, g = C.load(name), T.load_grads(name)
    blk = C.our_block(fx, torch.float32, dev)
    x = fx["x"].float().to(dev)
    with torch.no_grad():
        inference = blk(x)
    blk.own_training = True
    calls, restore = _recorded(["convnext_dwconv_ln", "convnext_dwconv_ln_backward", "convnext_scale_residual_drop",
                                "convnext_scale_residual_backward"])
    try:
        xa = x.clone().requires_grad_(True)
        out = blk(xa)
        assert last() == "convnext_scale_residual"
        out.backward(g["grad_out"].float().to(dev))
        assert last().startswith("convnext_dwconv_ln_backward<")
    finally:
        restore()
    assert calls == ["convnext_dwconv_ln", "convnext_scale_residual_drop", "convnext_scale_residual_backward", "convnext_dwconv_ln_backward"]
    assert bits(out) == bits(inference)
    grads = dict({"grad.x": xa.grad}, **{"grad." + n: p.grad for n, p in blk.named_parameters()})
    assert set(grads) == {k for k in g if k.startswith("grad.")} and len(grads) == (10 if name == "block_c32" else 9)
    for k, v in grads.items():
        check(v, g[k], "%s %s" % (name, k))


def test_small_network_under_autograd_on_the_kernels(dev):
    fx, g = C.load("net_small"), T.load_grads("net_small")
    net = C.our_net(fx, torch.float32, dev)
    x = fx["x"].float().to(dev)
    with torch.no_grad():
        inference = net(x)
    net.set_own_training(True)
    calls, restore = _recorded(["convnext_dwconv_ln_backward", "convnext_scale_residual_backward", "layernorm_channels_first_backward",
                                "patch_embed_backward"])
    try:
        xa = x.clone().requires_grad_(True)
        out = net(xa)
        keys = sorted(out)
        torch.autograd.backward([out[k] for k in keys], [g["grad_out." + k].float().to(dev) for k in keys])
    finally:
        restore()
    assert calls.count("convnext_dwconv_ln_backward") == calls.count("convnext_scale_residual_backward") == sum(C.NET_DEPTHS)
    assert calls.count("layernorm_channels_first_backward") == 7 and calls.count("patch_embed_backward") == 4
    for k in keys:
        assert bits(out[k]) == bits(inference[k]), k
    grads = dict({"grad.x": xa.grad}, **{"grad." + n: p.grad for n, p in net.named_parameters()})
    assert set(grads) == {k for k in g if k.startswith("grad.")}
    for k, v in grads.items():
        check(v, g[k], "net_small " + k)


def _drop_block(dev):
    from uninext_amd.backbone import Block
    fx = C.load("block_c32")
    blk = Block(32, drop_path=0.5, layer_scale_init_value=1.0)
    blk.load_state_dict(fx["state"], strict=True)
    g = torch.Generator().manual_seed(12)
    x = torch.cat([fx["x"].float(), C.dyadic(torch.randn(2, 32, 9, 13, generator=g, dtype=torch.float64)).float()])
    return blk.to(dev).train(), x.to(dev), torch.randn(x.shape, generator=g).to(dev)


def _seed_that_drops_some(x):
    """(seed, mask [4]): the first seed whose draw -- DropPath's own call -- drops some of the four samples, not all."""
    for seed in range(16):
        torch.manual_seed(seed)
        mask = x.new_empty((4, 1, 1, 1)).bernoulli_(0.5).view(-1)
        if 0 < int(mask.sum()) < 4:
            return seed, mask
    raise AssertionError("no seed below 16 drops some samples and keeps some")


def test_drop_path_draws_the_composition_s_mask(dev):
    blk, x, grad = _drop_block(dev)
    seed, mask = _seed_that_drops_some(x)
    dropped = [b for b in range(4) if float(mask[b]) == 0.0]
    assert dropped and len(dropped) < 4
    runs = {}
    for flag in (False, True):
        blk.own_training = flag
        blk.zero_grad()
        xa = x.clone().requires_grad_(True)
        torch.manual_seed(seed)
        out = blk(xa)
        out.backward(grad)
        runs[flag] = (out.detach(), xa.grad, [p.grad.clone() for p in blk.parameters()])
        assert last().startswith("convnext_dwconv_ln_backward<") == flag
    off, on = runs[False], runs[True]
    check(on[0], off[0].double().cpu(), "drop path: output against the composition")
    check(on[1], off[1].double().cpu(), "drop path: grad_x against the composition")
    for (n, _), a, b in zip(blk.named_parameters(), on[2], off[2]):
        check(a, b.double().cpu(), "drop path: grad %s against the composition" % n)
    for b in dropped:
        assert torch.equal(on[0][b], x[b]) and torch.equal(off[0][b], x[b])
        assert torch.equal(on[1][b], grad[b])                    # the branch adds exactly nothing to a dropped sample's gradient
    kept = [b for b in range(4) if b not in dropped]
    assert not torch.equal(on[0][kept[0]], x[kept[0]])


def test_drop_path_tail_of_the_module_is_bitwise_the_composition_s_on_equal_y(dev):
    """The module's own plumbing of the mask (Block._sample_scale into ConvNeXtTailFunction): the flag-on block is given the y the
    composition's pwconv2 put out (a forward hook swaps it in, the heads differ in rounding) and draws under the same seed.  Output
    and grad_y are then the composition's to the bit, a dropped sample's grad_y is zero, and x gets grad_out alone."""
    blk, x, grad = _drop_block(dev)
    seed, mask = _seed_that_drops_some(x)
    kept = {}

    def keep(mod, inp, out):
        out.retain_grad()
        kept["y"] = out

    def swap(mod, inp, out):
        kept["leaf"] = kept["y"].detach().clone().requires_grad_(True)
        return kept["leaf"]

    hook = blk.pwconv2.register_forward_hook(keep)
    blk.own_training = False
    torch.manual_seed(seed)
    off = blk(x.clone().requires_grad_(True))
    off.backward(grad)
    hook.remove()
    g_gamma_off = blk.gamma.weight.grad.clone()
    blk.zero_grad()
    hook = blk.pwconv2.register_forward_hook(swap)
    blk.own_training = True
    xa = x.clone().requires_grad_(True)
    torch.manual_seed(seed)
    on = blk(xa)
    assert last() == "convnext_scale_residual_drop"
    on.backward(grad)
    hook.remove()
    assert last() == "convnext_scale_residual_backward"          # y is a leaf here: nothing flows on to the head
    assert bits(on) == bits(off)
    assert bits(kept["leaf"].grad) == bits(kept["y"].grad)
    assert torch.equal(xa.grad, grad)
    for b in range(4):
        assert (float(kept["leaf"].grad[b].abs().max()) == 0.0) == (float(mask[b]) == 0.0)
    s = (mask / 0.5).double().view(-1, 1, 1, 1)
    ref = ((grad.double() * s).permute(0, 2, 3, 1) * kept["y"].detach().double()).sum((0, 1, 2)).view(1, -1).cpu()
    check(blk.gamma.weight.grad, ref, "drop path: grad_gamma on the composition's y", g_gamma_off)


def test_checkpoint_passes_are_bitwise_equal(dev):
    from uninext_amd.backbone import ConvNeXt
    fx = C.load("net_small")
    grads = {}
    for ckpt in (False, True):
        net = ConvNeXt(in_chans=3, depths=C.NET_DEPTHS, dims=C.NET_DIMS, drop_path_rate=0.5, layer_scale_init_value=1.0, use_checkpoint=ckpt)
        net.load_state_dict(fx["state"], strict=True)
        net = net.to(dev).train().set_own_training(True)
        xa = fx["x"].float().to(dev).requires_grad_(True)
        torch.manual_seed(3)
        out = net(xa)
        torch.autograd.backward([out[k] for k in sorted(out)], [torch.ones_like(out[k]) for k in sorted(out)])
        assert last().startswith(("convnext_", "layernorm_cf_backward"))
        grads[ckpt] = [bits(xa.grad)] + [bits(p.grad) for p in net.parameters()] + [bits(out[k]) for k in sorted(out)]
    assert grads[True] == grads[False]


def test_gradients_bitwise_repeatable_across_runs_and_streams(dev):
    from uninext_amd import ext
    inputs, grad_out, _ = T.head_reference(T.WIDE_HEAD_CASE)
    x, dw_w, dw_b, ln_w, _ = to(dev, *inputs)
    go = grad_out.to(dev)
    g = torch.Generator().manual_seed(4)
    y, gamma, s, tgo = to(dev, torch.randn(2, 23, 31, 192, generator=g), torch.randn(192, generator=g), torch.tensor([2.0, 0.0]),
                          torch.randn(2, 192, 23, 31, generator=g))
    cf = to(dev, *C.cf_case(5, 2, 192, 23, 31))
    band_inputs, band_go, _ = T.head_reference(T.BAND_HEAD_CASES[0])    # several tiles a band in pass two
    bx, bw, bb, blw, _ = to(dev, *band_inputs)
    bgo = band_go.to(dev)
    runs = {"head": lambda: ext.convnext_dwconv_ln_backward(x, dw_w, dw_b, ln_w, C.EPS, go),
            "head, bands": lambda: ext.convnext_dwconv_ln_backward(bx, bw, bb, blw, C.EPS, bgo),
            "tail": lambda: ext.convnext_scale_residual_backward(tgo, y, gamma, s),
            "ln": lambda: ext.layernorm_channels_first_backward(cf[0], cf[1], C.EPS, tgo)}
    for name, run in runs.items():
        a, b, c3 = run(), run(), run()
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            c = run()
        side.synchronize()
        for i in range(len(a)):
            assert bits(a[i]) == bits(b[i]) == bits(c3[i]) == bits(c[i]), (name, i)
