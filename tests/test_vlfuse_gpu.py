"""Early vision-language fusion on the GPU: the fused HIP core (include/biattn_hip.h) against the float64 restatement
(tests/vlfuse_ref.py), the reference-minted fixtures and the module's own PyTorch composition.  Bound: max abs error <= 1e-4 of
the output's max abs (the project's bound); the exact-score family is held to 1e-6."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vlfuse_cases as C   # noqa: E402
import vlfuse_ref as R     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def fused(q, k, vv, vl, mask, H, scale):
    from uninext_amd import ext
    return ext.bi_attention_forward(q, k, vv, vl, mask, H, scale)


def check(got, want, tol, what):
    for g, w, side in zip(got, want, ("out_v", "out_l")):
        err = C.rel_err(g, w)
        print("%s %s: %.3g of scale" % (what, side, err))
        assert err <= tol, (what, side, err)


def make_mask(kind, B, T, gen):
    if kind == "none":
        return None
    m = (torch.rand(B, T, generator=gen) > 0.4).long()
    if kind == "full":
        m[B - 1] = 0                         # one fully masked image
    if kind == "f32":
        m = m.float()
    return m.to(DEV)


@pytest.mark.parametrize("name", C.EXPECTED)
def test_core_on_fixtures(name):
    fx = C.load(name)
    q, k, vv, vl, m, H, scale = C.core_inputs(fx, torch.float32, DEV)
    got = fused(q.contiguous(), k.contiguous(), vv.contiguous(), vl.contiguous(), m, H, scale)
    check(got, R.core(q, k, vv, vl, m, H, scale), C.TOL, name + " vs restatement")
    # and against the reference's own float64 numbers (the fp32 inputs of the core differ from them by the projections'
    # round-off); images whose tokens are all masked stay out of the image side: see tests/vlfuse_ref.py
    keep = [b for b in range(q.shape[0]) if b not in C.fully_masked_images(fx)]
    assert C.rel_err(got[0][keep].cpu(), torch.from_numpy(fx["core_out_v"])[keep]) <= C.TOL
    assert C.rel_err(got[1].cpu(), torch.from_numpy(fx["core_out_l"])) <= C.TOL


@pytest.mark.parametrize("BH", [(1, 1), (2, 8)])
@pytest.mark.parametrize("T", [1, 16, 37, 255, 256])
@pytest.mark.parametrize("S", [1, 63, 1065, 5573])
def test_core_seeded(S, T, BH):
    B, H = BH
    gen = torch.Generator().manual_seed(1000 * S + 10 * T + B)
    E = H * 256
    for kind in ("none", "i64", "f32", "full"):
        q = (torch.randn(B, S, E, generator=gen) * 3).to(DEV)
        k = (torch.randn(B, T, E, generator=gen) * 2).to(DEV)
        vv = torch.randn(B, S, E, generator=gen).to(DEV)
        vl = torch.randn(B, T, E, generator=gen).to(DEV)
        m = make_mask(kind, B, T, gen)
        got = fused(q, k, vv, vl, m, H, 256 ** -0.5)
        assert float(R.scores(q, k, H, 256 ** -0.5).abs().max()) < 500
        check(got, R.core(q, k, vv, vl, m, H, 256 ** -0.5), C.TOL, "S%d T%d BH%d %s" % (S, T, B * H, kind))


@pytest.mark.parametrize("S,T,B,H", [(70, 9, 1, 2), (300, 37, 2, 1), (1, 1, 1, 1), (200, 1, 1, 2), (4129, 256, 1, 1), (33, 2, 2, 2)])
def test_exact_score_family(S, T, B, H):
    """Integer scores (tests/vlfuse_ref.py: exact_case): ties at the +-50000 clamp share weight equally on both axes, the mask
    adds +1 / sets -9e15, a fully masked image is uniform, T = 1, and with S = 4129 = 129 * 32 + 1 the last range of S holds one
    token -- which is given the column maximum."""
    q, k, vv, vl, scale = R.exact_case(11 * S + T, B, H, S, T, device=DEV)
    if S == 4129:
        q[:, S // 2] = q[:, S - 1] * 0 + torch.randint(-8, 9, (B, H * 256)).float().to(DEV)   # un-tie: only token 0 and ...
        q[:, S - 1] = q[:, 0]                                                                   # ... the LAST one reach the clamp
    s = R.scores(q, k, H, scale)
    assert float(s.max()) == R.CLAMP
    if S == 4129:
        assert bool((s[:, :, S - 1, 0] == R.CLAMP).all())
    gen = torch.Generator().manual_seed(S)
    for kind in ("none", "i64", "f32", "full"):
        m = make_mask(kind, B, T, gen)
        got = fused(q, k, vv, vl, m, H, scale)
        want = R.core(q, k, vv, vl, m, H, scale)
        check(got, want, C.TOL_EXACT, "exact S%d T%d %s" % (S, T, kind))
        if kind == "full":
            mean = vl[B - 1].double().view(T, H, 256).mean(dim=0).reshape(1, H * 256)
            assert float((got[0][B - 1].double() - mean).abs().max()) <= 1e-6 * float(mean.abs().max())


def full_size_inputs():
    gen = torch.Generator().manual_seed(7)
    B, H, S, T = 2, 8, 22223, 256
    q = (torch.randn(B, S, H * 256, generator=gen) * 3).to(DEV)
    k = (torch.randn(B, T, H * 256, generator=gen) * 2).to(DEV)
    vv = torch.randn(B, S, H * 256, generator=gen).to(DEV)
    vl = torch.randn(B, T, H * 256, generator=gen).to(DEV)
    m = (torch.rand(B, T, generator=gen) > 0.3).long().to(DEV)
    return q, k, vv, vl, m, H


def test_full_size_against_the_float64_composition():
    """bs 2, S 22223, T 256, 8 x 256 against the module's PyTorch composition in float64 on the device."""
    from uninext_amd.modules import BiMultiHeadAttention
    q, k, vv, vl, m, H = full_size_inputs()
    got = fused(q, k, vv, vl, m, H, 1.0 / 16)
    a = BiMultiHeadAttention(16, 24, H * 256, H, cfg=C.vlfuse_cfg(16, 24, H * 256)).eval()
    with torch.no_grad():
        # per image, to bound the float64 [8, S, T] temporaries; q is scaled in fp32 first, as the module does
        want = [a._core_torch((q[b:b + 1] * a.scale).double(), k[b:b + 1].double(), vv[b:b + 1].double(), vl[b:b + 1].double(),
                              m[b:b + 1]) for b in range(q.shape[0])]
    want = (torch.cat([w[0] for w in want]), torch.cat([w[1] for w in want]))
    check(got, want, C.TOL, "full size")


def test_bitwise_repeatable_and_stream_independent():
    q, k, vv, vl, m, H = full_size_inputs()
    q, vv = q[:, :5573].contiguous(), vv[:, :5573].contiguous()
    a = fused(q, k, vv, vl, m, H, 1.0 / 16)
    b = fused(q, k, vv, vl, m, H, 1.0 / 16)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = fused(q, k, vv, vl, m, H, 1.0 / 16)
    side.synchronize()
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_unsupported_arguments_raise():
    from uninext_amd import ext
    q = torch.zeros(1, 4, 256, device=DEV)
    k = torch.zeros(1, 3, 256, device=DEV)
    assert not ext.bi_attention_supported(q, k, q, k, None, 2)                         # head_dim 128
    assert not ext.bi_attention_supported(q, k, q, k, torch.ones(1, 3, device=DEV).bool(), 1)
    assert ext.bi_attention_supported(q, k, q, k, torch.ones(1, 3, device=DEV).long(), 1)
    with pytest.raises(RuntimeError):
        ext.bi_attention_forward(q, k, q, k, None, 2, 1.0)


# ---- module level ---------------------------------------------------------------------------------------------------

@pytest.fixture
def fused_on():
    from uninext_amd.modules import BiMultiHeadAttention
    old = BiMultiHeadAttention.fused_core
    BiMultiHeadAttention.fused_core = True
    yield BiMultiHeadAttention
    BiMultiHeadAttention.fused_core = old


@pytest.fixture
def calls(monkeypatch):
    """Counts the calls of the fused entry point."""
    from uninext_amd import ext
    n = {"fused": 0}
    real = ext.bi_attention_forward

    def counted(*a, **kw):
        n["fused"] += 1
        return real(*a, **kw)
    monkeypatch.setattr(ext, "bi_attention_forward", counted)
    return n


@pytest.mark.parametrize("name", C.EXPECTED)
def test_modules_on_fixtures(name, fused_on, calls):
    from uninext_amd import _lib
    fx = C.load(name)
    blk = C.block_from(fx, torch.float32, DEV)
    top = C.vlfuse_from(fx, torch.float32, DEV)
    v, l, m = C.inputs(fx, torch.float32, DEV)
    keep = [b for b in range(v.shape[0]) if b not in C.fully_masked_images(fx)]
    with torch.no_grad():
        out_v, out_l = blk(v, l, m, None)
        nv, nl = blk.layer_norm_v(v), blk.layer_norm_l(l)
        a_v, a_l = blk.attn(nv, nl, attention_mask_l=m)
        lang = {"hidden": l, "masks": m}
        x = {"visual": v, "lang": lang}
        y = top(x)
    assert calls["fused"] == 3 and "biattn_image" in _lib.last_kernel("biattn") and "biattn_text" in _lib.last_kernel("biattn")
    # the reference's dict: same keys out, the lang dict is the caller's own object with `hidden` replaced, masks untouched
    assert set(y) == {"visual", "lang"} and y["lang"] is lang and y["lang"]["masks"] is m and set(lang) == {"hidden", "masks"}
    for got, key, image_side in ((out_v, "out_visual", True), (out_l, "out_hidden", False), (a_v, "attn_out_v", True),
                                 (a_l, "attn_out_l", False), (y["visual"], "out_visual", True),
                                 (y["lang"]["hidden"], "out_hidden", False)):
        want = torch.from_numpy(fx[key])
        g = got.cpu()
        if image_side:
            g, want = g[keep], want[keep]
        err = C.rel_err(g, want)
        print(name, key, "%.3g of scale" % err)
        assert err <= C.TOL, (key, err)


def seeded_module(T, mask_kind, dropout=0.1):
    from uninext_amd.modules import BiMultiHeadAttention
    torch.manual_seed(T)
    a = BiMultiHeadAttention(32, 48, 4 * 256, 4, dropout=dropout, cfg=C.vlfuse_cfg(32, 48, 4 * 256)).to(DEV).eval()
    with torch.no_grad():
        a.v_proj.weight.mul_(12.0)
        a.l_proj.weight.mul_(12.0)
    gen = torch.Generator().manual_seed(T + 1)
    v = torch.randn(2, 777, 32, generator=gen).to(DEV)
    l = torch.randn(2, T, 48, generator=gen).to(DEV)
    return a, v, l, make_mask(mask_kind, 2, T, gen)


@pytest.mark.parametrize("T,mask_kind", [(1, "none"), (16, "i64"), (100, "f32"), (256, "full")])
def test_fused_route_against_the_torch_route(T, mask_kind, fused_on, calls):
    a, v, l, m = seeded_module(T, mask_kind)
    with torch.no_grad():
        got = a(v, l, attention_mask_l=m)
        assert calls["fused"] == 1
        fused_on.fused_core = False
        want = a(v, l, attention_mask_l=m)
        assert calls["fused"] == 1
    for g, w in zip(got, want):
        assert C.rel_err(g, w) <= C.TOL


def test_fallbacks_on_the_gpu(fused_on, calls):
    a, v, l, m = seeded_module(16, "i64")
    with torch.no_grad():
        a(v, l, attention_mask_l=m.bool())                   # bool mask
        a(v, torch.cat([l] * 20, dim=1), attention_mask_l=None)   # T = 320
        a(v.transpose(0, 1).contiguous().transpose(0, 1), l, attention_mask_l=m)   # not contiguous
        a.train()
        a(v, l, attention_mask_l=m)                          # dropout active
        a.eval()
    assert calls["fused"] == 0
    out_v, out_l = a(v, l, attention_mask_l=m)               # autograd records: PyTorch path, gradients flow
    assert calls["fused"] == 0
    (out_v.sum() + out_l.sum()).backward()
    assert a.v_proj.weight.grad is not None and float(a.values_l_proj.weight.grad.abs().max()) > 0
    with torch.no_grad():
        a(v, l, attention_mask_l=m)
    assert calls["fused"] == 1


def test_peak_memory_at_full_size(fused_on):
    """Peak allocation of BiMultiHeadAttention.forward above its inputs and outputs: the fused route never holds anything of
    the size of one [B * heads, S, T] fp32 tensor (364 MB) besides the projections it is handed."""
    from uninext_amd.modules import BiMultiHeadAttention
    B, H, S, T = 2, 8, 22223, 256
    torch.manual_seed(3)
    a = BiMultiHeadAttention(256, 768, H * 256, H, cfg=C.vlfuse_cfg(256, 768, H * 256)).to(DEV).eval()
    v = torch.randn(B, S, 256, device=DEV)
    l = torch.randn(B, T, 768, device=DEV)
    m = torch.ones(B, T, dtype=torch.int64, device=DEV)
    matrix = B * H * S * T * 4
    peaks = {}
    for route in (True, False):
        fused_on.fused_core = route
        with torch.no_grad():
            # the four projections ([B, S | T, 2048]) are the core's inputs, the two [B, S | T, 2048] tensors its outputs
            q, k, vv, vl = a.v_proj(v), a.l_proj(l), a.values_v_proj(v), a.values_l_proj(l)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            if route:
                from uninext_amd import ext
                out = ext.bi_attention_forward(q, k, vv, vl, m, H, a.scale)
            else:
                out = a._core_torch(q * a.scale, k, vv, vl, m)
            torch.cuda.synchronize()
            peaks[route] = torch.cuda.max_memory_allocated() - base - sum(o.numel() * 4 for o in out)
            del out, q, k, vv, vl
    print("peak above inputs and outputs: fused %.1f MB, PyTorch %.1f MB, one attention matrix %.1f MB"
          % (peaks[True] / 1e6, peaks[False] / 1e6, matrix / 1e6))
    assert peaks[True] < matrix
