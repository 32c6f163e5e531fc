"""ViT attention core on the GPU (patch_embed_hip_vit_attn_f32) and the modules of uninext_amd/vit.py on it."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vit_cases as C   # noqa: E402
import vit_ref as R     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def gpu(t):
    return None if t is None else t.to(DEV)


def run_kernel(qkv, th, tw, heads, hw, scale):
    from uninext_amd import ext
    out = ext.vit_attention(gpu(qkv), gpu(th), gpu(tw), heads, hw, scale)
    torch.cuda.synchronize()
    return out


def check(qkv, th, tw, heads, hw, scale, tol=C.TOL):
    want = R.core(qkv, th, tw, heads, hw, scale)
    got = run_kernel(qkv, th, tw, heads, hw, scale)
    assert torch.isfinite(got).all()
    err = C.rel_err(got, want)
    print("B %d heads %d hw %s D %d: err %.2e" % (qkv.shape[0], heads, hw, qkv.shape[2] // (3 * heads), err))
    assert err < tol, err
    return got, want


@pytest.mark.parametrize("D", [64, 80])
@pytest.mark.parametrize("hw", C.SHAPES)
def test_kernel_matches_the_restatement(hw, D):
    from uninext_amd import _lib
    B, heads = (1, 2) if hw == (37, 61) else (2, 2)
    qkv, th, tw, scale = C.random_case(7, B, heads, hw, D)
    _, want = check(qkv, th, tw, heads, hw, scale)
    assert _lib.last_kernel("vit_attn") == "vit_rel<%d>+vit_attn<%d,rel>" % (D, D)
    if hw[0] != hw[1]:   # distinct tables: a transposed lookup gives another answer, far outside the bound
        th2, tw2 = R.resize_table(tw, 2 * hw[0] - 1), R.resize_table(th, 2 * hw[1] - 1)
        swapped = R.core(qkv, th2, tw2, heads, hw, scale)
        assert C.rel_err(swapped, want) > 100 * C.TOL


@pytest.mark.parametrize("D", [64, 80])
def test_tables_null_and_zero(D):
    from uninext_amd import _lib
    hw = (9, 15)
    qkv, th, tw, scale = C.random_case(8, 1, 1, hw, D)                       # B' * heads = 1
    got_none, _ = check(qkv, None, None, 1, hw, scale)
    assert _lib.last_kernel("vit_attn") == "vit_attn<%d>" % D
    got_zero, _ = check(qkv, torch.zeros_like(th), torch.zeros_like(tw), 1, hw, scale)
    assert C.rel_err(got_zero, got_none.cpu()) < 1e-6
    qkv, th, tw, scale = C.random_case(9, 7, 1, (3, 5), D)                   # B' * heads = 7
    check(qkv, th, tw, 1, (3, 5), scale)
    qkv, th, tw, scale = C.random_case(9, 1, 7, (14, 14), D)
    check(qkv, th, tw, 7, (14, 14), scale)


@pytest.mark.parametrize("D", [64, 80])
def test_late_maximum_flat_and_large_scores(D):
    hw, heads = (9, 15), 2
    S = hw[0] * hw[1]
    # late maximum: q = e0; k[:, 0] = 8 on key 0, 40 on the last key, 0 elsewhere: every row's largest score sits in the last key
    # tile, the second largest (far below) in the first; the accumulator is rescaled by exp(-32 scale ...) on the way
    t = torch.zeros(1, S, 3, heads, D)
    t[:, :, 0, :, 0] = 4.0
    t[:, 0, 1, :, 0] = 8.0
    t[:, S - 1, 1, :, 0] = 40.0
    t[:, :, 2] = torch.randn(1, S, heads, D, generator=torch.Generator().manual_seed(3))
    qkv = t.reshape(1, S, -1)
    got, want = check(qkv, None, None, heads, hw, 0.125)
    assert C.rel_err(got, t[:, S - 1:S, 2].reshape(1, 1, -1).expand(1, S, -1)) < 1e-3      # nearly one-hot on the last key
    # flat: all scores equal, the output is the mean of v
    t[:, :, 1] = 0.0
    got, _ = check(t.reshape(1, S, -1), None, None, heads, hw, 0.125)
    assert C.rel_err(got, t[:, :, 2].mean(dim=1, keepdim=True).reshape(1, 1, -1).expand(1, S, -1)) < 1e-5
    # scores of +-1e4: finite and within the bound
    t[:, :, 0] = 0.0
    t[:, :, 0, :, 0] = 100.0
    t[:, :, 1, :, 0] = (torch.randint(0, 2, (1, S, heads), generator=torch.Generator().manual_seed(4)) * 2 - 1).float() * 100.0
    qkv = t.reshape(1, S, -1)
    assert float(R.scores(qkv, None, None, heads, hw, 1.0).abs().max()) == 1e4
    check(qkv, None, None, heads, hw, 1.0)


@pytest.mark.parametrize("D,hw", [(64, (9, 15)), (80, (14, 14))])
def test_exact_family(D, hw):
    qkv, th, tw, scale = R.exact_case(5, 2, 2, hw, D)
    check(qkv, th, tw, 2, hw, scale, tol=C.TOL_EXACT)


def test_bitwise_repeatable_across_runs_and_streams():
    from uninext_amd import ext
    hw = (20, 23)
    qkv, th, tw, scale = C.random_case(11, 2, 2, hw, 80)
    qkv, th, tw = gpu(qkv), gpu(th), gpu(tw)
    a = ext.vit_attention(qkv, th, tw, 2, hw, scale)
    b = ext.vit_attention(qkv, th, tw, 2, hw, scale)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = ext.vit_attention(qkv, th, tw, 2, hw, scale)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)
    assert ext.vit_attention(qkv[:0], th, tw, 2, hw, scale).shape == (0, 460, 160)       # an empty batch


@pytest.mark.parametrize("name", C.EXPECTED)
def test_modules_fp32_match_the_fixtures(name):
    from uninext_amd import _lib, ext, vit
    fx = C.load(name)
    m = C.module_from(name, fx, torch.float32, DEV)
    x = torch.from_numpy(fx["x"]).float().to(DEV)
    old = vit.Attention.fused_core
    try:
        for fused in (False, True):
            vit.Attention.fused_core = fused
            D = m.state_dict()[[k for k in fx["keys"] if k.endswith("rel_pos_h")][0]].shape[1]
            other = 144 - D                                                  # a call of the other head size: last_kernel must change
            ext.vit_attention(torch.zeros(1, 1, 3 * other, device=DEV), None, None, 1, (1, 1), 1.0)
            assert _lib.last_kernel("vit_attn") == "vit_attn<%d>" % other
            out, _, core_out = C.run_with_core(m, x)
            torch.cuda.synchronize()
            outs = out if isinstance(out, dict) else {"out": out}
            for k in outs:
                err = C.rel_err(C.stored_view(fx, k, outs[k]), fx[k])
                print(name, "fused" if fused else "torch", k, "%.2e" % err)
                assert err < C.TOL, (k, fused, err)
            assert C.rel_err(C.stored_view(fx, "core_out", core_out), fx["core_out"]) < C.TOL
            want_kernel = "vit_rel<%d>+vit_attn<%d,rel>" % (D, D) if fused else "vit_attn<%d>" % other
            assert _lib.last_kernel("vit_attn") == want_kernel
    finally:
        vit.Attention.fused_core = old


@pytest.mark.parametrize("name", ["attn_win_d80", "block_win_padded", "attn_global_interp"])
def test_fused_route_runs_the_hip_kernel(name):
    """The windowed, the padded and the interpolating case: with fused_core on, the core's output is the kernel's, bitwise."""
    from uninext_amd import ext, vit
    fx = C.load(name)
    m = C.module_from(name, fx, torch.float32, DEV)
    x = torch.from_numpy(fx["x"]).float().to(DEV)
    old = vit.Attention.fused_core
    try:
        vit.Attention.fused_core = True
        _, core_in, core_out = C.run_with_core(m, x)
        a = C.first_attention(m)
        S = core_in.shape[1]
        hw = (14, 14) if S == 196 else (17, 20)
        assert a._use_hip(torch.empty(1, hw[0], hw[1], a.qkv.in_features, device=DEV)) is False      # parameters require grad
        with torch.no_grad():
            assert a._use_hip(torch.empty(1, hw[0], hw[1], a.qkv.in_features, device=DEV))
            th, tw = a._resized_tables(*hw)
            assert th.shape[0] == 2 * hw[0] - 1 and tw.shape[0] == 2 * hw[1] - 1
            direct = ext.vit_attention(core_in.contiguous(), th, tw, a.num_heads, hw, a.scale)
        assert torch.equal(direct, core_out)
        vit.Attention.fused_core = False
        _, _, core_torch = C.run_with_core(m, x)
        assert C.rel_err(core_torch, core_out.cpu()) < C.TOL
    finally:
        vit.Attention.fused_core = old


def test_autograd_takes_the_torch_route_with_equal_gradients():
    from uninext_amd import vit
    fx = C.load("block_win_padded")
    x0 = torch.from_numpy(fx["x"]).float().to(DEV)
    old = vit.Attention.fused_core
    grads = []
    try:
        for fused in (True, False):
            vit.Attention.fused_core = fused
            m = C.module_from("block_win_padded", fx, torch.float32, DEV)
            x = x0.clone().requires_grad_(True)
            assert not m.attn._use_hip(torch.empty(4, 14, 14, 128, device=DEV))
            m(x).square().sum().backward()
            grads.append([x.grad.clone()] + [p.grad.clone() for p in m.parameters()])
    finally:
        vit.Attention.fused_core = old
    assert len(grads[0]) == len(grads[1]) > 10
    for g_on, g_off in zip(*grads):
        assert torch.equal(g_on, g_off) and float(g_on.abs().max()) > 0
