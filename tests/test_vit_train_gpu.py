"""The ViT attention core's training route on the GPU (patch_embed_hip_vit_attn_train_f32, patch_embed_hip_vit_attn_backward_f32)
and the modules of uninext_amd/vit.py on it (Attention.own_training)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vit_cases as C          # noqa: E402
import vit_ref as R            # noqa: E402
import vit_train_cases as T    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def gpu(t):
    return None if t is None else t.to(DEV)


def run_kernels(qkv, th, tw, heads, hw, scale, G):
    """{"dq", "dk", "dv"[, "dth", "dtw"]} of the two entries, and (out, lse)."""
    from uninext_amd import ext
    q, h, w = gpu(qkv), gpu(th), gpu(tw)
    out, lse = ext.vit_attention_train(q, h, w, heads, hw, scale)
    gq, gh, gw = ext.vit_attention_backward(q, h, w, out, lse, gpu(G), heads, hw, scale)
    torch.cuda.synchronize()
    dq, dk, dv = T.split_qkv_grad(gq, heads)
    got = {"dq": dq, "dk": dk, "dv": dv}
    if th is not None:
        got.update(dth=gh, dtw=gw)
    return got, out, lse


def check(case, hw, G, want, comp=None, tol=C.TOL, label=""):
    """Every group separately: max abs error <= tol of that group's max abs.  Prints each figure (and the ratio to the fp32
    composition's own error) before it asserts."""
    qkv, th, tw, scale = case
    heads = want["dq"].shape[2]
    got, out, lse = run_kernels(qkv, th, tw, heads, hw, scale, G)
    errs = T.group_err(got, want)
    cerr = T.group_err(comp, want) if comp is not None else {}
    for k in want:
        assert torch.isfinite(got[k]).all(), k
        ratio = errs[k] / cerr[k] if cerr.get(k) else float("nan")
        print("%s %-3s err %.2e  composition %.2e  ratio %.1f" % (label, k, errs[k], cerr.get(k, float("nan")), ratio))
    for k in want:
        assert errs[k] <= tol, (k, errs[k])
    return got, out, lse


@pytest.mark.parametrize("D", [64, 80])
@pytest.mark.parametrize("hw", T.SHAPES)
def test_backward_matches_float64_autograd(hw, D):
    from uninext_amd import _lib
    B, heads = (1, 1) if hw == (37, 61) else (2, 2)
    case, G, want, comp, _ = T.random_reference(7, B, heads, hw, D)
    check(case, hw, G, want, comp, label="hw %s D %d" % (hw, D))
    assert _lib.last_kernel("vit_attn_bwd") == "vit_rel<%d>+vit_bwd_q<%d,rel>+vit_bwd_kv<%d,rel>+vit_bwd_tables<%d>" % (D, D, D, D)
    if hw[0] != hw[1]:   # distinct tables: a transposed lookup gives other gradients, far outside the bound
        qkv, th, tw, scale = case
        th2, tw2 = R.resize_table(tw, 2 * hw[0] - 1), R.resize_table(th, 2 * hw[1] - 1)
        swapped, _ = T.reference_grads(qkv, th2, tw2, heads, hw, scale, G)
        for k in ("dq", "dk", "dv"):
            assert C.rel_err(swapped[k], want[k]) > 100 * C.TOL, k


@pytest.mark.parametrize("D", [64, 80])
@pytest.mark.parametrize("hw", [(2, 100), (1, 256), (2, 256)])
def test_wide_grids_take_the_large_lds_opt_in(hw, D):
    """q_w above 78 (D = 80) / 94 (D = 64): the width bins of the query pass and its two tiles need more than 64 KiB of LDS, which
    the launcher opts into; q_w = 256 is the route's limit (about 150 KiB at D = 80).  All five groups against float64, and a
    bitwise repeat."""
    from uninext_amd import _lib, ext
    assert 4 * hw[1] * 32 * 4 + 2 * 32 * (D + 4 if D == 64 else 100) * 4 > 64 * 1024
    case, G, want, comp, _ = T.random_reference(17, 1, 2, hw, D)
    got, out, lse = check(case, hw, G, want, comp, label="wide hw %s D %d" % (hw, D))
    assert _lib.last_kernel("vit_attn_bwd") == "vit_rel<%d>+vit_bwd_q<%d,rel>+vit_bwd_kv<%d,rel>+vit_bwd_tables<%d>" % (D, D, D, D)
    qkv, th, tw, scale = case
    again = ext.vit_attention_backward(gpu(qkv), gpu(th), gpu(tw), out, lse, gpu(G), 2, hw, scale)
    torch.cuda.synchronize()
    dq, dk, dv = T.split_qkv_grad(again[0], 2)
    for k, t in (("dq", dq), ("dk", dk), ("dv", dv), ("dth", again[1]), ("dtw", again[2])):
        assert torch.equal(t, got[k]), k


@pytest.mark.parametrize("D", [64, 80])
def test_tables_none_zero_and_the_reduction_over_images_and_heads(D):
    from uninext_amd import _lib
    hw = (9, 15)
    case, G, want, comp, _ = T.random_reference(8, 1, 1, hw, D, rel=False)            # B' * heads = 1, no tables
    got_none, _, _ = check(case, hw, G, want, comp, label="none D %d" % D)
    assert _lib.last_kernel("vit_attn_bwd") == "vit_bwd_q<%d>+vit_bwd_kv<%d>" % (D, D)
    qkv, _, _, scale = case
    zh, zw = torch.zeros(2 * hw[0] - 1, D), torch.zeros(2 * hw[1] - 1, D)
    want_zero, _ = T.reference_grads(qkv, zh, zw, 1, hw, scale, G)
    assert float(want_zero["dth"].abs().max()) > 0 and float(want_zero["dtw"].abs().max()) > 0
    got_zero, _, _ = check((qkv, zh, zw, scale), hw, G, want_zero, label="zero D %d" % D)
    for k in ("dq", "dk", "dv"):
        assert C.rel_err(got_zero[k], got_none[k].cpu()) < 1e-6, k
    for B, heads, shape in ((7, 1, (3, 5)), (1, 7, (14, 14))):                         # B' * heads = 7
        case, G, want, comp, _ = T.random_reference(9, B, heads, shape, D)
        check(case, shape, G, want, comp, label="B %d heads %d D %d" % (B, heads, D))


@pytest.mark.parametrize("D", [64, 80])
def test_late_maximum_flat_and_large_scores_give_finite_gradients(D):
    hw, heads = (9, 15), 2
    S = hw[0] * hw[1]
    G = T.upstream(3, 1, S, heads * D)
    t = torch.zeros(1, S, 3, heads, D)
    t[:, :, 0, :, 0] = 4.0
    t[:, 0, 1, :, 0] = 8.0
    t[:, S - 1, 1, :, 0] = 40.0
    t[:, :, 2] = torch.randn(1, S, heads, D, generator=torch.Generator().manual_seed(3))
    cases = [(t.reshape(1, S, -1).clone(), 0.125)]                      # late maximum
    t[:, :, 1] = 0.0
    cases.append((t.reshape(1, S, -1).clone(), 0.125))                  # flat
    t[:, :, 0] = 0.0
    t[:, :, 0, :, 0] = 100.0
    t[:, :, 1, :, 0] = (torch.randint(0, 2, (1, S, heads), generator=torch.Generator().manual_seed(4)) * 2 - 1).float() * 100.0
    cases.append((t.reshape(1, S, -1).clone(), 1.0))                    # scores of +-1e4
    for qkv, scale in cases:
        got, out, lse = run_kernels(qkv, None, None, heads, hw, scale, G)
        want, _ = T.reference_grads(qkv, None, None, heads, hw, scale, G)
        for k in want:
            print(k, "%.2e" % (C.rel_err(got[k], want[k]) if float(want[k].abs().max()) > 0 else 0.0))
            assert torch.isfinite(got[k]).all(), k
        assert torch.isfinite(lse).all() and torch.isfinite(out).all()


@pytest.mark.parametrize("D,hw", [(64, (9, 15)), (80, (14, 14))])
def test_exact_family(D, hw):
    qkv, th, tw, scale = R.exact_case(5, 2, 2, hw, D)
    G = T.upstream(5, 2, hw[0] * hw[1], 2 * D)
    want, _ = T.reference_grads(qkv, th, tw, 2, hw, scale, G)
    check((qkv, th, tw, scale), hw, G, want, T.composition_grads(qkv, th, tw, 2, hw, scale, G), label="exact D %d" % D)


@pytest.mark.parametrize("D,hw,rel", [(64, (9, 15), True), (80, (14, 14), True), (80, (20, 23), False), (64, (1, 1), True)])
def test_training_forward_is_the_inference_forward_plus_lse(D, hw, rel):
    from uninext_amd import ext
    qkv, th, tw, scale = C.random_case(12, 2, 2, hw, D, rel=rel)
    out, lse = ext.vit_attention_train(gpu(qkv), gpu(th), gpu(tw), 2, hw, scale)
    assert torch.equal(out, ext.vit_attention(gpu(qkv), gpu(th), gpu(tw), 2, hw, scale))
    S = hw[0] * hw[1]
    want = torch.logsumexp(R.scores(qkv, th, tw, 2, hw, scale), dim=-1).reshape(4, S)
    assert lse.shape == (4, (S + 31) // 32 * 32) and torch.isfinite(lse).all()
    err = C.rel_err(lse[:, :S], want)
    print("lse err %.2e" % err)
    assert err < 1e-6


def own_training(flag):
    from uninext_amd import vit

    class Scope:
        def __enter__(self):
            self.old = vit.Attention.own_training
            vit.Attention.own_training = flag

        def __exit__(self, *exc):
            vit.Attention.own_training = self.old
    return Scope()


@pytest.mark.parametrize("name", T.EXPECTED)
def test_modules_on_the_own_route_match_the_fixtures(name):
    from uninext_amd import _lib
    fx = T.load(name)
    m = T.module_from(name, fx, torch.float32, DEV)
    D = m.state_dict()[[k for k in fx["keys"] if k.endswith("rel_pos_h")][0]].shape[1]
    with own_training(True):
        got = T.gradients(m, fx, torch.float32, DEV)
    torch.cuda.synchronize()
    assert _lib.last_kernel("vit_attn_bwd") == "vit_rel<%d>+vit_bwd_q<%d,rel>+vit_bwd_kv<%d,rel>+vit_bwd_tables<%d>" % (D, D, D, D)
    assert sorted(got) == sorted(fx["grad"])
    for k, want in fx["grad"].items():
        err = C.rel_err(T.stored_view(fx, k, got[k]), want)
        print(name, k, "%.2e" % err)
        assert float(want.abs().max()) > 0, k
        assert err <= C.TOL, (k, err)


def test_flag_off_is_the_torch_route_bitwise():
    """own_training off (the default): ViTAttentionFunction is never entered, and the gradients are those of the PyTorch
    composition written out by hand."""
    from uninext_amd import vit
    fx = T.load("attn_win_d80_grad")
    m = T.module_from("attn_win_d80_grad", fx, torch.float32, DEV)
    assert vit.Attention.own_training is False
    entered = []
    old = vit.ViTAttentionFunction.apply
    vit.ViTAttentionFunction.apply = lambda *a: entered.append(1) or old(*a)
    try:
        got = T.gradients(m, fx, torch.float32, DEV)
        assert not entered
        with own_training(True):
            T.gradients(m, fx, torch.float32, DEV)
        assert entered
    finally:
        vit.ViTAttentionFunction.apply = old
    x = torch.from_numpy(fx["x"]).float().to(DEV).requires_grad_(True)
    for p in m.parameters():
        p.grad = None
    B, H, W, _ = x.shape
    T.loss_of(m.proj(m._core_torch(m.qkv(x).reshape(B, H * W, -1), H, W).view(B, H, W, -1)), fx, DEV).backward()
    assert torch.equal(got["x"], x.grad)
    for n, p in m.named_parameters():
        assert torch.equal(got[n], p.grad), n


def test_checkpointing_gives_the_same_bits():
    """ViT(use_act_checkpoint=True) against the same net without, route on: bitwise for the outputs, the input's gradient and
    every parameter's but two.  pos_embed (through the bicubic resize) and fpn1.0.weight (transposed convolution) get their
    gradients from PyTorch's own backward kernels, which add with atomics: the test shows that what those two kernels are GIVEN
    is bitwise the same in both runs -- res4, which is fpn1's input (the last block's map); the gradient that arrives at the
    patch embedding's output, which is the resize's incoming gradient; the upstream gradient is the fixture's -- and holds
    their results to 1e-5 of their scale.  res3 is the output of the same transposed convolution, whose forward is PyTorch's
    too and differs between two runs on a bitwise equal input; it is held to 1e-5 as well (the loss is linear in the outputs,
    so no gradient depends on it)."""
    from uninext_amd import vit
    fx = T.load("net_small_grad")
    x = torch.from_numpy(fx["x"]).float().to(DEV)
    runs = []
    for ckpt in (False, True):
        m = T.module_from("net_small_grad", fx, torch.float32, DEV)
        m.use_act_checkpoint = ckpt
        m.set_own_training(True)
        assert all(b.attn.own_training for b in m.blocks) and m.patch_embed.own_exact_training and not vit.Attention.own_training
        seen = {}
        hook = m.patch_embed.register_forward_hook(lambda mod, i, o: o.register_hook(lambda g: seen.__setitem__("tokens", g.clone())) and None)
        xi = x.clone().requires_grad_(True)
        out = m(xi)
        T.loss_of(out, fx, DEV).backward()
        hook.remove()
        grads = dict([("x", xi.grad), ("grad at the patch embedding's output", seen["tokens"])] + [(n, p.grad) for n, p in m.named_parameters()])
        runs.append(({k: v.detach() for k, v in out.items()}, grads))
    (out_a, a), (out_b, b) = runs
    assert sorted(out_a) == ["res3", "res4", "res5"]
    assert torch.equal(out_a["res4"], out_b["res4"]) and torch.equal(out_a["res5"], out_b["res5"])
    assert C.rel_err(out_a["res3"], out_b["res3"].cpu()) < 1e-5
    assert len(a) > 50 and sorted(a) == sorted(b)
    for n in a:
        assert float(a[n].abs().max()) > 0, n
        if n in ("pos_embed", "fpn1.0.weight"):
            assert C.rel_err(a[n], b[n].cpu()) < 1e-5, n
        else:
            assert torch.equal(a[n], b[n]), n


def test_repeatable_staged_and_empty():
    from uninext_amd import ext
    hw, heads, D = (20, 23), 2, 80
    qkv, th, tw, scale = C.random_case(11, 2, heads, hw, D)
    qkv, th, tw = gpu(qkv), gpu(th), gpu(tw)
    S, E = hw[0] * hw[1], heads * D
    G = gpu(T.upstream(11, 2, S, E))
    out, lse = ext.vit_attention_train(qkv, th, tw, heads, hw, scale)
    a = ext.vit_attention_backward(qkv, th, tw, out, lse, G, heads, hw, scale)
    b = ext.vit_attention_backward(qkv, th, tw, out, lse, G, heads, hw, scale)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = ext.vit_attention_backward(qkv, th, tw, out, lse, G, heads, hw, scale)
    side.synchronize()
    torch.cuda.synchronize()
    flat = torch.zeros(G.numel() + 1, device=DEV)
    flat[1:] = G.reshape(-1)
    misaligned = flat[1:].view_as(G)                                           # 4 bytes off a 16-byte boundary
    strided = G.transpose(0, 1).contiguous().transpose(0, 1)                   # the same values, not contiguous
    assert misaligned.data_ptr() % 16 != 0 and not strided.is_contiguous()
    d = ext.vit_attention_backward(qkv, th, tw, out, lse, misaligned, heads, hw, scale)
    e = ext.vit_attention_backward(qkv, th, tw, out, lse, strided, heads, hw, scale)
    for other in (b, c, d, e):
        for x, y in zip(a, other):
            assert torch.equal(x, y)
    out0, lse0 = ext.vit_attention_train(qkv[:0], th, tw, heads, hw, scale)
    g = ext.vit_attention_backward(qkv[:0], th, tw, out0, lse0, G[:0], heads, hw, scale)
    assert g[0].shape == (0, S, 3 * E) and g[1].shape == th.shape and float(g[1].abs().max()) == 0 and float(g[2].abs().max()) == 0


def test_peak_memory_stays_below_one_score_matrix():
    from uninext_amd import vit
    hw, B, heads, D = (37, 61), 1, 2, 64
    S = hw[0] * hw[1]
    qkv, th, tw, scale = C.random_case(13, B, heads, hw, D)
    qkv, th, tw = gpu(qkv).requires_grad_(True), gpu(th).requires_grad_(True), gpu(tw).requires_grad_(True)
    G = gpu(T.upstream(13, B, S, heads * D))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = vit.ViTAttentionFunction.apply(qkv, th, tw, heads, hw, scale)
    (out * G).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("peak %.1f MB, one score matrix %.1f MB" % (peak / 1e6, B * heads * S * S * 4 / 1e6))
    assert qkv.grad is not None and th.grad is not None
    assert peak < B * heads * S * S * 4
