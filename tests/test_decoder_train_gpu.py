"""The decoder self-attention core's training route on the GPU (biattn_hip_self_train_f32, biattn_hip_self_backward_f32) and the
modules of uninext_amd/modules/decoder_layer.py on it (DeformableTransformerDecoderLayer.own_training)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_cases as C          # noqa: E402
import decoder_train_cases as T    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME = {None: "dec_bwd_q<none>+dec_bwd_kv<none>", torch.bool: "dec_bwd_q<bool>+dec_bwd_kv<bool>",
        torch.float32: "dec_bwd_q<f32>+dec_bwd_kv<f32>"}
# lengths and what each is the smallest to reach (tiles of 32, 32 owned tokens per workgroup, two streamed ranges per workgroup)
LENS = [1,      # one key, one query
        31,     # a tail in the only tile; the second wave is idle
        32,     # exactly one tile
        33,     # a tail of 1 in the second tile and the second workgroup; one tile per wave
        63, 64,  # two tiles, with and without a tail
        65,     # three tiles: ranges of 2 and 1
        97]     # four tiles, two per wave; more than one workgroup per (b, h)


def gpu(t):
    return None if t is None else t.to(DEV)


def run_kernels(qk, v, heads, mask, G, scale=None):
    """({"dq", "dk", "dv"}, out, lse) of the two entries; q and k are the halves of qk on the device, and dq | dk come back in
    one [B, L, 2 E] buffer."""
    from uninext_amd import _lib, ext
    qk_d, v_d, m_d = gpu(qk), gpu(v), gpu(mask)
    E = v.shape[-1]
    q, k = qk_d[..., :E], qk_d[..., E:]
    out, lse = ext.decoder_self_attention_train(q, k, v_d, heads, m_d, scale)
    grads = ext.decoder_self_attention_backward(q, k, v_d, out, lse, gpu(G), heads, m_d, scale)
    torch.cuda.synchronize()
    assert _lib.last_kernel("dec_attn_bwd") == NAME[None if mask is None else mask.dtype]
    if qk.shape[0] * qk.shape[1] > 1:
        assert len(grads) == 2 and grads[0].shape == qk.shape and grads[0].is_contiguous()
        return {"dq": grads[0][..., :E], "dk": grads[0][..., E:], "dv": grads[1]}, out, lse
    return {"dq": grads[0], "dk": grads[1], "dv": grads[2]}, out, lse        # a single row: no row stride to tell the halves by


def check(qk, v, heads, mask, G, want, comp=None, label="", tol=C.TOL):
    """Every group separately: max abs error <= tol of that group's max abs, every entry.  Prints each figure (and the ratio to
    the fp32 composition's own error) before it asserts."""
    got, out, lse = run_kernels(qk, v, heads, mask, G)
    errs = T.group_err(got, want)
    cerr = T.group_err(comp, want) if comp is not None else {}
    for k in T.GROUPS:
        ratio = errs[k] / cerr[k] if cerr.get(k) else float("nan")
        print("%s %-3s err %.2e  composition %.2e  ratio %.1f" % (label, k, errs[k], cerr.get(k, float("nan")), ratio))
    for k in T.GROUPS:
        assert torch.isfinite(got[k]).all(), k
        assert errs[k] <= tol, (k, errs[k])
    return got, out, lse


@pytest.mark.parametrize("kind", ["none", "bool", "float"])
@pytest.mark.parametrize("L", LENS)
def test_backward_matches_float64_at_tile_and_wave_split_edges(L, kind):
    qk, v, mask, G, want, comp, _ = T.random_reference(20 + L, 2, L, 2, kind)
    check(qk, v, 2, mask, G, want, comp, label="L %d %s" % (L, kind))


@pytest.mark.parametrize("kind", ["none", "bool", "float"])
@pytest.mark.parametrize("B,heads", [(1, 1), (7, 1), (1, 7)])
def test_batch_and_head_counts(B, heads, kind):
    qk, v, mask, G, want, comp, _ = T.random_reference(40 + B, B, 33, heads, kind)
    check(qk, v, heads, mask, G, want, comp, label="B %d heads %d %s" % (B, heads, kind))


def test_wholly_excluded_tiles_bool_and_inf_masks_give_the_same_bits():
    """dn_mask(64 + 37, 64, 2): the matching queries (from 64 on) see no key of the first two tiles, and each group's 32 queries
    skip the other group's tile -- in the query pass as key tiles, in the key pass as query tiles."""
    L = 64 + 37
    mask = C.dn_mask(L, 64, 2)
    assert bool(mask[64:, :64].all()) and bool(mask[:32, 32:64].all()) and bool(mask[32:64, :32].all()) and not bool(mask.all(1).any())
    qk, v = C.kernel_case(61, 2, L, 2)
    G = T.upstream(61, 2, L, 64)
    want, _ = T.reference_grads(qk, v, 2, mask, G)
    comp = T.composition_grads(qk, v, 2, mask, G)
    got_b, out_b, lse_b = check(qk, v, 2, mask, G, want, comp, label="dn bool")
    fmask = torch.zeros(L, L).masked_fill(mask, float("-inf"))
    got_f, out_f, lse_f = check(qk, v, 2, fmask, G, want, comp, label="dn -inf")
    assert torch.equal(out_b, out_f) and torch.equal(lse_b, lse_f)
    for k in T.GROUPS:
        assert torch.equal(got_b[k], got_f[k]), k


@pytest.mark.parametrize("kind", ["bool", "float"])
def test_a_query_with_every_key_excluded(kind):
    L, dead = 40, 17
    qk, v = C.kernel_case(62, 2, L, 2)
    G = T.upstream(62, 2, L, 64)
    mask = T.mask_of(kind, 62, L)
    mask[dead] = True if kind == "bool" else float("-inf")
    want, _ = T.reference_grads(qk, v, 2, mask, G, dead=(dead,))
    got, out, lse = run_kernels(qk, v, 2, mask, G)
    keep = [i for i in range(L) if i != dead]
    assert torch.isnan(out[:, dead]).all() and torch.isnan(got["dq"][:, dead]).all()
    assert torch.isfinite(out[:, keep]).all() and torch.isfinite(got["dq"][:, keep]).all()
    assert torch.isfinite(got["dk"]).all() and torch.isfinite(got["dv"]).all()
    assert bool((lse.view(4, -1)[:, dead] == float("-inf")).all())
    got["dq"], want["dq"] = got["dq"][:, keep], want["dq"][:, keep]
    errs = T.group_err(got, want)
    print("dead row", kind, errs)
    for k in T.GROUPS:
        assert errs[k] <= C.TOL, (k, errs[k])


def test_late_maximum_flat_and_large_scores_give_finite_gradients():
    L, heads = 97, 2
    G = T.upstream(3, 1, L, heads * 32)
    q = torch.zeros(1, L, heads, 32)
    k = torch.zeros(1, L, heads, 32)
    q[..., 0] = 4.0
    k[:, 0, :, 0] = 8.0
    k[:, L - 1, :, 0] = 40.0
    v = torch.randn(1, L, heads * 32, generator=torch.Generator().manual_seed(3))
    pack = lambda: torch.cat([q.reshape(1, L, -1), k.reshape(1, L, -1)], -1).clone()
    cases = [(pack(), 0.125)]                                            # late maximum: the last key of the second range
    k[:] = 0.0
    cases.append((pack(), 0.125))                                        # flat
    q[:] = 0.0
    q[..., 0] = 100.0
    k[..., 0] = (torch.randint(0, 2, (1, L, heads), generator=torch.Generator().manual_seed(4)) * 2 - 1).float() * 100.0
    cases.append((pack(), 1.0))                                          # scores of +-1e4
    for qk, scale in cases:
        got, out, lse = run_kernels(qk, v, heads, None, G, scale)
        want, _ = T.reference_grads(qk, v, heads, None, G, scale)
        for key in T.GROUPS:
            print(key, "%.2e" % (C.rel_err(got[key], want[key]) if float(want[key].abs().max()) > 0 else 0.0))
            assert torch.isfinite(got[key]).all(), key
        assert torch.isfinite(lse).all() and torch.isfinite(out).all()


@pytest.mark.parametrize("kind", ["none", "bool", "float"])
@pytest.mark.parametrize("L", [1, 33, 97])
def test_training_forward_is_the_inference_forward_plus_lse(L, kind):
    from uninext_amd import ext
    qk, v, mask, _, _, _, _ = T.random_reference(20 + L, 2, L, 2, kind)
    qk_d, v_d, m_d = gpu(qk), gpu(v), gpu(mask)
    q, k = qk_d[..., :64], qk_d[..., 64:]
    out, lse = ext.decoder_self_attention_train(q, k, v_d, 2, m_d)
    assert torch.equal(out, ext.decoder_self_attention(q, k, v_d, 2, m_d))
    split = lambda t: t.double().reshape(2, L, 2, 32).permute(0, 2, 1, 3)
    s = split((qk[..., :64] * 32 ** -0.5)) @ split(qk[..., 64:]).transpose(-1, -2)
    if mask is not None:
        s = s.masked_fill(mask, float("-inf")) if mask.dtype == torch.bool else s + mask.double()
    want = torch.logsumexp(s, dim=-1).reshape(4, L)
    assert lse.shape == (4, (L + 31) // 32 * 32) and torch.isfinite(lse).all()
    err = C.rel_err(lse[:, :L], want)
    print("lse err %.2e" % err)
    assert err < 1e-6


def test_repeatable_staged_and_empty():
    from uninext_amd import ext
    L, heads = 97, 2
    qk, v, mask, G, _, _, _ = T.random_reference(20 + L, 2, L, heads, "bool")
    qk, v, mask, G = gpu(qk), gpu(v), gpu(mask), gpu(G)
    E = heads * 32
    q, k = qk[..., :E], qk[..., E:]
    out, lse = ext.decoder_self_attention_train(q, k, v, heads, mask)
    back = lambda g: ext.decoder_self_attention_backward(q, k, v, out, lse, g, heads, mask)
    a, b = back(G), back(G)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = back(G)
    side.synchronize()
    torch.cuda.synchronize()
    flat = torch.zeros(G.numel() + 1, device=DEV)
    flat[1:] = G.reshape(-1)
    misaligned = flat[1:].view_as(G)                                           # 4 bytes off a 16-byte boundary
    strided = G.transpose(0, 1).contiguous().transpose(0, 1)                   # the same values, not contiguous
    assert misaligned.data_ptr() % 16 != 0 and not strided.is_contiguous()
    d, e = back(misaligned), back(strided)
    sep = ext.decoder_self_attention_backward(q.contiguous(), k.contiguous(), v, out, lse, G, heads, mask)   # three tensors
    assert len(a) == 2 and len(sep) == 3
    for other in (b, c, d, e, (torch.cat(sep[:2], -1), sep[2])):
        for x, y in zip(a, other):
            assert torch.equal(x, y)
    out0, lse0 = ext.decoder_self_attention_train(q[:0], k[:0], v[:0], heads, mask)
    g0 = ext.decoder_self_attention_backward(q[:0], k[:0], v[:0], out0, lse0, G[:0], heads, mask)
    assert out0.shape == (0, L, E) and all(t.shape[0] == 0 and t.shape[1] == L for t in g0)


def build(name, cfg, state, **args):
    if cfg["kind"] == "decoder":
        args.setdefault("look_forward_twice", True)
    return C.build(name, cfg, state, torch.float32, DEV, **args)


def own(m, flag=True):
    for mod in m.modules():
        if hasattr(mod, "fused_self_attn"):
            mod.own_training = flag
    return m


@pytest.mark.parametrize("name", T.EXPECTED)
def test_modules_on_the_own_route_match_the_fixtures(name):
    from uninext_amd import _lib
    from uninext_amd.modules import decoder_layer as D
    cfg, state, x = C.make_case(name)
    fx = T.load(name)
    m = build(name, cfg, state)
    m = m.set_own_training(True) if cfg["kind"] == "decoder" else own(m)
    entered = []
    old = D.DecoderSelfAttentionFunction.apply
    D.DecoderSelfAttentionFunction.apply = lambda *a: entered.append(1) or old(*a)
    try:
        got, _ = T.gradients(cfg, m, x, fx["G"], torch.float32, DEV)
    finally:
        D.DecoderSelfAttentionFunction.apply = old
    torch.cuda.synchronize()
    assert len(entered) == cfg["layers"]
    assert _lib.last_kernel("dec_attn_bwd") == NAME[{None: None, "dn": torch.bool, "float": torch.float32}[cfg["mask"]]]
    assert sorted(got) == sorted(fx["grad"])
    for k, want in fx["grad"].items():
        err = C.rel_err(T.stored_view(fx, k, got[k]), want)
        print(name, k, "%.2e" % err)
        assert float(want.abs().max()) > 0, k
        assert err <= C.TOL, (k, err)


def through_grad_value(n):
    """Gradients that pass through grad_value of the deformable cross-attention's backward, which adds with float atomics and is
    not deterministic (include/msda_hip.h), with the route on or off: `src` and the value projection's parameters."""
    return n == "src" or "cross_attn.value_proj." in n


def test_flag_off_is_the_torch_route_bitwise():
    """own_training off (the default): DecoderSelfAttentionFunction is never entered, and the gradients are bitwise those of the
    reference's composition written out by hand -- but for through_grad_value's three, held to 1e-5 of their scale."""
    from uninext_amd.modules import decoder_layer as D
    name = "layer_dn_mask"
    cfg, state, x = C.make_case(name)
    G = T.fixture_upstream(name)
    m = build(name, cfg, state)
    assert D.DeformableTransformerDecoderLayer.own_training is False and not m.own_training
    entered = []
    old = D.DecoderSelfAttentionFunction.apply
    D.DecoderSelfAttentionFunction.apply = lambda *a: entered.append(1) or old(*a)
    try:
        got, _ = T.gradients(cfg, m, x, G, torch.float32, DEV)
        got = {k: v.clone() for k, v in got.items()}
        assert not entered
        own(m)
        T.gradients(cfg, m, x, G, torch.float32, DEV)
        assert entered
        own(m, False)
    finally:
        D.DecoderSelfAttentionFunction.apply = old
    leaves = {k: x[k].float().to(DEV).requires_grad_(True) for k in T.INPUT_KEYS["layer"]}
    for p in m.parameters():
        p.grad = None
    tgt, pos = leaves["tgt"], leaves["query_pos"]
    qk = (tgt + pos).transpose(0, 1)
    tgt2 = m.self_attn(qk, qk, tgt.transpose(0, 1), attn_mask=x["attn_mask"].to(DEV))[0].transpose(0, 1)
    t = m.norm2(tgt + m.dropout2(tgt2))
    t2 = m.cross_attn(t + pos, leaves["ref"], leaves["src"], x["shapes"].to(DEV), x["lsi"].to(DEV), x["padding_mask"].to(DEV))
    t = m.norm1(t + m.dropout1(t2))
    out = m.norm3(t + m.dropout4(m.linear2(m.dropout3(F.relu(m.linear1(t))))))
    (out * G[0].float().to(DEV)).sum().backward()
    for n, g in [(k, leaf.grad) for k, leaf in leaves.items()] + [(n, p.grad) for n, p in m.named_parameters()]:
        if through_grad_value(n):
            assert C.rel_err(got[n], g.cpu()) < 1e-5, n
        else:
            assert torch.equal(got[n], g), n


def test_checkpointing_gives_the_same_bits():
    """DeformableTransformerDecoder(use_checkpoint=True) against the same decoder without, route on.  Bitwise: both outputs (the
    segment's pass without autograd takes the training route too, DeformableTransformerDecoderLayer._checkpointed), and every
    gradient of the last layer and of the box heads.  The named exceptions, held to 1e-5 of their scale:
      * through_grad_value's: `src` and each layer's cross_attn.value_proj parameters (float atomics, different between any two
        runs);
      * everything upstream of the boundary between the two layers -- layers.0.*, ref_point_head.*, `tgt`, `ref`.  Layer 0's
        output has five consumers (the stack, the box head, and the next layer's residual, q | k and v inputs).  Without
        checkpointing autograd adds the five gradients one by one; with it the next layer's three are summed inside the
        recomputed segment first.  The same five fp32 numbers in another association: PyTorch's accumulation, not a kernel's."""
    name = "decoder_2layers"
    cfg, state, x = C.make_case(name)
    G = T.fixture_upstream(name)
    runs = []
    for ckpt in (False, True):
        m = build(name, cfg, state, use_checkpoint=ckpt).set_own_training(True)
        got, outs = T.gradients(cfg, m, x, G, torch.float32, DEV)
        runs.append((outs, {k: v.clone() for k, v in got.items()}))
    (out_a, a), (out_b, b) = runs
    for x_a, x_b in zip(out_a, out_b):
        assert torch.equal(x_a, x_b)
    assert sorted(a) == sorted(b) and len(a) > 60
    upstream = lambda n: n in ("tgt", "ref") or n.startswith("layers.0.") or n.startswith("ref_point_head.")
    print("not bitwise:", [n for n in a if not torch.equal(a[n], b[n])])
    bitwise = 0
    for n in a:
        assert float(a[n].abs().max()) > 0, n
        if through_grad_value(n) or upstream(n):
            assert C.rel_err(a[n], b[n].cpu()) < 1e-5, n
        else:
            assert torch.equal(a[n], b[n]), n
            bitwise += 1
    assert bitwise == 20 + 12          # the last layer's parameters but value_proj's two, and the two box heads


def test_peak_memory_stays_below_one_score_matrix():
    from uninext_amd.modules import DecoderSelfAttentionFunction
    B, heads, L = 1, 2, 1100
    qk, v = C.kernel_case(13, B, L, heads)
    qk, v = gpu(qk).requires_grad_(True), gpu(v).requires_grad_(True)
    mask = gpu(C.dn_mask(L, 200, 5))
    G = gpu(T.upstream(13, B, L, heads * 32))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = DecoderSelfAttentionFunction.apply(qk, v, heads, mask)
    (out * G).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("peak %.1f MB, one score matrix %.1f MB" % (peak / 1e6, B * heads * L * L * 4 / 1e6))
    assert qk.grad is not None and v.grad is not None and torch.isfinite(qk.grad).all()
    assert peak < B * heads * L * L * 4
