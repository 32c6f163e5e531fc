"""GPU: the training route of the text encoder's attention core (uninext_amd/csrc/bert_attn_bwd.hip: attn_train, bwd_q, bwd_kv,
dropout_keep) against tests/text_encoder_train_cases.py's float64 core, and BertModel.set_own_training on the small config
against the gradient fixtures of tests/golden/text_encoder_train/.

Every parity figure is max abs error over the group's max abs against float64, bound text_encoder_cases.TOL = 1e-4 (the project's
fp32 bound); each is printed with its ratio to the fp32 composition's own error before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_measure as PM  # noqa: E402
import text_encoder_cases as C  # noqa: E402
import text_encoder_train_cases as TC  # noqa: E402

from uninext_amd import _lib, ext, text_encoder as TE  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEADS, D = 2, 64
KINDS = ("none", "key_i64", "key_u8", "full_u8")
LENGTHS = (1, 31, 32, 33, 63, 64, 65, 97)
OUTPUTS = ("out", "dq", "dk", "dv")


def make(B, T, heads=HEADS, name=""):
    """qkv [B, T, 3 E] and grad_out [B, T, E] on the device: dyadics, q and k doubled so that the scores are far from flat"""
    E = heads * D
    r = PM.rng("text_encoder_train_%d_%d_%d_%s" % (B, T, heads, name))
    qkv = PM.dy(r.standard_normal((B, T, 3 * E)))
    qkv[..., :2 * E] = PM.dy(qkv[..., :2 * E], 2.0)
    g = PM.dy(r.standard_normal((B, T, E)))
    assert PM.is_dyadic(qkv) and PM.is_dyadic(g)
    return torch.from_numpy(qkv).to(DEV), torch.from_numpy(g).to(DEV)


def mask_of(kind, B, T, valid):
    """The keep mask (CPU) of a kind: batch 0 keeps its first `valid` keys, the others all; the full kind also drops a random
    70 % of the (query, key) pairs but keeps at least one of every query's first `valid` keys."""
    if kind == "none":
        return None
    n = torch.full((B,), T)
    n[0] = valid
    key = torch.arange(T)[None, :] < n[:, None]
    if kind == "key_i64":
        return key.long()
    if kind == "key_u8":
        return key
    g = torch.Generator().manual_seed(1000 * T + valid)
    full = torch.rand(B, T, T, generator=g) < 0.3
    full[torch.arange(B)[:, None], torch.arange(T)[None, :], (torch.rand(B, T, generator=g) * n[:, None]).long()] = True
    return full & key[:, None, :]


def thirds(qkv):
    E = qkv.shape[-1] // 3
    return qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]


def run(qkv, g, mask, p=0.0, seed=None, heads=HEADS, separate=False):
    """The two entry points on the thirds of qkv (or on contiguous copies): out, lse, dq, dk, dv"""
    q, k, v = (t.contiguous() for t in thirds(qkv)) if separate else thirds(qkv)
    m = None if mask is None else mask.to(DEV)
    out, lse = ext.bert_self_attention_train(q, k, v, heads, m, dropout_p=p, seed=seed)
    grad = ext.bert_self_attention_backward(q, k, v, out, lse, g, heads, m, dropout_p=p, seed=seed)
    assert torch.is_tensor(grad) != separate or qkv.shape[1] == 1
    dq, dk, dv = thirds(grad) if torch.is_tensor(grad) else grad
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv)


def check(who, got, qkv, g, mask, keep=None, p=0.0, heads=HEADS):
    """out, lse, dq, dk, dv within TOL of the float64 core; the figures are printed first."""
    T = qkv.shape[1]
    want = TC.core(*thirds(qkv), heads, mask, g, keep, p)
    comp = TC.core(*thirds(qkv), heads, mask, g, keep, p, dt=torch.float32)
    worst = TC.report(who, TC.group_errors(got, want, comp, OUTPUTS))
    lse, wl = got["lse"].cpu().double(), want["lse"]
    dead = torch.isinf(wl)
    assert torch.equal(torch.isinf(lse[:, :T]) & (lse[:, :T] < 0), dead) and not lse[:, T:].any()
    lerr = float((lse[:, :T][~dead] - wl[~dead]).abs().max() / wl[~dead].abs().max()) if (~dead).any() else 0.0
    print("%-44s %-8s err %.3e" % (who, "lse", lerr))
    assert all(torch.isfinite(got[n]).all() for n in OUTPUTS)
    assert worst <= TC.TOL and lerr <= TC.TOL, (who, worst, lerr)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", LENGTHS)
def test_kernel_parity_against_float64(T, kind):
    qkv, g = make(2, T)
    valids = (1, 31, 32, 33, 97) if T == 97 else (max(1, (T + 1) // 2),)
    for valid in valids[:1] if kind == "none" else valids:            # without a mask the valid count changes nothing
        mask = mask_of(kind, 2, T, valid)
        got = run(qkv, g, mask)
        assert _lib.last_kernel("bert_attn_train") == "bert_attn_train<%s>" % kind
        assert _lib.last_kernel("bert_attn_bwd") == "bert_bwd_q<%s>+bert_bwd_kv<%s>" % (kind, kind)
        check("T %d %s valid %d" % (T, kind, valid), got, qkv, g, mask)
        if kind.startswith("key"):                                    # padding keys: dk = dv = 0 exactly
            assert not got["dk"][0, valid:].any() and not got["dv"][0, valid:].any()


@pytest.mark.parametrize("B,heads", [(1, 1), (7, 1), (1, 7)])
def test_batch_and_head_counts(B, heads):
    qkv, g = make(B, 33, heads)
    for kind in ("key_i64", "full_u8"):
        mask = mask_of(kind, B, 33, 20)
        check("B %d heads %d %s" % (B, heads, kind), run(qkv, g, mask, heads=heads), qkv, g, mask, heads=heads)


@pytest.mark.parametrize("T", [33, 97])
def test_strided_views_and_one_buffer_give_the_same_bits(T):
    qkv, g = make(2, T)
    seed = torch.from_numpy(TC.seed_of("strided")).to(DEV)
    for kind, p in (("none", 0.0), ("key_i64", 0.0), ("full_u8", 0.25)):
        mask = mask_of(kind, 2, T, 20)
        a = run(qkv, g, mask, p, seed if p else None)
        b = run(qkv, g, mask, p, seed if p else None, separate=True)
        assert a["dq"].stride(1) == 3 * HEADS * D and b["dq"].is_contiguous()     # one [B, T, 3 E] buffer against three tensors
        assert all(torch.equal(a[n], b[n]) for n in a), (T, kind)
        wide = torch.zeros(2, T, 2 * HEADS * D, device=DEV)                       # a grad_out that has to be staged
        wide[..., :HEADS * D] = g
        c = run(qkv, wide[..., :HEADS * D], mask, p, seed if p else None)
        assert all(torch.equal(a[n], c[n]) for n in a), (T, kind)


def test_results_with_dropout_off():
    T = 70
    qkv, g = make(2, T)
    for kind in KINDS:
        mask = mask_of(kind, 2, T, 37)
        m = None if mask is None else mask.to(DEV)
        got = run(qkv, g, mask)
        assert torch.equal(got["out"], ext.bert_self_attention(*thirds(qkv), HEADS, m)), kind   # bitwise the inference kernel's
        assert got["lse"].shape == (2 * HEADS, 96) and not got["lse"][:, T:].any()              # 0 on the rows past len
        assert torch.isfinite(got["lse"][:, :T]).all()
    key = torch.zeros(2, T, dtype=torch.long)
    key[1, :3] = 1                                                    # a whole prompt without a kept key
    got = run(qkv, g, key)
    assert (got["lse"][:HEADS, :T] == -float("inf")).all() and torch.isfinite(got["lse"][HEADS:, :T]).all()
    assert not any(got[n][0].any() for n in OUTPUTS) and all(torch.isfinite(got[n]).all() for n in OUTPUTS)
    assert not got["dk"][1, 3:].any() and not got["dv"][1, 3:].any() and got["dk"][1, :3].any()


def test_a_query_that_keeps_no_key():
    T = 70
    qkv, g = make(2, T)
    full = torch.ones(2, T, T, dtype=torch.uint8)
    full[0, 5] = 0
    full[1, 69] = 0
    got = run(qkv, g, full)
    rows = ((0, 5), (1, 69))
    for b, i in rows:
        assert not got["out"][b, i].any() and not got["dq"][b, i].any()
        assert (got["lse"].view(2, HEADS, -1)[b, :, i] == -float("inf")).all()
    assert all(torch.isfinite(got[n]).all() for n in OUTPUTS)
    g0 = g.clone()
    for b, i in rows:
        g0[b, i] = 0
    zeroed = run(qkv, g0, full)
    assert torch.equal(got["dk"], zeroed["dk"]) and torch.equal(got["dv"], zeroed["dv"])   # it contributes exactly nothing
    check("zero rows", got, qkv, g, full)


@pytest.mark.parametrize("T", [1, 33, 97, 129])
def test_dropout_export_equals_the_mirror(T):
    for p in (0.1, 0.5):
        seed = TC.seed_of("export_%d" % T)
        got = ext.bert_dropout_keep(torch.from_numpy(seed).to(DEV), p, 2, HEADS, T)
        assert got.dtype == torch.uint8 and got.shape == (2 * HEADS, T, T)
        assert np.array_equal(got.cpu().numpy(), TC.keep_matrix(seed, p, 2 * HEADS, T).astype(np.uint8))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_parity_on_the_exported_mask(p):
    for T, kind in ((33, "key_i64"), (97, "none"), (97, "key_u8"), (97, "full_u8")):
        qkv, g = make(2, T)
        seed = torch.from_numpy(TC.seed_of("parity_%d_%s" % (T, kind))).to(DEV)
        mask = mask_of(kind, 2, T, 33)
        got = run(qkv, g, mask, p, seed)
        assert _lib.last_kernel("bert_attn_train") == "bert_attn_train<%s,drop>" % kind
        assert _lib.last_kernel("bert_attn_bwd") == "bert_bwd_q<%s,drop>+bert_bwd_kv<%s,drop>" % (kind, kind)
        keep = ext.bert_dropout_keep(seed, p, 2, HEADS, T).cpu().numpy()
        check("p %.1f T %d %s" % (p, T, kind), got, qkv, g, mask, keep, p)


def test_dropout_bits_p0_repeats_streams_and_seeds():
    T = 97
    qkv, g = make(2, T)
    mask = mask_of("key_i64", 2, T, 50)
    seed = torch.from_numpy(TC.seed_of("bits")).to(DEV)
    plain = run(qkv, g, mask)
    with_seed = run(qkv, g, mask, 0.0, seed)                          # p = 0 with a seed: the no-dropout bits
    assert all(torch.equal(plain[n], with_seed[n]) for n in plain)
    a = run(qkv, g, mask, 0.1, seed)
    b = run(qkv, g, mask, 0.1, seed)
    assert all(torch.equal(a[n], b[n]) for n in a) and not torch.equal(a["out"], plain["out"])
    assert torch.equal(a["lse"], plain["lse"])                        # the statistics run over all kept keys
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        c = run(qkv, g, mask, 0.1, seed)
    stream.synchronize()
    assert all(torch.equal(a[n], c[n]) for n in a)
    other = run(qkv, g, mask, 0.1, torch.from_numpy(TC.seed_of("other bits")).to(DEV))
    assert not torch.equal(a["out"], other["out"]) and not torch.equal(a["dv"], other["dv"])


def test_rejected_calls_leave_the_outputs_untouched():
    lib = _lib.load()
    T, E = 16, HEADS * D
    qkv, g = make(1, T)
    q, k, v = thirds(qkv)
    out, lse = ext.bert_self_attention_train(q, k, v, HEADS, None)
    marker = (_lib.last_kernel("bert_attn_train"), _lib.last_kernel("bert_attn_bwd"))
    seed = torch.from_numpy(TC.seed_of("rejected")).to(DEV)
    poison = lambda *shape: torch.full(shape, 7.0, device=DEV)
    o2, l2, grads, ws = poison(1, T, E), poison(HEADS, 32), poison(1, T, 3 * E), poison(256)
    need = lib.bert_hip_self_attention_backward_workspace_bytes(1, HEADS, T, D)

    def train(p=0.0, sd=None, head_dim=D, length=T, stride=3 * E):
        return lib.bert_hip_self_attention_train_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), stride, stride, stride, None, 0, 1, HEADS,
                                                     length, head_dim, 0.125, o2.data_ptr(), l2.data_ptr(), p, sd, None)

    def bwd(p=0.0, sd=None, ws_bytes=need, gstride=3 * E, batch=1):
        dq, dk, dv = thirds(grads)
        return lib.bert_hip_self_attention_backward_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), 3 * E, 3 * E, 3 * E, None, 0,
                                                        out.data_ptr(), lse.data_ptr(), g.data_ptr(), batch, HEADS, T, D, 0.125,
                                                        dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), gstride, gstride, gstride,
                                                        ws.data_ptr(), ws_bytes, p, sd, None)
    assert [train(p=1.0, sd=seed.data_ptr()), train(p=-0.1, sd=seed.data_ptr()), train(p=float("nan"), sd=seed.data_ptr())] == [-2] * 3
    assert train(p=0.1) == -1 and train(head_dim=32) == -5 and train(length=513) == -5 and train(stride=3 * E + 2) == -5
    assert bwd(p=1.0, sd=seed.data_ptr()) == -2 and bwd(p=0.1) == -1 and bwd(gstride=E - 4) == -2
    assert bwd(ws_bytes=need - 1) == _lib.BERT_ERR_WORKSPACE
    assert bwd(batch=0) == 0                                          # an empty batch returns 0 and enqueues nothing
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (o2, l2, grads, ws))
    assert marker == (_lib.last_kernel("bert_attn_train"), _lib.last_kernel("bert_attn_bwd"))
    empty = torch.zeros(0, T, 3 * E, device=DEV)
    o, l = ext.bert_self_attention_train(*thirds(empty), HEADS, None)
    assert o.shape == (0, T, E) and l.shape == (0, 32)
    with pytest.raises(RuntimeError, match="needs a seed"):
        ext.bert_self_attention_train(q, k, v, HEADS, None, dropout_p=0.1)
    with pytest.raises(RuntimeError, match="unsupported arguments"):
        ext.bert_self_attention_train(q, k, v, HEADS, None, dropout_p=1.0, seed=seed)


# ---- the module, small config, train() ---------------------------------------------------------------------------------------
def build_train(attention_p, hidden_p=0.0):
    m = C.build(torch.float32, DEV, fused=True).train()
    for mod in m.modules():
        if isinstance(mod, nn.Dropout):
            mod.p = hidden_p
    for layer in m.encoder.layer:
        layer.attention.self.dropout.p = attention_p
    return m


def check_params(who, grads, want, fixture=None):
    worst = 0.0
    for k in grads:
        ref = fixture if fixture is not None and k in fixture else want
        err = TC.param_err(k, grads[k], ref)
        print("%-14s %-58s err %.3e (%s)" % (who, k, err, "fixture" if ref is fixture else "float64"))
        worst = max(worst, err)
    assert worst <= TC.TOL, (who, worst)


@pytest.mark.parametrize("name", sorted(TC.FIXTURES))
def test_module_own_training_matches_the_fixtures(name):
    fx = TC.load(name)
    m = build_train(0.0).set_own_training(True)
    hidden, grads, gemb = TC.module_grads(m, name, torch.float32, DEV)
    kind = "full_u8" if TC.FIXTURES[name][1] else "key_i64"
    assert _lib.last_kernel("bert_attn_bwd") == "bert_bwd_q<%s>+bert_bwd_kv<%s>" % (kind, kind)       # the route ran
    assert _lib.last_kernel("bert_attn_train") == "bert_attn_train<%s>" % kind
    ids, _, core_mask = TC.fixture_inputs(name)
    _, want, _ = TC.model_grads(ids, core_mask, TC.loss_weights())
    errs = (C.rel_err(hidden, fx["hidden"]), C.rel_err(gemb, fx["grad_embeddings_output"]))
    print(name, "hidden err %.3e  grad of the embeddings' output err %.3e" % errs)
    assert max(errs) <= TC.TOL
    check_params(name, grads, want, {k[5:]: fx[k] for k in fx if k.startswith("grad/")})


def test_module_own_dropout_matches_float64_on_the_exported_masks(monkeypatch):
    m = build_train(0.1).set_own_training(True, dropout=True)
    seeds, real = [], ext.bi_attention_seed

    def recording(device):
        seeds.append(real(device))
        return seeds[-1]
    monkeypatch.setattr(ext, "bi_attention_seed", recording)
    hidden, grads, gemb = TC.module_grads(m, "padded", torch.float32, DEV)
    assert len(seeds) == C.CONFIG["num_hidden_layers"]               # one draw per layer and forward
    assert _lib.last_kernel("bert_attn_bwd") == "bert_bwd_q<key_i64,drop>+bert_bwd_kv<key_i64,drop>"
    heads = C.CONFIG["num_attention_heads"]
    keeps = [ext.bert_dropout_keep(s, 0.1, C.B, heads, C.T).cpu().numpy() for s in seeds]
    assert not np.array_equal(keeps[0], keeps[1]) and 0.85 < keeps[0].mean() < 0.95
    ids, _, core_mask = TC.fixture_inputs("padded")
    hid64, want, gemb64 = TC.model_grads(ids, core_mask, TC.loss_weights(), keeps=keeps, p=0.1)
    errs = (C.rel_err(hidden, hid64[-1]), C.rel_err(gemb, gemb64))
    print("dropout: hidden err %.3e  grad of the embeddings' output err %.3e" % errs)
    assert max(errs) <= TC.TOL
    check_params("dropout", grads, want)


def test_routes_outside_the_opt_in_are_unchanged(monkeypatch):
    ids, mask, _ = TC.fixture_inputs("padded")
    ids, mask = ids.to(DEV), mask.to(DEV)
    m = build_train(0.1, 0.1).eval()
    with torch.no_grad():
        base = m(ids, mask).hidden_states                             # today's inference route
    kernel = _lib.last_kernel("bert_attn")
    m.train()
    torch.manual_seed(3)
    comp = m(ids, mask).last_hidden_state                             # today's training route: the composition

    def boom(*a, **k):
        raise AssertionError("the training kernels were reached")
    monkeypatch.setattr(ext, "bert_self_attention_train", boom)
    m.set_own_training(True)                                          # own_training alone, attention dropout active
    m.zero_grad(set_to_none=True)
    torch.manual_seed(3)
    out = m(ids, mask).last_hidden_state
    out.sum().backward()                                              # and so does its backward
    assert torch.equal(out, comp) and m.encoder.layer[0].attention.self.query.weight.grad is not None
    m.set_own_training(True, dropout=True)
    with pytest.raises(AssertionError, match="training kernels"):
        m(ids, mask)                                                  # with own_dropout the same call does take the route
    with torch.no_grad():                                             # no-grad in train(): the composition, as before
        torch.manual_seed(3)
        assert torch.equal(m(ids, mask).last_hidden_state, comp)
    m.eval()
    with torch.no_grad():
        again = m(ids, mask).hidden_states
    assert all(torch.equal(a, b) for a, b in zip(again, base)) and _lib.last_kernel("bert_attn") == kernel
    with pytest.raises(AssertionError, match="training kernels"):
        m(ids, mask)                                                  # eval under autograd with the flag on: the route (no dropout)
    assert not TE.BertSelfAttention.own_training
