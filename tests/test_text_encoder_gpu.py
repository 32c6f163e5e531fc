"""GPU: the text encoder's two kernels (uninext_amd/csrc/bert.hip) per entry against float64, and the module with fused=True
on every fixture of tests/golden/text_encoder/.

The per-entry bound is tests/parity_measure.py's: an entry may miss float64 by max(8 x the fp32 composition's error at the same
entry, 16 u s), s the float64 sum of absolute summands behind the entry.  For the attention core s is tests/attn_parity.py's
(1 + 2 A_i) sum_j p[i, j] |v[j, d]|, A_i the largest summed absolute summands of a kept score of query i: the rounding of a score
reaches the entry through exp (tests/text_encoder_ref.py: attention_core).
For the embedding LayerNorm, out = (x - mean) rstd g + b with x = word + type + position:
s = (|word| + |type| + |position| + mean of that over the row) rstd |g| + |b| -- the rounding of x, the error of the mean (which
every entry carries, however close x is to it) and the relative error of rstd, which multiplies (x - mean) rstd g, all scale with
those terms."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_measure as PM  # noqa: E402
import text_encoder_cases as C  # noqa: E402
import text_encoder_ref as R  # noqa: E402

from uninext_amd import _lib, ext, text_encoder as TE  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEADS, D = 2, 64
E = HEADS * D
LENGTHS = (1, 31, 32, 33, 64, 65, 256, 512)


def prefix_mask(valid, T):
    return (torch.arange(T)[None, :] < torch.as_tensor(valid)[:, None]).long()


def masks_of(T):
    """name -> keep mask (CPU) for B = 2: none; key masks with valid counts {1, 17, 32, 33, T} in batch 0 (batch 1 keeps all), as
    int64, the last also as bool; the identity-among-valid full mask; a random full mask with at least one kept key per row."""
    out = {"none": None}
    for n in sorted({c for c in (1, 17, 32, 33, T) if c <= T}):
        out["key%d" % n] = prefix_mask((n, T), T)
    out["key_bool"] = prefix_mask((T, max(1, T // 2)), T).bool()
    out["identity"] = TE.parallel_det_mask(prefix_mask((T, max(1, (2 * T) // 3)), T))
    g = torch.Generator().manual_seed(T)
    rnd = torch.rand(2, T, T, generator=g) < 0.3
    rnd[:, torch.arange(T), torch.randint(0, T, (T,), generator=g)] = True
    out["random_full"] = rnd
    return out


def core_inputs(T):
    r = PM.rng("text_encoder_core_%d" % T)
    qkv = PM.dy(r.standard_normal((2, T, 3 * E)))
    qkv[..., :2 * E] = PM.dy(qkv[..., :2 * E], 2.0)                   # scores that are far from flat
    assert PM.is_dyadic(qkv)
    return torch.from_numpy(qkv).to(DEV)


def composition(q, k, v, mask):
    """The module's fused=False statements in the inputs' precision."""
    B, T, _ = q.shape
    split = lambda t: t.reshape(B, T, HEADS, D).permute(0, 2, 1, 3)
    s = torch.matmul(split(q), split(k).transpose(-1, -2)) / (D ** 0.5)
    if mask is not None:
        s = s + TE.extended_attention_mask(mask, s.dtype)
    return torch.matmul(torch.softmax(s, -1), split(v)).permute(0, 2, 1, 3).reshape(B, T, E)


@pytest.mark.parametrize("T", LENGTHS)
def test_attention_core_per_entry_parity(T):
    qkv = core_inputs(T)
    q, k, v = qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]
    qc, kc, vc = q.contiguous(), k.contiguous(), v.contiguous()
    for name, mask in masks_of(T).items():
        m = None if mask is None else mask.to(DEV)
        got = ext.bert_self_attention(q, k, v, HEADS, m)               # views of one [B, T, 3 hidden] tensor, read in place
        sep = ext.bert_self_attention(qc, kc, vc, HEADS, m)
        assert torch.equal(got, sep), (T, name)
        assert torch.equal(got, ext.bert_self_attention(q, k, v, HEADS, m)), (T, name)   # repeatable
        kind = "none" if mask is None else "full_u8" if mask.dim() == 3 else "key_i64" if mask.dtype == torch.int64 else "key_u8"
        assert _lib.last_kernel("bert_attn") == "bert_attn<%s>" % kind
        want, mag = R.attention_core(q.double(), k.double(), v.double(), HEADS, m)
        comp = composition(q, k, v, m)
        e = PM.errors(got.double().cpu().numpy(), want.cpu().numpy(), mag.cpu().numpy(), comp.double().cpu().numpy())
        print("T %3d %-12s err %.3e comp %.3e bound %.3e ratio %.3f" % ((T, name) + e.row()))
        e.check(T, name)


def test_identity_mask_returns_the_values_bitwise():
    T = 65
    qkv = core_inputs(T)
    q, k, v = qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]
    valid = (T, 40)
    out = ext.bert_self_attention(q, k, v, HEADS, TE.parallel_det_mask(prefix_mask(valid, T)).to(DEV))
    for b, n in enumerate(valid):
        assert torch.equal(out[b, :n], v[b, :n])                      # the single probability is exp(0) / 1
    assert not torch.equal(out[1, 40:], v[1, 40:]) and torch.isfinite(out).all()


def test_a_row_with_no_kept_key_is_zeros():
    T = 70
    qkv = core_inputs(64)[:, :1].expand(2, T, 3 * E).contiguous() + torch.arange(T, device=DEV)[None, :, None] / 64.0
    q, k, v = qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]
    full = torch.ones(2, T, T, dtype=torch.uint8)
    full[0, 5] = 0
    full[1, 69] = 0
    out = ext.bert_self_attention(q, k, v, HEADS, full.to(DEV))
    assert not torch.isnan(out).any()
    assert not out[0, 5].any() and not out[1, 69].any()
    ref = ext.bert_self_attention(q, k, v, HEADS, None)
    keep = torch.ones(2, T, dtype=torch.bool)
    keep[0, 5] = keep[1, 69] = False
    assert torch.equal(out[keep], ref[keep])                          # the other rows: as without a mask
    key = torch.zeros(2, T, dtype=torch.long)
    key[1, :3] = 1
    out = ext.bert_self_attention(q, k, v, HEADS, key.to(DEV))        # a whole prompt without a kept key
    assert not out[0].any() and out[1].any() and not torch.isnan(out).any()


@pytest.mark.parametrize("hidden", [4, 128, 768, 4096])
@pytest.mark.parametrize("T", [1, 33])
def test_embedding_kernel_per_entry_parity(hidden, T):
    r = PM.rng("text_encoder_embed_%d_%d" % (hidden, T))
    vocab, positions, types, B, eps = 50, 40, 3, 2, 1e-12
    tab = lambda n, s: torch.from_numpy(PM.dy(r.standard_normal((n, hidden)), s)).to(DEV)
    word, pos, typ = tab(vocab, 1.0), tab(positions, 0.5), tab(types, 0.5)
    gamma = torch.from_numpy(PM.dy(1.0 + 0.1 * r.standard_normal(hidden))).to(DEV)
    beta = torch.from_numpy(PM.dy(r.standard_normal(hidden), 0.1)).to(DEV)
    ids = torch.from_numpy(r.randint(0, vocab, (B, T))).to(DEV)
    for tt in (None, torch.from_numpy(r.randint(0, types, (B, T))).to(DEV)):
        got = ext.bert_embed_layernorm(ids, tt, word, pos, typ, gamma, beta, eps)
        assert _lib.last_kernel("bert_embed") == ("bert_embed" if tt is None else "bert_embed<types>")
        assert torch.equal(got, ext.bert_embed_layernorm(ids, tt, word, pos, typ, gamma, beta, eps))
        t_ids = torch.zeros_like(ids) if tt is None else tt
        parts = [word.double()[ids], typ.double()[t_ids], pos.double()[:T][None].expand(B, T, hidden)]
        x = parts[0] + parts[1] + parts[2]
        want = R.layer_norm(x, gamma.double(), beta.double(), eps)
        ax = sum(p.abs() for p in parts)
        rstd = 1.0 / torch.sqrt(((x - x.mean(-1, keepdim=True)) ** 2).mean(-1, keepdim=True) + eps)
        mag = (ax + ax.mean(-1, keepdim=True)) * rstd * gamma.double().abs() + beta.double().abs()
        comp = torch.nn.functional.layer_norm((word[ids] + typ[t_ids]) + pos[:T][None], (hidden,), gamma, beta, eps)
        e = PM.errors(got.double().cpu().numpy(), want.cpu().numpy(), mag.cpu().numpy(), comp.double().cpu().numpy())
        print("hidden %4d T %2d types %-5s err %.3e comp %.3e bound %.3e ratio %.3f" % ((hidden, T, tt is not None) + e.row()))
        e.check(hidden, T, tt is not None)
    if T > 1:                                                         # an id out of range: a NaN row, the neighbours intact
        good = ext.bert_embed_layernorm(ids, None, word, pos, typ, gamma, beta, eps)
        for bad_id, bad_tt in ((vocab, 0), (-1, 0), (1 << 40, 0), (3, types)):
            ids2, tt2 = ids.clone(), torch.zeros_like(ids)
            ids2[1, 7], tt2[1, 7] = bad_id, bad_tt
            out = ext.bert_embed_layernorm(ids2, tt2, word, pos, typ, gamma, beta, eps)
            assert torch.isnan(out[1, 7]).all()
            rest = torch.ones(B, T, dtype=torch.bool)
            rest[1, 7] = False
            assert torch.equal(out[rest], good[rest])


@pytest.mark.parametrize("name", sorted(C.FIXTURES))
def test_module_fused_on_the_fixtures(name):
    fx = C.load(name)
    ids, mask, tt = (None if t is None else t.to(DEV) for t in C.make_inputs(name))
    m = C.build(torch.float32, DEV, fused=True)
    with torch.no_grad():
        out = m(ids, mask, tt)
        again = m(ids, mask, tt)
    assert _lib.last_kernel("bert_attn") == "bert_attn<key_i64>"
    assert _lib.last_kernel("bert_embed") == ("bert_embed" if tt is None else "bert_embed<types>")
    for n, (a, b) in enumerate(zip(out.hidden_states, again.hidden_states)):
        err = C.rel_err(a, fx["hidden_%d" % n])
        print(name, "hidden", n, "rel err %.3e" % err)
        assert err <= C.TOL and torch.equal(a, b)
    enc = TE.BertEncoder(m)
    with torch.no_grad():
        ret = enc({"input_ids": ids, "attention_mask": mask})
    assert ret["masks"] is mask and (tt is not None or torch.equal(ret["hidden"], out.last_hidden_state))


def test_parallel_det_fused_matches_the_restatement():
    ids, mask, _ = C.make_inputs("padded")
    want = R.model(C.state_dict(), C.CONFIG, ids, R.parallel_det_mask(mask))[-1]
    enc = TE.BertEncoder(C.build(torch.float32, DEV, fused=True), parallel_det=True)
    with torch.no_grad():
        ret = enc({"input_ids": ids.to(DEV), "attention_mask": mask.to(DEV)}, task="detection")
    assert _lib.last_kernel("bert_attn") == "bert_attn<full_u8>" and C.rel_err(ret["hidden"], want) <= C.TOL


def test_autograd_takes_the_composition(monkeypatch):
    ids, mask, _ = C.make_inputs("padded")
    ids, mask = ids.to(DEV), mask.to(DEV)
    m = C.build(torch.float32, DEV, fused=True)

    def boom(*a, **k):
        raise AssertionError("a kernel was reached under autograd")
    with torch.no_grad():
        want = m(ids, mask).last_hidden_state
    monkeypatch.setattr(ext, "bert_self_attention", boom)
    monkeypatch.setattr(ext, "bert_embed_layernorm", boom)
    out = m(ids, mask).last_hidden_state                              # parameters require grad and autograd records
    assert out.requires_grad and C.rel_err(out, want.cpu()) <= C.TOL
    x = out.detach().requires_grad_(True)                            # a layer alone, frozen, on an input that requires grad
    layer = m.encoder.layer[0]
    for p in layer.parameters():
        p.requires_grad_(False)
    y = layer(x, mask)
    y.sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    with torch.no_grad(), pytest.raises(AssertionError):
        layer(x, mask)                                                # without autograd the same call does reach the kernel


def test_no_score_matrix_is_allocated():
    B, heads, T = 2, 12, 512
    qkv = torch.randn(B, T, 3 * heads * D, device=DEV)
    Eb = heads * D
    q, k, v = qkv[..., :Eb], qkv[..., Eb:2 * Eb], qkv[..., 2 * Eb:]
    mask = prefix_mask((T, 300), T).to(DEV)
    ext.bert_self_attention(q, k, v, heads, mask)                     # warm: the library is loaded
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = ext.bert_self_attention(q, k, v, heads, mask)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before - out.numel() * 4
    assert extra < B * heads * T * T * 4, extra                       # one [B * heads, T, T] fp32 tensor: 25 MiB
    assert extra < 1 << 20, extra                                     # in fact nothing but the output


def test_refusals_launch_nothing():
    lib = _lib.load()
    T = 16
    x = torch.zeros(1, T, 2 * E, device=DEV)
    out = torch.zeros(1, T, E, device=DEV)
    ext.bert_self_attention(x[..., :E], x[..., :E], x[..., :E], HEADS, None)
    marker = _lib.last_kernel("bert_attn")
    assert marker == "bert_attn<none>"

    def call(head_dim=64, length=T, stride=2 * E, kind=_lib.BERT_MASK_NONE, heads=HEADS):
        rc = lib.bert_hip_self_attention_f32(x.data_ptr(), x.data_ptr(), x.data_ptr(), stride, stride, stride, None, kind, 1, heads,
                                             length, head_dim, 0.125, out.data_ptr(), None)
        return rc, _lib.last_error()
    assert call(head_dim=32, heads=4) == (-5, "bert_attn: head_dim must be 64")
    assert call(length=513) == (-5, "bert_attn: len must be at most 512")
    assert call(stride=2 * E + 2) == (-5, "bert_attn: row strides must be multiples of 4 floats")
    assert call(kind=_lib.BERT_MASK_KEY_U8) == (-1, "bert_attn: null pointer argument")
    torch.cuda.synchronize()
    assert _lib.last_kernel("bert_attn") == marker and not out.any()
    q32 = torch.zeros(1, T, 64, device=DEV)
    assert not ext.bert_self_attention_supported(q32, q32, q32, 2, None)            # head_dim 32
    big = torch.zeros(1, 513, E, device=DEV)
    assert not ext.bert_self_attention_supported(big, big, big, HEADS, None)
    with pytest.raises(RuntimeError, match="unsupported arguments"):
        ext.bert_self_attention(big, big, big, HEADS, None)
