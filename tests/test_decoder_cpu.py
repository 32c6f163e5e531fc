"""The decoder modules (uninext_amd/modules/decoder_layer.py) and the C ABI of their self-attention core, without a GPU: the
fixtures of tests/golden/decoder/ against the float64 restatement and against the modules in float64, the state-dict
contract, the routing, and the argument errors of biattn_hip_self_forward_f32."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_cases as C   # noqa: E402
import decoder_ref as R     # noqa: E402

NAMES = sorted(C.FIXTURES)
_cases = {}


def case(name):
    """(cfg, state, inputs, fixture), made once per name and left unchanged."""
    if name not in _cases:
        cfg, state, x = C.make_case(name)
        fx = C.load(name)
        assert C.digest(state) == float(fx["digest"]), "the generator no longer draws the parameters the fixture was minted with"
        for k, v in x.items():
            assert np.array_equal(v.numpy(), fx[k], equal_nan=True), k
        _cases[name] = (cfg, state, x, fx)
    return _cases[name]


def restated(name):
    cfg, st, x, _ = case(name)
    if cfg["kind"] == "layer":
        return (R.layer(st, x["tgt"], x["query_pos"], x["ref"], x["src"], x["shapes"], x["lsi"], x["padding_mask"],
                        x.get("attn_mask"), cfg["heads"]),)
    outs, pts = R.decoder(st, x["tgt"], x["ref"], x["src"], x["shapes"], x["lsi"], x["valid_ratios"], x["padding_mask"], None,
                          cfg["heads"], cfg["layers"], refine=cfg["kind"] == "decoder")
    return (outs, pts) if cfg["kind"] == "decoder" else (outs[-1],)


def wanted(name, fx, twice=False):
    if C.FIXTURES[name]["kind"] == "decoder":
        return (fx["out"], fx["points_twice" if twice else "points"])
    return (fx["out"],)


def test_fixtures_are_the_expected_set_and_small():
    files = sorted(f for f in os.listdir(C.HERE))
    assert files == sorted([n + ".npz" for n in NAMES] + ["state_dict_keys.json"])
    assert all(os.path.getsize(os.path.join(C.HERE, f)) < 500 * 1024 for f in files)
    cfg, _, x, fx = case("layer_dn_mask")
    m = x["attn_mask"]
    assert m.dtype == torch.bool and bool(m[C.DN_PAD:, :C.DN_PAD].all()) and not bool(m.all(1).any())
    f = case("layer_float_mask")[2]["attn_mask"]
    assert bool(torch.isinf(f).any()) and bool(torch.isfinite(f).any())


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_reference(name):
    fx = case(name)[3]
    for got, want in zip(restated(name), wanted(name, fx)):
        assert tuple(got.shape) == want.shape
        assert C.rel_err(got, want) < 1e-12
    if name == "decoder_2layers":
        assert np.array_equal(fx["points"], fx["points_twice"])


@pytest.mark.parametrize("name", NAMES)
def test_modules_float64_match_the_fixtures(name):
    cfg, st, x, fx = case(name)
    variants = [dict(look_forward_twice=False), dict(look_forward_twice=True)] if cfg["kind"] == "decoder" else [{}]
    for kw in variants:
        m = C.build(name, cfg, st, torch.float64, **kw)
        outs = C.run(cfg, m, x)
        for got, want in zip(outs, wanted(name, fx, kw.get("look_forward_twice", False))):
            assert tuple(got.shape) == want.shape
            assert C.rel_err(got, want) < 1e-12
    if cfg["kind"] == "decoder":       # without return_intermediate: the last layer's output and points
        m = C.build(name, cfg, st, torch.float64)
        m.return_intermediate = False
        out, pts = C.run(cfg, m, x)
        assert C.rel_err(out, fx["out"][-1]) < 1e-12 and C.rel_err(pts, fx["points"][-1]) < 1e-12
        m.use_checkpoint = True        # torch.utils.checkpoint around every layer changes nothing
        out2, _ = C.run(cfg, m, x)
        assert torch.equal(out, out2)


def test_helpers_match_their_fixtures():
    from uninext_amd import modules as M
    cfg, st, x, fx = case("decoder_2layers")
    sine = M.get_sine_pos_embed(torch.from_numpy(fx["sine_in"]))
    assert sine.shape == (1, 8, 512) and C.rel_err(sine, fx["sine_out"]) < 1e-12
    assert C.rel_err(R.sine_embed(torch.from_numpy(fx["sine_in"])), fx["sine_out"]) < 1e-12
    head = M.MLP(512, 256, 256, 2).double()
    head.load_state_dict({k[len("ref_point_head."):]: v for k, v in st.items() if k.startswith("ref_point_head.")}, strict=True)
    with torch.no_grad():
        assert C.rel_err(head(sine), fx["mlp_out"]) < 1e-12
    assert C.rel_err(M.inverse_sigmoid(x["ref"]), fx["logit_out"]) < 1e-12
    edge = torch.tensor([-1.0, 0.0, 1e-7, 0.5, 1.0, 2.0], dtype=torch.float64)
    assert torch.equal(M.inverse_sigmoid(edge), R.logit(edge)) and bool(torch.isfinite(M.inverse_sigmoid(edge)).all())
    assert M.get_sine_pos_embed(torch.zeros(2, 3, 2), num_pos_feats=8, exchange_xy=False).shape == (2, 3, 16)


def test_state_dict_keys_shapes_and_strict_load():
    from uninext_amd import modules as M
    rec = C.recorded_keys()
    assert sorted(rec) == ["DeformableReidHead", "DeformableTransformerDecoder", "DeformableTransformerDecoderLayer", "MLP"]
    listing = lambda m: [[k, list(v.shape)] for k, v in m.state_dict().items()]
    built = {}
    for name, cls in (("layer_plain", "DeformableTransformerDecoderLayer"), ("decoder_2layers", "DeformableTransformerDecoder"),
                      ("reid_head", "DeformableReidHead")):
        cfg, st, _, _ = case(name)
        m = built[cls] = C.build(name, cfg, st, torch.float32)          # strict=True inside
        assert listing(m) == rec[cls], cls
        assert list(st) == [k for k, _ in rec[cls]]
    assert listing(built["DeformableTransformerDecoder"].ref_point_head) == rec["MLP"]
    layer = built["DeformableTransformerDecoderLayer"]
    assert isinstance(layer.self_attn, torch.nn.MultiheadAttention) and isinstance(layer.cross_attn, M.MSDeformAttn)
    keys = set(layer.state_dict())
    assert {"self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "cross_attn.value_proj.weight",
            "norm1.weight", "norm2.bias", "norm3.weight", "linear1.weight", "linear2.bias"} <= keys
    dec = M.DeformableTransformerDecoder(256, M.DeformableTransformerDecoderLayer(), 6)
    assert dec.bbox_embed is None and dec.class_embed is None and len(dec.layers) == 6 and dec.layers[0] is not dec.layers[1]
    with pytest.raises(ValueError):
        built["DeformableReidHead"](torch.zeros(1, 2, 256), torch.zeros(1, 2, 2), None, None, None, None)


def test_autograd_never_reaches_the_kernel(monkeypatch):
    from uninext_amd import ext
    from uninext_amd.modules import DeformableTransformerDecoderLayer as Layer
    cfg, st, x, fx = case("layer_plain")

    def boom(*a, **k):
        raise AssertionError("decoder_self_attention called while autograd records")
    monkeypatch.setattr(ext, "decoder_self_attention", boom)
    monkeypatch.setattr(Layer, "fused_self_attn", True)
    m = C.build("layer_plain", cfg, st, torch.float64)
    assert any(p.requires_grad for p in m.parameters())
    with torch.enable_grad():
        assert not m._inference(x["tgt"], x["query_pos"], x["ref"], x["src"])
        out = m(x["tgt"], x["query_pos"], x["ref"], x["src"], x["shapes"], x["lsi"], x["padding_mask"], None)
        out.square().sum().backward()
    assert C.rel_err(out, fx["out"]) < 1e-12
    assert m.self_attn.in_proj_weight.grad is not None and float(m.self_attn.in_proj_weight.grad.abs().max()) > 0
    with torch.no_grad():      # CPU tensors: the composition as well
        assert not m._inference(x["tgt"], x["query_pos"], x["ref"], x["src"])
    m.train()                  # dropout active
    for p in m.parameters():
        p.requires_grad_(False)
    assert not m._inference()


def test_core_restatement_properties():
    qk, v = C.kernel_case(1, 2, 9, 2)
    q, k = qk[..., :64], qk[..., 64:]
    m = torch.zeros(9, 9, dtype=torch.bool)
    m[3] = True
    m[5, :8] = True
    out = R.core(q, k, v, 2, m)
    assert bool(torch.isnan(out[:, 3]).all()) and bool(torch.isfinite(out[:, [0, 1, 2, 4, 5, 6, 7, 8]]).all())
    assert C.rel_err(out[:, 5], v[:, 8].double()) < 1e-12                  # one open key: that key's value row
    f = torch.zeros(9, 9).masked_fill(m, float("-inf"))
    assert torch.equal(torch.nan_to_num(R.core(q, k, v, 2, f)), torch.nan_to_num(out))
    mha = torch.nn.MultiheadAttention(64, 2).double().eval()
    with torch.no_grad():
        w, b = mha.in_proj_weight, mha.in_proj_bias
        x = torch.randn(2, 9, 64, dtype=torch.float64)
        want = mha(x.transpose(0, 1), x.transpose(0, 1), x.transpose(0, 1), attn_mask=m)[0].transpose(0, 1)
        lin = lambda lo, hi: x @ w[lo:hi].t() + b[lo:hi]
        got = R.core(lin(0, 64), lin(64, 128), lin(128, 192), 2, m) @ mha.out_proj.weight.t() + mha.out_proj.bias
    assert bool(torch.isnan(want[:, 3]).all())                             # PyTorch's own answer for an empty row
    keep = [0, 1, 2, 4, 5, 6, 7, 8]
    assert C.rel_err(got[:, keep], want[:, keep]) < 1e-12


def test_supported_predicate_without_a_device():
    from uninext_amd import ext
    q = torch.zeros(1, 4, 64)
    assert not ext.decoder_self_attention_supported(q, q, q, 2, None)      # not on the GPU
    with pytest.raises(RuntimeError):
        ext.decoder_self_attention(q, q, q, 2)


def test_error_codes_without_a_device():
    from uninext_amd import _lib
    lib = _lib.load()
    assert lib.biattn_hip_self_last_kernel() == b""                        # no call of this process has enqueued anything
    assert _lib.last_kernel("dec_attn") == ""
    assert (_lib.BIATTN_MASK_BOOL, _lib.DEC_ATTN_HEAD_DIM) == (3, 32)
    fake = ctypes.c_void_p(1 << 20)      # never dereferenced: every check runs before the device is touched

    def call(mask=None, kind=_lib.BIATTN_MASK_NONE, batch=1, heads=2, length=10, head_dim=32, strides=(64, 64, 64), q=fake):
        return lib.biattn_hip_self_forward_f32(q, fake, fake, strides[0], strides[1], strides[2], mask, kind, batch, heads, length,
                                               head_dim, 0.25, fake, None)
    assert call(head_dim=64) == -5 and "head_dim" in _lib.last_error()
    assert call(mask=fake, kind=1) == -5 and "mask kind" in _lib.last_error()       # BIATTN_MASK_INT64 belongs to the other entry
    assert call(mask=fake, kind=7) == -5
    assert call(mask=None, kind=_lib.BIATTN_MASK_BOOL) == -1
    assert call(mask=None, kind=_lib.BIATTN_MASK_F32) == -1
    assert call(q=None) == -1
    assert call(length=0) == -2 and call(length=65536) == -2 and call(batch=-1) == -2 and call(heads=0) == -2
    assert call(strides=(64, 66, 64)) == -5 and "stride" in _lib.last_error()
    assert call(strides=(128, 128, 60)) == -2                                         # rows would overlap
    assert call(q=ctypes.c_void_p((1 << 20) + 4)) == -5 and "aligned" in _lib.last_error()
    assert call(batch=0) == 0 and call(batch=0, q=None) == 0                          # an empty batch: nothing is looked at
    assert lib.biattn_hip_self_last_kernel() == b""
