"""Early vision-language fusion (uninext_amd/modules/vl_fusion.py, include/biattn_hip.h): everything that needs no GPU."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vlfuse_cases as C   # noqa: E402
import vlfuse_ref as R     # noqa: E402


def keep_rows(fx, t):
    """Drop the images whose tokens are all masked (image-side tensors only)."""
    bad = C.fully_masked_images(fx)
    return t[[b for b in range(t.shape[0]) if b not in bad]]


def test_fixtures_load():
    assert C.NAMES == C.EXPECTED
    for name in C.NAMES:
        fx = C.load(name)
        B, S, _ = fx["visual"].shape
        T = fx["hidden"].shape[1]
        E = fx["state"]["attn.v_proj.weight"].shape[0]
        assert E == int(fx["num_heads"]) * 256
        assert fx["core_out_v"].shape == (B, S, E) and fx["core_out_l"].shape == (B, T, E)
        assert float(fx["score_absmax"]) < 500.0
        assert os.path.getsize(os.path.join(C.HERE, name + ".npz")) < 1 << 20
    assert C.fully_masked_images(C.load("t37_fullmask")) == [1]


@pytest.mark.parametrize("name", C.EXPECTED)
def test_restatement_matches_the_reference(name):
    """tests/vlfuse_ref.py against the reference-minted core outputs.  An image whose tokens are all masked is left out of the
    image side: the float64 reference adds -9e15 to the scores and keeps their differences, fp32 (and the restatement) land on
    the constant and give the mean of vl over all T tokens, which is asserted instead."""
    fx = C.load(name)
    q, k, vv, vl, m, H, scale = C.core_inputs(fx, torch.float64)
    out_v, out_l = R.core(q, k, vv, vl, m, H, scale)
    assert C.rel_err(out_l, torch.from_numpy(fx["core_out_l"])) < 1e-6          # stored rounded to float32
    assert C.rel_err(keep_rows(fx, out_v), keep_rows(fx, torch.from_numpy(fx["core_out_v"]))) < 1e-6
    for b in C.fully_masked_images(fx):
        mean = vl[b].mean(dim=0, keepdim=True).expand_as(out_v[b])
        assert float((out_v[b] - mean).abs().max()) < 1e-12


@pytest.mark.parametrize("name", C.EXPECTED)
def test_torch_path_float64_matches_the_fixtures(name):
    fx = C.load(name)
    blk = C.block_from(fx, torch.float64)
    v, l, m = C.inputs(fx, torch.float64)
    with torch.no_grad():
        out_v, out_l = blk(v, l, m, None)
        nv, nl = blk.layer_norm_v(v), blk.layer_norm_l(l)
        a_v, a_l = blk.attn(nv, nl, attention_mask_l=m)
        fused = C.vlfuse_from(fx, torch.float64)({"visual": v, "lang": {"hidden": l, "masks": m}})
    for got, key in ((out_v, "out_visual"), (out_l, "out_hidden"), (a_v, "attn_out_v"), (a_l, "attn_out_l"),
                     (fused["visual"], "out_visual"), (fused["lang"]["hidden"], "out_hidden")):
        assert C.rel_err(got, torch.from_numpy(fx[key])) < 1e-10, key     # same ops in float64, fully masked image included


@pytest.mark.parametrize("name", C.EXPECTED)
def test_torch_path_fp32_precondition(name):
    """The reference's op sequence in fp32 is itself inside 3e-5 of scale on every fixture: room for another summation order
    under the 1e-4 bound.  (On a fully masked image fp32 differs from float64 by design; it is compared with the restatement.)"""
    fx = C.load(name)
    q, k, vv, vl, m, H, scale = C.core_inputs(fx, torch.float32)
    blk = C.block_from(fx, torch.float32)
    with torch.no_grad():
        out_v, out_l = blk.attn._core_torch(q * scale, k, vv, vl, m)
    ref_v, ref_l = R.core(q, k, vv, vl, m, H, scale)
    assert C.rel_err(out_v, ref_v) < C.TOL_REFERENCE_FP32
    assert C.rel_err(out_l, ref_l) < C.TOL_REFERENCE_FP32
    # and end to end against the float64 fixture
    v, l, _ = C.inputs(fx, torch.float32)
    with torch.no_grad():
        o_v, o_l = blk(v, l, m, None)
    assert C.rel_err(keep_rows(fx, o_v), keep_rows(fx, torch.from_numpy(fx["out_visual"]))) < C.TOL_REFERENCE_FP32
    assert C.rel_err(o_l, torch.from_numpy(fx["out_hidden"])) < C.TOL_REFERENCE_FP32


def test_state_dict_names_and_strict_load():
    fx = C.load("t37_partial")
    want = {"layer_norm_v.weight", "layer_norm_v.bias", "layer_norm_l.weight", "layer_norm_l.bias", "gamma_v", "gamma_l"}
    want |= {"attn.%s.%s" % (p, w) for p in ("v_proj", "l_proj", "values_v_proj", "values_l_proj", "out_v_proj", "out_l_proj")
             for w in ("weight", "bias")}
    assert set(fx["state"]) == want
    blk = C.block_from(fx, torch.float32)           # load_state_dict(strict=True) inside
    assert set(blk.state_dict()) == want
    m = C.vlfuse_from(fx, torch.float32)
    assert set(m.state_dict()) == {"b_attn." + k for k in want}


def test_constructor_follows_the_reference():
    from uninext_amd.modules import BiAttentionBlockForCheckpoint, VLFuse
    m = VLFuse(C.vlfuse_cfg(256, 768, 2048))
    a = m.b_attn.attn
    assert (a.num_heads, a.head_dim, a.embed_dim, a.v_dim, a.l_dim, a.dropout) == (8, 256, 2048, 256, 768, 0.1)
    assert a.scale == 1.0 / 16 and m.use_checkpoint is False and m.max_query_len == 256
    assert torch.equal(m.b_attn.gamma_v.detach(), torch.full((256,), 1.0 / 6)) and all(float(p.bias.abs().max()) == 0 for p in
                                                                                 (a.v_proj, a.l_proj, a.out_v_proj))
    bound = (6.0 / (256 + 2048)) ** 0.5            # xavier_uniform_
    assert float(a.v_proj.weight.abs().max()) <= bound
    assert isinstance(m.b_attn.drop_path, torch.nn.Identity)
    other = C.vlfuse_cfg(256, 768, 2048)
    other.MODEL.LANGUAGE_BACKBONE.MODEL_TYPE = "something-large"
    assert VLFuse(other).lang_dim == 1024
    with pytest.raises(NotImplementedError):
        BiAttentionBlockForCheckpoint(16, 24, 512, 2, drop_path=0.1, cfg=C.vlfuse_cfg(16, 24, 512))


def test_bool_mask_adds_one_everywhere():
    """masked_fill(-9e15) on a bool mask yields all True: the reference adds +1 to every score, masking nothing."""
    fx = C.load("t37_partial")
    blk = C.block_from(fx, torch.float64)
    v, l, m = C.inputs(fx, torch.float64)
    with torch.no_grad():
        with_bool = blk(v, l, m.bool(), None)
        without = blk(v, l, None, None)
    assert C.rel_err(with_bool[0], without[0]) < 1e-12 and C.rel_err(with_bool[1], without[1]) < 1e-12


def test_routing_predicate():
    """`_inference` on stand-ins for GPU tensors is exercised on the GPU; here: everything that must go to PyTorch does."""
    from uninext_amd.modules import BiMultiHeadAttention
    a = BiMultiHeadAttention(16, 24, 512, 2, dropout=0.1, cfg=C.vlfuse_cfg(16, 24, 512)).eval()
    v, l = torch.zeros(1, 5, 16), torch.zeros(1, 3, 24)
    old = BiMultiHeadAttention.fused_core
    try:
        BiMultiHeadAttention.fused_core = True
        with torch.no_grad():
            assert not a._inference(v, l, None)                    # CPU tensors
        meta = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="meta")

        class OnGpu:   # a tensor stand-in that says it is on the GPU
            def __init__(self, t):
                self.t = t
                self.is_cuda, self.dtype, self.shape, self.requires_grad = True, t.dtype, t.shape, False
            def is_contiguous(self):
                return True
            def dim(self):
                return self.t.dim()
        gv, gl = OnGpu(meta(1, 5, 16)), OnGpu(meta(1, 3, 24))
        with torch.no_grad():
            assert a._inference(gv, gl, None)
            assert a._inference(gv, gl, OnGpu(meta(1, 3, dtype=torch.int64)))
            assert a._inference(gv, gl, OnGpu(meta(1, 3, dtype=torch.float32)))
            assert not a._inference(gv, gl, OnGpu(meta(1, 3, dtype=torch.bool)))       # bool mask
            assert not a._inference(gv, OnGpu(meta(1, 300, 24)), None)                 # T = 300
            assert not a._inference(OnGpu(meta(1, 5, 16, dtype=torch.float64)), gl, None)
            a.train()
            assert not a._inference(gv, gl, None)                                      # training with p > 0
            a.dropout = 0.0
            assert a._inference(gv, gl, None)
            a.eval()
            a.stable_softmax_2d = True
            assert not a._inference(gv, gl, None)
            a.stable_softmax_2d = False
            a.clamp_max_for_overflow = False
            assert not a._inference(gv, gl, None)
            a.clamp_max_for_overflow = True
            BiMultiHeadAttention.fused_core = False
            assert not a._inference(gv, gl, None)
            BiMultiHeadAttention.fused_core = True
        assert not a._inference(gv, gl, None)                                          # autograd records (parameters)
        small = BiMultiHeadAttention(16, 24, 256, 2, cfg=C.vlfuse_cfg(16, 24, 256)).eval()
        with torch.no_grad():
            assert not small._inference(gv, gl, None)                                  # head_dim 128
    finally:
        BiMultiHeadAttention.fused_core = old


def test_gradients_flow_on_the_torch_path():
    fx = C.load("t1_nomask")
    blk = C.block_from(fx, torch.float64)
    v, l, m = C.inputs(fx, torch.float64)
    v.requires_grad_(True)
    out_v, out_l = blk(v, l, m, None)
    (out_v.sum() + out_l.sum()).backward()
    assert v.grad is not None and float(v.grad.abs().max()) > 0
    assert blk.attn.values_v_proj.weight.grad is not None


def test_workspace_is_smaller_than_the_attention_matrix():
    from uninext_amd import _lib
    lib = _lib.load()
    B, H, S, T, D = 2, 8, 22223, 256, 256
    ws = lib.biattn_hip_workspace_bytes(B, H, S, T, D)
    assert 0 < ws < B * H * S * T * 4
    assert ws < 64 << 20                                  # tens of MB
    assert lib.biattn_hip_workspace_bytes(B, H, S, T, 128) == 0 and lib.biattn_hip_workspace_bytes(B, H, S, 257, D) == 0
    assert lib.biattn_hip_workspace_bytes(B, H, 0, T, D) == 0
    assert lib.biattn_hip_workspace_bytes(1, 1, 1, 1, D) > 0


def test_error_codes_without_a_device():
    from uninext_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(1 << 20)      # never dereferenced: every check runs before the device is touched
    call = lambda q, mask, kind, B, H, S, T, D, ws_bytes=1 << 30: lib.biattn_hip_forward_f32(
        q, fake, fake, fake, mask, kind, B, H, S, T, D, 0.0625, fake, fake, fake, ws_bytes, None)
    assert call(None, None, 0, 1, 2, 10, 5, 256) == -1 and "null" in _lib.last_error()
    assert call(fake, None, _lib.BIATTN_MASK_INT64, 1, 2, 10, 5, 256) == -1
    assert call(fake, None, 0, 1, 2, 0, 5, 256) == -2 and "dimensions" in _lib.last_error()
    assert call(fake, None, 0, 1, 0, 10, 5, 256) == -2
    assert call(fake, None, 0, 1, 2, 10, 5, 128) == -5 and "head_dim" in _lib.last_error()
    assert call(fake, None, 0, 1, 2, 10, 257, 256) == -5
    assert call(fake, fake, 7, 1, 2, 10, 5, 256) == -5
    assert call(fake, None, 0, 1, 2, 10, 5, 256, ws_bytes=16) == -6
    assert call(fake, None, 0, 0, 2, 10, 5, 256) == 0    # an empty batch enqueues nothing


def test_header_symbols_are_exported():
    import re
    from uninext_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "biattn_hip.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(biattn_hip_\w+)\s*\(", text)))
    assert names == sorted(_lib.BIATTN_EXPORTS)
    lib = _lib.load()
    for n in names:
        assert hasattr(lib, n), n


def test_exact_family_is_exact():
    """The seeded integer family: scores are the same integers in fp32 and float64, some beyond the clamp."""
    q, k, vv, vl, scale = R.exact_case(5, 1, 2, 70, 9)
    s64 = R.scores(q, k, 2, scale)
    s32 = torch.matmul(R.split_heads(q * scale, 2), R.split_heads(k, 2).transpose(-1, -2)).clamp(min=-R.CLAMP, max=R.CLAMP)
    assert torch.equal(s32.double(), s64)
    assert float(s64.max()) == R.CLAMP and float(s64.min()) == -R.CLAMP
    assert int((s64[0, 0, 0] == R.CLAMP).sum()) == 2 and int((s64[0, 0, :, 0] == R.CLAMP).sum()) == 2      # ties at the clamp
