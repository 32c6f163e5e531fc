"""CPU: the text encoder (uninext_amd/text_encoder.py) against the fixtures under tests/golden/text_encoder/, minted by
tests/golden/make_text_encoder_golden.py from transformers' BertModel through the reference's own BertEncoder.forward; the float64
restatement (tests/text_encoder_ref.py) against the same; the state-dict keys; the reference's dict and PARALLEL_DET mask; the
C ABI's refusals without a device; the new kernels' registers and scratch."""
import ctypes
import os
import shutil
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_encoder_cases as C  # noqa: E402
import text_encoder_ref as R  # noqa: E402

from uninext_amd import _lib, text_encoder as TE  # noqa: E402

NAMES = sorted(C.FIXTURES)


def hidden_of(fx):
    return [fx["hidden_%d" % n] for n in range(C.CONFIG["num_hidden_layers"] + 1)]


def test_fixtures_are_the_expected_set_and_small():
    files = sorted(os.listdir(C.HERE))
    assert files == sorted([n + ".npz" for n in NAMES] + ["state_dict_keys.json"])
    for f in files:
        assert os.path.getsize(os.path.join(C.HERE, f)) < 1 << 20
    state = C.state_dict()
    for n in NAMES:
        fx = C.load(n)
        assert float(fx["digest"]) == C.digest(state)                 # the parameters are the ones the reference saw
        ids, mask, tt = C.make_inputs(n)
        assert np.array_equal(fx["input_ids"], ids.numpy()) and np.array_equal(fx["attention_mask"], mask.numpy())
        assert ("token_type_ids" in fx) == (tt is not None)
        assert not any(k.endswith("weight") or k.endswith("bias") for k in fx)
    assert C.load("one_token")["attention_mask"][1].sum() == 1 and C.load("full")["attention_mask"].all()


@pytest.mark.parametrize("name", NAMES)
def test_module_float64_matches_the_fixtures(name):
    fx = C.load(name)
    ids, mask, tt = C.make_inputs(name)
    m = C.build(torch.float64)
    with torch.no_grad():
        out = m(ids, mask, tt)
    assert len(out.hidden_states) == C.CONFIG["num_hidden_layers"] + 1
    for got, want in zip(out.hidden_states, hidden_of(fx)):
        assert got.dtype == torch.float64 and C.rel_err(got, want) <= C.TOL64
    assert torch.equal(out.last_hidden_state, out.hidden_states[-1])
    m.fused = True                                                    # on the CPU and in float64 the flag changes nothing
    with torch.no_grad():
        again = m(ids, mask, tt)
    assert all(torch.equal(a, b) for a, b in zip(again.hidden_states, out.hidden_states))


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_fixtures(name):
    fx = C.load(name)
    ids, mask, tt = C.make_inputs(name)
    for got, want in zip(R.model(C.state_dict(), C.CONFIG, ids, mask, tt), hidden_of(fx)):
        assert C.rel_err(got, want) <= C.TOL64


def test_state_dict_keys_shapes_and_strict_load():
    m = TE.BertModel(TE.BertConfig(**C.CONFIG))
    recorded = C.recorded_keys()
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == recorded
    assert list(m.state_dict()) == list(recorded)                    # transformers' order too
    state = C.state_dict()
    m.load_state_dict(state, strict=True)
    assert all(torch.equal(v.double(), state[k]) for k, v in m.state_dict().items())
    # the buffers older transformers checkpoints carry are accepted and ignored
    old = dict(state)
    old["embeddings.position_ids"] = torch.arange(C.CONFIG["max_position_embeddings"])[None]
    old["embeddings.token_type_ids"] = torch.zeros(1, C.CONFIG["max_position_embeddings"], dtype=torch.long)
    m.load_state_dict(old, strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in state.items() if k != "encoder.layer.1.output.dense.bias"}, strict=True)
    # bert-base geometry by default, under the same names
    big = TE.BertConfig()
    assert (big.vocab_size, big.hidden_size, big.num_hidden_layers, big.num_attention_heads, big.intermediate_size,
            big.max_position_embeddings, big.layer_norm_eps) == (30522, 768, 12, 12, 3072, 512, 1e-12)
    for bad in (dict(hidden_act="relu"), dict(position_embedding_type="relative_key")):
        with pytest.raises(NotImplementedError):
            TE.BertConfig(**bad)


def test_encoder_returns_the_reference_dict_and_its_parallel_det_mask():
    m = C.build(torch.float64)
    ids, mask, _ = C.make_inputs("padded")
    fx = C.load("padded")
    enc = TE.BertEncoder(m, parallel_det=True)
    with torch.no_grad():
        ret = enc({"input_ids": ids, "attention_mask": mask})          # no task: the 2-D mask
        det = enc({"input_ids": ids, "attention_mask": mask}, task="detection")
        plain = TE.BertEncoder(m)({"input_ids": ids, "attention_mask": mask}, task="detection")
    assert sorted(ret) == ["hidden", "masks"] and ret["masks"] is mask
    assert C.rel_err(ret["hidden"], fx["hidden"]) <= C.TOL64 and np.array_equal(ret["masks"].numpy(), fx["masks"])
    assert torch.equal(plain["hidden"], ret["hidden"])                # parallel_det off: the task changes nothing
    # the mask: the reference's loop, restated for B = 2
    want = R.parallel_det_mask(mask)
    got = TE.parallel_det_mask(mask)
    assert got.dtype == torch.uint8 and got.shape == (C.B, C.T, C.T) and torch.equal(got.float(), want)
    assert torch.equal(got[1, :17, :17], torch.eye(17, dtype=torch.uint8)) and got[1, 17:, :17].all() and not got[1, :, 17:].any()
    # and what it does to the output: the float64 restatement on the reference's float mask
    hidden = R.model(C.state_dict(), C.CONFIG, ids, want)
    assert det["masks"] is mask and C.rel_err(det["hidden"], hidden[-1]) <= C.TOL64
    assert C.rel_err(det["hidden"], fx["hidden"]) > 1e-3              # it is another function of the prompt


def test_dropout_only_in_train_mode():
    m = C.build(torch.float64)
    ids, mask, _ = C.make_inputs("padded")
    with torch.no_grad():
        a = m(ids, mask).last_hidden_state
        m.train()
        torch.manual_seed(0)
        b = m(ids, mask).last_hidden_state
        m.eval()
        c = m(ids, mask).last_hidden_state
    assert torch.equal(a, c) and not torch.equal(a, b)


def test_package_reexports_without_transformers():
    import subprocess
    code = ("import sys, uninext_amd\n"
            "from uninext_amd import BertModel, BertEncoder, BertEmbeddings, BertSelfAttention, BertSelfOutput, BertAttention, "
            "BertIntermediate, BertOutput, BertLayer, BertConfig\n"
            "assert BertEncoder is uninext_amd.text_encoder.BertEncoder\n"
            "assert 'transformers' not in sys.modules\n")
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_supported_predicates_without_a_device():
    from uninext_amd import ext
    q = torch.zeros(2, 8, 128)
    assert not ext.bert_self_attention_supported(q, q, q, 2, None)    # not on the GPU
    ids = torch.zeros(2, 8, dtype=torch.long)
    w = torch.zeros(4, 128)
    assert not ext.bert_embed_layernorm_supported(ids, None, w, w, w, w[0], w[0])


def test_error_codes_without_a_device():
    """Every refusal comes before the device is touched: fake addresses never reach a kernel."""
    lib = _lib.load()
    fake = ctypes.c_void_p(1 << 20)

    def attn(mask=None, kind=_lib.BERT_MASK_NONE, batch=1, heads=2, length=10, head_dim=64, strides=(128, 128, 128), q=fake):
        rc = lib.bert_hip_self_attention_f32(q, fake, fake, *strides, mask, kind, batch, heads, length, head_dim, 0.125, fake, None)
        return rc, _lib.last_error()

    assert attn(head_dim=32) == (-5, "bert_attn: head_dim must be 64")
    assert attn(length=513) == (-5, "bert_attn: len must be at most 512")
    assert attn(strides=(128, 130, 128)) == (-5, "bert_attn: row strides must be multiples of 4 floats")
    assert attn(kind=_lib.BERT_MASK_FULL_U8) == (-1, "bert_attn: null pointer argument")
    assert attn(kind=_lib.BERT_MASK_KEY_I64) == (-1, "bert_attn: null pointer argument")
    assert attn(kind=7, mask=fake)[0] == -5
    assert attn(length=0)[0] == -2 and attn(strides=(64, 128, 128))[0] == -2
    assert attn(q=None) == (-1, "bert_attn: null pointer argument")
    assert attn(q=ctypes.c_void_p((1 << 20) + 4))[0] == -5
    assert attn(batch=0, q=None)[0] == 0                              # nothing to enqueue, no buffer is looked at

    def embed(hidden=128, length=8, positions=64, ids=fake, tt=None):
        rc = lib.bert_hip_embed_layernorm_f32(ids, tt, fake, fake, fake, fake, fake, 1e-12, 2, length, hidden, 64, positions, 2, fake, None)
        return rc, _lib.last_error()

    assert embed(hidden=130) == (-5, "bert_embed: hidden must be a multiple of 4 and <= 4096")
    assert embed(hidden=4100)[0] == -5
    assert embed(length=65) == (-2, "bert_embed: len exceeds the position table")
    assert embed(ids=None) == (-1, "bert_embed: null pointer argument")
    assert embed(hidden=0)[0] == -2


# (VGPRs at most, scratch bytes per lane): what the kernels of bert.hip compiled to on 2026-10-21
PINNED = {
    "bert::attn<0>": (223, 0), "bert::attn<1>": (226, 0), "bert::attn<2>": (226, 0), "bert::attn<3>": (223, 0),
    "bert::embed<1>": (28, 0), "bert::embed<2>": (32, 0), "bert::embed<4>": (50, 0), "bert::embed<8>": (205, 0),
    "bert::embed<16>": (110, 0),
}


@pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None, reason="needs hipcc")
def test_bert_kernels_keep_their_registers_and_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    got = kernel_resources.resources(os.path.join(ROOT, "uninext_amd", "csrc", "bert.hip"))
    assert set(PINNED) == set(got), sorted(set(PINNED) ^ set(got))
    for name, (vgprs, scratch) in PINNED.items():
        r = got[name]
        assert r["scratch"] == scratch and r.get("vgpr_spill", 0) == 0 and r["vgprs"] <= vgprs, (name, r)
