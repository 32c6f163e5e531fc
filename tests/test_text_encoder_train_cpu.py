"""CPU: the training route of the text encoder (uninext_amd/text_encoder.py: BertSelfAttentionFunction, set_own_training;
uninext_amd/csrc/bert_attn_bwd.hip) as far as it goes without a device: the gradient fixtures under
tests/golden/text_encoder_train/ (minted by tests/golden/make_text_encoder_train_golden.py from transformers' BertModel through
the reference's own BertEncoder.forward) against the float64 module under plain autograd and against the float64 restatement
with tests/text_encoder_train_cases.py's core inside; the flags on the CPU; the C ABI's refusals; the Philox mirror's keep share;
the new kernels' registers and scratch."""
import ctypes
import math
import os
import shutil
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_encoder_cases as C  # noqa: E402
import text_encoder_train_cases as TC  # noqa: E402

from uninext_amd import _lib, text_encoder as TE  # noqa: E402

NAMES = sorted(TC.FIXTURES)


module_grads = TC.module_grads


def test_fixtures_are_the_expected_set_and_small():
    files = sorted(os.listdir(TC.HERE))
    assert files == sorted(n + ".npz" for n in NAMES)
    state = C.state_dict()
    for n in NAMES:
        assert os.path.getsize(os.path.join(TC.HERE, n + ".npz")) < 1 << 20
        fx = TC.load(n)
        assert float(fx["digest"]) == C.digest(state)                 # the parameters are the ones the reference saw
        ids, mask, core_mask = TC.fixture_inputs(n)
        assert np.array_equal(fx["input_ids"], ids.numpy()) and np.array_equal(fx["attention_mask"], mask.numpy())
        assert np.array_equal(fx["U"], TC.loss_weights().numpy())
        if TC.FIXTURES[n][1]:                                         # the mask the reference's loop built
            assert np.array_equal(fx["core_mask"], core_mask.numpy().astype(np.uint8))
        grads = sorted(k[5:] for k in fx if k.startswith("grad/"))
        assert grads == sorted(k for k in state if TC.recorded(k))
        assert not any(k.endswith("weight") or k.endswith("bias") for k in fx if not k.startswith("grad/"))


@pytest.mark.parametrize("name", NAMES)
def test_module_float64_autograd_matches_the_fixtures(name):
    fx = TC.load(name)
    hidden, grads, gemb = module_grads(C.build(torch.float64), name)
    assert C.rel_err(hidden, fx["hidden"]) <= TC.TOL64
    assert C.rel_err(gemb, fx["grad_embeddings_output"]) <= TC.TOL64
    want = {k[5:]: fx[k] for k in fx if k.startswith("grad/")}
    for k in want:
        assert TC.param_err(k, grads[k], want) <= TC.TOL64, k


@pytest.mark.parametrize("name", NAMES)
def test_restatement_with_the_cases_core_matches_the_fixtures(name):
    fx = TC.load(name)
    ids, _, core_mask = TC.fixture_inputs(name)
    hidden, grads, gemb = TC.model_grads(ids, core_mask, TC.loss_weights())
    assert C.rel_err(hidden[-1], fx["hidden"]) <= TC.TOL64
    assert C.rel_err(gemb, fx["grad_embeddings_output"]) <= TC.TOL64
    want = {k[5:]: fx[k] for k in fx if k.startswith("grad/")}
    for k in want:
        assert TC.param_err(k, grads[k], want) <= TC.TOL64, k
    # and on the parameters the fixtures do not record it agrees with the module under plain autograd
    _, mgrads, _ = module_grads(C.build(torch.float64), name)
    for k in mgrads:
        assert TC.param_err(k, grads[k], mgrads) <= TC.TOL64, k


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_flags_change_nothing_on_the_cpu(dtype):
    m = C.build(dtype).train()                                       # train(): both dropouts active
    outs = []
    for flags in (None, (True, False), (True, True)):
        if flags is not None:
            assert m.set_own_training(*flags) is m
            assert all(l.attention.self.own_training and l.attention.self.own_dropout == flags[1] for l in m.encoder.layer)
        torch.manual_seed(5)
        outs.append(module_grads(m, "padded", dtype))
    for hidden, grads, gemb in outs[1:]:
        assert torch.equal(hidden, outs[0][0]) and torch.equal(gemb, outs[0][2])
        assert all(torch.equal(grads[k], outs[0][1][k]) for k in grads)
    enc = TE.BertEncoder(m)
    assert enc.set_own_training(False) is enc and not any(l.attention.self.own_training or l.attention.self.own_dropout
                                                         for l in m.encoder.layer)
    assert TE.BertSelfAttention.own_training is False and TE.BertSelfAttention.own_dropout is False    # off by default


def test_supported_predicate_and_exports_without_a_device():
    import uninext_amd
    from uninext_amd import ext
    assert uninext_amd.BertSelfAttentionFunction is TE.BertSelfAttentionFunction
    q = torch.zeros(2, 8, 128)
    assert not ext.bert_self_attention_train_supported(q, q, q, 2, None)            # not on the GPU
    assert not ext.bert_self_attention_train_supported(q, q, q, 2, None, 1.0)
    assert _lib.BERT_ERR_WORKSPACE == -6


def test_error_codes_without_a_device():
    """Every refusal comes before the device is touched: fake addresses never reach a kernel."""
    lib = _lib.load()
    fake = ctypes.c_void_p(1 << 20)
    odd = ctypes.c_void_p((1 << 20) + 4)

    def train(mask=None, kind=_lib.BERT_MASK_NONE, batch=1, heads=2, length=10, head_dim=64, strides=(128, 128, 128), q=fake, lse=fake,
              p=0.0, seed=None):
        rc = lib.bert_hip_self_attention_train_f32(q, fake, fake, *strides, mask, kind, batch, heads, length, head_dim, 0.125, fake, lse,
                                                   p, seed, None)
        return rc, _lib.last_error()

    def bwd(mask=None, kind=_lib.BERT_MASK_NONE, batch=1, heads=2, length=10, head_dim=64, strides=(128,) * 6, q=fake, dv=fake, ws=fake,
            ws_bytes=1 << 20, p=0.0, seed=None):
        rc = lib.bert_hip_self_attention_backward_f32(q, fake, fake, *strides[:3], mask, kind, fake, fake, fake, batch, heads, length,
                                                      head_dim, 0.125, fake, fake, dv, *strides[3:], ws, ws_bytes, p, seed, None)
        return rc, _lib.last_error()

    for call, who in ((train, "bert_attn_train"), (bwd, "bert_attn_bwd")):
        assert call(q=None) == (-1, who + ": null pointer argument")
        assert call(head_dim=32) == (-5, who + ": head_dim must be 64")
        assert call(length=0) == (-2, who + ": bad dimensions")
        assert call(length=513) == (-5, who + ": len must be at most 512")
        n = len(call.__defaults__[6])
        assert call(strides=(128, 130) + (128,) * (n - 2)) == (-5, who + ": row strides must be multiples of 4 floats")
        assert call(strides=(64,) + (128,) * (n - 1)) == (-2, who + ": a row stride is smaller than num_heads * head_dim")
        assert call(q=odd)[0] == -5 and "16-byte aligned" in call(q=odd)[1]
        assert call(kind=7, mask=fake) == (-5, who + ": unknown mask kind (none, key int64, key u8 or full u8)")
        assert call(kind=_lib.BERT_MASK_FULL_U8) == (-1, who + ": null pointer argument")
        assert call(kind=_lib.BERT_MASK_KEY_I64, mask=odd) == (-5, who + ": an int64 mask must be 8-byte aligned")
        for p in (1.0, -0.1, math.nan):
            assert call(p=p, seed=fake) == (-2, who + ": dropout_p must be in [0, 1)")
        assert call(p=0.1) == (-1, who + ": null seed with dropout_p > 0")
        assert call(p=0.1, seed=fake, batch=32768, length=1) == (-5, who + ": batch * num_heads must be at most 65535 with dropout")
        assert call(batch=0, q=None)[0] == 0                          # nothing to enqueue, no buffer is looked at
    assert train(lse=None) == (-1, "bert_attn_train: null pointer argument")
    assert bwd(dv=None) == (-1, "bert_attn_bwd: null pointer argument") and bwd(ws=None)[0] == -1
    assert bwd(strides=(128,) * 5 + (130,))[0] == -5                  # the outputs' strides are held to the inputs' limits

    need = lib.bert_hip_self_attention_backward_workspace_bytes(1, 2, 10, 64)
    assert need >= 2 * 32 * 4 and need % 256 == 0
    assert lib.bert_hip_self_attention_backward_workspace_bytes(2, 12, 256, 64) >= 2 * 12 * 256 * 4
    assert lib.bert_hip_self_attention_backward_workspace_bytes(1, 2, 10, 32) == 0 == lib.bert_hip_self_attention_backward_workspace_bytes(1, 2, 513, 64)
    assert bwd(ws_bytes=need - 1) == (_lib.BERT_ERR_WORKSPACE, "bert_attn_bwd: workspace smaller than the workspace_bytes query answers")

    def keep(seed=fake, p=0.1, batch=1, heads=2, length=10, out=fake):
        rc = lib.bert_hip_dropout_keep_u8(seed, p, batch, heads, length, out, None)
        return rc, _lib.last_error()

    assert keep(seed=None) == (-1, "bert_dropout_keep: null pointer argument") and keep(out=None)[0] == -1
    assert keep(p=1.0)[0] == -2 and keep(p=math.nan)[0] == -2 and keep(length=513)[0] == -5 and keep(length=0)[0] == -2
    assert keep(batch=32768)[0] == -5 and keep(batch=0, seed=None)[0] == 0


def test_mirror_keep_share_is_binomial():
    """The mask is a pure function of its inputs, so this holds or fails once: the share of kept entries at p = 0.1 over
    N = 2 * 2 * 97 * 97 entries lies within 5 standard deviations, 5 sqrt(0.1 * 0.9 / N), of 0.9."""
    keep = TC.keep_matrix(TC.seed_of("text_encoder_train_share"), 0.1, 4, 97)
    assert keep.shape == (4, 97, 97) and keep.dtype == np.bool_
    N = keep.size
    assert N == 2 * 2 * 97 * 97
    share = keep.mean()
    print("keep share %.5f of %d entries, bound %.5f" % (share, N, 5 * math.sqrt(0.09 / N)))
    assert abs(share - 0.9) <= 5 * math.sqrt(0.09 / N)
    assert TC.keep_matrix(TC.seed_of("text_encoder_train_share"), 0.0, 4, 97).all()     # p = 0 keeps everything
    assert not np.array_equal(keep, TC.keep_matrix(TC.seed_of("another"), 0.1, 4, 97))


# VGPRs at most (scratch 0, no spill, in all): what the kernels of bert_attn_bwd.hip compiled to on 2026-10-21, by
# (mask kind, dropout)
PINNED = {"dropout_keep": 16}
for kind, (tr, trd, bq, bqd, kv, kvd) in enumerate(((223, 237, 208, 222, 248, 247), (226, 240, 212, 226, 252, 251),
                                                    (226, 240, 212, 226, 252, 251), (223, 237, 210, 194, 252, 250))):
    PINNED.update({"attn_train<%d, false>" % kind: tr, "attn_train<%d, true>" % kind: trd, "bwd_q<%d, false>" % kind: bq,
                   "bwd_q<%d, true>" % kind: bqd, "bwd_kv<%d, false>" % kind: kv, "bwd_kv<%d, true>" % kind: kvd})


@pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None, reason="needs hipcc")
def test_training_kernels_keep_their_registers_and_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    got = kernel_resources.resources(os.path.join(ROOT, "uninext_amd", "csrc", "bert_attn_bwd.hip"))
    assert {"bert_attn_bwd::" + n for n in PINNED} == set(got), sorted({"bert_attn_bwd::" + n for n in PINNED} ^ set(got))
    for name, vgprs in PINNED.items():
        r = got["bert_attn_bwd::" + name]
        assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0 and r["vgprs"] <= vgprs <= 512, (name, r)
