"""Shared by tests/golden/make_text_encoder_golden.py, tests/test_text_encoder_cpu.py and tests/test_text_encoder_gpu.py: the
small config, the seeded parameters and inputs of the fixtures under tests/golden/text_encoder/, and the error measure.

Every parameter is an exact dyadic (a multiple of 2 ** -STEP_BITS), so fp32 holds what the float64 reference saw.  The fixtures
store inputs and the reference's hidden states; the parameters are re-drawn here from the same CPU generator on both sides and
pinned by the digest each fixture records, as tests/decoder_cases.py does."""
import json
import os

import numpy as np
import torch

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text_encoder")
TOL = 1e-4            # the project's fp32 bound: max abs error <= 1e-4 of the output's max abs, against float64
TOL64 = 1e-10         # float64 against float64
STEP_BITS = 10
SEED = 381

# vocab 64, hidden 128, 2 heads of 64, 2 layers, intermediate 256, 64 positions
CONFIG = dict(vocab_size=64, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
              max_position_embeddings=64, type_vocab_size=2, layer_norm_eps=1e-12)
B, T = 2, 40
# name -> valid tokens per prompt, token type ids given
FIXTURES = {
    "full": dict(valid=(40, 40), types=False),
    "padded": dict(valid=(40, 17), types=False),
    "one_token": dict(valid=(40, 1), types=False),
    "type_ids": dict(valid=(40, 23), types=True),
}


def dyadic(t, scale=1.0):
    step = float(1 << STEP_BITS)
    return torch.round(t.double() * scale * step) / step


def rel_err(got, want):
    want = torch.as_tensor(want).double()
    return float((got.detach().cpu().double() - want).abs().max() / want.abs().max())


def _linear(p, g, name, o, i, gain=1.0):
    p[name + ".weight"] = dyadic(torch.randn(o, i, generator=g), gain * i ** -0.5)
    p[name + ".bias"] = dyadic(torch.randn(o, generator=g), 0.1)


def _norm(p, g, name, d):
    p[name + ".weight"] = dyadic(1.0 + 0.1 * torch.randn(d, generator=g))
    p[name + ".bias"] = dyadic(torch.randn(d, generator=g), 0.1)


def state_dict():
    """The model's parameters in transformers' key order, float64 dyadics from SEED alone."""
    c = CONFIG
    g = torch.Generator().manual_seed(SEED)
    d = c["hidden_size"]
    p = {}
    p["embeddings.word_embeddings.weight"] = dyadic(torch.randn(c["vocab_size"], d, generator=g))
    p["embeddings.position_embeddings.weight"] = dyadic(torch.randn(c["max_position_embeddings"], d, generator=g), 0.5)
    p["embeddings.token_type_embeddings.weight"] = dyadic(torch.randn(c["type_vocab_size"], d, generator=g), 0.5)
    _norm(p, g, "embeddings.LayerNorm", d)
    for n in range(c["num_hidden_layers"]):
        pre = "encoder.layer.%d." % n
        _linear(p, g, pre + "attention.self.query", d, d, 3.0)       # scores that are far from flat
        _linear(p, g, pre + "attention.self.key", d, d, 3.0)
        _linear(p, g, pre + "attention.self.value", d, d)
        _linear(p, g, pre + "attention.output.dense", d, d)
        _norm(p, g, pre + "attention.output.LayerNorm", d)
        _linear(p, g, pre + "intermediate.dense", c["intermediate_size"], d)
        _linear(p, g, pre + "output.dense", d, c["intermediate_size"])
        _norm(p, g, pre + "output.LayerNorm", d)
    return p


def digest(state):
    return float(sum(float(v.double().abs().sum()) for v in state.values()))


def make_inputs(name):
    """input_ids, attention_mask (int64 [B, T], the first valid[b] tokens of prompt b) and token_type_ids or None."""
    cfg = FIXTURES[name]
    g = torch.Generator().manual_seed(SEED + 1 + sorted(FIXTURES).index(name))
    ids = torch.randint(1, CONFIG["vocab_size"], (B, T), generator=g)
    mask = (torch.arange(T)[None, :] < torch.as_tensor(cfg["valid"])[:, None]).long()
    ids = ids * mask                                                  # padding is token 0, as the tokenizer pads
    tt = torch.randint(0, CONFIG["type_vocab_size"], (B, T), generator=g) * mask if cfg["types"] else None
    return ids, mask, tt


def load(name):
    z = np.load(os.path.join(HERE, name + ".npz"))
    return {k: z[k] for k in z.files}


def recorded_keys():
    with open(os.path.join(HERE, "state_dict_keys.json")) as f:
        return json.load(f)


def build(dtype=torch.float64, device="cpu", fused=False):
    """The project's BertModel on CONFIG, loaded strictly from state_dict(), in eval mode."""
    from uninext_amd import text_encoder as TE
    m = TE.BertModel(TE.BertConfig(**CONFIG))
    m.load_state_dict(state_dict(), strict=True)
    m = m.to(dtype).to(device).eval()
    m.fused = fused
    return m
