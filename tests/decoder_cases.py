"""Shared by tests/golden/make_decoder_golden.py, tests/test_decoder_cpu.py and tests/test_decoder_gpu.py: the seeds, shapes,
parameters and inputs of the fixtures under tests/golden/decoder/, and the error measure.

Every parameter and input is an exact dyadic (a multiple of 2 ** -STEP_BITS), so fp32 holds what the float64 reference saw.
The fixtures store inputs and the reference's outputs; the parameters (up to 1.6 M values: the decoder needs d_model 256, since
the reference feeds `ref_point_head` 4 x 128 sine features) are re-drawn here from the same CPU generator on both sides and
pinned by the digest each fixture records, as tests/golden/encstack_6layers.npz does."""
import json
import os

import numpy as np
import torch

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder")
TOL = 1e-4            # the project's bound: max abs error <= 1e-4 of the output's max abs, against float64 (tests/vit_cases.py)
TOL_SAME = 1e-6       # two routes through the same kernel arithmetic
STEP_BITS = 10
LEVELS = [(6, 8), (3, 4), (2, 2), (1, 1)]      # a small pyramid: S = 65
N_LEVELS, N_POINTS = 4, 4

# name -> kind, seed, d_model, heads, d_ffn, layers, queries, mask
FIXTURES = {
    "layer_plain": dict(kind="layer", seed=101, d_model=64, heads=2, d_ffn=128, layers=1, lq=37, mask=None),
    "layer_dn_mask": dict(kind="layer", seed=102, d_model=64, heads=2, d_ffn=128, layers=1, lq=70, mask="dn"),
    "layer_float_mask": dict(kind="layer", seed=103, d_model=64, heads=2, d_ffn=128, layers=1, lq=37, mask="float"),
    "decoder_2layers": dict(kind="decoder", seed=104, d_model=256, heads=8, d_ffn=128, layers=2, lq=21, mask=None),
    "reid_head": dict(kind="reid", seed=105, d_model=256, heads=8, d_ffn=128, layers=1, lq=21, mask=None),
}
DN_PAD, DN_NUMBER = 40, 2          # layer_dn_mask: 2 groups of 20 denoising queries, then 30 matching queries


def dyadic(t, scale=1.0):
    step = float(1 << STEP_BITS)
    return torch.round(t.double() * scale * step) / step


def rel_err(got, want):
    want = torch.as_tensor(want).double()
    return float((got.detach().cpu().double() - want).abs().max() / want.abs().max())


def dn_mask(tgt_size, pad_size, groups):
    """The denoising attention mask by its meaning (True = may not attend): the first pad_size queries are `groups` equal
    groups of noised targets that see their own group and the matching queries; the matching queries see only each other."""
    m = torch.zeros(tgt_size, tgt_size, dtype=torch.bool)
    m[pad_size:, :pad_size] = True
    g = pad_size // groups
    for n in range(groups):
        m[n * g:(n + 1) * g, :n * g] = True
        m[n * g:(n + 1) * g, (n + 1) * g:pad_size] = True
    return m


def float_mask(g, lq):
    """Finite values and -inf (a quarter of the elements), column 0 open so that no row is empty."""
    m = dyadic(torch.randn(lq, lq, generator=g))
    m[torch.rand(lq, lq, generator=g) < 0.25] = float("-inf")
    m[:, 0] = 0.0
    return m


def _linear(p, g, name, o, i, wstd, bstd=0.1):
    p[name + ".weight"] = dyadic(torch.randn(o, i, generator=g), wstd)
    p[name + ".bias"] = dyadic(torch.randn(o, generator=g), bstd)


def _norm(p, g, name, d):
    p[name + ".weight"] = dyadic(1.0 + 0.1 * torch.randn(d, generator=g))
    p[name + ".bias"] = dyadic(torch.randn(d, generator=g), 0.1)


def layer_state(g, d, heads, d_ffn, prefix=""):
    """State dict of one decoder layer in the reference's key order."""
    p = {}
    _linear(p, g, "cross_attn.sampling_offsets", heads * N_LEVELS * N_POINTS * 2, d, 0.05, 0.75)
    _linear(p, g, "cross_attn.attention_weights", heads * N_LEVELS * N_POINTS, d, 0.2)
    _linear(p, g, "cross_attn.value_proj", d, d, d ** -0.5)
    _linear(p, g, "cross_attn.output_proj", d, d, d ** -0.5)
    _norm(p, g, "norm1", d)
    w = torch.randn(3 * d, d, generator=g) * d ** -0.5
    w[:2 * d] *= 2.0                                      # q and k rows: scores that are far from flat
    p["self_attn.in_proj_weight"] = dyadic(w)
    p["self_attn.in_proj_bias"] = dyadic(torch.randn(3 * d, generator=g), 0.1)
    _linear(p, g, "self_attn.out_proj", d, d, d ** -0.5)
    _norm(p, g, "norm2", d)
    _linear(p, g, "linear1", d_ffn, d, d ** -0.5)
    _linear(p, g, "linear2", d, d_ffn, d_ffn ** -0.5)
    _norm(p, g, "norm3", d)
    return {prefix + k: v for k, v in p.items()}


def stack_state(g, cfg, bbox):
    """State dict of a DeformableTransformerDecoder (bbox: with a 3-layer box MLP per layer) or a DeformableReidHead."""
    d = cfg["d_model"]
    p = {}
    for lid in range(cfg["layers"]):
        p.update(layer_state(g, d, cfg["heads"], cfg["d_ffn"], "layers.%d." % lid))
    _linear(p, g, "ref_point_head.layers.0", d, 2 * d, (2 * d) ** -0.5)
    _linear(p, g, "ref_point_head.layers.1", d, d, d ** -0.5)
    if bbox:
        for lid in range(cfg["layers"]):
            _linear(p, g, "bbox_embed.%d.layers.0" % lid, d, d, d ** -0.5)
            _linear(p, g, "bbox_embed.%d.layers.1" % lid, d, d, d ** -0.5)
            _linear(p, g, "bbox_embed.%d.layers.2" % lid, 4, d, 0.25 * d ** -0.5)
    return p


def digest(state):
    return float(sum(float(v.double().abs().sum()) for v in state.values()))


def make_case(name):
    """(cfg, state dict, inputs) of a fixture, float64, from its seed alone."""
    cfg = FIXTURES[name]
    g = torch.Generator().manual_seed(cfg["seed"])
    d, lq, B = cfg["d_model"], cfg["lq"], 2
    S = sum(h * w for h, w in LEVELS)
    shapes = torch.as_tensor(LEVELS, dtype=torch.long)
    x = {"shapes": shapes, "lsi": torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1])),
         "tgt": dyadic(torch.randn(B, lq, d, generator=g)), "src": dyadic(torch.randn(B, S, d, generator=g))}
    pad = torch.zeros(B, S, dtype=torch.bool)
    pad[1, -7:] = True
    x["padding_mask"] = pad
    if cfg["kind"] == "layer":
        state = layer_state(g, d, cfg["heads"], cfg["d_ffn"])
        x["query_pos"] = dyadic(torch.randn(B, lq, d, generator=g), 0.5)
        x["ref"] = dyadic(0.1 + 0.8 * torch.rand(B, lq, N_LEVELS, 2, generator=g))
        if cfg["mask"] == "dn":
            x["attn_mask"] = dn_mask(lq, DN_PAD, DN_NUMBER)     # the generator re-derives it with the reference's construction
        elif cfg["mask"] == "float":
            x["attn_mask"] = float_mask(g, lq)
    else:
        state = stack_state(g, cfg, bbox=cfg["kind"] == "decoder")
        cxcy = 0.2 + 0.6 * torch.rand(B, lq, 2, generator=g)
        wh = 0.05 + 0.3 * torch.rand(B, lq, 2, generator=g)
        x["ref"] = dyadic(torch.cat([cxcy, wh], -1))
        x["valid_ratios"] = dyadic(0.75 + 0.25 * torch.rand(B, N_LEVELS, 2, generator=g))
    return cfg, state, x


def load(name):
    z = np.load(os.path.join(HERE, name + ".npz"))
    return {k: z[k] for k in z.files}


def recorded_keys():
    with open(os.path.join(HERE, "state_dict_keys.json")) as f:
        return json.load(f)


def build(name, cfg, state, dtype, device="cpu", **decoder_args):
    """The project's module of a fixture, loaded strictly from `state`, in eval mode."""
    from uninext_amd import modules as M
    layer = M.DeformableTransformerDecoderLayer(cfg["d_model"], cfg["d_ffn"], 0.1, "relu", N_LEVELS, cfg["heads"], N_POINTS)
    if cfg["kind"] == "layer":
        m = layer
    elif cfg["kind"] == "decoder":
        m = M.DeformableTransformerDecoder(cfg["d_model"], layer, cfg["layers"], return_intermediate=True, **decoder_args)
        m.bbox_embed = torch.nn.ModuleList(M.MLP(cfg["d_model"], cfg["d_model"], 4, 3) for _ in range(cfg["layers"]))
    else:
        m = M.DeformableReidHead(cfg["d_model"], layer, cfg["layers"])
    m.load_state_dict(state, strict=True)
    return m.to(dtype).to(device).eval()


def run(cfg, m, x, device="cpu", dtype=torch.float64):
    """The module's output(s) as a tuple, on the inputs `x` of make_case."""
    t = lambda k: None if k not in x else (x[k].to(device) if x[k].dtype in (torch.bool, torch.long) else x[k].to(dtype).to(device))
    with torch.no_grad():
        if cfg["kind"] == "layer":
            return (m(t("tgt"), t("query_pos"), t("ref"), t("src"), t("shapes"), t("lsi"), t("padding_mask"), t("attn_mask")),)
        out = m(t("tgt"), t("ref"), t("src"), t("shapes"), t("lsi"), t("valid_ratios"), None, t("padding_mask"), None)
    return tuple(out) if isinstance(out, tuple) else (out,)


def kernel_case(seed, B, L, heads, gain=1.0):
    """q, k, v [B, L, heads * 32] fp32 for the kernel tests; q and k are the halves of one [B, L, 2 E] tensor."""
    g = torch.Generator().manual_seed(seed)
    E = heads * 32
    qk = torch.randn(B, L, 2 * E, generator=g) * gain
    v = torch.randn(B, L, E, generator=g)
    return qk, v
