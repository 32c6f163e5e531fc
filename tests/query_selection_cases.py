"""Shared by tests/golden/make_query_selection_golden.py, tests/test_query_selection_cpu.py and
tests/test_query_selection_gpu.py: the shapes, parameters and inputs of the fixtures under tests/golden/query_selection/, and
the error measure.

Every parameter and input is an exact dyadic (a multiple of 2 ** -STEP_BITS), so fp32 holds what the float64 reference saw.
The parameters are re-drawn here from the seed each fixture records (the generator moves on to the next seed until the
reference's own top-k is well separated, see there) and pinned by the digest the fixture records.

Pyramid (3, 50), (2, 25), (2, 13), (1, 7): S = 233, no multiple of 16, 32 or 64, so the last tile of an image is partial and a
tile straddles the two images.  Image 0 is unpadded: valid_W = 50 on level 0, where columns 0 and 49 fall on the last-bit edge
of the validity rule ((0 + 0.5) / 50 rounds to exactly fp32(0.01)).  Image 1 is padded on the right and at the bottom
(valid_W = 37, valid_H = 2 on level 0) and has a few masked tokens inside its valid area."""
import json
import os
import types

import numpy as np
import torch

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "query_selection")
TOL = 1e-4            # the project's bound: max abs error <= 1e-4 of the output's max abs, against float64 (tests/decoder_cases.py)
STEP_BITS = 10
D_MODEL, LANG_DIM = 256, 768
PYRAMID = [(3, 50), (2, 25), (2, 13), (1, 7)]
VALID_HW_IMAGE1 = [(2, 37), (1, 19), (1, 10), (1, 5)]      # (valid_H, valid_W) of image 1 per level of PYRAMID
# (level, y, x): masked tokens inside the valid area; the two in a level's first row lower that level's valid_W count by one
HOLES_IMAGE1 = [(0, 1, 5), (0, 1, 6), (0, 1, 20), (1, 0, 7), (2, 0, 3)]
MEMORY_ROW_STEP = 3   # output_memory is recorded for rows 0, 3, 6, ... and the last 8 of each image (file size)

# name -> class head, base seed, pyramid, proposals, padding on image 1
FIXTURES = {
    "vl_align": dict(head="vl_align", seed=201, levels=PYRAMID, topk=12, padded=True),
    "still": dict(head="still", seed=202, levels=PYRAMID, topk=12, padded=True),
    "one_level": dict(head="vl_align", seed=203, levels=[(1, 7)], topk=7, padded=False),
}


def vl_cfg(clamp=True):
    """The part of the reference's config VL_Align reads."""
    ns = types.SimpleNamespace
    return ns(MODEL=ns(DYHEAD=ns(PRIOR_PROB=0.01, LOG_SCALE=0.5, FUSE_CONFIG=ns(CLAMP_DOT_PRODUCT=clamp)),
                       LANGUAGE_BACKBONE=ns(LANG_DIM=LANG_DIM), DDETRS=ns(HIDDEN_DIM=D_MODEL)))


def dyadic(t, scale=1.0):
    step = float(1 << STEP_BITS)
    return torch.round(t.double() * scale * step) / step


def rel_err(got, want):
    want = torch.as_tensor(want).double()
    return float((got.detach().cpu().double() - want).abs().max() / want.abs().max())


def _linear(p, g, name, o, i, wstd, bstd=0.1):
    p[name + ".weight"] = dyadic(torch.randn(o, i, generator=g), wstd)
    p[name + ".bias"] = dyadic(torch.randn(o, generator=g), bstd)


def padding_mask(levels, padded):
    """[2, S] bool, True = padded."""
    S = sum(h * w for h, w in levels)
    mask = torch.zeros(2, S, dtype=torch.bool)
    if padded:
        start = 0
        for (H, W), (vh, vw) in zip(levels, VALID_HW_IMAGE1):
            m = torch.zeros(H, W, dtype=torch.bool)
            m[vh:, :] = True
            m[:, vw:] = True
            mask[1, start:start + H * W] = m.flatten()
            start += H * W
        starts = np.concatenate(([0], np.cumsum([h * w for h, w in levels])[:-1]))
        for lvl, y, x in HOLES_IMAGE1:
            mask[1, int(starts[lvl]) + y * levels[lvl][1] + x] = True
    return mask


def make_case(name, seed=None):
    """(cfg, states, inputs) of a fixture, float64, from its seed alone.  states: one reference-keyed state dict each for
    enc_output, enc_output_norm, class_embed and bbox_embed."""
    cfg = dict(FIXTURES[name])
    cfg["seed"] = cfg["seed"] if seed is None else int(seed)
    g = torch.Generator().manual_seed(cfg["seed"])
    d = D_MODEL
    S = sum(h * w for h, w in cfg["levels"])
    st = {"enc_output": {}, "enc_output_norm": {}, "class_embed": {}, "bbox_embed": {}}
    _linear(st["enc_output"], g, "", d, d, d ** -0.5)
    st["enc_output"] = {k[1:]: v for k, v in st["enc_output"].items()}
    st["enc_output_norm"]["weight"] = dyadic(1.0 + 0.1 * torch.randn(d, generator=g))
    st["enc_output_norm"]["bias"] = dyadic(torch.randn(d, generator=g), 0.1)
    if cfg["head"] == "vl_align":
        c = st["class_embed"]
        _linear(c, g, "dot_product_projection_text", d, LANG_DIM, 4.0 * LANG_DIM ** -0.5)
        c["log_scale"] = torch.tensor([0.5], dtype=torch.float64)
        c["bias_lang"] = dyadic(torch.randn(LANG_DIM, generator=g), 0.05)
        c["bias0"] = dyadic(torch.tensor([-4.59511985]))
    else:
        _linear(st["class_embed"], g, "body", 1, d, 2.0 * d ** -0.5)
    _linear(st["bbox_embed"], g, "layers.0", d, d, d ** -0.5)
    _linear(st["bbox_embed"], g, "layers.1", d, d, d ** -0.5)
    _linear(st["bbox_embed"], g, "layers.2", 4, d, d ** -0.5)
    x = {"memory": dyadic(torch.randn(2, S, d, generator=g)), "lang_feat_pool": dyadic(torch.randn(2, LANG_DIM, generator=g)),
         "mask": padding_mask(cfg["levels"], cfg["padded"]), "shapes": torch.as_tensor(cfg["levels"], dtype=torch.long)}
    return cfg, st, x


def digest(states):
    return float(sum(float(v.double().abs().sum()) for st in states.values() for v in st.values()))


def memory_rows(S):
    """The rows of each image whose output_memory the fixtures record."""
    return sorted(set(range(0, S, MEMORY_ROW_STEP)) | set(range(max(S - 8, 0), S)))


def load(name):
    z = np.load(os.path.join(HERE, name + ".npz"))
    return {k: z[k] for k in z.files}


def recorded_keys(fixture):
    return json.loads(str(fixture["keys_json"]))


def build(cfg, states, dtype, device="cpu"):
    """The project's modules of a fixture (enc_output, enc_output_norm, class_embed, bbox_embed), loaded strictly, eval mode."""
    from uninext_amd import modules as M
    mods = {"enc_output": torch.nn.Linear(D_MODEL, D_MODEL), "enc_output_norm": torch.nn.LayerNorm(D_MODEL),
            "class_embed": M.VL_Align(vl_cfg()) if cfg["head"] == "vl_align" else M.Still_Classifier(D_MODEL),
            "bbox_embed": M.MLP(D_MODEL, D_MODEL, 4, 3)}
    for k, m in mods.items():
        m.load_state_dict(states[k], strict=True)
        mods[k] = m.to(dtype).to(device).eval()
    return mods


def run(cfg, mods, x, device="cpu", dtype=torch.float64, fused=False, all_coords=True):
    """The five outputs of TwoStageQuerySelection on the inputs of make_case (no autograd)."""
    from uninext_amd import modules as M
    sel = M.TwoStageQuerySelection()
    sel.fused = fused
    with torch.no_grad():
        return sel(x["memory"].to(dtype).to(device), x["mask"].to(device), x["shapes"].to(device), mods["enc_output"],
                   mods["enc_output_norm"], mods["class_embed"], mods["bbox_embed"], x["lang_feat_pool"].to(dtype).to(device),
                   cfg["topk"], all_coords=all_coords)
