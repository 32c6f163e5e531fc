"""Mint golden vectors for the two-stage query selection with the REFERENCE's own code (build container only).

    python tests/golden/make_query_selection_golden.py

The reference's code runs as it is, in float64 on the CPU, cut out of its files with `ast` (the files import the whole model
zoo): `agg_lang_feat`, `MLP` and the method `gen_encoder_output_proposals` of DeformableTransformerVLDINO out of
models/deformable_detr/deformable_transformer_dino.py (the method runs on a stand-in `self` that carries `enc_output` and
`enc_output_norm`), `VL_Align` and `Still_Classifier` out of models/deformable_detr/deformable_detr.py.  The selection itself
is the five statements of DeformableTransformerVLDINO.forward (:216-224), restated in main() on the reference's objects.
Shapes, parameters and inputs come from tests/query_selection_cases.py.  Stored (tests/golden/query_selection/*.npz): the
inputs, the reference's outputs, every module's state-dict keys and shapes, the seed and the digest of the parameters.

The tests demand the reference's top-k indices EXACTLY, in order.  That is sound only where the reference's own logits are
well separated, which is a condition on the fixture, asserted here (the next seed is tried when it fails): among the k + 1
largest logits of each image consecutive gaps are at least 4 TOL max|logit|, and the logit that all padded and invalid rows
share lies below the k-th by the same margin.  An implementation within TOL max|logit| of every logit then has the same order.
"""
import ast
import json
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import query_selection_cases as C              # noqa: E402
import make_encoder_layer_golden as ENC        # noqa: E402

DETR = os.path.join(ENC.REF, "projects/UNINEXT/uninext/models/deformable_detr/deformable_detr.py")


def load_reference():
    ns = {"torch": torch, "nn": nn, "F": F, "math": math}
    dino = ast.parse(open(ENC.DINO).read())
    body = [n for n in dino.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in ("agg_lang_feat", "MLP")]
    owner = [n for n in dino.body if isinstance(n, ast.ClassDef) and n.name == "DeformableTransformerVLDINO"]
    method = [n for n in owner[0].body if isinstance(n, ast.FunctionDef) and n.name == "gen_encoder_output_proposals"]
    assert len(body) == 2 and len(owner) == 1 and len(method) == 1
    exec(compile(ast.Module(body=body + method, type_ignores=[]), ENC.DINO, "exec"), ns)
    heads = [n for n in ast.parse(open(DETR).read()).body
             if isinstance(n, ast.ClassDef) and n.name in ("VL_Align", "Still_Classifier")]
    assert len(heads) == 2
    exec(compile(ast.Module(body=heads, type_ignores=[]), DETR, "exec"), ns)
    return ns


def keys_of(m):
    return [[k, list(v.shape)] for k, v in m.state_dict().items()]


def well_separated(logits, dead, k):
    """The fixture condition of the module docstring on the reference's logits [B, S]; dead [B, S]: padded or invalid rows."""
    margin = 4 * C.TOL * float(logits.abs().max())
    for lg, dd in zip(logits, dead):
        top = torch.sort(lg, descending=True)[0][:k + 1]
        if len(top) > 1 and float((top[:-1] - top[1:]).min()) < margin:
            return False
        if bool(dd.any()):
            shared = lg[dd]
            assert float(shared.max() - shared.min()) == 0.0          # one row, LayerNorm(bias), scored once
            if float(top[k - 1] - shared[0]) < margin:
                return False
    return True


def reference_outputs(ns, cfg, states, x):
    mods = {"enc_output": nn.Linear(C.D_MODEL, C.D_MODEL), "enc_output_norm": nn.LayerNorm(C.D_MODEL),
            "class_embed": ns["VL_Align"](C.vl_cfg()) if cfg["head"] == "vl_align" else ns["Still_Classifier"](C.D_MODEL),
            "bbox_embed": ns["MLP"](C.D_MODEL, C.D_MODEL, 4, 3)}
    for k in mods:
        mods[k] = mods[k].double().eval()
        mods[k].load_state_dict(states[k], strict=True)
    owner = types.SimpleNamespace(enc_output=mods["enc_output"], enc_output_norm=mods["enc_output_norm"])
    with torch.no_grad():
        output_memory, output_proposals = ns["gen_encoder_output_proposals"](owner, x["memory"], x["mask"], x["shapes"])
        enc_outputs_class = mods["class_embed"](output_memory, x["lang_feat_pool"].unsqueeze(1))
        enc_outputs_coord_unact = mods["bbox_embed"](output_memory) + output_proposals
        topk_proposals = torch.topk(enc_outputs_class[..., 0], cfg["topk"], dim=1)[1]
        topk_coords_unact = torch.gather(enc_outputs_coord_unact, 1, topk_proposals.unsqueeze(-1).repeat(1, 1, 4))
        reference_points = topk_coords_unact.sigmoid()
    assert output_proposals.dtype == torch.float32 and enc_outputs_class.shape[-1] == 1
    out = dict(output_memory=output_memory, output_proposals=output_proposals, enc_outputs_class=enc_outputs_class,
               enc_outputs_coord_unact=enc_outputs_coord_unact, topk_proposals=topk_proposals,
               topk_coords_unact=topk_coords_unact, reference_points=reference_points)
    return mods, out


def main():
    ns = load_reference()
    os.makedirs(C.HERE, exist_ok=True)
    for name in C.FIXTURES:
        for attempt in range(200):
            cfg, states, x = C.make_case(name, C.FIXTURES[name]["seed"] + 1000 * attempt)
            mods, out = reference_outputs(ns, cfg, states, x)
            dead = torch.isinf(out["output_proposals"]).any(-1)
            if well_separated(out["enc_outputs_class"][..., 0], dead, cfg["topk"]):
                break
        else:
            raise AssertionError("%s: no seed with a well-separated top-k" % name)
        assert well_separated(out["enc_outputs_class"][..., 0], dead, cfg["topk"])
        S = x["memory"].shape[1]
        if cfg["padded"]:       # both last-bit columns of image 0 are out, its other level-0 columns are in, padding is out
            W = cfg["levels"][0][1]
            assert W == 50 and bool(dead[0, [0, 49, 50, 99]].all()) and not bool(dead[0, 1:49].any())
            assert bool(dead[1][x["mask"][1]].all()) and 0 < int(dead[1].sum()) < S
        else:
            assert not bool(dead.any())
        rows = C.memory_rows(S)
        arrays = {"memory": x["memory"].float().numpy(), "lang_feat_pool": x["lang_feat_pool"].float().numpy(),
                  "mask": x["mask"].numpy(), "shapes": x["shapes"].numpy(), "seed": np.int64(cfg["seed"]),
                  "digest": np.float64(C.digest(states)), "memory_rows": np.asarray(rows, dtype=np.int64),
                  "keys_json": np.array(json.dumps({k: keys_of(m) for k, m in mods.items()}))}
        assert np.array_equal(arrays["memory"].astype(np.float64), x["memory"].numpy())      # dyadic: fp32 holds them
        for k, v in out.items():
            arrays[k] = v[:, rows].numpy() if k == "output_memory" else v.numpy()
        if name == "vl_align":      # the pooling helper and the general head ([B, Q, hidden] x [B, L, lang_dim]) on their own
            g = torch.Generator().manual_seed(7)
            feats = C.dyadic(torch.randn(2, 5, C.LANG_DIM, generator=g))
            tokens = torch.tensor([[1, 1, 1, 0, 0], [1, 1, 1, 1, 1]], dtype=torch.bool)
            arrays["agg_features"], arrays["agg_mask"] = feats.numpy(), tokens.numpy()
            arrays["agg_average"] = ns["agg_lang_feat"](feats, tokens, "average").numpy()
            arrays["agg_max"] = ns["agg_lang_feat"](feats, tokens, "max").numpy()
            with torch.no_grad():
                arrays["align_general"] = mods["class_embed"](out["output_memory"][:, :9], feats).numpy()
        path = os.path.join(C.HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(name, "seed", cfg["seed"], "dead rows", [int(v) for v in dead.sum(1)], os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 900 * 1024


if __name__ == "__main__":
    main()
