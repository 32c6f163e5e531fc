"""Mint golden vectors for the decoder layer, the decoder and the re-id head with the REFERENCE's own code (build container
only).

    python tests/golden/make_decoder_golden.py

The reference's classes run as they are, in float64 on the CPU:
  * MSDeformAttn is loaded as tests/golden/make_encoder_layer_golden.py loads it (its CUDA extension stands replaced by the
    reference's own `ms_deform_attn_core_pytorch`);
  * DeformableTransformerDecoderLayer, DeformableTransformerDecoder, DeformableReidHead, MLP, get_sine_pos_embed, _get_clones
    and _get_activation_fn are cut out of models/deformable_detr/deformable_transformer_dino.py with `ast` (the file imports
    the whole model zoo), inverse_sigmoid out of util/misc.py;
  * the denoising mask of layer_dn_mask is built by the statements of prepare_for_cdn that build it (models/ddetrs_dn.py,
    from `attn_mask = ...` to the end of the loop over the groups), cut out the same way, with "cuda" read as "cpu".
Seeds, shapes, parameters and inputs come from tests/decoder_cases.py.  Only inputs, outputs and the digest of the
parameters are stored (tests/golden/decoder/*.npz), and every class's state-dict keys and shapes (state_dict_keys.json).
"""
import ast
import copy
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.utils.checkpoint as checkpoint

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import decoder_cases as C                      # noqa: E402
import make_encoder_layer_golden as ENC        # noqa: E402

UNINEXT = os.path.join(ENC.REF, "projects/UNINEXT/uninext")
MISC = os.path.join(UNINEXT, "util/misc.py")
DN = os.path.join(UNINEXT, "models/ddetrs_dn.py")
WANTED = ("DeformableTransformerDecoderLayer", "DeformableTransformerDecoder", "DeformableReidHead", "MLP", "get_sine_pos_embed",
          "_get_clones", "_get_activation_fn")


def load_reference():
    ENC.load_reference_layer()
    attn = sys.modules["refops.modules.ms_deform_attn"].MSDeformAttn
    misc = [n for n in ast.parse(open(MISC).read()).body if isinstance(n, ast.FunctionDef) and n.name == "inverse_sigmoid"]
    body = [n for n in ast.parse(open(ENC.DINO).read()).body
            if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in WANTED]
    assert len(misc) == 1 and len(body) == len(WANTED)
    ns = {"torch": torch, "nn": nn, "F": F, "MSDeformAttn": attn, "checkpoint": checkpoint, "copy": copy, "math": math}
    exec(compile(ast.Module(body=misc, type_ignores=[]), MISC, "exec"), ns)
    exec(compile(ast.Module(body=body, type_ignores=[]), ENC.DINO, "exec"), ns)
    return ns


def reference_dn_mask(tgt_size, pad_size, dn_number):
    """The mask as prepare_for_cdn builds it, for pad_size = single_padding * 2 * dn_number."""
    fn = [n for n in ast.walk(ast.parse(open(DN).read())) if isinstance(n, ast.FunctionDef) and n.name == "prepare_for_cdn"][0]
    found = []

    def search(stmts):
        for k, s in enumerate(stmts):
            if (isinstance(s, ast.Assign) and isinstance(s.targets[0], ast.Name) and s.targets[0].id == "attn_mask"
                    and k + 2 < len(stmts) and isinstance(stmts[k + 2], ast.For)):
                found.append(stmts[k:k + 3])
            for field in ("body", "orelse"):
                if isinstance(getattr(s, field, None), list):
                    search(getattr(s, field))
    search(fn.body)
    assert len(found) == 1

    class OnCpu(ast.NodeTransformer):
        def visit_Constant(self, node):
            return ast.copy_location(ast.Constant("cpu"), node) if node.value == "cuda" else node

    body = [OnCpu().visit(s) for s in found[0]]
    ns = {"torch": torch, "tgt_size": tgt_size, "pad_size": pad_size, "dn_number": dn_number,
          "single_padding": pad_size // (2 * dn_number)}
    exec(compile(ast.fix_missing_locations(ast.Module(body=body, type_ignores=[])), DN, "exec"), ns)
    return ns["attn_mask"]


def keys_of(m):
    return [[k, list(v.shape)] for k, v in m.state_dict().items()]


def main():
    ns = load_reference()
    os.makedirs(C.HERE, exist_ok=True)
    layer_args = lambda cfg: dict(d_model=cfg["d_model"], d_ffn=cfg["d_ffn"], dropout=0.1, activation="relu", n_levels=C.N_LEVELS,
                                  n_heads=cfg["heads"], n_points=C.N_POINTS)
    keys = {}
    for name in C.FIXTURES:
        cfg, state, x = C.make_case(name)
        layer = ns["DeformableTransformerDecoderLayer"](**layer_args(cfg))
        arrays = {k: v.numpy() for k, v in x.items()}
        arrays["digest"] = np.float64(C.digest(state))
        with torch.no_grad():
            if cfg["kind"] == "layer":
                m = layer.double().eval()
                m.load_state_dict(state, strict=True)
                if cfg["mask"] == "dn":
                    mask = reference_dn_mask(cfg["lq"], C.DN_PAD, C.DN_NUMBER)
                    assert mask.dtype == torch.bool and torch.equal(mask, x["attn_mask"])
                    assert bool(mask[C.DN_PAD:, :C.DN_PAD].all()) and not bool(mask.all(dim=1).any())
                arrays["out"] = m(x["tgt"], x["query_pos"], x["ref"], x["src"], x["shapes"], x["lsi"], x["padding_mask"],
                                  x.get("attn_mask")).numpy()
                keys["DeformableTransformerDecoderLayer"] = keys_of(m)
            elif cfg["kind"] == "decoder":
                for twice in (False, True):
                    m = ns["DeformableTransformerDecoder"](cfg["d_model"], layer, cfg["layers"], return_intermediate=True,
                                                           look_forward_twice=twice)
                    m.bbox_embed = nn.ModuleList(ns["MLP"](cfg["d_model"], cfg["d_model"], 4, 3) for _ in range(cfg["layers"]))
                    m = m.double().eval()
                    m.load_state_dict(state, strict=True)
                    out, pts = m(x["tgt"], x["ref"], x["src"], x["shapes"], x["lsi"], x["valid_ratios"], None, x["padding_mask"],
                                 None)
                    if twice:     # the undetached points: the same values, and the same layer outputs (stored once)
                        assert np.array_equal(arrays["out"], out.numpy())
                        arrays["points_twice"] = pts.numpy()
                    else:
                        arrays["out"], arrays["points"] = out.numpy(), pts.numpy()
                keys["DeformableTransformerDecoder"] = keys_of(m)
                keys["MLP"] = keys_of(m.ref_point_head)
                # the two helpers on their own
                arrays["sine_in"] = x["ref"][:1, :8].numpy()
                arrays["sine_out"] = ns["get_sine_pos_embed"](x["ref"][:1, :8]).numpy()
                arrays["mlp_out"] = m.ref_point_head(torch.from_numpy(arrays["sine_out"])).numpy()
                arrays["logit_out"] = ns["inverse_sigmoid"](x["ref"]).numpy()
            else:
                m = ns["DeformableReidHead"](cfg["d_model"], layer, cfg["layers"]).double().eval()
                m.load_state_dict(state, strict=True)
                arrays["out"] = m(x["tgt"], x["ref"], x["src"], x["shapes"], x["lsi"], x["valid_ratios"], None, x["padding_mask"],
                                  None).numpy()
                keys["DeformableReidHead"] = keys_of(m)
        path = os.path.join(C.HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(name, {k: tuple(v.shape) for k, v in arrays.items() if k.startswith(("out", "points"))}, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 500 * 1024
    with open(os.path.join(C.HERE, "state_dict_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)


if __name__ == "__main__":
    main()
