"""Mint golden vectors for the encoder's input preparation with the REFERENCE's own code (build container only).

    python tests/golden/make_encoder_input_golden.py

Cut out of the reference with `ast` and run as they are, on the CPU:
  * PositionEmbeddingSine (models/deformable_detr/position_encoding.py), in fp32: the class fixes that dtype itself;
  * get_valid_ratio and the flatten statements of DeformableTransformerVLDINO.forward, from `src_flatten = []` to
    `valid_ratios = ...` (models/deformable_detr/deformable_transformer_dino.py);
  * DeformableTransformerEncoderVL with its static get_reference_points, _get_clones and _get_clones_advanced (same file).
The loop over the backbone's features (models/ddetrs_dn.py:117-143) is restated here on plain tensors: a backbone level's mask is
the image mask resized as backbone.py resizes it, a further level's mask comes from masks[0]; input_proj is torch's own
nn.Sequential(Conv2d, GroupNorm(32, 256)) in float64.  Seeds, shapes and inputs come from tests/encoder_input_cases.py.  Only
inputs, outputs (tests/golden/encoder_input/*.npz) and state-dict keys and shapes (state_dict_keys.json) are stored."""
import ast
import copy
import json
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.utils.checkpoint as checkpoint

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import encoder_input_cases as C                # noqa: E402
import make_encoder_layer_golden as ENC        # noqa: E402

POS = os.path.join(ENC.REF, "projects/UNINEXT/uninext/models/deformable_detr/position_encoding.py")


def load_reference():
    ns = {"torch": torch, "nn": nn, "F": F, "math": math, "copy": copy, "checkpoint": checkpoint, "NestedTensor": object}
    body = [n for n in ast.parse(open(POS).read()).body if isinstance(n, ast.ClassDef) and n.name == "PositionEmbeddingSine"]
    assert len(body) == 1
    exec(compile(ast.Module(body=body, type_ignores=[]), POS, "exec"), ns)
    tree = ast.parse(open(ENC.DINO).read())
    wanted = ("DeformableTransformerEncoderVL", "_get_clones", "_get_clones_advanced")
    body = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in wanted]
    assert len(body) == len(wanted)
    exec(compile(ast.Module(body=body, type_ignores=[]), ENC.DINO, "exec"), ns)
    dino = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "DeformableTransformerVLDINO"][0]
    ratio = [n for n in dino.body if isinstance(n, ast.FunctionDef) and n.name == "get_valid_ratio"][0]
    ratio.decorator_list = []
    exec(compile(ast.Module(body=[ratio], type_ignores=[]), ENC.DINO, "exec"), ns)
    forward = [n for n in dino.body if isinstance(n, ast.FunctionDef) and n.name == "forward"][0]
    target = lambda s: s.targets[0].id if isinstance(s, ast.Assign) and isinstance(s.targets[0], ast.Name) else None
    first = [k for k, s in enumerate(forward.body) if target(s) == "src_flatten"][0]
    last = [k for k, s in enumerate(forward.body) if target(s) == "valid_ratios"][0]
    ns["flatten_code"] = compile(ast.Module(body=forward.body[first:last + 1], type_ignores=[]), ENC.DINO, "exec")
    return ns


def reference_run(ns, case):
    proj = nn.ModuleList(nn.Sequential(nn.Conv2d(c, C.D_MODEL, kernel_size=1), nn.GroupNorm(32, C.D_MODEL)) for c in C.IN_CHANNELS)
    proj.append(nn.Sequential(nn.Conv2d(C.IN_CHANNELS[-1], C.D_MODEL, kernel_size=3, stride=2, padding=1), nn.GroupNorm(32, C.D_MODEL)))
    proj.load_state_dict(case["state"], strict=True)
    keys = [[k, list(v.shape)] for k, v in proj.state_dict().items()]
    proj = proj.double().eval()
    embed = ns["PositionEmbeddingSine"](C.D_MODEL // 2, normalize=True)
    Nested = lambda t, m: types.SimpleNamespace(tensors=t, mask=m)
    feats, image_mask = [f.double() for f in case["features"]], case["image_mask"]
    srcs, masks, poses = [], [], []
    for l, feat in enumerate(feats):
        mask = F.interpolate(image_mask[None].float(), size=feat.shape[-2:]).to(torch.bool)[0]
        srcs.append(proj[l](feat))
        masks.append(mask)
        poses.append(embed(Nested(feat, mask)))
    for l in range(len(feats), len(proj)):
        src = proj[l](feats[-1]) if l == len(feats) else proj[l](srcs[-1])
        m = masks[0]
        mask = F.interpolate(m[None].float(), size=src.shape[-2:]).to(torch.bool)[0]
        srcs.append(src)
        masks.append(mask)
        poses.append(embed(Nested(src, mask)))
    assert all(p.dtype == torch.float32 for p in poses)
    self = types.SimpleNamespace(level_embed=case["level_embed"], get_valid_ratio=lambda m: ns["get_valid_ratio"](None, m))
    scope = {"torch": torch, "self": self, "srcs": srcs, "masks": masks, "pos_embeds": poses}
    exec(ns["flatten_code"], scope)
    out = {k: scope[k] for k in ("src_flatten", "mask_flatten", "lvl_pos_embed_flatten", "spatial_shapes", "level_start_index", "valid_ratios")}
    out["reference_points"] = ns["DeformableTransformerEncoderVL"].get_reference_points(out["spatial_shapes"], out["valid_ratios"], "cpu")
    assert out["src_flatten"].dtype == torch.float64 and out["lvl_pos_embed_flatten"].dtype == torch.float32
    assert out["reference_points"].dtype == torch.float32 and out["valid_ratios"].dtype == torch.float32
    return out, keys


def main():
    ns = load_reference()
    os.makedirs(C.HERE, exist_ok=True)
    keys = {}
    with torch.no_grad():
        for name in C.FIXTURES:
            case = C.make_case(name)
            out, keys["input_proj"] = reference_run(ns, case)
            assert tuple(map(tuple, out["spatial_shapes"].tolist())) == C.LEVELS
            arrays = {k: v.numpy() for k, v in out.items()}
            path = os.path.join(C.HERE, name + ".npz")
            np.savez_compressed(path, **arrays)
            print(name, {k: tuple(v.shape) for k, v in arrays.items()}, os.path.getsize(path), "bytes",
                  "masked tokens", int(out["mask_flatten"].sum()))
            assert os.path.getsize(path) < 500 * 1024
    enc = ns["DeformableTransformerEncoderVL"](nn.Linear(2, 2), nn.Linear(3, 3), nn.Identity(), C.ENCODER_VL_STUB["num_layers"],
                                               num_vl_layers=C.ENCODER_VL_STUB["num_vl_layers"])
    keys["DeformableTransformerEncoderVL"] = [[k, list(v.shape)] for k, v in enc.state_dict().items()]
    keys["DeformableTransformerEncoderVL.children"] = [[n, type(m).__name__, [type(c).__name__ for c in m]] for n, m in enc.named_children()]
    with open(os.path.join(C.HERE, "state_dict_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)


if __name__ == "__main__":
    main()
