"""Mint golden vectors for the decoder prediction heads with the REFERENCE's own code (build container only).

    python tests/golden/make_pred_heads_golden.py

The reference's code runs as it is, in float64 on the CPU, cut out of its files with `ast` (the files import the whole model
zoo): `VL_Align` and `Still_Classifier` out of models/deformable_detr/deformable_detr.py, `MLP` and `agg_lang_feat` out of
models/deformable_detr/deformable_transformer_dino.py, `inverse_sigmoid` out of util/misc.py.  The heads themselves are the
statements of DDETRSegmUniDN.coco_inference (models/ddetrs_dn.py:396-401, :413-435 and :468-483), restated in
reference_outputs() on the reference's objects.  Shapes, parameters and inputs come from tests/pred_heads_cases.py.  Stored
(tests/golden/pred_heads/*.npz): the reference's outputs, every submodule's state-dict keys and shapes, the seed and the
digest of the parameters; the inputs are re-drawn from the seed."""
import ast
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import pred_heads_cases as C                   # noqa: E402
import query_selection_cases as QC             # noqa: E402
import make_encoder_layer_golden as ENC        # noqa: E402

DETR = os.path.join(ENC.REF, "projects/UNINEXT/uninext/models/deformable_detr/deformable_detr.py")
MISC = os.path.join(ENC.REF, "projects/UNINEXT/uninext/util/misc.py")


def load_reference():
    ns = {"torch": torch, "nn": nn, "F": F, "math": math}
    for path, kinds, names in ((ENC.DINO, (ast.ClassDef, ast.FunctionDef), ("agg_lang_feat", "MLP")),
                               (DETR, (ast.ClassDef,), ("VL_Align", "Still_Classifier")),
                               (MISC, (ast.FunctionDef,), ("inverse_sigmoid",))):
        body = [n for n in ast.parse(open(path).read()).body if isinstance(n, kinds) and n.name in names]
        assert len(body) == len(names), path
        exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def keys_of(m):
    return [[k, list(v.shape)] for k, v in m.state_dict().items()]


def reference_outputs(ns, cfg, states, x):
    d = C.D_MODEL
    head = (lambda: ns["VL_Align"](QC.vl_cfg())) if cfg["head"] == "vl_align" else (lambda: ns["Still_Classifier"](d))
    mods = {"class_embed": nn.ModuleList(head() for _ in range(C.LEVELS)),
            "bbox_embed": nn.ModuleList(ns["MLP"](d, d, 4, 3) for _ in range(C.LEVELS)),
            "controller": ns["MLP"](d, d, cfg["P"], 3)}
    if cfg["iou"]:
        mods["iou_head"] = nn.ModuleList(nn.Linear(d, 1) for _ in range(C.LEVELS))
    for k in mods:
        mods[k] = mods[k].double().eval()
        mods[k].load_state_dict(states[k], strict=True)
    inverse_sigmoid, agg_lang_feat = ns["inverse_sigmoid"], ns["agg_lang_feat"]
    hs, init_reference, inter_references, task = x["hs"], x["init_reference"], x["inter_references"], cfg["task"]
    language_dict_features = {"hidden": x["hidden"], "masks": x["masks"]}
    outputs = {}
    with torch.no_grad():
        if task == "grounding" or task == "sot":
            lang_feat_pool = agg_lang_feat(language_dict_features["hidden"], language_dict_features["masks"],
                                           pool_type="average").unsqueeze(1)
        lvl = hs.shape[0] - 1
        reference = init_reference if lvl == 0 else inter_references[lvl - 1]
        reference = inverse_sigmoid(reference)
        if task == "grounding" or task == "sot":
            outputs_class = mods["class_embed"][lvl](hs[lvl], lang_feat_pool)
        else:
            outputs_class = mods["class_embed"][lvl](hs[lvl], language_dict_features["hidden"])
        tmp = mods["bbox_embed"][lvl](hs[lvl])
        if cfg["iou"]:
            outputs["pred_boxious"] = mods["iou_head"][lvl](hs[lvl])
        if reference.shape[-1] == 4:
            tmp += reference
        else:
            assert reference.shape[-1] == 2
            tmp[..., :2] += reference
        outputs["pred_logits"], outputs["pred_boxes"] = outputs_class, tmp.sigmoid()
        points = inter_references[-2, :, :, :2]
        dynamic_mask_head_params = mods["controller"](hs[lvl])
        reference_points = []
        for i, (orig_h, orig_w) in enumerate(x["image_sizes"]):
            scale_f = torch.stack([torch.as_tensor(orig_w).to(points[i]), torch.as_tensor(orig_h).to(points[i])], dim=0)
            reference_points.append((points[i] * scale_f[None, :]).unsqueeze(0))
        outputs["reference_points"] = torch.cat(reference_points, dim=1)
        outputs["mask_head_params"] = dynamic_mask_head_params.reshape(1, -1, dynamic_mask_head_params.shape[-1])
    return mods, outputs


def main():
    ns = load_reference()
    os.makedirs(C.HERE, exist_ok=True)
    for name in C.FIXTURES:
        cfg, states, x = C.make_case(name)
        for k in ("hs", "init_reference", "inter_references", "hidden"):      # dyadic: fp32 holds them
            assert torch.equal(x[k].float().double(), x[k]), k
        used = x["inter_references"][C.LEVELS - 2]
        for v in C.EDGE_VALUES:                                               # both clamps of inverse_sigmoid are hit
            assert bool((used[:, :4] == v).any()) and bool((used[:, -4:] == v).any())
        mods, out = reference_outputs(ns, cfg, states, x)
        T = C.tokens_of(cfg)
        assert tuple(out["pred_logits"].shape) == (C.B, C.Q, T) and tuple(out["pred_boxes"].shape) == (C.B, C.Q, 4)
        assert tuple(out["mask_head_params"].shape) == (1, C.B * C.Q, cfg["P"])
        assert tuple(out["reference_points"].shape) == (1, C.B * C.Q, 2) and ("pred_boxious" in out) == cfg["iou"]
        assert all(bool(torch.isfinite(v).all()) for v in out.values())
        arrays = {"seed": np.int64(cfg["seed"]), "digest": np.float64(C.digest(states)),
                  "keys_json": np.array(json.dumps({k: keys_of(m) for k, m in mods.items()}))}
        arrays.update({k: v.numpy() for k, v in out.items()})
        path = os.path.join(C.HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(name, "T", T, "max |logit| %.3f" % float(out["pred_logits"].abs().max()), os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 900 * 1024


if __name__ == "__main__":
    main()
