"""Mint known-answer loss dictionaries with the REFERENCE criterion (build container only).

    python tests/golden/make_criterion_golden.py

Takes `SetCriterion`, `DINOCriterion`, `compute_box_iou` and `dice_coefficient`
(projects/UNINEXT/uninext/models/deformable_detr/deformable_detr.py:290-784, :853-879) and `dice_loss`, `sigmoid_focal_loss`,
`token_sigmoid_binary_focal_loss` (segmentation.py:74-166) out of the reference checkout with `ast` at generation time (the
modules themselves import detectron2, fvcore and friends) and executes them on the seeded CPU inputs of
tests/criterion_cases.py, with stand-ins for what they take from outside: `box_ops` (uninext_amd.matcher's box helpers),
`nested_tensor_from_tensor_list` (uninext_amd.criterion.pad_masks), `giou_loss` (fvcore is not installed:
uninext_amd.criterion.giou_loss, the restatement tests/test_criterion_cpu.py pins by hand), `is_dist_avail_and_initialized` and
`get_world_size` (one process).  The reference hard-codes `.cuda()` / `.to("cuda")` in compute_dn_loss; the syntax tree is
rewritten to stay on the CPU before it is compiled.  The encoder's proposals are matched by uninext_amd.matcher's
HungarianMatcherVL (index-for-index the reference's, tests/test_matcher_cpu.py); the decoder layers' indices are precomputed.

Nothing of the reference's text is stored: a fixture (tests/golden/criterion/*.npz) holds the inputs and the reference's loss
values under "expect.<key>".
"""
import ast
import copy
import os
import random
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import criterion_cases as C  # noqa: E402
from uninext_amd import criterion as ours  # noqa: E402
from uninext_amd import matcher  # noqa: E402

REF = os.environ.get("UNINEXT_REFERENCE", "/root/reference")
DDETR = os.path.join(REF, "projects/UNINEXT/uninext/models/deformable_detr/deformable_detr.py")
SEG = os.path.join(REF, "projects/UNINEXT/uninext/models/deformable_detr/segmentation.py")
OUT = os.path.join(HERE, "criterion")


class StayOnCpu(ast.NodeTransformer):
    """x.cuda() -> x;  x.to("cuda") -> x.to("cpu")"""

    def visit_Call(self, node):
        self.generic_visit(node)
        if isinstance(node.func, ast.Attribute) and node.func.attr == "cuda" and not node.args:
            return node.func.value
        if isinstance(node.func, ast.Attribute) and node.func.attr == "to" and len(node.args) == 1 \
                and isinstance(node.args[0], ast.Constant) and node.args[0].value == "cuda":
            node.args[0] = ast.Constant("cpu")
        return node


def pick(path, names):
    tree = ast.parse(open(path).read())
    found = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert sorted(n.name for n in found) == sorted(names), [n.name for n in found]
    return [ast.fix_missing_locations(StayOnCpu().visit(n)) for n in found]


def load_reference():
    ns = {"torch": torch, "F": F, "nn": nn, "copy": copy, "random": random,
          "box_ops": types.SimpleNamespace(box_cxcywh_to_xyxy=matcher.box_cxcywh_to_xyxy, box_area=matcher.box_area),
          "nested_tensor_from_tensor_list": lambda masks, size_divisibility=1, split=True: types.SimpleNamespace(
              decompose=lambda: (ours.pad_masks(masks, size_divisibility), None)),
          "giou_loss": ours.giou_loss, "is_dist_avail_and_initialized": lambda: False, "get_world_size": lambda: 1}
    body = pick(SEG, ["dice_loss", "sigmoid_focal_loss", "token_sigmoid_binary_focal_loss"]) + \
        pick(DDETR, ["compute_box_iou", "dice_coefficient", "SetCriterion", "DINOCriterion"])
    exec(compile(ast.Module(body=body, type_ignores=[]), DDETR, "exec"), ns)
    return ns


def main():
    ns = load_reference()
    os.makedirs(OUT, exist_ok=True)
    for name, cfg in C.CASES.items():
        flat = C.make_inputs(cfg)
        outputs, targets, indices_list, dn_metas = C.rebuild({k: v.clone() for k, v in flat.items()}, cfg)
        crit = ns["DINOCriterion"](matcher.HungarianMatcherVL(**C.WEIGHTS), {}, C.LOSSES, focal_alpha=0.25,
                                   mask_out_stride=C.STRIDE, ota=cfg["ota"], still_cls_for_encoder=cfg["still"])
        losses = crit(outputs, targets, indices_list, dn_metas)
        save = {k: v.numpy() for k, v in flat.items()}
        for key, value in losses.items():
            save["expect." + key] = np.float64(float(value))
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **save)
        print(name, len(losses), "keys", os.path.getsize(path) // 1024, "KB", {k: round(float(v), 4) for k, v in sorted(losses.items())[:6]})
        assert os.path.getsize(path) <= 256 * 1024


if __name__ == "__main__":
    main()
