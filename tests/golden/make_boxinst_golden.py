"""Mint the BoxInst fixtures with the REFERENCE's functions (build container only).

    python tests/golden/make_boxinst_golden.py

Takes `SetCriterion` with `loss_masks_boxinst`, `unfold_wo_center`, `compute_project_term`, `compute_pairwise_term`,
`dice_coefficient` (projects/UNINEXT/uninext/models/deformable_detr/deformable_detr.py) and `prepare_image_targets_boxinst`,
`add_bitmasks_from_boxes`, `get_images_color_similarity`, `unfold_wo_center` (projects/UNINEXT/uninext/uninext_img.py:529-659) out
of the reference checkout with `ast` at generation time, as tests/golden/make_criterion_golden.py does (whose namespace of
stand-ins is reused), and executes them on the seeded CPU inputs of tests/boxinst_cases.py.  Stand-ins for what the two methods of
the meta-architecture take from outside: `ImageList.from_tensors` (zero padding to the divisibility, detectron2's rule), the
normalizer and `prepare_targets_boxinst` (identities: their results are not part of the fixture), an `Instances` look-alike that
holds `gt_boxes.tensor`, and -- skimage is not installed here -- `skimage.color` is replaced by THIS repository's
`uninext_amd.boxinst.rgb2lab`, the restatement tests/test_boxinst_cpu.py anchors on published Lab values.  So the targets fixture
pins everything around the Lab conversion with the reference's own code, and the conversion itself only as far as those anchors go.

Nothing of the reference's text is stored: tests/golden/boxinst/targets.npz holds the reference's bitmasks and colour
similarities, the loss fixtures their inputs and the reference's two losses under "expect.<key>" with `_iter` after the call.
"""
import ast
import os
import random
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import boxinst_cases as B  # noqa: E402
import make_criterion_golden as M  # noqa: E402
from uninext_amd import boxinst as ours  # noqa: E402

IMG = os.path.join(M.REF, "projects/UNINEXT/uninext/uninext_img.py")
OUT = os.path.join(HERE, "boxinst")


def pick_methods(path, names):
    """The named methods of whichever class of the file defines them, and the named module-level functions."""
    tree = ast.parse(open(path).read())
    found = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    for cls in (n for n in tree.body if isinstance(n, ast.ClassDef)):
        found += [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in found) == sorted(names), [n.name for n in found]
    return [ast.fix_missing_locations(n) for n in found]


class FakeInstances:
    def __init__(self, boxes):
        self.gt_boxes = types.SimpleNamespace(tensor=boxes)

    def to(self, device):
        return self

    def __len__(self):
        return len(self.gt_boxes.tensor)


def reference_targets():
    image_list = types.SimpleNamespace(from_tensors=lambda tensors, size_divisibility=0, pad_value=0.0: types.SimpleNamespace(
        tensor=ours._pad_batch(tensors, size_divisibility, pad_value)))
    ns = {"torch": torch, "F": F, "ImageList": image_list, "color": types.SimpleNamespace(rgb2lab=ours.rgb2lab)}
    names = ["prepare_image_targets_boxinst", "add_bitmasks_from_boxes", "get_images_color_similarity", "unfold_wo_center"]
    exec(compile(ast.Module(body=pick_methods(IMG, names), type_ignores=[]), IMG, "exec"), ns)
    images, heights, boxes = B.make_target_inputs()
    me = types.SimpleNamespace(device="cpu", normalizer=lambda x: x.float(), bottom_pixels_removed=10, mask_stride=B.STRIDE,
                               pairwise_size=B.SIZE, pairwise_dilation=B.DILATION, prepare_targets_boxinst=lambda inst: inst)
    me.add_bitmasks_from_boxes = lambda *a: ns["add_bitmasks_from_boxes"](me, *a)
    batched = [{"image": im, "instances": FakeInstances(bx), "height": ht} for im, bx, ht in zip(images, boxes, heights)]
    _, instances = ns["prepare_image_targets_boxinst"](me, batched)
    save = {}
    for b, inst in enumerate(instances):
        sim = inst.image_color_similarity
        assert all(torch.equal(sim[0], s) for s in sim)                 # the reference's G_i copies are one tensor
        save["masks.%d" % b] = inst.gt_bitmasks_full.bool().numpy()
        save["sim.%d" % b] = sim[0].numpy()
    return save


def main():
    os.makedirs(OUT, exist_ok=True)
    save = reference_targets()
    path = os.path.join(OUT, "targets.npz")
    np.savez_compressed(path, **save)
    B.load_targets.cache_clear()
    print("targets", {k: v.shape for k, v in save.items()}, os.path.getsize(path) // 1024, "KB")
    ns = M.load_reference()
    names = ["unfold_wo_center", "compute_project_term", "compute_pairwise_term"]
    exec(compile(ast.Module(body=M.pick(M.DDETR, names), type_ignores=[]), M.DDETR, "exec"), ns)
    for name, cfg in B.LOSS_CASES.items():
        flat = B.make_loss_inputs(cfg)
        outputs, targets, indices = B.rebuild_loss({k: v.clone() for k, v in flat.items()}, cfg)
        crit = ns["SetCriterion"](None, {}, ["masks_boxinst"], mask_out_stride=B.STRIDE, cfg=B.boxinst_cfg(cfg))
        crit._iter.fill_(cfg["iter0"])
        if cfg["rseed"] is not None:
            random.seed(cfg["rseed"])
        losses = crit.loss_masks_boxinst(outputs, targets, indices, 7.0)
        out = {k: v.numpy() for k, v in flat.items()}
        for key, value in losses.items():
            out["expect." + key] = np.float64(float(value))
        out["expect.iter"] = np.float64(float(crit._iter))
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print(name, {k: round(float(v), 6) for k, v in losses.items()}, "iter", float(crit._iter), os.path.getsize(path) // 1024, "KB")
        assert os.path.getsize(path) <= 256 * 1024


if __name__ == "__main__":
    main()
