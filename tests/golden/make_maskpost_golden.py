"""Mint known-answer masks and keep flags with the REFERENCE mask post-processing (build container only).

    python tests/golden/make_maskpost_golden.py

Takes, with `ast` at generation time, the mask lines of `UNINEXT_IMG.inference` (projects/UNINEXT/uninext/uninext_img.py:474-480,
the `if self.mask_on:` statement), `segmentation_postprocess` (models/deformable_detr/segmentation.py:25-71) and `mask_iou` /
`mask_nms` (models/tracker.py:17-46) out of the reference checkout and executes them on seeded CPU inputs, with stand-ins for
the `Instances` and `Boxes` containers.  Nothing of the reference's text is stored.  tests/golden/maskpost/binarize.npz holds
the logit planes and, per case of tests/maskpost_cases.py, the reference's masks bit-packed with np.packbits;
tests/golden/maskpost/nms.npz holds, per case, the ellipses the logits are rebuilt from (tests/maskpost_cases.py: nms_logits;
300 planes of logits would not fit a fixture), the reference's binarised masks bit-packed, and its keep flags.

The generator ASSERTS, and reseeds until they hold:
  (a) with the float64 logit of every output pixel (F.interpolate on doubles) and the band 8 * 2^-23 * max(1, max |logit|) around
      logit(thres): at most 1e-4 of a case's pixels lie in the band, and outside it the reference's fp32 masks equal the float64
      decision;
  (b) every mask IoU of an NMS case is at least 1e-4 away from the threshold (and the restatement of mask_nms from the matrix of
      all pairs, which the tests use beyond the fixtures, gives the reference's flags).
"""
import ast
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import maskpost_cases as M  # noqa: E402

REF = os.environ.get("UNINEXT_REFERENCE", "/root/reference")
UNINEXT = os.path.join(REF, "projects/UNINEXT/uninext")
MAX_BYTES = 540 * 1024          # the largest file of tests/golden/postprocess/


class Boxes:
    def __init__(self, tensor):
        self.tensor = tensor.clone()

    def scale(self, scale_x, scale_y):
        self.tensor[:, 0::2] *= scale_x
        self.tensor[:, 1::2] *= scale_y

    def clip(self, box_size):
        h, w = box_size
        self.tensor[:, 0::2] = self.tensor[:, 0::2].clamp(min=0, max=w)
        self.tensor[:, 1::2] = self.tensor[:, 1::2].clamp(min=0, max=h)

    def nonempty(self, threshold=0.0):
        return ((self.tensor[:, 2] - self.tensor[:, 0]) > threshold) & ((self.tensor[:, 3] - self.tensor[:, 1]) > threshold)

    def __getitem__(self, item):
        return Boxes(self.tensor[item])


class Instances:
    def __init__(self, image_size, **fields):
        object.__setattr__(self, "image_size", image_size)
        object.__setattr__(self, "_fields", dict(fields))

    def __setattr__(self, name, value):
        self._fields[name] = value

    def __getattr__(self, name):
        try:
            return self._fields[name]
        except KeyError:
            raise AttributeError(name)

    def has(self, name):
        return name in self._fields

    def get_fields(self):
        return self._fields

    def __getitem__(self, item):
        return Instances(self.image_size, **{k: v[item] for k, v in self._fields.items()})


def _functions(path, names):
    tree = ast.parse(open(path).read())
    picked = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in picked) == sorted(names), path
    return picked


def load_reference():
    """(mask_lines(me, mask_pred_i, image_size) -> result, segmentation_postprocess, mask_nms) from the reference's source."""
    src = os.path.join(UNINEXT, "uninext_img.py")
    inference, = _functions(src, ["inference"])
    lines = [n for n in ast.walk(inference) if isinstance(n, ast.If) and ast.unparse(n.test) == "self.mask_on"]
    assert len(lines) == 1
    code = compile(ast.Module(body=lines, type_ignores=[]), src, "exec")

    def mask_lines(me, mask_pred_i, image_size):
        ns = {"self": me, "mask_pred_i": mask_pred_i, "image_size": image_size, "result": Instances(image_size), "F": F,
              "torch": torch}
        exec(code, ns)
        return ns["result"]

    seg = os.path.join(UNINEXT, "models/deformable_detr/segmentation.py")
    ns = {"torch": torch, "F": F, "Instances": Instances}
    exec(compile(ast.Module(body=_functions(seg, ["segmentation_postprocess"]), type_ignores=[]), seg, "exec"), ns)
    trk = os.path.join(UNINEXT, "models/tracker.py")
    ns2 = {"torch": torch, "F": F}
    exec(compile(ast.Module(body=_functions(trk, ["mask_iou", "mask_nms"]), type_ignores=[]), trk, "exec"), ns2)
    return mask_lines, ns["segmentation_postprocess"], ns2["mask_nms"]


def reference_masks(mask_lines, seg_post, planes, rows, stride, crop, out, thres):
    me = types.SimpleNamespace(mask_on=True, mask_stride=stride, mask_thres=thres)
    result = mask_lines(me, planes[list(rows)].unsqueeze(1), crop)
    assert tuple(result.pred_masks.shape) == (len(rows), 1) + tuple(crop) and result.pred_masks.dtype == torch.bool
    result.pred_boxes = Boxes(torch.tensor([[0.0, 0.0, crop[1], crop[0]]]).repeat(len(rows), 1))
    result = seg_post(result, out[0], out[1])
    masks = result.pred_masks
    assert tuple(masks.shape) == (len(rows),) + tuple(out) and masks.dtype == torch.uint8
    if out == crop:                 # the nearest step is the identity: these are inference()'s masks
        assert torch.equal(masks, mask_lines(me, planes[list(rows)].unsqueeze(1), crop).pred_masks[:, 0].byte())
    return masks


def binarize_fixture(mask_lines, seg_post):
    for seed in range(1, 200):
        planes = {name: M.blob_planes(seed + 1000 * k, *shape) for k, (name, shape) in enumerate(M.PLANES.items())}
        save, ok = {"seed": np.int64(seed)}, True
        for name, p in planes.items():
            save["planes." + name] = p.numpy()
        for name, (plane_set, rows, stride, crop, out, thres) in M.BINARIZE_CASES.items():
            masks = reference_masks(mask_lines, seg_post, planes[plane_set], rows, stride, crop, out, thres)
            decide, excluded = M.float64_decision(planes[plane_set], rows, stride, crop, out, thres)
            share = float(excluded.float().mean())
            wrong = int(((masks != decide) & ~excluded).sum())
            print("binarize seed %d %-24s share in the band %.2e, disagreements outside it %d, set %.3f"
                  % (seed, name, share, wrong, float(masks.float().mean())))
            if share > M.MAX_EXCLUDED_SHARE or wrong or (masks.numel() > 1000 and not 0.02 < float(masks.float().mean()) < 0.98):
                ok = False
                break
            save[name + ".masks"] = np.packbits(masks.numpy().reshape(-1))
            save[name + ".config"] = np.asarray((stride,) + crop + out, dtype=np.int64)
            save[name + ".thres"] = np.float64(thres)
            save[name + ".rows"] = np.asarray(rows, dtype=np.int64)
        if ok:
            return save
    raise SystemExit("binarize: no seed satisfies assertion (a)")


def nms_fixture(mask_nms):
    save = {}
    for name in M.NMS_HAND:
        logits, by_hand = M.hand_logits(name)
        keep = mask_nms(logits, [0.0] * len(logits), None, nms_thr=M.NMS_THR)
        assert keep == by_hand, (name, keep)
        save[name + ".keep"] = np.asarray(keep)
        save[name + ".masks"] = np.packbits((logits.sigmoid() > 0.5).numpy().reshape(-1))
    for h, w in M.NMS_SIZES:
        for n in M.NMS_COUNTS:
            name = "n%d_%dx%d" % (n, h, w)
            for seed in range(1, 200):
                params = M.nms_params(seed, n, h, w)
                logits = M.nms_logits(params, h, w, seed)
                _, _, restated, margin = M.mask_nms_restated(logits, M.NMS_THR)
                if margin >= M.IOU_MARGIN and (n < 3 or 2 <= restated.sum() < 0.9 * n):
                    break
            else:
                raise SystemExit("%s: no seed satisfies assertion (b)" % name)
            keep = mask_nms(logits, [0.0] * n, None, nms_thr=M.NMS_THR)
            assert keep == [bool(k) for k in restated], name
            masks = logits.sigmoid() > 0.5
            assert torch.equal(masks, logits > 0)
            print("nms %-12s seed %d: %d of %d kept, IoU margin %.2e" % (name, seed, sum(keep), n, margin))
            save[name + ".params"] = params
            save[name + ".geometry"] = np.asarray((h, w, seed), dtype=np.int64)
            save[name + ".keep"] = np.asarray(keep)
            save[name + ".masks"] = np.packbits(masks.numpy().reshape(-1))
    return save


def main():
    mask_lines, seg_post, mask_nms = load_reference()
    os.makedirs(M.GOLDEN, exist_ok=True)
    for name, save in (("binarize", binarize_fixture(mask_lines, seg_post)), ("nms", nms_fixture(mask_nms))):
        path = os.path.join(M.GOLDEN, name + ".npz")
        np.savez_compressed(path, **save)
        print(path, os.path.getsize(path) // 1024, "KB")
        assert os.path.getsize(path) <= MAX_BYTES


if __name__ == "__main__":
    main()
