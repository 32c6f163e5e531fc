"""Shared by tests/golden/make_pred_heads_golden.py, tests/test_pred_heads_cpu.py and tests/test_pred_heads_gpu.py: the shapes,
parameters and inputs of the fixtures under tests/golden/pred_heads/, and the error measure.

Every parameter and input is an exact dyadic (a multiple of 2 ** -STEP_BITS, helpers of tests/query_selection_cases.py), so fp32
holds what the float64 reference saw; they are re-drawn here from the seed each fixture records and pinned by its digest.

B = 2, Q = 37: one full 32-row tile and a 5-row tile per image.  Two decoder levels with their own heads (the last one is
evaluated) and three reference-point sets, so `inter_references[lvl - 1]` and `inter_references[-2]` are different tensors.
The last level's reference points hold, in the first and the last four rows of each image (one group in each tile), the
entries 0, 1, 2 ** -20 and 1 - 2 ** -20: both clamps of inverse_sigmoid (eps 1e-5) are hit, and all four are exact in fp32."""
import json
import os

import numpy as np
import torch

import query_selection_cases as QC

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pred_heads")
TOL = QC.TOL          # the project's bound: max abs error <= 1e-4 of the output's max abs, against float64
D_MODEL, LANG_DIM = QC.D_MODEL, QC.LANG_DIM
B, Q, LEVELS = 2, 37, 2
P_SHIPPED = 169       # the shipped controller: 80 + 64 + 8 weights, 8 + 8 + 1 biases
IMAGE_SIZES = [(480, 640), (333, 500)]      # (height, width)
EDGE_VALUES = [0.0, 1.0, 2.0 ** -20, 1.0 - 2.0 ** -20]
EDGE_ROWS = [0, 1, 2, 3, Q - 4, Q - 3, Q - 2, Q - 1]
OUTPUTS = ("pred_logits", "pred_boxes", "pred_boxious", "mask_head_params", "reference_points")

# name -> class head, seed, task, text tokens of `hidden`, generated parameters, reference width, IoU branch.  T, the width of
# the logits: L for detection, 1 for grounding (the tokens pooled under a mask of unequal lengths) and for a Still_Classifier.
FIXTURES = {
    "detection": dict(head="vl_align", seed=411, task="detection", L=70, P=P_SHIPPED, ref_dim=4, iou=True),
    "grounding": dict(head="vl_align", seed=412, task="grounding", L=9, P=P_SHIPPED, ref_dim=4, iou=True),
    "full_text": dict(head="vl_align", seed=413, task="detection", L=256, P=P_SHIPPED, ref_dim=4, iou=True),
    "ref2_plain": dict(head="still", seed=414, task="detection", L=3, P=P_SHIPPED, ref_dim=2, iou=False),
}
TEXT_LENGTHS = [5, 9]     # real tokens of each image's text under the "grounding" mask


def tokens_of(cfg):
    return cfg["L"] if cfg["head"] == "vl_align" and cfg["task"] == "detection" else 1


def make_case(name):
    """(cfg, states, inputs) of a fixture, float64, from its seed alone.  states: one reference-keyed state dict each for
    class_embed, bbox_embed, iou_head (when there is one) and controller; the first three are ModuleLists ("<lvl>.<key>")."""
    cfg = dict(FIXTURES[name])
    g = torch.Generator().manual_seed(cfg["seed"])
    d = D_MODEL
    st = {"class_embed": {}, "bbox_embed": {}, "controller": {}}
    if cfg["iou"]:
        st["iou_head"] = {}
    for lvl in range(LEVELS):
        c, pre = st["class_embed"], "%d." % lvl
        if cfg["head"] == "vl_align":
            QC._linear(c, g, pre + "dot_product_projection_text", d, LANG_DIM, 4.0 * LANG_DIM ** -0.5)
            c[pre + "log_scale"] = torch.tensor([0.5], dtype=torch.float64)
            c[pre + "bias_lang"] = QC.dyadic(torch.randn(LANG_DIM, generator=g), 0.05)
            c[pre + "bias0"] = QC.dyadic(torch.tensor([-4.59511985]))
        else:
            QC._linear(c, g, pre + "body", 1, d, 2.0 * d ** -0.5)
        QC._linear(st["bbox_embed"], g, pre + "layers.0", d, d, d ** -0.5)
        QC._linear(st["bbox_embed"], g, pre + "layers.1", d, d, d ** -0.5)
        QC._linear(st["bbox_embed"], g, pre + "layers.2", 4, d, d ** -0.5)
        if cfg["iou"]:
            QC._linear(st["iou_head"], g, "%d" % lvl, 1, d, d ** -0.5)
    QC._linear(st["controller"], g, "layers.0", d, d, d ** -0.5)
    QC._linear(st["controller"], g, "layers.1", d, d, d ** -0.5)
    QC._linear(st["controller"], g, "layers.2", cfg["P"], d, d ** -0.5)
    refs = QC.dyadic(torch.rand(LEVELS + 1, B, Q, cfg["ref_dim"], generator=g))
    for k, row in enumerate(EDGE_ROWS):          # every edge value in every column, in both tiles of both images
        for col in range(cfg["ref_dim"]):
            refs[LEVELS - 2, :, row, col] = EDGE_VALUES[(k + col) % len(EDGE_VALUES)]
    masks = torch.ones(B, cfg["L"], dtype=torch.bool)
    if cfg["task"] == "grounding":
        for b, n in enumerate(TEXT_LENGTHS):
            masks[b, n:] = False
    x = {"hs": QC.dyadic(torch.randn(LEVELS, B, Q, d, generator=g)),
         "init_reference": QC.dyadic(torch.rand(B, Q, cfg["ref_dim"], generator=g)), "inter_references": refs,
         "hidden": QC.dyadic(torch.randn(B, cfg["L"], LANG_DIM, generator=g)), "masks": masks, "image_sizes": IMAGE_SIZES}
    return cfg, st, x


def digest(states):
    return QC.digest(states)


def load(name):
    z = np.load(os.path.join(HERE, name + ".npz"))
    return {k: z[k] for k in z.files}


def recorded_keys(fixture):
    return json.loads(str(fixture["keys_json"]))


def build(cfg, states, dtype, device="cpu"):
    """The project's DetectionHeads of a fixture, every submodule loaded strictly, eval mode."""
    from torch import nn
    from uninext_amd import modules as M
    head = (lambda: M.VL_Align(QC.vl_cfg())) if cfg["head"] == "vl_align" else (lambda: M.Still_Classifier(D_MODEL))
    mods = {"class_embed": nn.ModuleList(head() for _ in range(LEVELS)),
            "bbox_embed": nn.ModuleList(M.MLP(D_MODEL, D_MODEL, 4, 3) for _ in range(LEVELS)),
            "controller": M.MLP(D_MODEL, D_MODEL, cfg["P"], 3)}
    if cfg["iou"]:
        mods["iou_head"] = nn.ModuleList(nn.Linear(D_MODEL, 1) for _ in range(LEVELS))
    for k, m in mods.items():
        m.load_state_dict(states[k], strict=True)
    heads = M.DetectionHeads(mods["class_embed"], mods["bbox_embed"], mods.get("iou_head"), mods["controller"])
    return heads.to(dtype).to(device).eval()


def inputs(x, dtype, device="cpu"):
    """The tensor arguments of DetectionHeads.inference in the given type, on the given device."""
    to = lambda t: t.to(dtype).to(device).contiguous()
    return to(x["hs"]), to(x["init_reference"]), to(x["inter_references"]), \
        {"hidden": to(x["hidden"]), "masks": x["masks"].to(device)}


def run(cfg, heads, x, device="cpu", dtype=torch.float64, fused=False):
    """DetectionHeads.inference on the inputs of make_case (no autograd); `fused` is set on the object, not on the class."""
    heads.fused = fused
    hs, init_reference, inter_references, text = inputs(x, dtype, device)
    with torch.no_grad():
        return heads.inference(hs, init_reference, inter_references, text, cfg["task"], x["image_sizes"])
