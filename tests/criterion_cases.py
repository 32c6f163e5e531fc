"""What tests/test_criterion_cpu.py, tests/test_criterion_gpu.py, tests/golden/make_criterion_golden.py and
tools/criterion_bench.py share: the seeded inputs of the criterion fixtures (tests/golden/criterion/*.npz hold them together with
the reference's loss dictionaries), seeded inputs for the four kernels, and the float64 evaluation of the reference's formulas
that is the yardstick of the fused losses."""
import functools
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "criterion")
MARGIN = 1e-4                 # the project's fp32 tolerance, relative to the value's scale (scaled_error)
BS, Q, T, T_VALID = 2, 30, 16, (12, 9)          # text masks with trailing zeros
DN_NUM, SINGLE_PADDING = 2, 5                   # 10 denoising queries: two groups, padded to the 5 targets of image 0
MASK_HW, STRIDE = (8, 16), 4                    # 32 x 64 ground truth: already a multiple of 32
WEIGHTS = dict(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0)
LOSSES = ["labelsVL", "boxes", "masks", "cardinality"]

# every run the issue asks for: OTA on / off, with / without dn_metas, an image without targets, text masks with trailing zeros
# (all of them), still_cls_for_encoder
CASES = {
    "ota_dn": dict(seed=11, ota=True, still=False, dn=True, aux=2, empty_image=False, boxiou=True),
    "hungarian_nodn_empty_image": dict(seed=12, ota=False, still=False, dn=False, aux=1, empty_image=True, boxiou=False),
    "ota_still_cls_dn_empty_image": dict(seed=13, ota=True, still=True, dn=True, aux=1, empty_image=True, boxiou=True),
    "ota_nodn": dict(seed=14, ota=True, still=False, dn=False, aux=1, empty_image=False, boxiou=False),
    "hungarian_dn": dict(seed=15, ota=False, still=False, dn=True, aux=1, empty_image=False, boxiou=True),
}


def _boxes(g, *shape):
    return torch.cat([0.3 + 0.4 * torch.rand(*shape, 2, generator=g), 0.1 + 0.3 * torch.rand(*shape, 2, generator=g)], -1)


def _head(g, flat, name, queries, tokens, boxiou):
    flat[name + ".pred_logits"] = torch.randn(BS, queries, tokens, generator=g) * 2.0 - 1.0
    flat[name + ".pred_boxes"] = _boxes(g, BS, queries)
    mask = torch.zeros(BS, tokens, dtype=torch.int64)
    for b in range(BS):
        mask[b, :min(T_VALID[b], tokens)] = 1
    flat[name + ".text_masks"] = mask
    if boxiou:
        flat[name + ".pred_boxious"] = torch.randn(BS, queries, 1, generator=g)


def make_inputs(cfg):
    """{flat key: tensor} of one fixture's inputs, drawn from cfg["seed"]."""
    g = torch.Generator().manual_seed(cfg["seed"])
    flat = {}
    counts = [5, 0 if cfg["empty_image"] else 3]
    sizes = [(32, 64), (30, 50)]
    for b in range(BS):
        G = counts[b]
        pm = torch.zeros(G, T, dtype=torch.bool)
        for k in range(G):
            first = int(torch.randint(0, T_VALID[b] - 2, (1,), generator=g))
            pm[k, first:first + 1 + int(torch.randint(0, 3, (1,), generator=g))] = True
        flat["tgt%d.labels" % b] = torch.randint(0, 80, (G,), generator=g)
        flat["tgt%d.boxes" % b] = _boxes(g, G)
        flat["tgt%d.positive_map" % b] = pm
        flat["tgt%d.masks" % b] = torch.rand(G, *sizes[b], generator=g) < 0.4
    layers = cfg["aux"] + 1
    for layer in range(layers):                                     # the last entry belongs to the final outputs
        for b in range(BS):
            G = counts[b]
            if G == 0:
                src = tgt = torch.zeros(0, dtype=torch.int64)
            elif cfg["ota"]:                                          # dynamic-k: several queries per target, sorted by query
                src = torch.randperm(Q, generator=g)[:8].sort()[0]
                tgt = torch.randint(0, G, (8,), generator=g)
            else:                                                     # one-to-one
                src = torch.randperm(Q, generator=g)[:G]
                tgt = torch.randperm(G, generator=g)
            flat["idx%d.%d.src" % (layer, b)], flat["idx%d.%d.tgt" % (layer, b)] = src, tgt
    for layer in range(layers):
        name = "out" if layer == layers - 1 else "aux%d" % layer
        _head(g, flat, name, Q, T, cfg["boxiou"])
        for b in range(BS):
            n = flat["idx%d.%d.src" % (layer, b)].numel()
            flat["%s.pred_masks.%d" % (name, b)] = torch.randn(1, n, 1, *MASK_HW, generator=g) * 2.0
    _head(g, flat, "enc", Q + 7, 1 if cfg["still"] else T, False)
    if cfg["dn"]:
        for layer in range(layers):
            _head(g, flat, "dn" if layer == layers - 1 else "dnaux%d" % layer, DN_NUM * SINGLE_PADDING, T, cfg["boxiou"])
    return flat


def rebuild(flat, cfg, device="cpu"):
    """(outputs, targets, indices_list, dn_metas) as the criterion takes them, from the flat tensors."""
    to = lambda t: t.to(device)
    layers = cfg["aux"] + 1

    def head(name, masks):
        out = {k: to(flat["%s.%s" % (name, k)]) for k in ("pred_logits", "pred_boxes", "text_masks")}
        if name + ".pred_boxious" in flat:
            out["pred_boxious"] = to(flat[name + ".pred_boxious"])
        if masks:
            out["pred_masks"] = [to(flat["%s.pred_masks.%d" % (name, b)]) for b in range(BS)]
        return out

    outputs = head("out", True)
    outputs["aux_outputs"] = [head("aux%d" % i, True) for i in range(cfg["aux"])]
    outputs["enc_outputs"] = head("enc", False)
    targets = [{k: to(flat["tgt%d.%s" % (b, k)]) for k in ("labels", "boxes", "positive_map", "masks")} for b in range(BS)]
    indices_list = [[(to(flat["idx%d.%d.src" % (l, b)]), to(flat["idx%d.%d.tgt" % (l, b)])) for b in range(BS)] for l in range(layers)]
    dn_metas = None
    if cfg["dn"]:
        known = head("dn", False)
        known["aux_outputs"] = [head("dnaux%d" % i, False) for i in range(cfg["aux"])]
        dn_metas = {"output_known_lbs_bboxes": known, "dn_num": DN_NUM, "single_padding": SINGLE_PADDING}
    return outputs, targets, indices_list, dn_metas


@functools.lru_cache(maxsize=None)
def load(name):
    """(flat inputs, {loss key: the reference's value}) of a stored fixture."""
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        flat = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("expect.")}
        expect = {k[len("expect."):]: float(z[k]) for k in z.files if k.startswith("expect.")}
    return flat, expect


def build_criterion(cfg, fused, device="cpu"):
    from uninext_amd.criterion import DINOCriterion
    from uninext_amd.matcher import HungarianMatcherVL
    crit = DINOCriterion(HungarianMatcherVL(**WEIGHTS), {}, LOSSES, focal_alpha=0.25, mask_out_stride=STRIDE, ota=cfg["ota"],
                         still_cls_for_encoder=cfg["still"])
    crit.fused = fused
    return crit.to(device)


def run_fixture(name, fused, device="cpu", requires_grad=False):
    """The loss dictionary of this repository's DINOCriterion on a stored fixture."""
    cfg = CASES[name]
    flat, _ = load(name)
    flat = {k: v.clone() for k, v in flat.items()}
    outputs, targets, indices_list, dn_metas = rebuild(flat, cfg, device)
    leaves = []
    if requires_grad:
        heads = [outputs] + outputs["aux_outputs"] + [outputs["enc_outputs"]]
        if dn_metas:
            heads += [dn_metas["output_known_lbs_bboxes"]] + dn_metas["output_known_lbs_bboxes"]["aux_outputs"]
        for h in heads:
            leaves.append(h["pred_logits"].requires_grad_(True))
            leaves += [m.requires_grad_(True) for m in h.get("pred_masks", [])]
    losses = build_criterion(cfg, fused, device)(outputs, targets, indices_list, dn_metas)
    return (losses, leaves) if requires_grad else losses


def scaled_error(got, want):
    """max |got - want| / max |want|: the error relative to the value's OWN scale, however small that is (the gradient of a mask
    loss is of order 1 / (pixels * num_boxes)).  Where the expected values are all zero the error is the absolute one."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.size == 0:
        return 0.0
    scale = float(np.max(np.abs(want)))
    return float(np.max(np.abs(got - want))) / (scale if scale > 0.0 else 1.0)


def within(got, want, what=""):
    """scaled_error(got, want) <= MARGIN, and got is finite; returns the error."""
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all(), what
    err = scaled_error(got, want)
    assert err <= MARGIN, (what, err)
    return err


# ---- the kernels' own cases ---------------------------------------------------------------------------------------------------
TOKEN_GEOMETRIES = [(1, 1, 1), (2, 65, 255), (2, 64, 256), (3, 130, 77)]
# every one but "nomask" and "bool*" has an int64 mask; the last crosses the bool mask with fractional targets and extreme logits
TOKEN_VARIANTS = ["nomask", "int64", "bool", "zero_image", "unmatched", "fractional", "extreme", "bool_fractional_extreme"]
ALPHA = 0.25


@functools.lru_cache(maxsize=None)
def token_case(B, Q_, T_, variant):
    """(logits [B, Q, T], text_mask or None, row_target [B, Q] int32, positive_map_all [G, T] fp32, loss, grad): loss and grad
    (of the plain sum, scale 1) are the float64 evaluation of token_sigmoid_binary_focal_loss on the one-hot targets."""
    from uninext_amd.criterion import token_sigmoid_binary_focal_loss
    g = torch.Generator().manual_seed(100 + 7 * B + 3 * Q_ + T_ + 1000 * TOKEN_VARIANTS.index(variant))
    logits = torch.randn(B, Q_, T_, generator=g) * 3.0
    G = 5
    pm = (torch.rand(G, T_, generator=g) < 0.2).float()
    if "fractional" in variant:
        pm = torch.rand(G, T_, generator=g)
    if "extreme" in variant:
        flat = logits.view(-1)
        vals = torch.tensor([30.0, -30.0, 100.0, -100.0])
        flat[torch.arange(flat.numel()) % 5 == 0] = vals[torch.randint(0, 4, (int((torch.arange(flat.numel()) % 5 == 0).sum()),), generator=g)]
        pm[0] = 1.0                                                  # +-100 against both targets
    row_target = torch.full((B, Q_), -1, dtype=torch.int32)
    if variant != "unmatched":
        hit = torch.rand(B, Q_, generator=g) < 0.4
        hit.view(-1)[0] = True
        row_target[hit] = torch.randint(0, G, (int(hit.sum()),), generator=g).int()
    mask = None
    if variant != "nomask":
        mask = torch.zeros(B, T_, dtype=torch.int64)
        for b in range(B):
            mask[b, :max(1, T_ - 3 * b - T_ // 4)] = 2 - b % 2       # any value > 0 counts
        if variant == "zero_image":
            mask[B - 1] = 0
        if variant.startswith("bool"):
            mask = mask > 0
    x = logits.double().requires_grad_(True)
    onehot = torch.zeros(B, Q_, T_, dtype=torch.float64)
    onehot[row_target >= 0] = pm.double()[row_target[row_target >= 0].long()]
    loss = token_sigmoid_binary_focal_loss(x, onehot, alpha=ALPHA, text_mask=mask)
    loss.backward()
    return logits, mask, row_target, pm, float(loss.detach()), x.grad.clone()


MASK_GEOMETRIES = [(1, 1, 1, 1, 1), (3, 1, 7, 9, 4), (2, 2, 13, 21, 4), (26, 1, 50, 84, 4), (4, 1, 200, 336, 4)]
MASK_NUM_BOXES = 3.0


def target_pixels(gt, gt_row, F_, h, w, stride):
    """[n, F, h, w] bool: the strided pixels of rows gt_row[i] .. gt_row[i] + F of the padded masks gt [R, H_im, W_im]."""
    start = stride // 2
    rows = gt_row.long()[:, None] + torch.arange(F_)[None, :]
    return gt[rows][:, :, start::stride, start::stride][:, :, :h, :w]


@functools.lru_cache(maxsize=None)
def mask_case(n, F_, h, w, stride):
    """(src [n, F, h, w], gt bool [B, G_max, H_im, W_im], gt_row [n] int32, (loss_mask, loss_dice), grad of loss_mask + 2 loss_dice)
    in float64 at MASK_NUM_BOXES.  Instance 0's target is all zero, the last one's all one (n >= 2), instances 1 and 2 share a
    row (n >= 3)."""
    from uninext_amd.criterion import dice_loss, sigmoid_focal_loss
    g = torch.Generator().manual_seed(500 + n + 10 * F_ + 100 * h + w)
    B, slots = 2, max(2, (n + 1) // 2) * F_
    gt = torch.rand(B, slots, h * stride, w * stride, generator=g) < 0.35
    instance = torch.randperm(B * (slots // F_), generator=g)[:n] if n <= B * (slots // F_) else torch.randint(0, B * (slots // F_), (n,), generator=g)
    if n >= 3:
        instance[2] = instance[1]
    gt_row = (instance * F_).int()
    gt.view(-1, h * stride, w * stride)[gt_row[0].long():gt_row[0].long() + F_] = False
    if n >= 2:
        gt.view(-1, h * stride, w * stride)[gt_row[-1].long():gt_row[-1].long() + F_] = True
    src = torch.randn(n, F_, h, w, generator=g) * 3.0
    x = src.double().requires_grad_(True)
    tgt = target_pixels(gt.view(-1, h * stride, w * stride), gt_row, F_, h, w, stride).double()
    loss_mask = sigmoid_focal_loss(x.flatten(1), tgt.flatten(1), MASK_NUM_BOXES)
    loss_dice = dice_loss(x.flatten(1), tgt.flatten(1), MASK_NUM_BOXES)
    (loss_mask + 2.0 * loss_dice).backward()
    return src, gt, gt_row, (float(loss_mask.detach()), float(loss_dice.detach())), x.grad.clone()
