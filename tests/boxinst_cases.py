"""What tests/test_boxinst_cpu.py, tests/test_boxinst_gpu.py, tests/golden/make_boxinst_golden.py and tools/boxinst_bench.py share: the
seeded inputs of the BoxInst fixtures (tests/golden/boxinst/*.npz hold them together with the reference's outputs), seeded inputs
for the kernels of uninext_amd/csrc/boxinst.hip, and the float64 evaluation of the reference's formulas that is the yardstick of
the fused losses."""
import functools
import os
import types

import numpy as np
import torch

from criterion_cases import MARGIN, scaled_error, target_pixels, within  # noqa: F401  (the project's bound and its measure)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "boxinst")
STRIDE, DILATION, SIZE = 4, 2, 3
BS = 2

# ---- the targets fixture: a 2-image batch of unequal sizes ----------------------------------------------------------------------
IMAGE_SIZES = [(64, 96), (40, 72)]              # H_i, W_i: padded to 64 x 96
HEIGHTS = [128, 40]                             # batched_inputs[i]["height"]: int(10 * 64 / 128) = 5 and 10 bottom rows removed
BOXES = [
    # edge-touching (the whole first row / column), fractional, over the right and the bottom edge, one pixel
    [[0.0, 0.0, 95.0, 0.0], [0.0, 3.0, 0.0, 63.0], [10.25, 7.75, 40.5, 30.99], [80.5, 50.5, 200.0, 300.0], [17.0, 9.0, 17.0, 9.0]],
    [[5.9, 0.2, 71.0, 39.0], [30.0, 12.5, 71.999, 39.999], [60.0, 20.0, 95.0, 63.0]],
]


def make_target_inputs():
    """(images: list of uint8 [3, H_i, W_i] BGR, heights, boxes: list of fp32 [G_i, 4])."""
    g = torch.Generator().manual_seed(41)
    images = []
    for H, W in IMAGE_SIZES:
        # smooth colour fields with noise on top: similarities on both sides of the 0.3 threshold
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        base = torch.stack([128 + 70 * torch.sin(yy / 45 + c) * torch.cos(xx / 60 - c) for c in range(3)])
        images.append((base + 4 * torch.randn(3, H, W, generator=g)).clamp(0, 255).to(torch.uint8))
    return images, list(HEIGHTS), [torch.tensor(b, dtype=torch.float32) for b in BOXES]


@functools.lru_cache(maxsize=None)
def load_targets():
    """The stored targets fixture: {"masks.b", "sim.b"} of the reference per image b."""
    with np.load(os.path.join(GOLDEN, "targets.npz")) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


# ---- the loss fixtures ------------------------------------------------------------------------------------------------------------
MASK_HW = (16, 24)
# pairs per image; topk, threshold, warm-up iterations, `_iter` before the call, random.seed
LOSS_CASES = {
    "plain": dict(seed=51, pairs=(4, 3), topk=64, thresh=0.3, warmup=10000, iter0=0, rseed=None, scalar=False),
    "over_topk": dict(seed=52, pairs=(3, 2), topk=3, thresh=0.3, warmup=10000, iter0=20000, rseed=7, scalar=False),
    "no_gt": dict(seed=53, pairs=(0, 0), topk=64, thresh=0.3, warmup=10000, iter0=5, rseed=None, scalar=False),
    "scalar_pred": dict(seed=54, pairs=(0, 0), topk=64, thresh=0.3, warmup=10000, iter0=5, rseed=None, scalar=True),
    "warmup_mid": dict(seed=55, pairs=(2, 3), topk=64, thresh=0.3, warmup=10, iter0=3, rseed=None, scalar=False),
    "no_weight": dict(seed=56, pairs=(2, 2), topk=64, thresh=2.0, warmup=10, iter0=50, rseed=None, scalar=False),
}


def make_loss_inputs(cfg):
    """{flat key: tensor} of one loss fixture's inputs, drawn from cfg["seed"]: the predicted masks and the matcher's indices."""
    g = torch.Generator().manual_seed(cfg["seed"])
    flat = {}
    for b in range(BS):
        n, G = cfg["pairs"][b], len(BOXES[b])
        flat["idx.%d.src" % b] = torch.randperm(30, generator=g)[:n]
        flat["idx.%d.tgt" % b] = torch.randint(0, G, (n,), generator=g)
        flat["pred_masks.%d" % b] = torch.randn(1, n, 1, *MASK_HW, generator=g) * 2.0
    return flat


def boxinst_cfg(cfg):
    """An object with the reference's MODEL.BOXINST.* attributes."""
    ns = types.SimpleNamespace
    return ns(MODEL=ns(BOXINST=ns(ENABLED=True, BOTTOM_PIXELS_REMOVED=10, TOPK=cfg["topk"],
                                  PAIRWISE=ns(SIZE=SIZE, DILATION=DILATION, COLOR_THRESH=cfg["thresh"], WARMUP_ITERS=cfg["warmup"]))))


def rebuild_loss(flat, cfg, device="cpu"):
    """(outputs, targets, indices) as loss_masks_boxinst takes them; the targets are the stored reference targets."""
    stored = load_targets()
    targets = [{"masks": stored["masks.%d" % b].to(device), "image_color_similarity": stored["sim.%d" % b].to(device)[None].expand(
        len(BOXES[b]), -1, -1, -1)} for b in range(BS)]
    indices = [(flat["idx.%d.src" % b].to(device), flat["idx.%d.tgt" % b].to(device)) for b in range(BS)]
    pred = torch.tensor(0.25, device=device) if cfg["scalar"] else [flat["pred_masks.%d" % b].to(device) for b in range(BS)]
    return {"pred_masks": pred}, targets, indices


@functools.lru_cache(maxsize=None)
def load_loss(name):
    """(flat inputs, {key: the reference's value}) of a stored loss fixture; "iter" is `_iter` after the call."""
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        flat = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("expect.")}
        expect = {k[len("expect."):]: float(z[k]) for k in z.files if k.startswith("expect.")}
    return flat, expect


def run_loss_fixture(name, fused, device="cpu", requires_grad=False, cls=None):
    """({loss_prj, loss_pairwise}, criterion[, leaves]) of this repository's BoxInstDINOCriterion on a stored fixture."""
    import random
    from uninext_amd.boxinst import BoxInstDINOCriterion
    cfg = LOSS_CASES[name]
    flat, _ = load_loss(name)
    outputs, targets, indices = rebuild_loss({k: v.clone() for k, v in flat.items()}, cfg, device)
    crit = (cls or BoxInstDINOCriterion)(None, {}, ["masks_boxinst"], mask_out_stride=STRIDE, cfg=boxinst_cfg(cfg)).to(device)
    crit.fused_boxinst = fused
    crit._iter.fill_(cfg["iter0"])
    leaves = []
    if requires_grad and not cfg["scalar"]:
        leaves = [m.requires_grad_(True) for m in outputs["pred_masks"]]
    if cfg["rseed"] is not None:
        random.seed(cfg["rseed"])
    losses = crit.loss_masks_boxinst(outputs, targets, indices, 7.0)
    return (losses, crit, leaves) if requires_grad else (losses, crit)


# ---- the kernels' own cases -------------------------------------------------------------------------------------------------------
# (n, h, w).  The loss kernels work on bands of 8 whole rows with 256 threads, a wave per row for the rows' maxima and a thread per
# column for the columns'; 16 bytes a load where w % 4 == 0.  So besides the geometries the issue names:
KERNEL_GEOMETRIES = [
    (1, 1, 1),                  # one pixel: every neighbour outside
    (1, 3, 5),                  # every neighbour of some pixels outside (dilation 2)
    (2, 5, 4),
    (3, 17, 33),                # scalar path, three bands
    (2, 40, 68),                # vec4 path, five bands
    (1, 7, 6), (1, 8, 6), (1, 9, 6),                # one row either side of the band edge (8 rows)
    (1, 15, 8), (1, 16, 8), (1, 17, 8),             # ... of the second band's edge, vec4
    (1, 9, 31), (1, 9, 32), (1, 9, 33),             # a band of 8 x 32 pixels is one pixel a thread (256 threads)
    (1, 3, 63), (1, 3, 64), (1, 3, 65),             # the row maximum's wave takes 64 columns a step
    (1, 9, 127), (1, 9, 128), (1, 9, 129),          # vec4: a band of 8 x 128 pixels is four pixels a thread
    (1, 2, 255), (1, 2, 256), (1, 2, 257),          # the column maxima take 256 columns a step
    (1, 2, 597),                                    # the widest row the LDS tile holds at dilation 2 (12 rows x 9 bytes x w <= 63 KiB)
]
KERNEL_VARIANTS = ["plain", "extreme", "bad_gt_row", "second_image", "subset", "thresh_negative", "no_weight"]
# every variant at the issue's geometries, "plain" and "extreme" at the edges
KERNEL_CASES = [(g, v) for g in KERNEL_GEOMETRIES[:5] for v in KERNEL_VARIANTS] + \
    [(g, v) for g in KERNEL_GEOMETRIES[5:] for v in ("plain", "extreme")]
WARMUP = 0.4


@functools.lru_cache(maxsize=None)
def kernel_case(n, h, w, variant):
    """dict: src [N, 1, h, w], inst [n] int32, gt bool [2, G_max, 4 h, 4 w], gt_row [n] int32, sim [2, 8, h, w], img [n] int32, thresh,
    and in float64 `want` = (loss_prj, loss_pairwise), `want_grad` [N, 1, h, w] of loss_prj + 2 loss_pairwise, `sum_w`."""
    from uninext_amd.boxinst import compute_pairwise_term, compute_project_term
    g = torch.Generator().manual_seed(900 + 131 * n + 17 * h + w + 10000 * KERNEL_VARIANTS.index(variant))
    if variant == "bad_gt_row":
        n += 1                                    # one instance more, the one whose row is out of range
    N = n + 2 if variant == "subset" else n
    src = torch.randn(N, 1, h, w, generator=g) * 3.0
    if variant == "extreme":                      # one extreme a row and a column: the maxima stay unique in sigmoid space
        vals = [30.0, -30.0, 100.0, -100.0]
        for i in range(N):
            for y in range(min(h, w)):
                src[i, 0, y, (7 * y + 3 + i) % w] = vals[(y + i) % 4]
    inst = torch.randperm(N, generator=g)[:n].int()
    G_max = max(2, n)
    H_im, W_im = h * STRIDE, w * STRIDE
    gt = torch.zeros(BS, G_max, H_im, W_im, dtype=torch.bool)
    for slot in gt.view(-1, H_im, W_im):                 # box masks
        y1, x1 = int(torch.randint(0, H_im, (1,), generator=g)), int(torch.randint(0, W_im, (1,), generator=g))
        y2, x2 = int(torch.randint(y1, H_im, (1,), generator=g)), int(torch.randint(x1, W_im, (1,), generator=g))
        slot[max(0, y1 - 3):y2 + 4, max(0, x1 - 3):x2 + 4] = True
    img = torch.randint(0, BS, (n,), generator=g).int()
    if variant == "second_image":
        img[:] = 1
    gt_row = (img * G_max + torch.randint(0, G_max, (n,), generator=g).int()).int()
    if variant == "bad_gt_row":
        gt_row[-1] = BS * G_max + 5
    sim = torch.rand(BS, 8, h, w, generator=g)
    gt.view(-1, H_im, W_im)[gt_row[0].long(), STRIDE // 2, STRIDE // 2] = True       # pixel (0, 0) of instance 0 always has weight
    sim[img[0].long(), :, 0, 0] = 0.9
    thresh = {"thresh_negative": -1.0, "no_weight": 2.0}.get(variant, 0.3)
    # float64: the reference's formulas
    x_all = src.double().requires_grad_(True)
    x = x_all[inst.long()]
    rows = gt_row.long()
    ok = (rows >= 0) & (rows < BS * G_max)
    tgt = target_pixels(gt.view(-1, H_im, W_im), rows.clamp(0, BS * G_max - 1), 1, h, w, STRIDE) & ok[:, None, None, None]
    tgt = tgt.double()
    weights = (sim[img.long()] >= thresh).double() * tgt
    # sigmoid as 1 / (1 + exp(-x)): torch.sigmoid's backward forms p (1 - p), and at a logit of 30 the float64 1 - p has lost three of
    # its digits (the yardstick's gradient was 1e-3 off where the maximum of a row is saturated); this form's backward does not cancel
    loss_prj = compute_project_term(1.0 / (1.0 + torch.exp(-x)), tgt)
    loss_pairwise = (compute_pairwise_term(x, SIZE, DILATION) * weights).sum() / weights.sum().clamp(min=1.0) * WARMUP
    (loss_prj + 2.0 * loss_pairwise).backward()
    # Where every weighted neighbour is outside the image the exact pairwise loss is -log(p + (1 - p)) = 0 and float64 returns its own
    # rounding noise (terms of order 1, so a few 1e-16): that is the yardstick's error, not a scale to hold an fp32 result to
    # 1e-4 of.  Such a value counts as the 0 it stands for, and scaled_error then measures the absolute error.
    if abs(float(loss_pairwise.detach())) < 1e-12:
        loss_pairwise = loss_pairwise.detach() * 0.0
    return dict(src=src, inst=inst, gt=gt, gt_row=gt_row, sim=sim, img=img, thresh=thresh, tgt=tgt.bool(),
                want=(float(loss_prj.detach()), float(loss_pairwise.detach())), want_grad=x_all.grad.clone(), sum_w=float(weights.sum()))


def ulp32(values):
    """One fp32 unit in the last place of max(|value|, 1), per element (float64 array)."""
    v = np.maximum(np.abs(np.asarray(values, dtype=np.float64)), 1.0).astype(np.float32)
    return (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64)
