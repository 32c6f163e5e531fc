#!/usr/bin/env python
"""A/B of the training criterion (uninext_amd/criterion.py: DINOCriterion.fused) against the same module with fused = False, i.e.
the reference's composition of PyTorch operations, on one GPU, alternating in one process with rotating inputs.  The training
shape of the README's dynamic-mask row: bs 2, 900 queries + 200 denoising queries, 256 tokens, 6 decoder layers + the encoder's
proposals + the denoising groups, 26 instance masks of 200 x 336 against 800 x 1344 ground truth at stride 4, simOTA-style indices
(several queries per target), precomputed: the matcher is not what is measured (the encoder's Hungarian matching runs inside the
criterion on both routes alike).

    python tools/criterion_bench.py [--iters 20] [--warmup 5] [--errors]

One call = forward of the criterion + backward of the summed losses to the logits and mask logits.  Medians and spreads (p10..p90)
of per-call wall times around a device synchronisation; "faster" means the medians differ by more than the larger of the two
spreads.  Host synchronisations per call are what torch.cuda.set_sync_debug_mode("warn") reports on a warm call; peak memory is
torch.cuda.max_memory_allocated over one warm call, above what the inputs hold.  --errors adds the table of scaled errors
(max |value - float64| / max |float64|, the value's own scale) of the fused kernels and of the fp32 composition on the kernel cases of
tests/criterion_cases.py."""
import argparse
import os
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from uninext_amd.criterion import DINOCriterion   # noqa: E402
from uninext_amd.matcher import HungarianMatcherVL   # noqa: E402

ROTATE = 3
BS, Q, T, LAYERS = 2, 900, 256, 6
DN_NUM, SINGLE_PADDING = 20, 5             # 100 denoising queries an image padded to 5 targets: 200 in the batch
G, PER_IMAGE = 5, 13                       # 5 targets an image, 13 matched queries an image: 26 instances
MASK_HW, IM_HW, STRIDE = (200, 336), (800, 1344), 4
LOSSES = ["labelsVL", "boxes", "masks", "cardinality"]


def boxes(g, *shape):
    return torch.cat([0.3 + 0.4 * torch.rand(*shape, 2, generator=g), 0.1 + 0.3 * torch.rand(*shape, 2, generator=g)], -1)


def make_inputs(seed, dev):
    g = torch.Generator().manual_seed(seed)
    text_masks = torch.zeros(BS, T, dtype=torch.int64)
    text_masks[0, :200], text_masks[1, :140] = 1, 1

    def head(queries, masks=False, indices=None):
        out = {"pred_logits": (torch.randn(BS, queries, T, generator=g) * 2.0 - 3.0).to(dev).requires_grad_(True),
               "pred_boxes": boxes(g, BS, queries).to(dev), "text_masks": text_masks.to(dev),
               "pred_boxious": torch.randn(BS, queries, 1, generator=g).to(dev)}
        if masks:
            out["pred_masks"] = [(torch.randn(1, PER_IMAGE, 1, *MASK_HW, generator=g) * 2.0).to(dev).requires_grad_(True) for _ in range(BS)]
        return out

    targets = []
    for b in range(BS):
        pm = torch.zeros(G, T, dtype=torch.bool)
        for k in range(G):
            pm[k, 3 * k + 1:3 * k + 3] = True
        targets.append({"labels": torch.randint(0, 80, (G,), generator=g).to(dev), "boxes": boxes(g, G).to(dev),
                        "positive_map": pm.to(dev), "masks": (torch.rand(G, *IM_HW, generator=g) < 0.3).to(dev)})
    indices_list = [[(torch.randperm(Q, generator=g)[:PER_IMAGE].sort()[0].to(dev), torch.randint(0, G, (PER_IMAGE,), generator=g).to(dev))
                     for _ in range(BS)] for _ in range(LAYERS)]
    outputs = head(Q, masks=True)
    outputs["aux_outputs"] = [head(Q, masks=True) for _ in range(LAYERS - 1)]
    outputs["enc_outputs"] = {k: v for k, v in head(Q).items() if k != "pred_boxious"}
    known = head(DN_NUM * SINGLE_PADDING)
    known["aux_outputs"] = [head(DN_NUM * SINGLE_PADDING) for _ in range(LAYERS - 1)]
    dn_metas = {"output_known_lbs_bboxes": known, "dn_num": DN_NUM, "single_padding": SINGLE_PADDING}
    return outputs, targets, indices_list, dn_metas


def leaves_of(x):
    outputs, _, _, dn_metas = x
    heads = [outputs] + outputs["aux_outputs"] + [outputs["enc_outputs"], dn_metas["output_known_lbs_bboxes"]] \
        + dn_metas["output_known_lbs_bboxes"]["aux_outputs"]
    return [h["pred_logits"] for h in heads] + [m for h in heads for m in h.get("pred_masks", [])]


def route(fused):
    crit = DINOCriterion(HungarianMatcherVL(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0), {}, LOSSES, mask_out_stride=STRIDE, ota=True)
    crit.fused = fused

    def step(x):
        for leaf in leaves_of(x):
            leaf.grad = None
        losses = crit(*x)
        sum(v for v in losses.values() if v.requires_grad).backward()
        return losses
    return step


def timed(fns, inputs, iters, warmup):
    """Per-route sorted times in ms; the routes alternate call by call, the inputs rotate."""
    times = [[] for _ in fns]
    for it in range(warmup + iters):
        for r, fn in enumerate(fns):
            x = inputs[it % len(inputs)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(x)
            torch.cuda.synchronize()
            if it >= warmup:
                times[r].append(1e3 * (time.perf_counter() - t0))
    return [sorted(t) for t in times]


def stats(t):
    return t[len(t) // 2], t[int(0.9 * (len(t) - 1))] - t[int(0.1 * (len(t) - 1))]


def host_syncs(fn, x):
    """Synchronising calls of one warm call, or None where the build does not report them."""
    fn(x)
    try:
        torch.cuda.set_sync_debug_mode("warn")
    except Exception:
        return None
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn(x)
        return sum("synchroniz" in str(w.message).lower() for w in seen)
    finally:
        torch.cuda.set_sync_debug_mode("default")


def peak_mib(fn, x):
    fn(x)
    torch.cuda.synchronize()
    for leaf in leaves_of(x):
        leaf.grad = None
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn(x)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


def errors_table(dev):
    import criterion_cases as C
    from uninext_amd import ext
    from uninext_amd.criterion import dice_loss, sigmoid_focal_loss, token_sigmoid_binary_focal_loss

    def scaled(got, want):
        return C.scaled_error(torch.as_tensor(got).detach().cpu().numpy(), torch.as_tensor(want).numpy())

    print("scaled errors against float64: max |value - float64| / max |float64|; tolerance of the tests %.0e" % C.MARGIN)
    print("  %-34s %-12s %-12s %-12s %-12s" % ("token focal (B, Q, T) variant", "fused loss", "fused grad", "torch loss", "torch grad"))
    one = torch.ones(1, device=dev)
    for geom in C.TOKEN_GEOMETRIES:
        for variant in C.TOKEN_VARIANTS:
            logits, mask, rows, pm, want, want_grad = C.token_case(*geom, variant)
            x, m = logits.to(dev), None if mask is None else mask.to(dev)
            loss = ext.token_focal_loss_forward(x, m, rows.to(dev), pm.to(dev), C.ALPHA)
            grad = ext.token_focal_loss_backward(x, m, rows.to(dev), pm.to(dev), C.ALPHA, one)
            xr = logits.to(dev).requires_grad_(True)
            onehot = torch.zeros_like(xr)
            hit = rows.to(dev) >= 0
            onehot[hit] = pm.to(dev)[rows.to(dev)[hit].long()]
            ref = token_sigmoid_binary_focal_loss(xr, onehot, alpha=C.ALPHA, text_mask=m)
            ref.backward()
            print("  %-34s %-12.3e %-12.3e %-12.3e %-12.3e" % ("%s %s" % (geom, variant), scaled(loss[0], want), scaled(grad, want_grad),
                                                               scaled(ref.detach(), want), scaled(xr.grad, want_grad)), flush=True)
    print("  %-34s %-10s %-10s %-10s %-10s %-10s %-10s" % ("mask losses (n, F, h, w, stride)", "fused mask", "fused dice", "fused grad",
                                                           "torch mask", "torch dice", "torch grad"))
    for geom in C.MASK_GEOMETRIES:
        n, F_, h, w, stride = geom
        src, gt, rows, want, want_grad = C.mask_case(*geom)
        x = src.to(dev)
        losses, sums = ext.mask_losses_forward(x, gt.to(dev), rows.to(dev), stride, C.MASK_NUM_BOXES)
        grad = ext.mask_losses_backward(x, gt.to(dev), rows.to(dev), stride, C.MASK_NUM_BOXES, sums, one, 2.0 * one)
        xr = src.to(dev).requires_grad_(True)
        t = C.target_pixels(gt.view(-1, *gt.shape[-2:]), rows, F_, h, w, stride).to(dev).float().flatten(1)
        lm, ld = sigmoid_focal_loss(xr.flatten(1), t, C.MASK_NUM_BOXES), dice_loss(xr.flatten(1), t, C.MASK_NUM_BOXES)
        (lm + 2.0 * ld).backward()
        print("  %-34s %-10.2e %-10.2e %-10.2e %-10.2e %-10.2e %-10.2e" % (
            geom, scaled(losses[0], want[0]), scaled(losses[1], want[1]), scaled(grad, want_grad), scaled(lm.detach(), want[0]),
            scaled(ld.detach(), want[1]), scaled(xr.grad, want_grad)), flush=True)


def C_scaled(got, want):
    import criterion_cases as C
    return C.scaled_error(got, want)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--errors", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "criterion_bench measures on the GPU"
    dev = "cuda:0"
    print(torch.cuda.get_device_name(0), "torch", torch.__version__)
    print("bs %d, %d + %d queries, %d tokens, %d decoder layers + encoder + denoising, %d masks of %d x %d at stride %d; forward + backward"
          % (BS, Q, BS * DN_NUM * SINGLE_PADDING, T, LAYERS, BS * PER_IMAGE, *MASK_HW, STRIDE))
    xs = [make_inputs(seed, dev) for seed in range(ROTATE)]
    fused, torch_ = route(True), route(False)
    a, b = fused(xs[0]), torch_(xs[0])
    worst = max(C_scaled(float(a[k].detach()), float(b[k].detach())) for k in b)
    print("  %d loss keys on both routes; largest scaled difference between them %.2e" % (len(b), worst))
    assert set(a) == set(b)
    (tf, sf), (tt, st) = [stats(t) for t in timed([fused, torch_], xs, args.iters, args.warmup)]
    verdict = "fused faster" if tt - tf > max(sf, st) else ("torch faster" if tf - tt > max(sf, st) else "within spread")
    print("  fused %9.3f ms (spread %.3f, %s host syncs, peak %.1f MiB)   torch %9.3f ms (spread %.3f, %s host syncs, peak %.1f MiB)   x%.2f  %s"
          % (tf, sf, host_syncs(fused, xs[1]), peak_mib(fused, xs[1]), tt, st, host_syncs(torch_, xs[1]), peak_mib(torch_, xs[1]),
             tt / tf, verdict), flush=True)
    if args.errors:
        errors_table(dev)


if __name__ == "__main__":
    main()
