"""BoxInst at the shape of the Objects365 R50 training config (BASELINE configs[4]): forward + backward of `loss_masks_boxinst` at
batch 2, 64 kept instances of 200 x 336 mask logits, and `boxinst_targets` for two 800 x 1344 images with 32 boxes each; fused on
against fused off on the same GPU and the same seeded inputs, alternating: p10 / p50 / p90 after warm-up, host synchronisations per
call (PyTorch's sync debug mode, "warn"), peak memory above the inputs.

    python tools/boxinst_bench.py [--steps 30] [--warmup 5] [--out profiles/rNN_boxinst.txt]
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uninext_amd import boxinst  # noqa: E402

BS, KEPT, HW, IMAGE_HW, BOXES, STRIDE = 2, 64, (200, 336), (800, 1344), 32, 4


def make_inputs(dev):
    g = torch.Generator().manual_seed(31)
    H, W = IMAGE_HW
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    images, boxes = [], []
    for b in range(BS):
        base = torch.stack([128 + 90 * torch.sin(yy / (150 + 40 * c) + b) * torch.cos(xx / (210 - 30 * c) - c) for c in range(3)])
        images.append((base + 3 * torch.randn(3, H, W, generator=g)).clamp(0, 255).to(torch.uint8).to(dev))
        xy = torch.rand(BOXES, 2, generator=g) * torch.tensor([W * 0.7, H * 0.7])
        wh = 20 + torch.rand(BOXES, 2, generator=g) * torch.tensor([W * 0.3, H * 0.3])
        boxes.append(torch.cat([xy, xy + wh], 1).to(dev))
    per = KEPT // BS
    pred = [(torch.randn(1, per, 1, *HW, generator=g) * 2.0).to(dev).requires_grad_(True) for _ in range(BS)]
    indices = [(torch.arange(per, device=dev), torch.randint(0, BOXES, (per,), generator=g).to(dev)) for _ in range(BS)]
    return images, boxes, pred, indices


def measure(run, steps, warmup):
    """{fused: (times in ms, host syncs a call, peak bytes above what was allocated before the call)}; the routes alternate."""
    for _ in range(warmup):
        for fused in (False, True):
            run(fused)
    times = {False: [], True: []}
    for _ in range(steps):
        for fused in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(fused)
            torch.cuda.synchronize()
            times[fused].append((time.perf_counter() - t0) * 1e3)
    out = {}
    for fused in (False, True):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        run(fused)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            run(fused)
        torch.cuda.set_sync_debug_mode("default")
        out[fused] = (np.asarray(times[fused]), sum("synchroniz" in str(w.message) for w in caught), peak)
    return out


def report(name, result, lines):
    for fused in (False, True):
        t, syncs, peak = result[fused]
        lines.append("%-8s fused=%-5s p10 %.3f  p50 %.3f  p90 %.3f ms  host syncs / call %d  peak memory above inputs %.2f MiB"
                     % (name, fused, np.percentile(t, 10), np.median(t), np.percentile(t, 90), syncs, peak / 2 ** 20))
    off, on = result[False][0], result[True][0]
    apart = np.percentile(on, 90) < np.percentile(off, 10)
    lines.append("%-8s speed-up (p50, composition / fused): x%.2f; p10-p90 ranges %s" % (name, np.median(off) / np.median(on),
                                                                                        "apart, fused faster" if apart else "NOT apart"))
    return apart


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "boxinst_bench needs the GPU: it measures nothing without one"
    dev = "cuda:0"
    images, boxes, pred, indices = make_inputs(dev)
    heights = [IMAGE_HW[0]] * BS
    targets = boxinst.boxinst_targets(images, heights, boxes, fused=True)
    crit = boxinst.BoxInstSetCriterion(None, {}, ["masks_boxinst"], mask_out_stride=STRIDE).to(dev)
    crit._iter.fill_(20000)
    values = {}

    def loss_step(fused):
        crit.fused_boxinst = fused
        for p in pred:
            p.grad = None
        losses = crit.loss_masks_boxinst({"pred_masks": pred}, targets, indices, 64.0)
        (losses["loss_prj"] + losses["loss_pairwise"]).backward()
        values[fused] = losses

    def target_step(fused):
        values["t", fused] = boxinst.boxinst_targets(images, heights, boxes, fused=fused)

    lines = ["python tools/boxinst_bench.py --steps %d --warmup %d   (%s; loss: forward + backward of loss_masks_boxinst, batch %d, %d kept "
             "instances of %d x %d; targets: boxinst_targets, %d images of %d x %d, %d boxes each; fused on against off alternating on the "
             "same GPU and inputs; times per call in ms)" % (a.steps, a.warmup, torch.cuda.get_device_name(0), BS, KEPT, *HW, BS, *IMAGE_HW,
                                                                BOXES), ""]
    loss_apart = report("loss", measure(loss_step, a.steps, a.warmup), lines)
    lines.append("loss     values: fused %s | composition %s" % tuple(
        {k: round(float(v.detach()), 6) for k, v in values[f].items()} for f in (True, False)))
    target_apart = report("targets", measure(target_step, a.steps, a.warmup), lines)
    same = all(torch.equal(x["masks"], y["masks"]) for x, y in zip(values["t", True], values["t", False]))
    diff = max(float((x["image_color_similarity"][0] - y["image_color_similarity"][0]).abs().max()) for x, y in zip(values["t", True], values["t", False]))
    lines.append("targets  bitmasks equal: %s; largest similarity difference %.3e" % (same, diff))
    lines.append("")
    lines.append("fused faster with the ranges apart: loss %s, targets %s" % (loss_apart, target_apart))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
