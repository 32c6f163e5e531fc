"""Forward + backward of select_pos_neg + loss_reid at the shape of the shipped video config (video_joint_r50: 2 key / reference
pairs, 900 queries, 256 channels, 256 tokens, 10 targets per image with one invalid), fused=True against fused=False on the same
GPU and the same seeds: median and p10-p90 after warm-up, host synchronisations per call (PyTorch's sync debug mode, "warn"),
peak memory.

    python tools/reid_bench.py [--steps 30] [--warmup 5]
"""
import argparse
import os
import random
import sys
import time
import warnings

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import reid_cases as C  # noqa: E402
from uninext_amd import reid  # noqa: E402

SHAPE = {"seed": 21, "Q": 900, "Qk": 900, "C": 256, "T": 256,
         "images": [C._img(10, valid=[1, 1, 1, 0, 1, 1, 1, 1, 1, 1]), C._img(10, valid=[1, 1, 1, 1, 1, 1, 1, 0, 1, 1])]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    head = nn.Sequential(nn.Linear(256, 256), nn.ReLU(), nn.Linear(256, 256)).to(dev)
    ref_box, all_indices, targets, det_targets, hs_key, hs_ref, ref_cls = C.rebuild(C.make_inputs(SHAPE), 2, device=dev)
    hs_key.requires_grad_(True)
    hs_ref.requires_grad_(True)
    params = torch.ones((), device=dev, requires_grad=True)

    def step(fused, seed):
        random.seed(seed)
        items = reid.select_pos_neg(ref_box, all_indices, targets, det_targets, head, hs_key, hs_ref, ref_cls, fused=fused)
        losses = reid.loss_reid({"pred_qd": items, "reid_params": params}, None, None, 1.0)
        total = losses["loss_reid"] + 2.0 * losses["loss_reid_aux"]
        head.zero_grad(set_to_none=True)
        hs_key.grad = hs_ref.grad = None
        total.backward()
        return len(items), losses

    print("device", torch.cuda.get_device_name(0), "| shape", {k: v for k, v in SHAPE.items() if k != "images"}, "| targets 10 + 10, one invalid each")
    for i in range(a.warmup):
        for fused in (False, True):
            step(fused, i)
    torch.cuda.synchronize()
    times, peak = {False: [], True: []}, {}
    for i in range(a.steps):                       # the routes alternate, on the same rotating seeds
        for fused in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(fused, 100 + i)
            torch.cuda.synchronize()
            times[fused].append((time.perf_counter() - t0) * 1e3)
    for fused in (False, True):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(fused, 7)
        torch.cuda.synchronize()
        peak[fused] = torch.cuda.max_memory_allocated() - base
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            n_items, losses = step(fused, 7)
        torch.cuda.set_sync_debug_mode("default")
        syncs = sum("synchroniz" in str(w.message) for w in caught)
        t = np.asarray(times[fused])
        print("fused=%-5s items %d  median %.3f ms  p10 %.3f  p90 %.3f  host syncs / call %d  peak memory above resident %.2f MiB  loss_reid %.6f  loss_reid_aux %.6f"
              % (fused, n_items, np.median(t), np.percentile(t, 10), np.percentile(t, 90), syncs, peak[fused] / 2 ** 20,
                 float(losses["loss_reid"].detach()), float(losses["loss_reid_aux"].detach())))
    print("speed-up (median, composition / fused): x%.2f" % (np.median(times[False]) / np.median(times[True])))


if __name__ == "__main__":
    main()
