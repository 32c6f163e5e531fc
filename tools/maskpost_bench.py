#!/usr/bin/env python
"""A/B of the mask post-processing (uninext_amd/postprocess.py: MaskPostProcess and mask_nms with fused = True) against the same
code with fused = False, i.e. the reference's sequence of PyTorch ops, on one GPU, alternating in one process with rotating
inputs.

    python tools/maskpost_bench.py [--iters 30] [--warmup 10]

Rows: masks of 100 instances from 200x336 logits at stride 4, cropped to 800x1333, at the image size and at 480x640; 10 instances
to 720x1280; mask_nms of 30 and of 100 detections at 200x336.  Medians and spreads (p10..p90) of per-call wall times around a
device synchronisation; "faster" means the medians differ by more than the larger of the two spreads.  Host synchronisations per
call are what torch.cuda.set_sync_debug_mode("warn") reports on a warm call; peak memory is the allocator's high-water mark of a
warm call above what was allocated before it (the inputs) and the result it returns."""
import argparse
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uninext_amd.postprocess import MaskPostProcess, mask_nms   # noqa: E402

ROTATE = 3
H, W, STRIDE = 200, 336, 4
CROP = (800, 1333)


def make_logits(seed, n, dev, spread=1.0):
    """[n, H, W] fp32: 1.5 x an ellipse's signed distance plus noise; `spread` < 1 draws the ellipses closer (more overlap)."""
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    c = (0.5 + spread * (torch.rand(n, 2, generator=g) - 0.5) * 0.6) * torch.tensor([H, W])
    r = (0.1 + 0.25 * torch.rand(n, 2, generator=g)) * torch.tensor([H, W])
    rho = torch.sqrt(((ys - c[:, 0, None, None]) / r[:, 0, None, None]) ** 2 + ((xs - c[:, 1, None, None]) / r[:, 1, None, None]) ** 2)
    return (1.5 * (1 - rho) * r.min(1)[0][:, None, None] + 0.3 * torch.randn(n, H, W, generator=g)).to(dev)


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


def peak_mb(fn, x):
    """High-water mark of a warm call above the memory held before it and the tensor it returns, in MB."""
    fn(x)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn(x)
    torch.cuda.synchronize()
    kept = out.numel() * out.element_size() if torch.is_tensor(out) else 0
    return (torch.cuda.max_memory_allocated() - base - kept) / 1e6


def row(label, fused, torch_, xs, iters, warmup, agree):
    (tf, sf), (tt, st) = [stats(t) for t in timed([fused, torch_], xs, iters, warmup)]
    verdict = "fused faster" if tt - tf > max(sf, st) else ("torch faster" if tf - tt > max(sf, st) else "within spread")
    print("  %-44s fused %9.3f ms (spread %.3f, %s host syncs, peak %8.1f MB)   torch %9.3f ms (spread %.3f, %s host syncs, peak %8.1f MB)"
          "   x%.2f  %s" % (label, tf, sf, host_syncs(fused, xs[1]), peak_mb(fused, xs[1]), tt, st, host_syncs(torch_, xs[1]),
                           peak_mb(torch_, xs[1]), tt / tf, verdict), flush=True)
    print("      %s" % agree(fused(xs[0]), torch_(xs[0])), flush=True)
    return verdict == "fused faster"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    dev = "cuda:0"
    print(torch.cuda.get_device_name(0), "torch", torch.__version__)
    print("%dx%d logits, stride %d, crop %dx%d, thres 0.5; mask_nms at 0.5" % (H, W, STRIDE, CROP[0], CROP[1]))
    ahead = []
    for n, out in ((100, CROP), (100, (480, 640)), (10, (720, 1280))):
        xs = [(make_logits(seed, n, dev), torch.randperm(n, generator=torch.Generator().manual_seed(seed)).to(dev)) for seed in range(ROTATE)]

        def route(fused, out=out):
            post = MaskPostProcess(STRIDE, 0.5, fused=fused)
            return lambda x: post(x[0], x[1], CROP, out)

        ahead.append(row("%d instances -> %dx%d" % (n, out[0], out[1]), route(True), route(False), xs, args.iters, args.warmup,
                         lambda a, b: "bytes that differ between the routes: %d of %d" % (int((a != b).sum()), a.numel())))
        del xs
        torch.cuda.empty_cache()
    for n in (30, 100):
        xs = [(make_logits(10 + seed, n, dev, spread=0.6).unsqueeze(1),) for seed in range(ROTATE)]

        def route(fused, n=n):
            return lambda x: mask_nms(x[0], [0.0] * n, None, nms_thr=0.5, fused=fused)

        ahead.append(row("mask_nms, %d detections" % n, route(True), route(False), xs, max(3, args.iters // 3), max(2, args.warmup // 3),
                         lambda a, b: "kept %d of %d; the routes' lists are %s" % (sum(a), len(a), "equal" if a == b else "DIFFERENT")))
    print("fused faster at every shape: %s" % ("yes" if all(ahead) else "no"))


if __name__ == "__main__":
    main()
