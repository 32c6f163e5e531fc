#!/usr/bin/env python
"""A/B of the detection post-processing (uninext_amd/postprocess.py: DetectionPostProcess.fused) against the same object with
fused = False, i.e. the composition of PyTorch ops that follows the reference image by image, on one GPU, alternating in one
process with rotating inputs: bs 2, 900 queries, 80 classes, 256 tokens, NMS at 0.7 and the top 100.

    python tools/postprocess_bench.py [--iters 30] [--warmup 10]

Rows: without a score threshold and with one (0.3).  Medians and spreads (p10..p90) of per-call wall times around a device
synchronisation (the step ends in host-side slicing, so the host's share counts); "faster" means the medians differ by more than
the larger of the two spreads.  Host synchronisations per call are what torch.cuda.set_sync_debug_mode("warn") reports on a warm
call.  The reference itself cannot run here (it needs torchvision); the composition is its restatement."""
import argparse
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uninext_amd.postprocess import DetectionPostProcess   # noqa: E402

ROTATE = 3
B, Q, C, T = 2, 900, 80, 256


def make_inputs(seed, dev):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, Q, T, generator=g) * 2.0 - 3.0
    centres = 0.2 + 0.6 * torch.rand(B, 12, 2, generator=g)
    cluster = torch.randint(0, 12, (B, Q), generator=g)
    cxcy = torch.gather(centres, 1, cluster.unsqueeze(-1).expand(-1, -1, 2)) + 0.03 * torch.randn(B, Q, 2, generator=g)
    wh = 0.02 + 0.38 * torch.rand(B, Q, 2, generator=g) ** 2
    iou = torch.randn(B, Q, 1, generator=g)
    return logits.to(dev), torch.cat([cxcy, wh], -1).to(dev), iou.to(dev)


def positive_map():
    pm, t = {}, 1
    for c in range(C):
        n = 1 + c % 4
        pm[c + 1] = list(range(t, t + n)) if t + n <= T else [t % T]
        t += n
    return pm


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    dev = "cuda:0"
    print(torch.cuda.get_device_name(0), "torch", torch.__version__)
    print("bs %d, %d queries, %d classes, %d tokens; NMS at 0.7, top 100" % (B, Q, C, T))
    xs = [make_inputs(seed, dev) for seed in range(ROTATE)]
    pm = positive_map()
    sizes = [(800, 1200), (750, 1333)]
    all_faster = True
    for thres in (0.0, 0.3):

        def route(fused):
            post = DetectionPostProcess(ota=True, fused=fused)
            return lambda x: post(x[0], x[1], x[2], sizes, pm, C, score_thres=thres)

        fused, torch_ = route(True), route(False)
        a, b = fused(xs[0]), torch_(xs[0])
        same = [float((ra["query_index"] == rb["query_index"]).float().mean()) if len(ra["scores"]) == len(rb["scores"]) else 0.0
                for ra, rb in zip(a, b)]
        (tf, sf), (tt, st) = [stats(t) for t in timed([fused, torch_], xs, args.iters, args.warmup)]
        verdict = "fused faster" if tt - tf > max(sf, st) else ("torch faster" if tf - tt > max(sf, st) else "within spread")
        all_faster &= verdict == "fused faster"
        print("  score_thres %.1f   fused %8.3f ms (spread %.3f, %s host syncs)   torch %8.3f ms (spread %.3f, %s host syncs)   x%.2f  %s"
              % (thres, tf, sf, host_syncs(fused, xs[1]), tt, st, host_syncs(torch_, xs[1]), tt / tf, verdict), flush=True)
        print("      instances per image %s; same query in %s %% of the places (random inputs keep no margins)"
              % ([len(r["scores"]) for r in a], ["%.1f" % (100 * s) for s in same]), flush=True)
    print("fused faster at both settings: %s" % ("yes" if all_faster else "no"))


if __name__ == "__main__":
    main()
