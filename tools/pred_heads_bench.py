#!/usr/bin/env python
"""A/B of the decoder prediction heads (uninext_amd/modules/prediction_heads.py: DetectionHeads.fused) against the same object
with fused = False, i.e. the reference's composition of PyTorch ops, on one GPU, alternating in one process with rotating
inputs: bs 2, 900 queries, d_model 256, 169 generated mask-head parameters, VL_Align with IoU branch, reference width 4.

    python tools/pred_heads_bench.py [--iters 200] [--warmup 30]

Rows: T = 256 text tokens (detection) and T = 1 pooled token (grounding); the text pooling is outside the timed call.  Per row
and route: median and p10..p90 of per-call times (host clock around a synchronised call), the launches of one call (counted by
torch.profiler) and the peak memory of one warm call above its inputs and outputs.  "faster" means the p10..p90 ranges are
apart.  The fused route is timed on both of its grids ("split": the branch is a grid dimension; "tile": one workgroup per 32
rows), the grid behind `auto` is the one named in the verdict line."""
import argparse
import os
import sys
import time
import types

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uninext_amd import _lib, ext   # noqa: E402
from uninext_amd.modules import MLP, DetectionHeads, VL_Align   # noqa: E402

ROTATE = 3
BS, Q, E, P, LANG, LEVELS = 2, 900, 256, 169, 768, 6


def cfg():
    ns = types.SimpleNamespace
    return ns(MODEL=ns(DYHEAD=ns(PRIOR_PROB=0.01, LOG_SCALE=0.0, FUSE_CONFIG=ns(CLAMP_DOT_PRODUCT=True)),
                       LANGUAGE_BACKBONE=ns(LANG_DIM=LANG), DDETRS=ns(HIDDEN_DIM=E)))


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
    return t[len(t) // 2], t[int(0.1 * (len(t) - 1))], t[int(0.9 * (len(t) - 1))]


def launches(fn, x):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn(x)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn(x)
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    except Exception as e:      # a build without the tracer
        return "n/a (%s)" % type(e).__name__


def peak_above(fn, x):
    fn(x)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn(x)
    torch.cuda.synchronize()
    kept = sum(t.numel() * t.element_size() for t in out if t is not None)
    return (torch.cuda.max_memory_allocated() - before - kept) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    args = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    print(torch.cuda.get_device_name(0), "torch", torch.__version__)
    tiles = BS * ((Q + 31) // 32)
    print("bs %d, %d queries, d_model %d, P %d; grids: split %d workgroups, tile %d" % (BS, Q, E, P, 3 * tiles, tiles))
    heads = DetectionHeads(nn.ModuleList(VL_Align(cfg()) for _ in range(LEVELS)),
                           nn.ModuleList(MLP(E, E, 4, 3) for _ in range(LEVELS)),
                           nn.ModuleList(nn.Linear(E, 1) for _ in range(LEVELS)), MLP(E, E, P, 3)).to(dev).eval()
    with torch.no_grad():
        for m in heads.controller.layers:       # the reference zeroes these biases; any values time alike
            m.bias.uniform_(-0.1, 0.1)
    lvl = LEVELS - 1

    def route(fused, variant="auto"):
        def call(x):
            heads.fused = fused
            ext.pred_heads_set_variant(variant)
            with torch.no_grad():
                return heads.forward_level(lvl, x["hs"], x["reference"], x["text"])
        return call

    all_faster = True
    for row, T in (("detection, T = 256", 256), ("grounding, T = 1", 1)):
        xs = [dict(hs=torch.randn(BS, Q, E, device=dev), reference=torch.rand(BS, Q, 4, device=dev),
                   text=torch.randn(BS, T, LANG, device=dev)) for _ in range(ROTATE)]
        fns = {"fused split": route(True, "split"), "fused tile": route(True, "tile"), "torch": route(False)}
        a, b = fns["fused split"](xs[0]), fns["torch"](xs[0])
        assert _lib.last_kernel("pred_heads") == "pred_heads<split>"
        print("%s: max |fused - torch| logits %.2e, boxes %.2e, iou %.2e, params %.2e; split and tile bitwise equal: %s" % (
            (row,) + tuple(float((s - t).abs().max()) for s, t in zip(a, b))
            + (all(torch.equal(s, t) for s, t in zip(a, fns["fused tile"](xs[0]))),)), flush=True)
        res = dict(zip(fns, (stats(t) for t in timed(list(fns.values()), xs, args.iters, args.warmup))))
        for name, fn in fns.items():
            m, lo, hi = res[name]
            print("  %-12s median %7.3f ms (p10 %.3f .. p90 %.3f), %s launches, peak %6.2f MiB above inputs and outputs" % (
                name, m, lo, hi, launches(fn, xs[1]), peak_above(fn, xs[1])), flush=True)
        ext.pred_heads_set_variant("auto")
        route(True)(xs[0])
        auto = "fused " + _lib.last_kernel("pred_heads")[len("pred_heads<"):-1]
        (mf, lf, hf), (mt, lt, ht) = res[auto], res["torch"]
        verdict = "fused faster" if hf < lt else ("torch faster" if ht < lf else "ranges overlap")
        all_faster &= verdict == "fused faster"
        print("  auto is %s: x%.2f of torch, %s" % (auto, mt / mf, verdict), flush=True)
    heads.fused = False
    print("fused faster with the ranges apart in both rows: %s" % ("yes" if all_faster else "no"))


if __name__ == "__main__":
    main()
