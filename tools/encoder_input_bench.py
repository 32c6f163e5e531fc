#!/usr/bin/env python
"""A/B of the encoder's input preparation (uninext_amd/modules/encoder_input.py: prepare_encoder_inputs) with fused = True against
fused = False, the reference's statements, on one GPU, alternating in one process with rotating inputs: bs 2, an R50 backbone's
three outputs (512, 1024, 2048 channels) plus the fourth level, 256 channels, at workloads.R50_LEVELS_INFER (800 x 1333) and
R50_LEVELS_TRAIN (800 x 1344, padded per image).

    python tools/encoder_input_bench.py [--iters 30] [--warmup 10]

Two rows per shape: the whole step, and the step after the input_proj convolutions (which are torch on both routes).  Medians
and p10 .. p90 of per-call wall times around a device synchronisation; "faster" means the p10 .. p90 ranges do not overlap.  Kernel
launches are counted by torch.profiler on one warm call, peak memory is the allocator's high-water mark of one warm call above what
was allocated before it plus the outputs."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uninext_amd import ext, workloads   # noqa: E402
from uninext_amd.modules import encoder_input as EI   # noqa: E402

ROTATE = 3
BS, CHANNELS = 2, (512, 1024, 2048)
SHAPES = {"r50_infer": (workloads.R50_LEVELS_INFER, (800, 1333)), "r50_train": (workloads.R50_LEVELS_TRAIN, (800, 1344))}


def make_inputs(levels, image, seed, dev, padded):
    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn((BS, c, h, w), generator=g).to(dev) for c, (h, w) in zip(CHANNELS, levels)]
    mask = torch.zeros((BS,) + image, dtype=torch.bool)
    if padded:      # the second image is smaller, as in a training batch
        mask[1, image[0] - 96 - 8 * seed:, :] = True
        mask[1, :, image[1] - 160 - 8 * seed:] = True
    return feats, mask.to(dev)


def timed(fns, inputs, iters, warmup):
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
    kept = sum(t.numel() * t.element_size() for t in out)
    return (torch.cuda.max_memory_allocated() - before - kept) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    dev = "cuda:0"
    print(torch.cuda.get_device_name(0), "torch", torch.__version__)
    proj = EI.build_input_proj(CHANNELS, 256, 4).to(dev).eval()
    with torch.no_grad():
        for p in proj:
            p[1].weight.uniform_(0.5, 1.5)
            p[1].bias.uniform_(-0.3, 0.3)
    level_embed = torch.randn((4, 256), device=dev)
    embed = EI.PositionEmbeddingSine(128, normalize=True)
    all_faster = True
    for name, (levels, image) in SHAPES.items():
        xs = [make_inputs(levels, image, seed, dev, name == "r50_train") for seed in range(ROTATE)]
        tokens = sum(h * w for h, w in levels)
        print("%s: bs %d, image %d x %d, %d tokens an image" % (name, BS, image[0], image[1], tokens))

        def convs_of(x):
            with torch.no_grad():
                return [proj[l][0](x[0][min(l, 2)]).contiguous() for l in range(4)]

        def whole(fused):
            def run(x):
                with torch.no_grad():
                    return EI.prepare_encoder_inputs(x[0], x[1], proj, level_embed, embed, fused=fused)
            return run

        def after_fused(x):
            return ext.encoder_input_prepare(x[2], x[1], [-1, -1, -1, 0], [p[1].weight for p in proj], [p[1].bias for p in proj],
                                             [p[1].eps for p in proj], level_embed, embed.dim_t(dev), embed.scale)

        def after_torch(x):
            with torch.no_grad():
                srcs, masks, poses = [], [], []
                for l, conv in enumerate(x[2]):
                    src = proj[l][1](conv)
                    mask = EI.interpolate_mask(x[1] if l < 3 else masks[0], src.shape[-2:])
                    srcs.append(src)
                    masks.append(mask)
                    poses.append(embed(EI.NestedTensor(src, mask)))
                flat = EI.flatten_encoder_inputs(srcs, masks, poses, level_embed)
                return flat + (EI.get_reference_points(flat[3], flat[5], dev),)

        xs = [x + (convs_of(x),) for x in xs]
        a, b = whole(True)(xs[0]), whole(False)(xs[0])
        print("  agreement of the routes: src_flatten max |diff| %.2e, pos %.2e, masks equal %s, reference_points equal %s"
              % (float((a.src_flatten - b.src_flatten).abs().max()), float((a.lvl_pos_embed_flatten - b.lvl_pos_embed_flatten).abs().max()),
                 torch.equal(a.mask_flatten, b.mask_flatten), torch.equal(a.reference_points, b.reference_points)))
        for row, (f, t) in (("whole step (with the input_proj convolutions)", (whole(True), whole(False))),
                            ("after the convolutions", (after_fused, after_torch))):
            (mf, lf, hf), (mt, lt, ht) = [stats(v) for v in timed([f, t], xs, args.iters, args.warmup)]
            verdict = "fused faster" if hf < lt else ("torch faster" if ht < lf else "ranges overlap")
            all_faster &= verdict == "fused faster"
            print("  %-46s fused %7.3f ms (p10 %.3f .. p90 %.3f), %s launches, peak %6.1f MiB above inputs and outputs" % (
                row, mf, lf, hf, launches(f, xs[1]), peak_above(f, xs[1])), flush=True)
            print("  %-46s torch %7.3f ms (p10 %.3f .. p90 %.3f), %s launches, peak %6.1f MiB above inputs and outputs   x%.2f  %s" % (
                "", mt, lt, ht, launches(t, xs[1]), peak_above(t, xs[1]), mt / mf, verdict), flush=True)
    print("fused faster with the ranges apart in every row: %s" % ("yes" if all_faster else "no"))


if __name__ == "__main__":
    main()
