#!/usr/bin/env python
"""A/B of the ViT attention core (uninext_amd/vit.py: Attention.fused_core) against the PyTorch composition of the same module,
on one GPU, alternating in one process: the core alone, Attention.forward and Block.forward, at the windowed and the global block
of ViT-H and ViT-B for a batch of two 800 x 1344 images (50 x 84 tokens), with medians, spreads (p10..p90) and peak memory above
what is allocated before the call.

    python tools/vit_bench.py [--iters 20] [--warmup 5] [--models ViT-huge ViT-Base]
    python tools/vit_bench.py --train        forward + backward, Attention.own_training on ("fused") against off ("torch"), at the
                                             ViT-H windowed core (25 windows of 14 x 14) and global cores (64 x 64, and
                                             50 x 84 with interpolated tables): the core alone and one Block of each
                                             kind, with peak memory over the step

"Faster" in the last column: the medians differ by more than the larger of the two spreads.  The fp32 matrix rate counts
2 * 2 * S^2 * D per head for the two products plus 2 * S * (q_h + q_w) * D per head for the relative-position terms."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uninext_amd import ext, vit   # noqa: E402

ROTATE = 3


def timed(fns, inputs, iters, warmup):
    """Per-route sorted times in ms; the routes alternate call by call, the inputs rotate."""
    times = [[] for _ in fns]
    for it in range(warmup + iters):
        for r, fn in enumerate(fns):
            x = inputs[it % len(inputs)]
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn(x)
            stop.record()
            stop.synchronize()
            if it >= warmup:
                times[r].append(start.elapsed_time(stop))
    return [sorted(t) for t in times]


def stats(t):
    return t[len(t) // 2], t[int(0.9 * (len(t) - 1))] - t[int(0.1 * (len(t) - 1))]


def peak(fn, x):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn(x)
    torch.cuda.synchronize()
    held = out.numel() * out.element_size()
    del out
    return (torch.cuda.max_memory_allocated() - base - held) / 2 ** 20


def report(label, fns, inputs, args, flops=None):
    (tf, sf), (tt, st) = [stats(t) for t in timed(fns, inputs, args.iters, args.warmup)]
    mf, mt = peak(fns[0], inputs[0]), peak(fns[1], inputs[0])
    verdict = "fused faster" if tt - tf > max(sf, st) else ("torch faster" if tf - tt > max(sf, st) else "within spread")
    rate = "  %.1f TFLOP/s fp32" % (flops / tf / 1e9) if flops else ""
    print("  %-22s fused %8.3f ms (spread %.3f, peak +%.0f MiB)   torch %8.3f ms (spread %.3f, peak +%.0f MiB)   x%.2f  %s%s" % (
        label, tf, sf, mf, tt, st, mt, tt / tf, verdict, rate), flush=True)


def train_leg(args, dev):
    kw = vit.vit_kwargs("ViT-huge")
    dim, heads = kw["embed_dim"], kw["num_heads"]
    D = dim // heads
    for kind, window, grid in (("windowed", 14, (70, 70)), ("global", 0, (64, 64)), ("global", 0, (50, 84))):
        blk = vit.Block(dim, heads, use_rel_pos=True, rel_pos_zero_init=False, window_size=window, input_size=(64, 64),
                        norm_layer=kw["norm_layer"]).to(dev).eval()
        a = blk.attn
        xs = [torch.randn(1, grid[0], grid[1], dim, device=dev) for _ in range(ROTATE)]
        with torch.no_grad():
            ax = [vit.window_partition(blk.norm1(x), 14)[0] if window else blk.norm1(x) for x in xs]
            Bp, H, W, _ = ax[0].shape
            S = H * W
            qkvs = [a.qkv(x).reshape(Bp, S, -1) for x in ax]
        print("ViT-huge %s block, training step: B' %d, S %d (%d x %d), %d heads x %d" % (kind, Bp, S, H, W, heads, D))

        def step(fn, own):
            def call(x):
                old, vit.Attention.own_training = vit.Attention.own_training, own
                try:
                    for p in blk.parameters():
                        p.grad = None
                    x = x.detach().requires_grad_(True)
                    out = fn(x)
                    out.backward(torch.ones_like(out))
                    return x.grad
                finally:
                    vit.Attention.own_training = old
            return call

        def core_own(qkv):
            th, tw = vit.resize_rel_pos(a.rel_pos_h, 2 * H - 1).contiguous(), vit.resize_rel_pos(a.rel_pos_w, 2 * W - 1).contiguous()
            return vit.ViTAttentionFunction.apply(qkv, th, tw, heads, (H, W), a.scale)

        def core_torch(qkv):
            return a._core_torch(qkv, H, W)

        flops = Bp * heads * (14.0 * S * S * D)      # forward 2 products, backward 5 (the recomputed scores included)
        report("attention core", [step(core_own, True), step(core_torch, False)], qkvs, args, flops)
        report("Block", [step(blk, True), step(blk, False)], xs, args)
        del blk, xs, ax, qkvs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--models", nargs="+", default=["ViT-huge", "ViT-Base"])
    ap.add_argument("--train", action="store_true", help="the training leg: forward + backward with Attention.own_training on / off")
    args = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    print(torch.cuda.get_device_name(0), "torch", torch.__version__)
    if args.train:
        return train_leg(args, dev)
    for name in args.models:
        kw = vit.vit_kwargs(name)
        dim, heads = kw["embed_dim"], kw["num_heads"]
        D = dim // heads
        for kind, window in (("windowed", 14), ("global", 0)):
            blk = vit.Block(dim, heads, use_rel_pos=True, rel_pos_zero_init=False, window_size=window, input_size=(64, 64),
                            norm_layer=kw["norm_layer"]).to(dev).eval()
            a = blk.attn
            xs = [torch.randn(2, 50, 84, dim, device=dev) for _ in range(ROTATE)]
            with torch.no_grad():
                ax = [vit.window_partition(blk.norm1(x), 14)[0] if window else blk.norm1(x) for x in xs]
                Bp, H, W, _ = ax[0].shape
                S = H * W
                qkvs = [a.qkv(x).reshape(Bp, S, -1) for x in ax]
                th, tw = a._resized_tables(H, W)
            print("%s %s block: B' %d, S %d (%d x %d), %d heads x %d" % (name, kind, Bp, S, H, W, heads, D))

            def route(fn, fused):
                def call(x):
                    old, vit.Attention.fused_core = vit.Attention.fused_core, fused
                    try:
                        with torch.no_grad():
                            return fn(x)
                    finally:
                        vit.Attention.fused_core = old
                return call

            def core_torch(qkv):
                return a._core_torch(qkv, H, W)

            flops = Bp * heads * (4.0 * S * S * D + 2.0 * S * (H + W) * D)
            report("attention core", [route(lambda q: ext.vit_attention(q, th, tw, heads, (H, W), a.scale), True), route(core_torch, False)],
                   qkvs, args, flops)
            report("Attention.forward", [route(a, True), route(a, False)], ax, args)
            report("Block.forward", [route(blk, True), route(blk, False)], xs, args)
            del blk, xs, ax, qkvs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
