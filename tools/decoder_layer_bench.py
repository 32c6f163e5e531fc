#!/usr/bin/env python
"""A/B of the decoder layer's fused self-attention (uninext_amd/modules/decoder_layer.py: fused_self_attn) against the PyTorch
composition, on one GPU, alternating in one process with rotating inputs: bs 2, d_model 256, 8 heads, the R50 800 x 1333 memory
(S = 22 223), at Lq = 900 without a mask and Lq = 1100 with a denoising-shaped bool mask (pad_size 200: 5 groups of 40).

    python tools/decoder_layer_bench.py [--iters 30] [--warmup 10]

Legs: the kernel alone; the self-attention block from (tgt, query_pos) to norm2's output, against nn.MultiheadAttention on
[L, B, E] views + add + nn.LayerNorm as the reference calls it; the whole layer and the six-layer decoder (ref_point_head, box
refinement) with fused_self_attn on against off.  Medians and spreads (p10..p90) of per-call event times; "faster" means the
medians differ by more than the larger of the two spreads.

    python tools/decoder_layer_bench.py --train [--iters 30] [--warmup 10] [--out profiles/r32_decoder_train.txt]

The training route instead (own_training): forward + backward of the self-attention block (the two projections, the core,
out_proj) and of the whole layer in train() with dropout 0, on the same two cases (the mask: 200 noised queries as 5 groups of 40
in the reference's group layout), own_training on against the same module with the flag off.  Rotating inputs, the routes
alternate call by call; p10 / median / p90 of per-call event times, and the peak memory of one call above what is allocated
before it (inputs, parameters).  "faster" means the two p10..p90 ranges are apart."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uninext_amd import ext   # noqa: E402
from uninext_amd.modules import DeformableTransformerDecoder, DeformableTransformerDecoderLayer as Layer, MLP   # noqa: E402

ROTATE = 3
LEVELS = [(100, 167), (50, 84), (25, 42), (13, 21)]


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


def report(label, fns, inputs, args):
    (tf, sf), (tt, st) = [stats(t) for t in timed(fns, inputs, args.iters, args.warmup)]
    verdict = "fused faster" if tt - tf > max(sf, st) else ("torch faster" if tf - tt > max(sf, st) else "within spread")
    print("  %-22s fused %8.3f ms (spread %.3f)   torch %8.3f ms (spread %.3f)   x%.2f  %s" % (label, tf, sf, tt, st, tt / tf, verdict),
          flush=True)


def dn_shaped_mask(lq, pad, groups, dev):
    m = torch.zeros(lq, lq, dtype=torch.bool, device=dev)
    m[pad:, :pad] = True
    g = pad // groups
    for n in range(groups):
        m[n * g:(n + 1) * g, :n * g] = True
        m[n * g:(n + 1) * g, (n + 1) * g:pad] = True
    return m


def train_legs(args, dev, emit):
    B, E, heads = 2, 256, 8
    S = sum(h * w for h, w in LEVELS)
    shapes = torch.as_tensor(LEVELS, dtype=torch.long, device=dev)
    lsi = torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))
    srcs = [torch.randn(B, S, E, device=dev) for _ in range(ROTATE)]
    ratios = torch.ones(B, 4, 2, device=dev)
    layer = Layer(E, 1024, 0.0, "relu", 4, heads, 4).to(dev).train()

    def pct(t, q):
        return t[int(q * (len(t) - 1))]

    for lq, mask in ((900, None), (1100, dn_shaped_mask(1100, 200, 5, dev))):
        emit("Lq %d, %s: bs %d, %d heads x %d, S %d, forward + backward" % (
            lq, "no mask" if mask is None else "bool denoising mask (200 noised queries: 5 groups of 40)", B, heads, E // heads, S))
        xs = []
        for n in range(ROTATE):
            ref = torch.rand(B, lq, 4, device=dev) * 0.5 + 0.25
            xs.append(dict(tgt=torch.randn(B, lq, E, device=dev).requires_grad_(True),
                           pos=torch.randn(B, lq, E, device=dev).requires_grad_(True),
                           ref_in=(ref[:, :, None] * torch.cat([ratios, ratios], -1)[:, None]).contiguous(),
                           src=srcs[n].clone().requires_grad_(True), G=torch.randn(B, lq, E, device=dev)))

        def block(x):
            if layer.own_training:
                out = layer._self_attn_fused(x["tgt"], x["pos"], mask, train=True)
            else:
                out = layer._self_attn_composition(x["tgt"], x["pos"], mask)
            out.backward(x["G"])

        def whole(x):
            layer(x["tgt"], x["pos"], x["ref_in"], x["src"], shapes, lsi, None, mask).backward(x["G"])

        def route(fn, flag):
            def call(x):
                layer.own_training = flag
                for t in [x["tgt"], x["pos"], x["src"]] + list(layer.parameters()):
                    t.grad = None
                fn(x)
            return call

        def peak(fn, x):
            fn(x)
            torch.cuda.synchronize()
            for t in [x["tgt"], x["pos"], x["src"]] + list(layer.parameters()):
                t.grad = None
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            fn(x)
            torch.cuda.synchronize()
            return (torch.cuda.max_memory_allocated() - before) / 2 ** 20

        for label, fn in (("self-attention block", block), ("whole layer", whole)):
            on, off = route(fn, True), route(fn, False)
            t_on, t_off = timed([on, off], xs, args.iters, args.warmup)
            lo_on, hi_on, lo_off, hi_off = pct(t_on, 0.1), pct(t_on, 0.9), pct(t_off, 0.1), pct(t_off, 0.9)
            verdict = "own faster" if hi_on < lo_off else ("torch faster" if hi_off < lo_on else "ranges overlap")
            emit("  %-22s own   p10 %7.3f  median %7.3f  p90 %7.3f ms   peak %7.1f MiB" % (
                label, lo_on, pct(t_on, 0.5), hi_on, peak(on, xs[0])))
            emit("  %-22s torch p10 %7.3f  median %7.3f  p90 %7.3f ms   peak %7.1f MiB   x%.2f  %s" % (
                "", lo_off, pct(t_off, 0.5), hi_off, peak(off, xs[0]), pct(t_off, 0.5) / pct(t_on, 0.5), verdict))
    layer.own_training = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--train", action="store_true", help="the training route (own_training) instead of the inference legs")
    ap.add_argument("--out", default=None, help="--train: also append the lines to this file")
    args = ap.parse_args()
    dev = "cuda:0"
    if args.train:
        torch.manual_seed(0)
        lines = []

        def emit(line):
            print(line, flush=True)
            lines.append(line)
        emit("%s torch %s: decoder layer training route, own_training on against off (iters %d, warmup %d, %d rotating inputs)" % (
            torch.cuda.get_device_name(0), torch.__version__, args.iters, args.warmup, ROTATE))
        train_legs(args, dev, emit)
        if args.out:
            with open(args.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    torch.manual_seed(0)
    print(torch.cuda.get_device_name(0), "torch", torch.__version__)
    B, E, heads = 2, 256, 8
    S = sum(h * w for h, w in LEVELS)
    shapes = torch.as_tensor(LEVELS, dtype=torch.long, device=dev)
    lsi = torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))
    srcs = [torch.randn(B, S, E, device=dev) for _ in range(ROTATE)]
    ratios = torch.ones(B, 4, 2, device=dev)

    layer = Layer(E, 1024, 0.0, "relu", 4, heads, 4).to(dev).eval()
    dec = DeformableTransformerDecoder(E, layer, 6, return_intermediate=True).to(dev).eval()
    dec.bbox_embed = torch.nn.ModuleList(MLP(E, E, 4, 3) for _ in range(6)).to(dev)
    mha, norm2 = layer.self_attn, layer.norm2

    def route(fn, fused):
        def call(x):
            old, Layer.fused_self_attn = Layer.fused_self_attn, fused
            try:
                with torch.no_grad():
                    return fn(x)
            finally:
                Layer.fused_self_attn = old
        return call

    for lq, mask in ((900, None), (1100, dn_shaped_mask(1100, 200, 5, dev))):
        print("Lq %d, %s: bs %d, %d heads x %d, S %d; kernel grid %d workgroups x 2 waves" % (
            lq, "no mask" if mask is None else "bool mask (pad_size 200, 5 groups of 40)", B, heads, E // heads, S,
            B * heads * ((lq + 31) // 32)))
        xs = []
        for n in range(ROTATE):
            ref = torch.rand(B, lq, 4, device=dev) * 0.5 + 0.25
            xs.append(dict(tgt=torch.randn(B, lq, E, device=dev), pos=torch.randn(B, lq, E, device=dev), ref=ref,
                           ref_in=(ref[:, :, None] * torch.cat([ratios, ratios], -1)[:, None]).contiguous(), src=srcs[n],
                           qk=torch.randn(B, lq, 2 * E, device=dev), v=torch.randn(B, lq, E, device=dev)))

        def kernel(x):
            return ext.decoder_self_attention(x["qk"][..., :E], x["qk"][..., E:], x["v"], heads, mask)

        def block_fused(x):
            return layer._add_norm(layer._self_attn_fused(x["tgt"], x["pos"], mask), x["tgt"], norm2)

        def block_reference(x):          # deformable_transformer_dino.py:411-414
            qk = (x["tgt"] + x["pos"]).transpose(0, 1)
            tgt2 = mha(qk, qk, x["tgt"].transpose(0, 1), attn_mask=mask)[0].transpose(0, 1)
            return norm2(x["tgt"] + tgt2)

        def whole_layer(x):
            return layer(x["tgt"], x["pos"], x["ref_in"], x["src"], shapes, lsi, None, mask)

        def decoder(x):
            return dec(x["tgt"], x["ref"], x["src"], shapes, lsi, ratios, None, None, mask)

        with torch.no_grad():
            err = (block_fused(xs[0]) - block_reference(xs[0])).abs().max()
        print("  self-attention block, fused against torch: max abs difference %.2e" % float(err))
        report("kernel alone (vs block)", [route(kernel, True), route(block_reference, False)], xs, args)
        report("self-attention block", [route(block_fused, True), route(block_reference, False)], xs, args)
        report("whole layer", [route(whole_layer, True), route(whole_layer, False)], xs, args)
        report("six-layer decoder", [route(decoder, True), route(decoder, False)], xs, args)


if __name__ == "__main__":
    main()
