#!/usr/bin/env python
"""A/B of the encoder layer's training routes (uninext_amd/modules/encoder_layer.py: own_training / own_dropout) against the layer
with the flags off -- the composition of PyTorch ops around MSDeformAttn, the module as it was before the route existed -- on
one GPU, alternating in one process with rotating inputs: forward + backward of ONE DeformableTransformerEncoderLayer in train(),
bs 2, 22 223 tokens per image (800 x 1333), d_model 256, d_ffn 2048, every parameter and the input trainable.

    python tools/encoder_layer_train_bench.py [--iters 30] [--warmup 8] [--out profiles/r40_encoder_layer_train.txt]

Routes: composition and set_own_training(True) at dropout 0; composition and set_own_training(True, dropout=True) at dropout 0.1.
Then the two ops alone, forward + backward, against their PyTorch compositions at the layer's shapes ([44 446, 256] and
[44 446, 2048]).  p10 / median / p90 of per-call event times over --iters calls after --warmup, the device kernels one call
launches (torch.profiler) and the peak memory of one call above what is allocated before it (parameters, inputs; gradients are
released first).  "faster" means the two p10..p90 ranges are apart."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uninext_amd import ext, workloads                                                   # noqa: E402
from uninext_amd.functions import DropoutAddLayerNormFunction, ReluDropoutFunction      # noqa: E402
from uninext_amd.modules import DeformableTransformerEncoderLayer                       # noqa: E402

ROTATE = 3
B, D_MODEL, D_FFN = 2, 256, 2048
LEVELS = workloads.R50_LEVELS_INFER


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


def pct(t, q):
    return t[int(q * (len(t) - 1))]


def launches(fn, x):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn(x)
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception:   # a build without the device profiler: the column is empty
        return -1


def peak(fn, x, release):
    release()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn(x)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 2 ** 20


def report(emit, tag, routes, pairs, inputs, args, release):
    ts = timed([fn for _, fn in routes], inputs, args.iters, args.warmup)
    for (name, fn), t in zip(routes, ts):
        emit("  %-6s %-22s p10 %8.3f  median %8.3f  p90 %8.3f ms   %4d launches   peak %8.1f MiB" % (
            tag, name, pct(t, 0.1), pct(t, 0.5), pct(t, 0.9), launches(fn, inputs[0]), peak(fn, inputs[0], release)))
    for own, base in pairs:
        apart = pct(ts[own], 0.9) < pct(ts[base], 0.1)
        behind = pct(ts[base], 0.9) < pct(ts[own], 0.1)
        emit("  %-6s %-22s against %-22s x%.2f  %s" % (tag, routes[own][0], routes[base][0], pct(ts[base], 0.5) / pct(ts[own], 0.5),
                                                       "own faster" if apart else "own slower" if behind else "ranges overlap"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)

    def emit(line):
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    S = sum(h * w for h, w in LEVELS)
    rows = B * S
    emit("encoder layer TRAINING step (forward + backward, train()), bs %d, %d tokens per image, d_model %d, d_ffn %d, fp32, %s, torch %s; "
         "%d iters after %d warm-up, routes alternate, %d input sets" % (B, S, D_MODEL, D_FFN, torch.cuda.get_device_name(0),
                                                                          torch.__version__, args.iters, args.warmup, ROTATE))
    layer = DeformableTransformerEncoderLayer(d_model=D_MODEL, d_ffn=D_FFN, dropout=0.1).to(dev).train()
    with torch.no_grad():
        layer.self_attn.sampling_offsets.weight.normal_(0, 0.02)
        layer.self_attn.attention_weights.weight.normal_(0, 0.1)
    ref = workloads.encoder_reference_points(LEVELS, dev)[None, :, None, :].expand(B, S, 4, 2).contiguous()
    shapes, lsi = workloads.level_tensors(LEVELS, dev)
    pos = torch.randn(B, S, D_MODEL, device=dev) * 0.3
    inputs = [torch.randn(B, S, D_MODEL, device=dev).requires_grad_(True) for _ in range(ROTATE)]
    grad = torch.randn(B, S, D_MODEL, device=dev)

    def release():
        layer.zero_grad(set_to_none=True)
        for x in inputs:
            x.grad = None

    def route(own, own_dropout, p):
        def call(x):
            layer.own_training, layer.own_dropout = own, own_dropout
            for d in (layer.dropout1, layer.dropout2, layer.dropout3):
                d.p = p
            release()
            layer(x, pos, ref, shapes, lsi, None).backward(grad)
        return call
    routes = (("composition p 0", route(False, False, 0.0)), ("own p 0", route(True, False, 0.0)),
              ("composition p 0.1", route(False, False, 0.1)), ("own dropout p 0.1", route(True, True, 0.1)))
    emit("  peak: of one step above the parameters and inputs; the gradients of the previous step are released first")
    report(emit, "layer", routes, ((1, 0), (3, 2)), inputs, args, release)
    layer.own_training = layer.own_dropout = False
    release()

    # the two ops alone, forward + backward, at the layer's shapes
    gamma = torch.ones(D_MODEL, device=dev, requires_grad=True)
    beta = torch.zeros(D_MODEL, device=dev, requires_grad=True)
    for p in (0.0, 0.1):
        xs = [(torch.randn(rows, D_MODEL, device=dev).requires_grad_(True), torch.randn(rows, D_MODEL, device=dev).requires_grad_(True))
              for _ in range(ROTATE)]
        g = torch.randn(rows, D_MODEL, device=dev)

        def ln_release():
            gamma.grad = beta.grad = None
            for a, b in xs:
                a.grad = b.grad = None

        def ln_own(x):
            ln_release()
            seed = ext.bi_attention_seed(dev) if p > 0 else None
            DropoutAddLayerNormFunction.apply(x[0], x[1], gamma, beta, 1e-5, p, seed).backward(g)

        def ln_comp(x):
            ln_release()
            F.layer_norm(x[1] + F.dropout(x[0], p, True), (D_MODEL,), gamma, beta, 1e-5).backward(g)
        report(emit, "p %.1f" % p, (("add+LN composition", ln_comp), ("add+LN own", ln_own)), ((1, 0),), xs, args, ln_release)
        del xs, g
        hs = [torch.randn(rows, D_FFN, device=dev).requires_grad_(True) for _ in range(ROTATE)]
        gh = torch.randn(rows, D_FFN, device=dev)

        def relu_release():
            for h in hs:
                h.grad = None

        def relu_own(h):
            relu_release()
            seed = ext.bi_attention_seed(dev) if p > 0 else None
            ReluDropoutFunction.apply(h, p, seed).backward(gh)

        def relu_comp(h):
            relu_release()
            F.dropout(F.relu(h), p, True).backward(gh)
        report(emit, "p %.1f" % p, (("relu+dropout composition", relu_comp), ("relu+dropout own", relu_own)), ((1, 0),), hs, args,
               relu_release)
        del hs, gh


if __name__ == "__main__":
    main()
