#!/usr/bin/env python
"""A/B of the text encoder's fused route (uninext_amd/text_encoder.py: BertModel.fused) against the reference-era composition
(fused=False) and against the same module with F.scaled_dot_product_attention as its core, on one GPU, alternating in one process
with rotating inputs: bert-base geometry (12 layers, 768 wide, 12 heads of 64), bs 2, T = 256 (MAX_QUERY_LEN), with 20 and with
256 valid tokens per prompt.

    python tools/text_encoder_bench.py [--iters 40] [--warmup 10] [--out profiles/r38_text_encoder.txt]

The three routes alternate call by call on ROTATE input sets; p10 / median / p90 of per-call event times over --iters calls
after --warmup, the device kernels one call launches (torch.profiler) and the peak memory of one call above what is allocated
before it (parameters, inputs).  "faster" means the two p10..p90 ranges are apart.  Also the attention kernel alone at the two
occupancies, the number behind the choice of its grid."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uninext_amd import ext, text_encoder as TE   # noqa: E402

ROTATE = 3
B, T = 2, 256


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


def peak(fn, x):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn(x)
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - before) / 2 ** 20


def sdpa_core(self, q, k, v, additive_mask):
    return F.scaled_dot_product_attention(q, k, v, attn_mask=additive_mask)


def train_leg(args, dev, emit):
    """--train: forward + backward of the whole encoder in train() with the shipped dropouts (0.1 hidden, 0.1 attention), every
    parameter trainable: the composition (the flags off: the module as it was before the training route existed) against
    set_own_training(True) with the attention dropout set to 0 and against set_own_training(True, dropout=True)."""
    model = TE.BertModel().to(dev).train()
    attention = [layer.attention.self for layer in model.encoder.layer]
    emit("text encoder TRAINING step (forward + backward, train(), hidden dropout 0.1), bert-base geometry, bs %d, T %d, fp32, %s, "
         "torch %s; %d iters after %d warm-up, routes alternate, %d input sets"
         % (B, T, torch.cuda.get_device_name(0), torch.__version__, args.iters, args.warmup, ROTATE))

    def route(own, own_dropout, attention_p):
        def call(x):
            model.set_own_training(own, own_dropout)
            for a in attention:
                a.dropout.p = attention_p
            model.zero_grad(set_to_none=True)
            model(x[0], x[1]).last_hidden_state.sum().backward()
        return call
    routes = (("composition p 0.1", route(False, False, 0.1)), ("composition p 0", route(False, False, 0.0)),
              ("own p 0", route(True, False, 0.0)), ("own dropout p 0.1", route(True, True, 0.1)))
    grad_mib = sum(p.numel() for p in model.parameters()) * 4 / 2 ** 20

    def train_peak(fn, x):
        """peak() with the previous step's gradients released first, so that they do not hide the activations"""
        model.zero_grad(set_to_none=True)
        return peak(fn, x)
    emit("  peak: of one step above the parameters and inputs; the %.0f MiB of parameter gradients every route ends with are "
         "released before the step and counted in it" % grad_mib)
    for valid in (20, 256):
        mask = (torch.arange(T, device=dev)[None, :] < valid).long().expand(B, T).contiguous()
        inputs = [(torch.randint(1, 30522, (B, T), device=dev) * mask, mask) for _ in range(ROTATE)]
        ts = timed([fn for _, fn in routes], inputs, args.iters, args.warmup)
        for (name, fn), t in zip(routes, ts):
            emit("  valid %3d  %-18s p10 %7.3f  median %7.3f  p90 %7.3f ms   %4d launches   peak %7.1f MiB" % (
                valid, name, pct(t, 0.1), pct(t, 0.5), pct(t, 0.9), launches(fn, inputs[0]), train_peak(fn, inputs[0])))
        for own, base in ((2, 1), (3, 0)):
            apart = pct(ts[own], 0.9) < pct(ts[base], 0.1)
            behind = pct(ts[base], 0.9) < pct(ts[own], 0.1)
            emit("  valid %3d  %-18s against %-18s x%.2f  %s" % (valid, routes[own][0], routes[base][0], pct(ts[base], 0.5) / pct(ts[own], 0.5),
                                                                 "own faster" if apart else "own slower" if behind else "ranges overlap"))
    model.set_own_training(False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--train", action="store_true", help="the training step (forward + backward) instead of the inference routes")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)

    def emit(line):
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    if args.train:
        return train_leg(args, dev, emit)

    model = TE.BertModel().to(dev).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    emit("text encoder, bert-base geometry, bs %d, T %d, fp32, %s, torch %s; %d iters after %d warm-up, routes alternate, %d input sets"
         % (B, T, torch.cuda.get_device_name(0), torch.__version__, args.iters, args.warmup, ROTATE))

    plain_core = TE.BertSelfAttention.core

    def route(fused, core=plain_core):
        def call(x):
            model.fused = fused
            TE.BertSelfAttention.core = core
            with torch.no_grad():
                return model(x[0], x[1]).last_hidden_state
        return call
    routes = (("fused", route(True)), ("composition", route(False)), ("sdpa", route(False, sdpa_core)))

    for valid in (20, 256):
        mask = (torch.arange(T, device=dev)[None, :] < valid).long().expand(B, T).contiguous()
        inputs = [(torch.randint(1, 30522, (B, T), device=dev) * mask, mask) for _ in range(ROTATE)]
        ref = routes[1][1](inputs[0])
        for name, fn in routes:
            err = float((fn(inputs[0]) - ref)[:, :valid].abs().max() / ref[:, :valid].abs().max())
            emit("  valid %3d  %-12s max abs difference from the composition on the valid tokens: %.2e of its scale" % (valid, name, err))
        ts = timed([fn for _, fn in routes], inputs, args.iters, args.warmup)
        for (name, fn), t in zip(routes, ts):
            emit("  valid %3d  %-12s p10 %7.3f  median %7.3f  p90 %7.3f ms   %4d launches   peak %7.1f MiB" % (
                valid, name, pct(t, 0.1), pct(t, 0.5), pct(t, 0.9), launches(fn, inputs[0]), peak(fn, inputs[0])))
        for other in (1, 2):
            apart = pct(ts[0], 0.9) < pct(ts[other], 0.1)
            behind = pct(ts[other], 0.9) < pct(ts[0], 0.1)
            emit("  valid %3d  fused against %-12s x%.2f  %s" % (valid, routes[other][0], pct(ts[other], 0.5) / pct(ts[0], 0.5),
                                                               "fused faster" if apart else "fused slower" if behind else "ranges overlap"))

        # the attention core alone: the kernel against matmul / softmax / matmul on the same projections
        qkvs = [torch.randn(B, T, 3 * 768, device=dev) for _ in range(ROTATE)]
        add = TE.extended_attention_mask(mask, torch.float32)
        attn = model.encoder.layer[0].attention.self

        def kernel(qkv):
            return ext.bert_self_attention(qkv[..., :768], qkv[..., 768:1536], qkv[..., 1536:], 12, mask)

        def composed(qkv):
            h = lambda t: t.view(B, T, 12, 64).permute(0, 2, 1, 3)
            return plain_core(attn, h(qkv[..., :768]), h(qkv[..., 768:1536]), h(qkv[..., 1536:]), add).permute(0, 2, 1, 3).reshape(B, T, 768)
        tk, tc = timed([kernel, composed], qkvs, args.iters, args.warmup)
        emit("  valid %3d  core alone: kernel p10 %6.3f median %6.3f p90 %6.3f ms   composition p10 %6.3f median %6.3f p90 %6.3f ms" % (
            valid, pct(tk, 0.1), pct(tk, 0.5), pct(tk, 0.9), pct(tc, 0.1), pct(tc, 0.5), pct(tc, 0.9)))


if __name__ == "__main__":
    main()
