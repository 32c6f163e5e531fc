#!/usr/bin/env python
"""A/B of the ConvNeXt block's fused route against the PyTorch composition OF THE SAME MODULE, at the four ConvNeXt-L stage shapes
(800 x 1344 image, batch 2):

    python tools/convnext_bench.py [--repeats 5] [--iters 20] [--warmup 5] [--stages 0,1,2,3] [--once | --train]

Per stage: the block's head (depthwise 7x7 + permute + LayerNorm), its tail (layer scale + permute + residual), the whole block
(head, the two Linears and the GELU, tail) and the channels-first LayerNorm.  The two routes alternate in one process,
`--repeats` times; a figure is the median over the repeats of the mean over `--iters` launches between two device events, the
spread is min .. max over the repeats.  Next to the fused time stands the algorithmic traffic over it: 8 B C H W bytes for the
head and the LayerNorm (one read, one write), 12 B C H W for the tail (two reads, one write).  --once: one fused pass per
stage and nothing else (for a kernel trace).  --train: forward + backward of one Block (drop path 0 and 0.7, training mode) and of
a channels-first LayerNorm with own_training on against off -- the same module, the same seed: the median over the repeats with
their 10th .. 90th percentile, and the peak of allocated memory above the inputs during one step."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uninext_amd import ext                                          # noqa: E402
from uninext_amd.backbone import Block, LayerNorm                    # noqa: E402

STAGES = [(192, 200, 336), (384, 100, 168), (768, 50, 84), (1536, 25, 42)]
BATCH = 2


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1000.0 / iters        # microseconds


def ab(fused, composed, args):
    a, b = [], []
    for _ in range(args.repeats):
        a.append(timed(fused, args.iters, args.warmup))
        b.append(timed(composed, args.iters, args.warmup))
    return a, b


def report(what, a, b, nbytes=None):
    ma, mb = statistics.median(a), statistics.median(b)
    verdict = "faster" if max(a) < min(b) else ("slower" if min(a) > max(b) else "inside the spread")
    line = "  %-14s fused %8.1f us (%7.1f .. %7.1f)   PyTorch %8.1f us (%7.1f .. %7.1f)   x%5.2f  %s" % (
        what, ma, min(a), max(a), mb, min(b), max(b), mb / ma, verdict)
    if nbytes is not None:
        line += "   %6.1f MB -> %5.2f TB/s" % (nbytes / 1e6, nbytes / ma / 1e6)
    print(line, flush=True)


def p10_p90(v):
    """The 10th and the 90th percentile of the repeats (linear interpolation between the sorted values)."""
    q = statistics.quantiles(v, n=10, method="inclusive") if len(v) > 1 else [v[0]] * 9
    return q[0], q[8]


def train_leg(args, dev):
    """own_training on against off: one training step (forward + backward, every parameter and the input with a gradient)."""
    for s in (int(k) for k in args.stages.split(",")):
        C, H, W = STAGES[s]
        print("stage %d: C %d, %d x %d" % (s + 1, C, H, W), flush=True)
        x = torch.randn(BATCH, C, H, W, device=dev, requires_grad=True)
        grad = torch.randn(BATCH, C, H, W, device=dev)
        modules = [("block dp 0", Block(C, layer_scale_init_value=1.0)), ("block dp 0.7", Block(C, drop_path=0.7, layer_scale_init_value=1.0)),
                   ("layernorm_cf", LayerNorm(C, data_format="channels_first"))]
        for what, m in modules:
            m = m.to(dev).train()

            def step(flag, m=m):
                def run():
                    m.own_training = flag
                    torch.manual_seed(1)
                    x.grad = None
                    m.zero_grad(set_to_none=True)
                    m(x).backward(grad)
                return run

            def peak(run):
                run()
                torch.cuda.synchronize()
                x.grad = None
                m.zero_grad(set_to_none=True)
                base = torch.cuda.memory_allocated(dev)
                torch.cuda.reset_peak_memory_stats(dev)
                run()
                torch.cuda.synchronize()
                return (torch.cuda.max_memory_allocated(dev) - base) / 1e6
            a, b = ab(step(True), step(False), args)
            ma, mb = statistics.median(a), statistics.median(b)
            (a10, a90), (b10, b90) = p10_p90(a), p10_p90(b)
            verdict = "faster" if a90 < b10 else ("slower" if a10 > b90 else "inside the spread")
            print("  %-14s own %8.1f us (%7.1f .. %7.1f)   PyTorch %8.1f us (%7.1f .. %7.1f)   x%5.2f  %-17s peak above inputs: own %7.1f MB, PyTorch %7.1f MB" % (
                what, ma, a10, a90, mb, b10, b90, mb / ma, verdict, peak(step(True)), peak(step(False))), flush=True)
            del m
        del x, grad
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--stages", default="0,1,2,3")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--train", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    defaults = Block.fused, LayerNorm.fused
    torch.manual_seed(0)
    print("ConvNeXt-L stage shapes, batch %d, fp32; %d repeats x %d launches, routes alternating; %s" % (
        BATCH, args.repeats, args.iters, torch.cuda.get_device_name(0)))
    if args.train:
        return train_leg(args, dev)
    with torch.no_grad():
        for s in (int(k) for k in args.stages.split(",")):
            C, H, W = STAGES[s]
            blk = Block(C, layer_scale_init_value=1.0).to(dev).eval()
            blk.dwconv.weight.mul_(10.0)                    # taps of size 0.2: a convolution output LayerNorm has something to do on
            ln = LayerNorm(C, data_format="channels_first").to(dev).eval()
            x = torch.randn(BATCH, C, H, W, device=dev)
            y = torch.randn(BATCH, H, W, C, device=dev)
            conv, norm, gamma = blk.dwconv, blk.norm, blk.gamma.weight[0]
            nw, nb = norm.weight.weight[0], norm.bias.weight[0]
            elems = BATCH * C * H * W

            def block_route(fused):
                def run():
                    Block.fused = fused
                    return blk(x)
                return run

            def ln_route(fused):
                def run():
                    LayerNorm.fused = fused
                    return ln(x)
                return run
            head = (lambda: ext.convnext_dwconv_ln(x, conv.weight, conv.bias, nw, nb, norm.eps),
                    lambda: F.layer_norm(conv(x).permute(0, 2, 3, 1), (C,), nw, nb, norm.eps))
            tail = (lambda: ext.convnext_scale_residual(y, gamma, x), lambda: x + (gamma * y).permute(0, 3, 1, 2))
            print("stage %d: C %d, %d x %d" % (s + 1, C, H, W), flush=True)
            if args.once:
                head[0](), tail[0](), block_route(True)(), ln_route(True)()
                torch.cuda.synchronize()
                Block.fused, LayerNorm.fused = defaults
                continue
            try:
                report("head", *ab(*head, args), nbytes=8 * elems)
                report("tail", *ab(*tail, args), nbytes=12 * elems)
                report("block", *ab(block_route(True), block_route(False), args))
                report("layernorm_cf", *ab(ln_route(True), ln_route(False), args), nbytes=8 * elems)
            finally:
                Block.fused, LayerNorm.fused = defaults
            del blk, ln, x, y
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
