#!/usr/bin/env python
"""Backward of the patch-embedding convolutions at the bench shapes (tools/patch_embed_bench.py SHAPES; GPU box only):
patch_embed_hip_backward_f32 (include/patch_embed_hip.h, the opt-in training route) vs PyTorch-ROCm's convolution backward
(MIOpen), which the default training route runs.

    python tools/patch_embed_train_bench.py [--reps 20]
    python tools/patch_embed_train_bench.py --own-only     # only the opt-in route under autograd, e.g. under
                                                           # rocprofv3 --kernel-trace --stats: no MIOpen / rocBLAS kernel

Per shape: own grad-weight + grad-bias, grad-bias alone and grad-input (layers whose input needs a gradient: the ConvNeXt
downsample convolutions) as launch time (HIP events), TFLOP/s and fraction of the 157.3 TFLOP/s dense fp32 matrix peak;
aten.convolution_backward for the same gradients (grad_out as autograd hands it over: the permuted view for ViT); the first
call on a new image size for both routes (wall clock, synchronised, making the inputs on the host included; MIOpen searches its
solvers per shape); and whether two
calls of the own route are bitwise equal.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from uninext_amd import ext  # noqa: E402
from patch_embed_bench import PEAK_TF, SHAPES, timeit  # noqa: E402


def inputs(B, C, H, W, E, k, cl, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g).to(dev)
    w = (torch.randn(E, C, k, k, generator=g) / (C * k * k) ** 0.5).to(dev)
    go = torch.randn((B, H // k, W // k, E) if cl else (B, E, H // k, W // k), generator=g).to(dev)
    return x, w, go


def torch_bwd(x, w, go, k, cl, mask):
    g = go.permute(0, 3, 1, 2) if cl else go        # what autograd passes to ConvolutionBackward0 after the permute
    return torch.ops.aten.convolution_backward(g, x, w, [w.shape[0]], [k, k], [0, 0], [1, 1], False, [0, 0], 1, mask)


def own_bwd(x, w, go, cl, need_input, need_weight, need_bias):
    return ext.patch_embed_backward(x, w, go, cl, need_input=need_input, need_weight=need_weight, need_bias=need_bias)


def first_call(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def own_route_only(dev, reps):
    """Forward + backward of every bench shape through PatchEmbed / patch_conv2d with the opt-in training route."""
    from uninext_amd.backbone import PatchEmbed, patch_conv2d
    for name, B, C, H, W, E, k, cl in SHAPES:
        x, w, go = inputs(B, C, H, W, E, k, cl, dev)
        x.requires_grad_(C > 3)
        if cl:
            layer = PatchEmbed(kernel_size=(k, k), stride=(k, k), in_chans=C, embed_dim=E).to(dev)
            layer.own_exact_training = True
            run = lambda: layer(x)
        else:
            layer = torch.nn.Conv2d(C, E, kernel_size=k, stride=k).to(dev)
            run = lambda: patch_conv2d(x, layer, own_training=True)
        for _ in range(reps):
            out = run()
            assert type(out.grad_fn).__name__ == "PatchEmbedFunctionBackward", name
            out.backward(go)
        torch.cuda.synchronize()
        print("own route fwd + bwd x%d: %s" % (reps, name))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--own-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cudnn.allow_tf32 = False
    if args.own_only:
        own_route_only(dev, 3)
        return
    print("%-46s %7s %5s %5s | %-38s | %-38s | %-26s | %s" % ("shape", "M", "E", "K", "own gW+gb", "own gX", "MIOpen gW+gb / gX",
                                                             "first call own / MIOpen"))
    for name, B, C, H, W, E, k, cl in SHAPES:
        x, w, go = inputs(B, C, H, W, E, k, cl, dev)
        M, K = B * (H // k) * (W // k), C * k * k
        flop = 2.0 * M * E * K
        want_x = C > 3                                   # the image itself needs no gradient
        with torch.no_grad():
            # first calls on a size this process has not seen (each route on its own new size)
            t_first_own = first_call(lambda: own_bwd(*inputs(B, C, H + k, W + k, E, k, cl, dev)[:3], cl, want_x, True, True))
            t_first_torch = first_call(lambda: torch_bwd(*inputs(B, C, H + 2 * k, W + 2 * k, E, k, cl, dev), k, cl,
                                                         [want_x, True, True]))
            t_wb = timeit(lambda: own_bwd(x, w, go, cl, False, True, True), args.reps)
            t_b = timeit(lambda: own_bwd(x, w, go, cl, False, False, True), args.reps)
            t_x = timeit(lambda: own_bwd(x, w, go, cl, True, False, False), args.reps) if want_x else float("nan")
            t_twb = timeit(lambda: torch_bwd(x, w, go, k, cl, [False, True, True]), args.reps)
            t_tx = timeit(lambda: torch_bwd(x, w, go, k, cl, [True, False, False]), args.reps) if want_x else float("nan")
            a = own_bwd(x, w, go, cl, want_x, True, True)
            b = own_bwd(x, w, go, cl, want_x, True, True)
            same = all(torch.equal(u, v) for u, v in zip(a, b) if u is not None)
            ref = torch_bwd(x, w, go, k, cl, [want_x, True, True])
            err = max(float((u - v).abs().max()) / float(v.abs().max()) for u, v in zip(a, ref) if u is not None)
        tf = lambda t: flop / t * 1e-6
        sx = ("%7.1f us %5.1f TF/s = %4.1f %%" % (t_x, tf(t_x), 100 * tf(t_x) / PEAK_TF)) if want_x else "(image: no grad-input)"
        print("%-46s %7d %5d %5d | %7.1f us %5.1f TF/s = %4.1f %% (gb %5.1f) | %-38s | %7.1f / %7.1f us    | %6.1f / %7.1f ms"
              "  bitwise-repeat %s  max rel err vs MIOpen %.1e"
              % (name, M, E, K, t_wb, tf(t_wb), 100 * tf(t_wb) / PEAK_TF, t_b, sx, t_twb, t_tx, t_first_own, t_first_torch,
                 "yes" if same else "NO", err))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
