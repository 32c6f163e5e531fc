#!/usr/bin/env python
"""Static mask head TRAINING step (MaskHeadSmallConv forward + backward) at the training shapes (bs 2, padded 800 x 1344: stride
8 / 16 / 32 maps 100 x 168, 50 x 84, 25 x 42; 256 hidden channels) on the own exact route (MaskHeadSmallConv.own_exact_training:
conv3x3_hip_packed_exact_f32 forward, conv3x3_hip_backward_exact_f32 backward) and on the PyTorch-ROCm / MIOpen route (GPU box only).

    python tools/maskhead_train_bench.py [--reps 20]        # per-layer backward parts, head fwd + bwd, first calls on new sizes
    python tools/maskhead_train_bench.py --trace-only own   # a few head steps on one route only (for rocprofv3 --kernel-trace)
"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uninext_amd import ext  # noqa: E402
from uninext_amd.mask_head import MaskHeadSmallConv  # noqa: E402

PEAK_TF = 157.3
B = 2
LAYERS = [("lay3", 256, 256, 25, 42), ("lay4", 256, 256, 50, 84), ("jia_dcn", 256, 256, 100, 168),
          ("lay1", 256, 64, 100, 168), ("lay2", 64, 8, 100, 168)]
MAPS = ((100, 168), (50, 84), (25, 42))
# three padded image sizes of the MIN_SIZE_TRAIN range (short side 512 / 608 / 704, aspect 1333 / 800) that no earlier call used
NEW_SIZES = ((512, 864), (608, 1024), (704, 1184))


def timeit(fn, reps):
    """Mean time per call in us over `reps` calls between two HIP events (after 3 warm-up calls)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def median_us(fn, reps):
    """Median over `reps` single calls, each between its own pair of HIP events (after 3 warm-up calls)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def head_inputs(dev, maps, gen):
    return [torch.randn(B, 256, h, w, generator=gen).to(dev).requires_grad_(True) for h, w in maps]


def head_step(head, xs, grad_out):
    head.zero_grad(set_to_none=True)
    out = head(xs, None)
    out.backward(grad_out)
    return out


def per_layer(dev, reps):
    print("== per layer, bs 2: backward parts (HIP events, mean of %d) ==" % reps)
    gen = torch.Generator().manual_seed(1)
    tot_own = tot_lib = 0.0
    for name, cin, cout, H, W in LAYERS:
        conv = torch.nn.Conv2d(cin, cout, 3, padding=1).to(dev)
        x = torch.randn(B, cin, H, W, generator=gen).to(dev)
        go = torch.randn(B, cout, H, W, generator=gen).to(dev)
        w = conv.weight.detach()
        with torch.no_grad():
            out = F.relu(conv(x))
        flop = 2.0 * B * H * W * cout * cin * 9
        pd = ext.conv3x3_pack_weight_dgrad(w)
        cp = (cout + 15) // 16 * 16
        g = torch.zeros(B, cp, H, W, device=dev)
        g[:, :cout] = go * (out > 0)
        t_rb = timeit(lambda: ext.conv3x3_backward(x, None, out, go, cout, need_input=False, need_weight=False), reps)
        t_din = timeit(lambda: ext.conv3x3_packed_forward(g, pd, cin, None, relu=False, exact=True), reps)
        t_wonly = timeit(lambda: ext.conv3x3_backward(x, None, out, go, cout, need_input=False, need_bias=False), reps)
        t_all = timeit(lambda: ext.conv3x3_backward(x, pd, out, go, cout), reps)
        # MIOpen route: threshold_backward, then the convolution backward for the input and for weight + bias
        conv_bwd = torch.ops.aten.convolution_backward
        args = ([1, 1], [1, 1], [1, 1], False, [0, 0], 1)
        t_lrelu = timeit(lambda: torch.ops.aten.threshold_backward(go, out, 0), reps)
        gm = torch.ops.aten.threshold_backward(go, out, 0)
        t_lin = timeit(lambda: conv_bwd(gm, x, w, [cout], *args, [True, False, False]), reps)
        t_lw = timeit(lambda: conv_bwd(gm, x, w, [cout], *args, [False, True, True]), reps)
        t_lall = timeit(lambda: conv_bwd(torch.ops.aten.threshold_backward(go, out, 0), x, w, [cout], *args, [True, True, True]), reps)
        tot_own += t_all
        tot_lib += t_lall
        print("%-8s %3d->%3d @ %3dx%3d %5.1f GFLOP/pass | own: relu+bias %6.1f  grad-input %6.1f us (%4.1f %%)  grad-weight(+relu pass) %6.1f us "
              "(%4.1f %%)  all %6.1f us | MIOpen: relu %6.1f  grad-input %6.1f  grad-weight+bias %6.1f  all %6.1f us"
              % (name, cin, cout, H, W, flop * 1e-9, t_rb, t_din, 100 * flop / t_din * 1e-6 / PEAK_TF, t_wonly,
                 100 * flop / t_wonly * 1e-6 / PEAK_TF, t_all, t_lrelu, t_lin, t_lw, t_lall))
    print("five layers' backward: own %.1f us, MIOpen %.1f us" % (tot_own, tot_lib))


def module(dev, reps):
    print("== MaskHeadSmallConv forward + backward, bs 2, median of %d (HIP events) ==" % reps)
    gen = torch.Generator().manual_seed(2)
    head = MaskHeadSmallConv(256, None, 256).to(dev)
    xs = head_inputs(dev, MAPS, gen)
    grad_out = torch.randn(B, 8, *MAPS[0], generator=gen).to(dev)
    res = {}
    for route in ("own", "miopen"):
        head.own_exact_training = route == "own"
        res[route] = median_us(lambda: head_step(head, xs, grad_out), reps)
        print("%-6s route: median %.1f us (min %.1f, max %.1f)" % ((route,) + res[route]))
    head.own_exact_training = True
    head_step(head, xs, grad_out)
    g_own = [p.grad.clone() for p in head.parameters()]
    head.own_exact_training = False
    head_step(head, xs, grad_out)
    err = max(float((a - p.grad).abs().max()) / max(1e-30, float(p.grad.abs().max())) for a, p in zip(g_own, head.parameters()))
    print("own / MIOpen: %.3f; largest parameter-gradient difference %.1e of its scale" % (res["own"][0] / res["miopen"][0], err))


def first_calls(dev):
    print("== first call of a head step on a previously unseen size (wall clock, synchronised) ==")
    gen = torch.Generator().manual_seed(3)
    head = MaskHeadSmallConv(256, None, 256).to(dev)
    for route in ("own", "miopen"):
        head.own_exact_training = route == "own"
        for (h, w) in NEW_SIZES:
            maps = ((h // 8, w // 8), (h // 16, w // 16), (h // 32, w // 32))
            xs = head_inputs(dev, maps, gen)
            grad_out = torch.randn(B, 8, *maps[0], generator=gen).to(dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            head_step(head, xs, grad_out)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            head_step(head, xs, grad_out)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            print("%-6s %4d x %4d (maps %s): first call %8.1f ms, second %6.2f ms" % (route, h, w, maps, (t1 - t0) * 1e3, (t2 - t1) * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace-only", choices=("own", "miopen"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.trace_only:
        gen = torch.Generator().manual_seed(2)
        head = MaskHeadSmallConv(256, None, 256).to(dev)
        head.own_exact_training = args.trace_only == "own"
        xs = head_inputs(dev, MAPS, gen)
        grad_out = torch.randn(B, 8, *MAPS[0], generator=gen).to(dev)
        for _ in range(5):
            head_step(head, xs, grad_out)
        torch.cuda.synchronize()
        print("traced 5 head steps on the %s route" % args.trace_only)
        return
    first_calls(dev)     # first: nothing has seen these sizes yet
    per_layer(dev, args.reps)
    module(dev, max(args.reps, 20))


if __name__ == "__main__":
    main()
