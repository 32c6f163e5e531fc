#!/usr/bin/env python
"""A/B of the two-stage query selection (uninext_amd/modules/query_selection.py: TwoStageQuerySelection.fused) against the same
object with fused = False, i.e. the reference's composition of PyTorch ops, on one GPU, alternating in one process with rotating
inputs: bs 2, d_model 256, the R50 800 x 1333 memory (S = 22 223), 900 proposals.

    python tools/query_selection_bench.py [--iters 30] [--warmup 10]

Rows: both class heads (VL_Align with one pooled 768-wide text token, Still_Classifier), without padding and with the second
image padded to 3/4 of the width and 2/3 of the height.  Medians and spreads (p10..p90) of per-call event times; "faster" means
the medians differ by more than the larger of the two spreads.  Peak memory is what a call allocates at its worst above what is
live before it (inputs, parameters) -- so it counts the outputs it returns on both routes alike."""
import argparse
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uninext_amd.modules import MLP, Still_Classifier, TwoStageQuerySelection, VL_Align   # noqa: E402

ROTATE = 3
LEVELS = [(100, 167), (50, 84), (25, 42), (13, 21)]
TOPK = 900


def cfg():
    ns = types.SimpleNamespace
    return ns(MODEL=ns(DYHEAD=ns(PRIOR_PROB=0.01, LOG_SCALE=0.0, FUSE_CONFIG=ns(CLAMP_DOT_PRODUCT=True)),
                       LANGUAGE_BACKBONE=ns(LANG_DIM=768), DDETRS=ns(HIDDEN_DIM=256)))


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


def peak_above_live(fn, x):
    torch.cuda.synchronize()
    live = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn(x)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - live
    del out
    return peak / 2 ** 20


def padded_mask(B, dev, pad):
    parts = []
    for H, W in LEVELS:
        m = torch.zeros(B, H, W, dtype=torch.bool, device=dev)
        if pad:
            m[1, (2 * H + 2) // 3:, :] = True
            m[1, :, (3 * W + 3) // 4:] = True
        parts.append(m.flatten(1))
    return torch.cat(parts, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    print(torch.cuda.get_device_name(0), "torch", torch.__version__)
    B, E = 2, 256
    S = sum(h * w for h, w in LEVELS)
    print("bs %d, d_model %d, S %d, %d proposals; scoring grid %d workgroups, box grid %d" % (
        B, E, S, TOPK, (B * S + 31) // 32, (B * TOPK + 31) // 32))
    shapes = torch.as_tensor(LEVELS, dtype=torch.long, device=dev)
    enc_output, norm = torch.nn.Linear(E, E).to(dev).eval(), torch.nn.LayerNorm(E).to(dev).eval()
    bbox = MLP(E, E, 4, 3).to(dev).eval()
    heads = {"VL_Align": VL_Align(cfg()).to(dev).eval(), "Still_Classifier": Still_Classifier(E).to(dev).eval()}
    xs = [dict(memory=torch.randn(B, S, E, device=dev), pool=torch.randn(B, 768, device=dev)) for _ in range(ROTATE)]
    all_faster = True
    for head_name, head in heads.items():
        for pad in (False, True):
            mask = padded_mask(B, dev, pad)

            def route(fused):
                sel = TwoStageQuerySelection()
                sel.fused = fused

                def call(x):
                    with torch.no_grad():
                        return sel(x["memory"], mask, shapes, enc_output, norm, head, bbox, x["pool"], TOPK)
                return call

            fused, torch_ = route(True), route(False)
            a, b = fused(xs[0]), torch_(xs[0])
            same = float((a[2] == b[2]).float().mean())
            fin = torch.isfinite(b[1])
            agree = a[2] == b[2]
            diff = float((a[1] - b[1])[fin & agree.unsqueeze(-1)].abs().max()) if bool((fin & agree.unsqueeze(-1)).any()) else 0.0
            (tf, sf), (tt, st) = [stats(t) for t in timed([fused, torch_], xs, args.iters, args.warmup)]
            verdict = "fused faster" if tt - tf > max(sf, st) else ("torch faster" if tf - tt > max(sf, st) else "within spread")
            all_faster &= verdict == "fused faster"
            print("  %-16s %-10s fused %8.3f ms (spread %.3f, peak %7.1f MiB)   torch %8.3f ms (spread %.3f, peak %7.1f MiB)   x%.2f  %s"
                  % (head_name, "padded" if pad else "unpadded", tf, sf, peak_above_live(fused, xs[1]), tt, st,
                     peak_above_live(torch_, xs[1]), tt / tf, verdict), flush=True)
            print("      logit max abs difference %.2e; same top-k index in %.1f %% of the places, box difference there %.2e"
                  % (float((a[3] - b[3]).abs().max()), 100 * same, diff), flush=True)
    print("fused faster in every row: %s" % ("yes" if all_faster else "no"))


if __name__ == "__main__":
    main()
