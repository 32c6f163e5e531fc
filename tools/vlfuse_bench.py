#!/usr/bin/env python
"""Early vision-language fusion: the fused HIP core (include/biattn_hip.h) against the PyTorch composition, on one GPU.

    python tools/vlfuse_bench.py [--out profiles/r08_vlfuse.txt] [--rounds 7] [--iters 5] [--no-trace]
    python tools/vlfuse_bench.py --kernels          # a few fused-core calls only (the child of the rocprofv3 run)
    python tools/vlfuse_bench.py --train [--out profiles/r36_vlfuse_train.txt]      # the training leg, see below
    python tools/vlfuse_bench.py --train-dropout [--out profiles/r37_vlfuse_dropout.txt]   # ... with the shipped dropout active

Times (HIP events, after warm-up, the two routes ALTERNATING round by round in one process) at bs 2, S = 22223, 8 heads x 256,
T = 256 and T = 16:
  core     ext.bi_attention_forward against BiMultiHeadAttention._core_torch on the same projections
  VLFuse   the whole VLFuse.forward with BiMultiHeadAttention.fused_core True against False
and reports the median, min and max over the rounds (the spread), FLOP/s of the core from the shape formula (three products
of 2 * B * H * S * T * D; the fused text side recomputes the scores, which is NOT counted), the share of the 157.3 TFLOP/s fp32
matrix peak, torch.cuda.max_memory_allocated of both routes, and a `rocprofv3 --kernel-trace --stats` summary of a separate
run of `--kernels` (skipped with --no-trace or when rocprofv3 is not installed).

--train: forward + backward under autograd at the same shapes, the own route (BiMultiHeadAttention.own_training: HIP training
forward and recomputing backward) and the PyTorch composition ALTERNATING round by round, in eval() (the shipped dropout 0.1 is
inactive there on both routes; active dropout selects the composition on both):
  attn     BiMultiHeadAttention on the normalised inputs, gradients to both inputs and all parameters
  VLFuse   the whole VLFuse.forward under its checkpoint(..., use_reentrant=False), the same gradients
and reports the median and the 10th - 90th percentile of the rounds, and the peak memory ABOVE what was allocated before the
call (inputs and parameters): torch.cuda.max_memory_allocated - memory_allocated.

--train-dropout: the same two legs in train() at the shipped dropout 0.1, which is what a stock training run has: the own route
with the dropout inside the kernels (own_training and own_dropout: biattn_hip_train_dropout_f32 /
biattn_hip_backward_dropout_f32) against the composition with F.dropout, and next to them the own route in eval() -- dropout
inactive, the kernels without the generator -- so that the generator's cost is visible.  The three ALTERNATE round by round; the
same report.
"""
import argparse
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
from types import SimpleNamespace as NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_TFLOPS = 157.3
B, H, S, D = 2, 8, 22223, 256


def cfg():
    fuse = NS(STABLE_SOFTMAX_2D=False, CLAMP_MIN_FOR_UNDERFLOW=True, CLAMP_MAX_FOR_OVERFLOW=True)
    return NS(MODEL=NS(VL_FUSION_USE_CHECKPOINT=True,
                       LANGUAGE_BACKBONE=NS(MODEL_TYPE="bert-base-uncased", MAX_QUERY_LEN=256, N_LAYERS=1, LANG_DIM=768),
                       DDETRS=NS(HIDDEN_DIM=256, VL_HIDDEN_DIM=H * D, ENC_LAYERS=6), DYHEAD=NS(FUSE_CONFIG=fuse)))


def make(T, dev):
    from uninext_amd.modules import VLFuse
    torch.manual_seed(T)
    m = VLFuse(cfg()).to(dev).eval()
    v = torch.randn(B, S, 256, device=dev)
    l = torch.randn(B, T, 768, device=dev)
    mask = torch.ones(B, T, dtype=torch.int64, device=dev)
    mask[:, T - T // 4:] = 0
    return m, v, l, mask


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated()


def stats(xs):
    return "median %8.3f  min %8.3f  max %8.3f ms" % (statistics.median(xs), min(xs), max(xs))


def bench(T, rounds, iters, dev, out):
    from uninext_amd import ext
    from uninext_amd.modules import BiMultiHeadAttention
    m, v, l, mask = make(T, dev)
    a = m.b_attn.attn
    with torch.no_grad():
        nv, nl = m.b_attn.layer_norm_v(v), m.b_attn.layer_norm_l(l)
        q, k, vv, vl = a.v_proj(nv), a.l_proj(nl), a.values_v_proj(nv), a.values_l_proj(nl)

        def whole(route):
            BiMultiHeadAttention.fused_core = route
            return m({"visual": v, "lang": {"hidden": l, "masks": mask}})
        routes = {
            "core   fused  ": lambda: ext.bi_attention_forward(q, k, vv, vl, mask, H, a.scale),
            "core   PyTorch": lambda: a._core_torch(q * a.scale, k, vv, vl, mask),
            "VLFuse fused  ": lambda: whole(True),
            "VLFuse PyTorch": lambda: whole(False),
        }
        for fn in routes.values():          # warm-up: allocator, kernels, BLAS plans
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {n: [] for n in routes}
        for _ in range(rounds):              # alternating
            for n, fn in routes.items():
                times[n].append(timed(fn, iters))
        peaks = {n: peak_of(fn) for n, fn in routes.items()}
    flop = 3 * 2.0 * B * H * S * T * D
    out.append("T = %d   (bs %d, S %d, %d heads x %d; %d rounds x %d calls, alternating)" % (T, B, S, H, D, rounds, iters))
    for n in routes:
        line = "  %s  %s   max_memory_allocated %8.1f MB" % (n, stats(times[n]), peaks[n] / 1e6)
        if n.startswith("core"):
            tf = flop / (statistics.median(times[n]) * 1e-3) / 1e12
            line += "   %6.1f TFLOP/s = %4.1f %% of the fp32 matrix peak" % (tf, 100 * tf / PEAK_TFLOPS)
        out.append(line)
    f, p = times["core   fused  "], times["core   PyTorch"]
    spread = max(max(f) - min(f), max(p) - min(p))
    faster = statistics.median(p) - statistics.median(f)
    out.append("  core: PyTorch - fused = %+.3f ms (medians), spread of the rounds %.3f ms -> fused %s" % (
        faster, spread, "faster by more than the spread" if faster > spread else "NOT faster by more than the spread"))
    out.append("")
    return faster > spread


def pct(xs, q):
    xs = sorted(xs)
    pos = q * (len(xs) - 1)
    lo = int(pos)
    hi = min(lo + 1, len(xs) - 1)
    return xs[lo] + (xs[hi] - xs[lo]) * (pos - lo)


def peak_above(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def bench_train(T, rounds, iters, dev, out):
    m, v, l, mask = make(T, dev)
    a = m.b_attn.attn
    v.requires_grad_()
    l.requires_grad_()
    with torch.no_grad():
        nv0, nl0 = m.b_attn.layer_norm_v(v), m.b_attn.layer_norm_l(l)
    nv, nl = nv0.detach().requires_grad_(), nl0.detach().requires_grad_()
    g = torch.Generator(device=dev).manual_seed(T)
    gv, gl = torch.randn(v.shape, device=dev, generator=g), torch.randn(l.shape, device=dev, generator=g)

    def clear():
        m.zero_grad(set_to_none=True)
        for t in (v, l, nv, nl):
            t.grad = None

    def attn(route):
        a.own_training = route
        clear()
        ov, ol = a(nv, nl, attention_mask_l=mask)
        torch.autograd.backward([ov, ol], [gv, gl])

    def whole(route):
        a.own_training = route
        clear()
        y = m({"visual": v, "lang": {"hidden": l, "masks": mask}})
        torch.autograd.backward([y["visual"], y["lang"]["hidden"]], [gv, gl])

    routes = {
        "attn   own    ": lambda: attn(True),
        "attn   PyTorch": lambda: attn(False),
        "VLFuse own    ": lambda: whole(True),
        "VLFuse PyTorch": lambda: whole(False),
    }
    for fn in routes.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in routes}
    for _ in range(rounds):                  # alternating
        for n, fn in routes.items():
            times[n].append(timed(fn, iters))
    clear()
    peaks = {n: peak_above(fn) for n, fn in routes.items()}
    clear()
    a.own_training = False
    out.append("T = %d   forward + backward (bs %d, S %d, %d heads x %d; %d rounds x %d calls, alternating, eval())" % (
        T, B, S, H, D, rounds, iters))
    for n in routes:
        out.append("  %s  median %8.3f  p10 %8.3f  p90 %8.3f ms   peak above the inputs %9.1f MB" % (
            n, statistics.median(times[n]), pct(times[n], 0.1), pct(times[n], 0.9), peaks[n] / 1e6))
    verdict = True
    for kind in ("attn  ", "VLFuse"):
        o, p = times[kind + " own    "], times[kind + " PyTorch"]
        spread = max(pct(o, 0.9) - pct(o, 0.1), pct(p, 0.9) - pct(p, 0.1))
        faster = statistics.median(p) - statistics.median(o)
        ok = faster > spread
        verdict = verdict and ok
        out.append("  %s: PyTorch - own = %+.3f ms (medians), spread of the rounds (p90 - p10) %.3f ms -> own route %s" % (
            kind.strip(), faster, spread, "faster by more than the spread" if ok else "NOT faster by more than the spread"))
    out.append("")
    return verdict


def bench_train_dropout(T, rounds, iters, dev, out):
    m, v, l, mask = make(T, dev)
    a = m.b_attn.attn
    assert a.dropout == 0.1
    v.requires_grad_()
    l.requires_grad_()
    with torch.no_grad():
        nv0, nl0 = m.b_attn.layer_norm_v(v), m.b_attn.layer_norm_l(l)
    nv, nl = nv0.detach().requires_grad_(), nl0.detach().requires_grad_()
    g = torch.Generator(device=dev).manual_seed(T)
    gv, gl = torch.randn(v.shape, device=dev, generator=g), torch.randn(l.shape, device=dev, generator=g)
    # route -> (train mode, own_training, own_dropout)
    modes = {"own  dropout 0.1": (True, True, True), "PyTorch dropout 0.1": (True, False, False), "own  dropout off": (False, True, False)}

    def step(mode, whole):
        m.train(modes[mode][0])
        a.own_training, a.own_dropout = modes[mode][1:]
        m.zero_grad(set_to_none=True)
        for t in (v, l, nv, nl):
            t.grad = None
        if whole:
            y = m({"visual": v, "lang": {"hidden": l, "masks": mask}})
            torch.autograd.backward([y["visual"], y["lang"]["hidden"]], [gv, gl])
        else:
            ov, ol = a(nv, nl, attention_mask_l=mask)
            torch.autograd.backward([ov, ol], [gv, gl])

    routes = {"%s %-19s" % (kind, mode): (lambda mode=mode, whole=whole: step(mode, whole))
              for kind, whole in (("attn  ", False), ("VLFuse", True)) for mode in modes}
    for fn in routes.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in routes}
    for _ in range(rounds):                  # alternating
        for n, fn in routes.items():
            times[n].append(timed(fn, iters))
    peaks = {n: peak_above(fn) for n, fn in routes.items()}
    m.eval()
    a.own_training = a.own_dropout = False
    out.append("T = %d   forward + backward (bs %d, S %d, %d heads x %d; %d rounds x %d calls, alternating)" % (
        T, B, S, H, D, rounds, iters))
    for n in routes:
        out.append("  %s  median %8.3f  p10 %8.3f  p90 %8.3f ms   peak above the inputs %9.1f MB" % (
            n, statistics.median(times[n]), pct(times[n], 0.1), pct(times[n], 0.9), peaks[n] / 1e6))
    for kind in ("attn  ", "VLFuse"):
        o, p = times["%s %-19s" % (kind, "own  dropout 0.1")], times["%s %-19s" % (kind, "PyTorch dropout 0.1")]
        z = times["%s %-19s" % (kind, "own  dropout off")]
        apart = pct(o, 0.9) < pct(p, 0.1) or pct(p, 0.9) < pct(o, 0.1)
        out.append("  %s: PyTorch - own at dropout 0.1 = %+.3f ms (medians), the p10 - p90 ranges are %s; the generator costs "
                   "the own route %+.3f ms" % (kind.strip(), statistics.median(p) - statistics.median(o),
                                               "apart" if apart else "NOT apart", statistics.median(o) - statistics.median(z)))
    out.append("")


def kernels_only(dev):
    from uninext_amd import ext
    for T in (256, 16):
        m, v, l, mask = make(T, dev)
        a = m.b_attn.attn
        with torch.no_grad():
            q, k, vv, vl = a.v_proj(v), a.l_proj(l), a.values_v_proj(v), a.values_l_proj(l)
            for _ in range(5):
                ext.bi_attention_forward(q, k, vv, vl, mask, H, a.scale)
        torch.cuda.synchronize()


def trace(out):
    if shutil.which("rocprofv3") is None:
        out.append("rocprofv3 --kernel-trace --stats: rocprofv3 not found, skipped")
        return
    d = tempfile.mkdtemp(prefix="vlfuse_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--kernels"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    dbs = sorted(glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True), key=os.path.getmtime)
    out.append("rocprofv3 --kernel-trace --stats -- python tools/vlfuse_bench.py --kernels   (5 calls at T = 256, 5 at T = 16; "
               "grid.y of biattn_text tells them apart: 2 and 1)")
    if r.returncode != 0 or not dbs:
        out.append("  failed (exit %d): %s" % (r.returncode, (r.stderr or "")[-300:]))
        return
    s = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rocprof_summary.py"), "trace", dbs[-1]], capture_output=True,
                       text=True, timeout=120)
    out.extend(l for l in s.stdout.splitlines() if "biattn" in l or l.startswith("kernel"))
    shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_vlfuse.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--train-dropout", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    if args.kernels:
        return kernels_only(dev)
    if args.train_dropout:
        out = ["tools/vlfuse_bench.py --train-dropout on %s" % torch.cuda.get_device_name(0), ""]
        for T in (256, 16):
            bench_train_dropout(T, args.rounds, args.iters, dev, out)
        out.append("own_dropout stays opt-in whatever the numbers: its keep masks are not F.dropout's.")
        text = "\n".join(out) + "\n"
        print(text)
        path = args.out if args.out != ap.get_default("out") else os.path.join(ROOT, "profiles", "r37_vlfuse_dropout.txt")
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
        return
    if args.train:
        out = ["tools/vlfuse_bench.py --train on %s" % torch.cuda.get_device_name(0), ""]
        both = [bench_train(T, args.rounds, args.iters, dev, out) for T in (256, 16)]
        out.append("own_training default by the rule 'faster at both T by more than the spread': %s" % all(both))
        text = "\n".join(out) + "\n"
        print(text)
        path = args.out if args.out != ap.get_default("out") else os.path.join(ROOT, "profiles", "r36_vlfuse_train.txt")
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
        return
    out = ["tools/vlfuse_bench.py on %s" % torch.cuda.get_device_name(0), ""]
    both = [bench(T, args.rounds, args.iters, dev, out) for T in (256, 16)]
    out.append("fused_core default by the rule 'faster at both T by more than the spread': %s" % all(both))
    out.append("")
    if not args.no_trace:
        trace(out)
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
