"""The training kernels of the blocks around the attention operator (include/dynmask_hip.h: dropout_add_layernorm_hip_train_f32,
dropout_add_layernorm_hip_backward_f32, relu_dropout_hip_f32, relu_dropout_hip_backward_f32, row_dropout_hip_keep_u8) for
tests/test_layer_train_cpu.py and tests/test_layer_train_gpu.py: the keep masks with exactly the header's counter layout (numpy
Philox: vlfuse_dropout_cases.philox4x32_10), float64 restatements of both ops, forward and backward, under a given mask, the same
formulas in float32 as the composition, and a per-entry magnitude for parity_measure.entry_bound.  Plain numpy.

Inputs are seeded by the case's name (parity_measure.rng) and dyadic (parity_measure.dy): fp32 holds exactly what float64 sees.
The backward is a function of (grad_out, z, gamma, the mask): its restatement takes the fp32 z it is given as exact.

THE MAGNITUDES, the sum of the absolute summands behind an entry, to first order in u = 2^-24, as tests/convnext_bwd_parity.py
derives them for its LayerNorm backward; nothing was fitted to what a kernel gives.  c = 1 / (1 - p), m the mask.
  z   = residual + c m x                  A = |residual| + c m |x|     (the backward: A = |z|, z is an input there)
  u = mean z, r = 1 / sqrt(mean (z - u)^2 + eps), xh = (z - u) r
      S_xh = r (A + mean A + |z| + |u| + |xh| rms A) + |xh|            the error scale of xh
  out = xh gamma + beta                   |gamma| (S_xh + |xh|) + |beta|
  g = grad_out gamma, m1 = mean g, m2 = mean (g xh), t = g - m1 - xh m2, grad_z = r t
      M2 = mean (|g| (|xh| + S_xh))
      s_gz = r (|g| + mean |g| + |xh| M2 + |m2| S_xh + |t| (1 + r rms A))
  grad_residual: s_gz + |grad_z|          grad_x: c m (s_gz + |grad_z|)   (0 where dropped: no room at all)
  grad_gamma = sum_rows grad_out xh       sum_rows |grad_out| (S_xh + |xh|)
  grad_beta  = sum_rows grad_out          sum_rows |grad_out|
  relu_dropout out = c m max(h, 0): one product, |out|;   its backward grad_h = c grad_out where out > 0: |grad_h|.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_measure as PM                                                 # noqa: E402
import vlfuse_dropout_cases as DC                                           # noqa: E402
from vlfuse_dropout_cases import MASK32, scale_of, seed_of, threshold_of    # noqa: E402,F401

EPS = float(np.float32(1e-5))
LN_OUTPUTS = ("z", "out")
LN_GRADS = ("gx", "gres", "ggamma", "gbeta")

# (rows, features, p, residual given, gamma / beta given): rows at the 4-rows-a-workgroup edge of the forward (1, 3, 4, 5) and
# past one (257) and many (1031) 32-row workgroups of the backward's partial sums; features at the 64-lane x float4 chunk edge
# (252, 256, 260), at every chunk count the kernels are instantiated for (1, 2, 4, 8, 16) and one past a boundary (1028); the
# options rotated so that every feature size sees two row counts and every p.
LN_CASES = [(1, 4, 0.1, True, True), (3, 4, 0.0, False, False), (4, 252, 0.5, True, False), (5, 252, 0.1, False, True),
            (257, 256, 0.1, True, True), (1031, 256, 0.0, True, True), (5, 256, 0.5, False, False), (3, 260, 0.1, True, False),
            (257, 260, 0.5, False, True), (4, 768, 0.0, True, True), (1031, 768, 0.1, True, True), (1, 1024, 0.5, False, True),
            (257, 1024, 0.1, True, False), (5, 1028, 0.0, True, False), (3, 1028, 0.5, True, True), (4, 2048, 0.1, False, True),
            (257, 2048, 0.0, True, True), (1, 4096, 0.1, True, True), (5, 4096, 0.5, True, False), (257, 4096, 0.1, False, False)]
# (rows, features, p): flat float4 streaming; 257 x 8192 and 1031 x 2048 are 2056 workgroups and more
RELU_CASES = [(1, 4, 0.1), (5, 252, 0.5), (257, 256, 0.0), (3, 260, 0.1), (1031, 2048, 0.1), (4, 8192, 0.5), (257, 8192, 0.1),
              (1, 65536, 0.1)]
EXPORT_ROWS, EXPORT_FEATURES, EXPORT_PS = (1, 5, 257), (4, 252, 256, 260, 4096), (0.1, 0.5)


def ln_name(case):
    return "ln/r%d_f%d_p%g_%s_%s" % (case[0], case[1], case[2], "res" if case[3] else "nores", "affine" if case[4] else "plain")


def relu_name(case):
    return "relu/r%d_f%d_p%g" % case


# ------------------------------------------------------------------------------------------------------------------ the masks

def keep_mask(seed, p, rows, features):
    """bool [rows, features] by the header's layout: key = the seed's two halves, counter = (offset low, offset high, row,
    column / 4), word column % 4, keep <=> word >= threshold."""
    assert features % 4 == 0 and rows < 2 ** 32
    sd, off = (int(x) for x in np.asarray(seed).view(np.uint64))
    row, g = np.meshgrid(np.arange(rows, dtype=np.uint64), np.arange(features // 4, dtype=np.uint64), indexing="ij")
    w = DC.philox4x32_10((off & MASK32, off >> 32, row, g), (sd & MASK32, sd >> 32))
    words = np.stack(w, axis=-1).reshape(rows, features)
    return words.astype(np.uint64) >= threshold_of(p)


# ----------------------------------------------------------------------------------------------------------------- the inputs

def ln_inputs(case):
    """x, res, gamma, beta, go as float32 dyadic arrays (None where the case has none) and the seed, from the case's name."""
    rows, f, p, with_res, affine = case
    name = ln_name(case)
    r = lambda what, *shape: PM.rng(name + "/" + what).standard_normal(shape)
    return dict(x=PM.dy(r("x", rows, f)), res=PM.dy(r("res", rows, f), 2.0) + np.float32(0.5) if with_res else None,
                gamma=PM.dy(1.0 + 0.25 * r("gamma", f)) if affine else None, beta=PM.dy(r("beta", f), 0.5) if affine else None,
                go=PM.dy(r("go", rows, f)), seed=seed_of(name), p=p, eps=EPS)


def relu_inputs(case):
    rows, f, p = case
    name = relu_name(case)
    r = lambda what: PM.rng(name + "/" + what).standard_normal((rows, f))
    return dict(h=PM.dy(r("h")), go=PM.dy(r("go")), seed=seed_of(name), p=p)


# ------------------------------------------------------------------------------------------------------------ the restatements

def _mean(a):
    return a.mean(-1, keepdims=True)


def _factor(keep, p, dt):
    return dt(scale_of(p)) * keep.astype(dt)


def _stats(z, A, eps, dt):
    u = _mean(z)
    d = z - u
    r = dt(1.0) / np.sqrt(_mean(d * d) + dt(eps))
    xh = d * r
    if dt is not np.float64:
        return u, r, xh, None, None
    rms = np.sqrt(_mean(A * A))
    S_xh = r * (A + _mean(A) + np.abs(z) + np.abs(u) + np.abs(xh) * rms) + np.abs(xh)
    return u, r, xh, rms, S_xh


def ln_forward(x, res, gamma, beta, eps, keep, p, dt=np.float64):
    """z = res + c m x, out = LayerNorm(z) gamma + beta in `dt`; in float64 also mag_z, mag_out."""
    cm = _factor(keep, p, dt)
    dropped = cm * x.astype(dt)
    z = dropped if res is None else res.astype(dt) + dropped
    A = np.abs(dropped) if res is None else np.abs(res.astype(dt)) + np.abs(dropped)
    u, r, xh, rms, S_xh = _stats(z, A, eps, dt)
    g = dt(1.0) if gamma is None else gamma.astype(dt)
    b = dt(0.0) if beta is None else beta.astype(dt)
    out = dict(z=z, out=xh * g + b)
    if dt is np.float64:
        out.update(mag_z=A, mag_out=np.abs(g) * (S_xh + np.abs(xh)) + np.abs(b))
    return out


LN_VARIANTS = ("mask_not_applied", "gres_masked", "m2_dropped")


def ln_backward(go, z, gamma, eps, keep, p, dt=np.float64, variant=None):
    """gx, gres, ggamma, gbeta of the header's formulas from the given z in `dt`; in float64 also their magnitudes."""
    cm = _factor(keep, p, dt)
    go, z = go.astype(dt), z.astype(dt)
    u, r, xh, rms, S_xh = _stats(z, np.abs(z), eps, dt)
    g = go * (dt(1.0) if gamma is None else gamma.astype(dt))
    m1, m2 = _mean(g), _mean(g * xh)
    if variant == "m2_dropped":
        m2 = m2 * dt(0.0)
    t = g - m1 - xh * m2
    gz = r * t
    out = dict(gx=gz if variant == "mask_not_applied" else cm * gz, gres=cm * gz if variant == "gres_masked" else gz,
               ggamma=(go * xh).sum(0), gbeta=go.sum(0))
    if dt is np.float64 and variant is None:
        M2 = _mean(np.abs(g) * (np.abs(xh) + S_xh))
        s = r * (np.abs(g) + _mean(np.abs(g)) + np.abs(xh) * M2 + np.abs(m2) * S_xh + np.abs(t) * (1.0 + r * rms)) + np.abs(gz)
        out.update(mag_gx=cm * s, mag_gres=s, mag_ggamma=(np.abs(go) * (S_xh + np.abs(xh))).sum(0), mag_gbeta=np.abs(go).sum(0))
    return out


def relu_forward(h, keep, p, dt=np.float64):
    out = _factor(keep, p, dt) * np.maximum(h.astype(dt), dt(0.0))
    return dict(out=out, mag_out=np.abs(out)) if dt is np.float64 else dict(out=out)


RELU_VARIANTS = ("gate_from_grad_out",)


def relu_backward(go, out, p, dt=np.float64, variant=None):
    """grad_h from the op's own result: c grad_out where out > 0."""
    go = go.astype(dt)
    gate = go > 0 if variant == "gate_from_grad_out" else out > 0
    gh = np.where(gate, go * dt(scale_of(p)), dt(0.0))
    return dict(gh=gh, mag_gh=np.abs(gh)) if dt is np.float64 else dict(gh=gh)


# ----------------------------------------------------------------------------------------------------------- the error measure

HEAD = "%-40s %-7s %10s %10s %10s %8s" % ("case", "output", "kernel err", "comp err", "bound", "ratio")
_T = PM.Table(HEAD, env="LAYER_TRAIN_PARITY_TABLE")
TABLE, WORST, report = _T.lines, _T.worst, _T.report        # WORST: output -> (ratio, table line)


def check(got, want, comp, names, who, record=True):
    """Every entry of got[name] within parity_measure.entry_bound(the fp32 composition's error at the entry, its magnitude) of
    the float64 restatement want[name]; a line per output and the worst ratio per output in WORST."""
    for name in names:
        g = np.asarray(got[name], dtype=np.float64).reshape(want[name].shape)
        assert np.isfinite(want[name]).all() and (want["mag_" + name] >= 0).all(), (who, name)
        assert np.isfinite(g).all(), (who, name, "non-finite entries", np.argwhere(~np.isfinite(g))[:8].tolist())
        e = PM.errors(g, want[name], want["mag_" + name], np.asarray(comp[name], dtype=np.float64).reshape(want[name].shape))
        if record:
            _T.add("%-40s %-7s %10.2e %10.2e %10.2e %8.3f" % ((who, name) + tuple(e.row())), name, e.worst)
        e.check(who, name)


def passes(got, want, comp, names):
    try:
        check(got, want, comp, names, "variant", record=False)
    except AssertionError:
        return False
    return True


def worst_table():
    return "\n".join("%-7s %s" % (k, WORST[k][1]) for k in sorted(WORST))
