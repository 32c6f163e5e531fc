"""Per-entry float64 parity of the ConvNeXt kernels (uninext_amd/csrc/convnext.hip: dwconv_ln<4|7|8>, scale_residual,
layernorm_cf<cached|streamed>): the cases, float64 restatements that return every output entry's VALUE and its MAGNITUDE, the
fp32 PyTorch compositions, the error measure, and a Python restatement of the host's tile and pixels-per-workgroup rules.  No
GPU is needed to import this.  tests/test_convnext_parity_cpu.py checks that the measure has teeth,
tests/test_convnext_parity_gpu.py holds the kernels to it.

The magnitude.  Per pixel, over the channels c: v_c the value that is normalised (the head: v = dw_b + sum x w over the 49
taps; layernorm_cf: v = x), A_c the sum of the absolute summands of v_c (the head: |dw_b| + sum |x| |w|; layernorm_cf: |x|, x
is exact), u = mean_c v, var = mean_c (v - u)^2, r = 1 / sqrt(var + eps), o^ = (v - u) r, o = g o^ + b.  In fp32, to first
order and in units of the round-off u32 = 2^-24:
  * the tap chain leaves an error dv_c of a multiple of u32 A_c in v_c, which o sees times r |g|:                     r |g| A
  * u moves by mean_c dv_c (at most u32 mean_c A) and by the roundings of its own sum (a multiple of u32 mean_c |v|, at most
    u32 mean_c A):                                                                                            r |g| mean_c A
  * the subtraction v - u rounds once, by at most u32 |v - u| <= u32 (|v| + |u|):                            r |g| (|v| + |u|)
  * var moves by mean_c 2 (v - u)(dv_c - du); the du part vanishes because mean_c (v - u) = 0, and by Cauchy-Schwarz the rest
    is at most 2 sqrt(var) u32 rms_c A.  d r / r = -d var / (2 (var + eps)) and sqrt(var) / (var + eps) <= r, so r moves by at
    most r^2 u32 rms_c A relative to 1, and o by |g| |v - u| r times that:                                r |g| |o^| rms_c A
  * the roundings of the variance's own sum, of the root, the division, the product with g and the sum with b are relative
    to |g o^| <= |o| + |b| and to |o|:                                                                             |o| + |b|
so  s = r |g| (A + mean_c A + |v| + |u| + |o^| rms_c A) + |o| + |b|.  It carries r: a pixel whose variance is comparable to
eps, or exactly 0, is a legitimate case here (the variance floor of tests/convnext_cases.py does not apply), its bound is
simply as wide as fp32 makes it.  The form is derived, not measured; no term was fitted.  An entry is held to entry_bound of
tests/parity_measure.py: max(8 x the fp32 PyTorch composition's error of the same entry, 16 u32 s), and the project's
1e-4 * max(1, max|ref|) is asserted on top.

Every input is seeded and dyadic (a multiple of 2^-10), so fp32 holds exactly what float64 sees; eps is the fp32 number the
kernel receives.  The stresses:
  plain    as the existing tests: zero-mean taps, eps = 1e-6, ordinary variances
  offset   every channel of a pixel shares a large common term (the head: in dw_bias; layernorm_cf: in x), |mean| / sigma of
           several hundred: a one-pass variance E[v^2] - mean^2 loses its digits here (sized in test_convnext_parity_cpu.py)
  loweps   a third of the pixels has channel variance exactly 0 (the answer is ln_bias, bitwise), a third a variance
           comparable to eps = 1e-6, the rest is ordinary: eps dropped, or outside the root, shows
  bigeps   eps = 0.5 on ordinary pixels
  floor    every pixel's variance near 1e-2, where the existing tests' variance floor is, with inputs as small: the regime
           the old suite allowed, on which its one-number bound cannot see eps (5e-5 relative) and the measure can

The tile classes.  choose_tile() below restates the host's rule.  The tallest tile the 160 KiB of LDS allow is th = 8 for
every width up to C = 384; 8, 6, 5 for TW = 4, 7, 8 at C = 768; 5, 3, 2 at C = 1536.  Every (C, TW) class of C in {32, 96,
192, 384, 768, 1536} has a case, the smallest maps that reach it among those with H no multiple of th and W no multiple of TW,
with one exception: <8> at C = 1536 (th = 2) is reached only by maps of H = 2 (at H >= 3 the narrower tiles are taller and
need no more rounds of workgroups for any W: the restatement finds no such map up to H = 40, W = 20000), so its case is 2 x
1793, H a multiple of th.  W = TW + 1 with a wide tile cannot be reached either (at W = 8 the narrow tile has as many columns
as <7>, at W = 9 <7> has as many as <8>, and of two widths with as many workgroups the narrower costs less); H = th + 1 and W = TW + 1 are run on the narrow class, H = th + 1 on the wide ones at th = 8.
"""
import functools
import os
import sys
import zlib

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnext_ref as R                                                    # noqa: E402
import decoder_cases as DC                                                  # noqa: E402
import parity_measure as PM                                                 # noqa: E402
from parity_measure import COMP_MARGIN, SUM_DEPTH, U, entry_bound          # noqa: E402,F401

assert DC.STEP_BITS == 10
dyadic = DC.dyadic
TOL = DC.TOL
EPS = 1e-6
BIG_EPS = 0.5
STRESSES = ("plain", "offset", "loweps", "bigeps", "floor")
HEAD_OFFSET = 512.0         # over a sigma of about 1.4: |mean| / sigma ~ 370
CF_OFFSET = 1024.0          # over a sigma of 2: |mean| / sigma ~ 510


def fp32(eps):
    return float(np.float32(eps))


def tol(want):
    """The project's parity bound (tests/convnext_cases.py): 1e-4 of the output scale, at least 1e-4."""
    return TOL * max(1.0, float(np.abs(want).max()))


# ------------------------------------------------------------------------------------------------ the host's rules, restated

LDS_BYTES = 160 * 1024
CHUNK, TAPS, MAX_TH, CUS = 32, 49, 8, 256
WIDTHS = (4, 7, 8)


def dwconv_lds_bytes(C, th, tw):
    halo = ((th + 6) * (tw + 6)) | 1
    return (th * tw * C + CHUNK * halo + CHUNK * TAPS + 3) // 4 * 4 * 4


def tallest(C, tw, H=MAX_TH):
    """The tile height of width tw: as tall as the LDS plane and the map allow; 0 if not even one row fits."""
    th = min(H, MAX_TH)
    while th > 1 and dwconv_lds_bytes(C, th, tw) > LDS_BYTES:
        th -= 1
    return th if dwconv_lds_bytes(C, th, tw) <= LDS_BYTES else 0


def choose_tile(B, C, H, W):
    """(th, tw) of dwconv_ln: per width the tallest tile, then the width with the least (rounds of workgroups over the 256 CUs)
    x (tw + 2), the wider on a tie."""
    best, best_cost = (0, 0), 0
    for tw in WIDTHS:
        th = tallest(C, tw, H)
        if not th:
            continue
        wgs = B * -(-H // th) * -(-W // tw)
        cost = -(-wgs // CUS) * (tw + 2)
        if best[0] == 0 or cost <= best_cost:
            best, best_cost = (th, tw), cost
    return best


def head_kernel(B, C, H, W):
    return "convnext_dwconv_ln<%d>" % choose_tile(B, C, H, W)[1]


def cf_rule(C):
    """(pixels per workgroup, cached) of layernorm_cf: 64 pixels while the [C][PX] block stays inside 128 KiB, then 32, then
    16; past that the streamed kernel, 64 pixels again."""
    budget, px_log2 = 128 * 1024, 6
    while px_log2 > 4 and (C << px_log2) * 4 > budget:
        px_log2 -= 1
    cached = (C << px_log2) * 4 <= budget
    return (1 << px_log2 if cached else 64), cached


def cf_kernel(C):
    return "layernorm_cf<cached>" if cf_rule(C)[1] else "layernorm_cf<streamed>"


# ------------------------------------------------------------------------------------------------------------------- the cases

CASES = {}


def _add(name, **spec):
    assert name not in CASES, name
    CASES[name] = spec


# (C, B, H, W, dw_bias given, every stress): the narrow tile.  Maps smaller than the 7 x 7 footprint (1 x 1, 3 x 20, 20 x 3),
# H = th + 1 with W = TW + 1 at th = 8 (C = 192, 768) and th = 5 (C = 1536), one and three images, dw_bias given and NULL; the
# maps that carry every stress are at least 21 long, so that a third of one holds pixels whose whole footprint is zero
HEAD_NARROW = [(32, 1, 1, 1, True, False), (32, 3, 3, 20, True, False), (32, 1, 17, 9, False, False), (96, 1, 20, 3, False, False), (96, 3, 11, 23, True, True),
               (192, 1, 9, 5, False, False), (384, 1, 13, 10, True, False), (768, 1, 9, 5, True, False), (768, 3, 6, 9, False, False),
               (768, 1, 9, 22, True, True), (1536, 1, 6, 5, True, False), (1536, 3, 11, 10, False, False), (1536, 1, 6, 23, True, True)]
# (C, B, H, W, dw_bias given, every stress, th, TW): the wide tiles, by class
HEAD_WIDE = [(32, 3, 9, 169, True, True, 8, 7), (32, 1, 9, 897, False, False, 8, 8),
             (96, 1, 9, 513, False, False, 8, 7), (96, 3, 9, 295, True, False, 8, 8),
             (192, 3, 9, 169, False, False, 8, 7), (192, 1, 9, 897, True, False, 8, 8),
             (384, 1, 65, 113, True, False, 8, 7), (384, 3, 9, 295, False, False, 8, 8),
             (768, 1, 65, 113, True, False, 6, 7), (768, 3, 9, 169, True, True, 6, 7), (768, 1, 73, 134, False, False, 5, 8),
             (1536, 1, 41, 113, False, False, 3, 7), (1536, 3, 7, 169, True, True, 3, 7), (1536, 1, 2, 1793, True, False, 2, 8)]
for _C, _B, _H, _W, _bias, _all in HEAD_NARROW:
    for _s in (STRESSES if _all else ("plain",)):
        _add("head/C%d_B%d_%dx%d/%s" % (_C, _B, _H, _W, _s), kernel="head", C=_C, B=_B, H=_H, W=_W, bias=_bias, stress=_s,
             tile=(tallest(_C, 4, _H), 4))
for _C, _B, _H, _W, _bias, _all, _th, _tw in HEAD_WIDE:
    for _s in (STRESSES if _all else ("plain",)):
        _add("head/C%d_B%d_%dx%d/%s" % (_C, _B, _H, _W, _s), kernel="head", C=_C, B=_B, H=_H, W=_W, bias=_bias, stress=_s,
             tile=(_th, _tw))

CF_CS = (1, 2, 15, 16, 17, 512, 513, 768, 1024, 1025, 2048, 2049)
CF_STRESSED = (512, 768, 2048, 2049)        # one C per class: 64, 32 and 16 pixels per workgroup, and the streamed kernel
for _C in CF_CS:
    _PX = cf_rule(_C)[0]
    for _HW in (1, _PX - 1, _PX, _PX + 1, 2 * _PX + 3):
        for _B in (1, 3):
            _add("cf/C%d_B%d_HW%d/plain" % (_C, _B, _HW), kernel="cf", C=_C, B=_B, H=1, W=_HW, stress="plain")
    if _C in CF_STRESSED:
        for _s in STRESSES[1:]:
            _add("cf/C%d_B3_HW%d/%s" % (_C, 2 * _PX + 3, _s), kernel="cf", C=_C, B=3, H=1, W=2 * _PX + 3, stress=_s)

TAIL_SIZES = (1, 63, 64, 65, 129)           # C and H * W each: below, at and past the 64 x 64 transpose tile, and two tiles + 1
for _C in TAIL_SIZES:
    for _HW in TAIL_SIZES:
        for _g in (True, False):
            _add("tail/C%d_HW%d/%s" % (_C, _HW, "gamma" if _g else "nogamma"), kernel="tail", C=_C, B=2, H=1, W=_HW, gamma=_g,
                 stress="plain")


def names(kernel, **want):
    return [n for n, c in CASES.items() if c["kernel"] == kernel and all(c[k] == v for k, v in want.items())]


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _thirds(n):
    """0, 1, 2 along an axis of n: the first third, the middle one, the rest"""
    return torch.arange(n) * 3 // max(n, 1)


def region(name):
    """loweps: [H, W] of 0 (variance exactly 0), 1 (comparable to eps), 2 (ordinary).  The head splits the longer axis into
    thirds (a pixel has variance 0 only where its whole footprint is zero); layernorm_cf takes every third pixel."""
    c = CASES[name]
    H, W = c["H"], c["W"]
    if c["kernel"] == "cf":
        return (torch.arange(H * W) % 3).view(H, W)
    return _thirds(W)[None, :].expand(H, W) if W >= H else _thirds(H)[:, None].expand(H, W)


@functools.lru_cache(maxsize=4)
def inputs(name):
    """Float64 dyadic inputs of a case from its name (plus eps, the fp32 number as a float); left unchanged."""
    c = CASES[name]
    g = _gen(name)
    B, C, H, W, stress = c["B"], c["C"], c["H"], c["W"], c["stress"]
    eps = fp32(BIG_EPS if stress == "bigeps" else EPS)
    rn = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    if c["kernel"] == "tail":
        x = dict(y=dyadic(rn(B, H, W, C)), inp=dyadic(rn(B, C, H, W)), gamma=dyadic(rn(C)) if c["gamma"] else None)
    elif c["kernel"] == "head":
        xs = dyadic(rn(B, C, H, W), 0.0625 if stress == "floor" else 1.0)
        dw_w = dyadic(rn(C, 1, 7, 7), 0.2)
        dw_b = dyadic(rn(C), 0.03125 if stress == "floor" else 0.5) if c["bias"] else None
        if stress == "offset":
            dw_b = dw_b + HEAD_OFFSET
        elif stress == "loweps":
            reg = region(name)
            tiny = dyadic(rn(B, C, H, W), 2.0 ** -10)              # -2 .. 2 steps of 2^-10
            xs = torch.where(reg == 2, xs, torch.where(reg == 1, tiny, torch.zeros_like(xs)))
            dw_b = torch.full((C,), 0.5, dtype=torch.float64) if c["bias"] else None
        x = dict(x=xs, dw_w=dw_w, dw_b=dw_b, ln_w=dyadic(1.0 + 0.25 * rn(C)), ln_b=dyadic(rn(C), 0.25), eps=eps)
    else:
        xs = dyadic(rn(B, C, H, W), 0.125) if stress == "floor" else dyadic(2.0 * rn(B, C, H, W) + 0.5)
        if stress == "offset":
            xs = xs + CF_OFFSET
        elif stress == "loweps":
            reg = region(name)
            tiny = 0.5 + dyadic(rn(B, C, H, W), 2.0 ** -10)
            xs = torch.where(reg == 2, xs, torch.where(reg == 1, tiny, torch.full_like(xs, 0.5)))
        x = dict(x=xs, ln_w=dyadic(1.0 + 0.25 * rn(C)), ln_b=dyadic(rn(C), 0.25), eps=eps)
    for key, t in x.items():
        if isinstance(t, torch.Tensor):
            x[key] = t = t + 0.0                                    # rounding to the dyadic grid leaves -0.0 behind: +0.0
            assert torch.equal(t.float().double(), t), (name, key)  # fp32 holds what float64 sees
    return x


# ------------------------------------------------------------------------------------------------------------ the restatements

def dwconv7_mag(x, weight, bias):
    """(v, A) [B, C, H, W] float64: the depthwise 7 x 7 convolution with zero padding 3 as a sum of 49 shifted slices, and the
    same sum over the absolute values of its summands."""
    B, C, H, W = x.shape
    xp = F.pad(x, (3, 3, 3, 3))
    xa = xp.abs()
    v = torch.zeros_like(x) if bias is None else bias.view(1, C, 1, 1).expand(B, C, H, W).clone()
    A = v.abs()
    for ky in range(7):
        for kx in range(7):
            w = weight[:, 0, ky, kx].view(1, C, 1, 1)
            v.addcmul_(xp[:, :, ky:ky + H, kx:kx + W], w)
            A.addcmul_(xa[:, :, ky:ky + H, kx:kx + W], w.abs())
    return v, A


def norm_mag(v, A, g, b, eps, dim):
    """LayerNorm of v along `dim` (biased variance, eps inside the root) and the magnitude of every entry: the module docstring."""
    shape = [1] * v.dim()
    shape[dim] = -1
    g, b = g.view(shape), b.view(shape)
    u = v.mean(dim, keepdim=True)
    d = v - u
    r = 1.0 / torch.sqrt((d * d).mean(dim, keepdim=True) + eps)
    oh = d * r
    o = oh * g + b
    rms = torch.sqrt((A * A).mean(dim, keepdim=True))
    s = r * g.abs() * (A + A.mean(dim, keepdim=True) + v.abs() + u.abs() + oh.abs() * rms) + o.abs() + b.abs()
    return o, s


def variance(name):
    """[B, H, W] float64: the channel variance of what the case normalises"""
    c, x = CASES[name], inputs(name)
    v = dwconv7_mag(x["x"], x["dw_w"], x["dw_b"])[0] if c["kernel"] == "head" else x["x"]
    return R.channel_variance(v, 1)


@functools.lru_cache(maxsize=4)
def reference(name):
    """(value, mag) float64 numpy of a case, in the kernel's output layout: computed once, shared, left unchanged."""
    c, x = CASES[name], inputs(name)
    if c["kernel"] == "head":
        v, A = dwconv7_mag(x["x"], x["dw_w"], x["dw_b"])
        o, s = norm_mag(v.permute(0, 2, 3, 1), A.permute(0, 2, 3, 1), x["ln_w"], x["ln_b"], x["eps"], 3)
    elif c["kernel"] == "cf":
        o, s = norm_mag(x["x"], x["x"].abs(), x["ln_w"], x["ln_b"], x["eps"], 1)
    else:
        prod = x["y"] if x["gamma"] is None else x["y"] * x["gamma"]
        o = x["inp"] + prod.permute(0, 3, 1, 2)
        s = o.abs() + prod.abs().permute(0, 3, 1, 2)                # two roundings: the product's and the sum's
    return np.ascontiguousarray(o.numpy()), np.ascontiguousarray(s.numpy())


def existing_restatement(name):
    """The value by tests/convnext_ref.py on the same inputs."""
    c, x = CASES[name], inputs(name)
    if c["kernel"] == "head":
        return R.dwconv_ln(x["x"], x["dw_w"], x["dw_b"], x["ln_w"], x["ln_b"], x["eps"]).numpy()
    if c["kernel"] == "cf":
        return R.layernorm_cf(x["x"], x["ln_w"], x["ln_b"], x["eps"]).numpy()
    return R.scale_residual(x["y"], x["gamma"], x["inp"]).numpy()


def stress_property(name):
    """Asserts, on the float64 variances and means, the property that names a stress case."""
    c, x = CASES[name], inputs(name)
    stress = c["stress"]
    if c["kernel"] == "tail":
        return
    var = variance(name)
    if stress == "offset":
        v = dwconv7_mag(x["x"], x["dw_w"], x["dw_b"])[0] if c["kernel"] == "head" else x["x"]
        assert float((v.mean(1).abs() / var.sqrt()).min()) > 200.0, name
    elif stress == "loweps":
        reg = region(name)[None].expand_as(var)
        zero, low, rest = var[reg == 0], var[reg == 1], var[reg == 2]
        assert zero.numel() and low.numel() and rest.numel(), name
        assert bool((zero == 0).any()) and bool(((low > 0.1 * EPS) & (low < 10 * EPS)).any()) and float(rest.max()) > 0.1, name
        if c["kernel"] == "cf":
            assert bool((zero == 0).all()), name
    elif stress == "bigeps":
        assert x["eps"] == 0.5 and float(var.min()) > 0.1, name
    elif stress == "floor":
        assert 1e-3 < float(var.min()) and float(var.max()) < 5e-2, (name, float(var.min()), float(var.max()))
    else:
        assert stress == "plain" and x["eps"] == fp32(EPS)


def zero_variance_pixels(name):
    """[B, H, W] bool: the pixels whose float64 channel variance is exactly 0 (there the answer is ln_bias, bitwise)"""
    return (variance(name) == 0).numpy()


# ----------------------------------------------------------------------------------------------------------- the compositions

def composition(name, device="cpu"):
    """The fp32 PyTorch composition on `device` as float64 numpy; it never runs the kernels.  The head: F.conv2d with groups
    and padding 3, then F.layer_norm.  layernorm_cf: mean, squared deviations, sqrt and division written out, as
    uninext_amd.backbone.LayerNorm does on its PyTorch route.  The tail: inp + (gamma * y).permute."""
    c, x = CASES[name], inputs(name)
    dev = lambda t: None if t is None else t.float().to(device)
    with torch.no_grad():
        if c["kernel"] == "head":
            C = c["C"]
            t = F.conv2d(dev(x["x"]), dev(x["dw_w"]), dev(x["dw_b"]), padding=3, groups=C).permute(0, 2, 3, 1)
            out = F.layer_norm(t, (C,), dev(x["ln_w"]), dev(x["ln_b"]), x["eps"])
        elif c["kernel"] == "cf":
            t = dev(x["x"])
            centred = t - t.mean(dim=1, keepdim=True)
            var = (centred * centred).mean(dim=1, keepdim=True)
            out = dev(x["ln_w"]).view(-1, 1, 1) * (centred / torch.sqrt(var + x["eps"])) + dev(x["ln_b"]).view(-1, 1, 1)
        else:
            y, gamma = dev(x["y"]), dev(x["gamma"])
            out = dev(x["inp"]) + (y if gamma is None else gamma * y).permute(0, 3, 1, 2)
        assert out.dtype == torch.float32
        return out.detach().cpu().double().contiguous().numpy()


# ---------------------------------------------------------------------------------------------------------- the error measure

HEAD = "%-36s %10s %10s %10s %8s" % ("case", "kernel err", "comp err", "bound", "ratio")
_T = PM.Table(HEAD, env="CONVNEXT_PARITY_TABLE")
TABLE, WORST, report = _T.lines, _T.worst, _T.report        # WORST: (kernel, stress) -> (ratio, table line)


def measure(case, got, want, mag, comp, check=True):
    """Every entry of `got` within entry_bound(the composition's error at the entry, s) of `want`, and the project's bound on top.
    Returns the largest error / bound; check=False only returns it (inf for a NaN in `got`) and adds no line.
    Non-finite: no NaN in `want`, `comp` or `got`.
    WORST: (kernel, stress).  Line: case, the worst entry's errors relative to its own magnitude.
    Tolerance: tol(want), TOL of the tensor's largest value and at least TOL."""
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape == comp.shape == mag.shape, (case, got.shape, want.shape, comp.shape, mag.shape)
    assert not np.isnan(want).any() and not np.isnan(comp).any(), (case, "the float64 value is NaN nowhere")
    if np.isnan(got).any():
        assert not check, (case, "NaN entries", np.argwhere(np.isnan(got))[:8].tolist())
        return float("inf")
    e = PM.errors(got, want, mag, comp)
    if not check:
        return e.worst
    _T.add("%-36s %10.2e %10.2e %10.2e %8.3f" % ((case,) + e.row()), (CASES[case]["kernel"], CASES[case]["stress"]), e.worst)
    e.check(case)
    assert float(e.err.max()) <= tol(want), (case, "the project's bound", float(e.err.max()), tol(want))
    return e.worst


def old_bound_passes(got, want):
    """The one number per call of tests/test_convnext_gpu.py: max abs error below 1e-4 * max(1, max|ref|)."""
    got = np.asarray(got, dtype=np.float64)
    return not np.isnan(got).any() and float(np.abs(got - want).max()) < tol(want)


def worst_table():
    return "\n".join("%-5s %-7s %s" % (k[0], k[1], WORST[k][1]) for k in sorted(WORST))
