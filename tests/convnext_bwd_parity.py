"""Per-entry float64 parity of the ConvNeXt backward kernels (uninext_amd/csrc/convnext_bwd.hip: head_bwd_gu<4|7|8>, head_bwd_xw,
tail_bwd, layernorm_cf_bwd<cached|streamed>, reduce_partials): the cases, an analytic float64 restatement that returns every
gradient entry's VALUE and its MAGNITUDE, the fp32 PyTorch composition, and the error measure.  No GPU and no built package is
needed to import this.  tests/test_convnext_bwd_parity_cpu.py checks that the measure has teeth,
tests/test_convnext_bwd_parity_gpu.py holds the kernels to it through the C ABI.

Every input, grad_out included, is seeded by the case's name and dyadic (a multiple of 2^-10): fp32 holds exactly what float64
sees; eps is the fp32 number the kernel receives.

THE RESTATEMENT, closed forms and no autograd (so that every entry has a magnitude).  Per pixel, over the channels c: v the
value that is normalised (the head: v = dw_b + sum x w over the 49 taps; layernorm_cf: v = x), u = mean v, var = mean (v - u)^2,
r = 1 / sqrt(var + eps), xh = (v - u) r; go the upstream gradient, lw the LayerNorm's weight:
    gwv = go lw        m1 = mean gwv        m2 = mean (gwv xh)        t = gwv - m1 - xh m2        grad_u = r t
    head:  gx[h, w] = sum_taps grad_u[h + 3 - ky, w + 3 - kx] w[ky, kx]   (the mirrored weights, zero outside the map)
           gw[ky, kx] = sum_pixels grad_u[h, w] x[h - 3 + ky, w - 3 + kx]        gb = sum_pixels grad_u
           glw = sum_pixels go xh                                                glb = sum_pixels go
    cf:    gx = grad_u        gw = sum_pixels go xh        gb = sum_pixels go
    tail:  gy[b, p, c] = (go[b, c, p] s_b) gamma_c        ggamma[c] = sum_{b, p} (go s_b) y        (s = 1, gamma = 1 when NULL)
agrees_with_autograd() holds it to float64 autograd through tests/convnext_ref.py (convnext_train_cases.head_grads / cf_grads)
to 1e-12 of each group's scale.

THE MAGNITUDES, derived to first order in u32 = 2^-24; nothing here was fitted to what a kernel gives.  A is the sum of the
absolute summands of v (the head: |dw_b| + sum |x| |w|; layernorm_cf: |x|), as in convnext_parity.norm_mag, whose derivation
gives the error scale of xh (the forward's o with g = 1, b = 0):
    S_xh = r (A + mean A + |v| + |u| + |xh| rms A) + |xh|
and the relative error of r itself, u32 r rms A (the variance moves by 2 sqrt(var) u32 rms A, d r / r = -d var / (2 (var +
eps)), sqrt(var) / (var + eps) <= r).  Then
  * gwv is one rounding: u32 |gwv|.
  * m1 is a fp32 sum of the rounded gwv: a multiple of u32 mean |gwv|.
  * every summand of m2 is gwv xh: it errs by |gwv| (the error of xh, u32 S_xh) and rounds relative to |gwv xh|; the sum's own
    roundings are relative to mean |gwv xh| again:                                    M2 = mean (|gwv| (|xh| + S_xh)) >= |m2|.
  * the product xh m2 errs by |xh| (the error of m2) + |m2| (the error of xh) and rounds relative to |xh m2| <= |xh| M2:
                                                                                                  |xh| M2 + |m2| S_xh.
  * the two subtractions round relative to |gwv - m1| <= |gwv| + mean |gwv| and to |t|.
  * the product with r carries r's relative error, u32 r rms A, and its own rounding (and the root's and the division's), all
    relative to |t|:                                                                                   |t| (1 + r rms A).
so  s_gu = r (|gwv| + mean |gwv| + |xh| M2 + |m2| S_xh + |t| (1 + r rms A)).  A sum of products of grad_u carries that error per
summand and rounds relative to its absolute summands:
    head gx: sum_taps |w| (s_gu + |grad_u|)      gw: sum_pixels |x| (s_gu + |grad_u|)      gb: sum_pixels (s_gu + |grad_u|)
    glw (cf gw): sum_pixels |go| (S_xh + |xh|)   glb (cf gb): sum_pixels |go|   (go is exact: only the sum rounds)
    cf gx: s_gu + |grad_u|
    tail gy: 2 |gy|, the two products' roundings       ggamma: sum |go s y|.
The magnitudes carry r once or twice: a pixel whose variance is comparable to eps, or exactly 0, is a legitimate case, its
bound is as wide as fp32 makes it.  An entry is held to parity_measure.entry_bound: max(COMP_MARGIN x the fp32 composition's
error at the entry, SUM_DEPTH u32 x the magnitude); a magnitude of 0 (a dropped sample's gy) leaves no room at all.  A group
that is exactly zero in float64 -- layernorm_cf at C = 1: gwv - m1 = 0 and xh = 0, so gx and gw vanish -- is asserted to be
zero in every entry, not measured.

The project's bound sits on top: TOL (1e-4) of max(1, the group's largest value).  It is lifted for the `loweps`, `offset` and
`common` cases only (LIFTED below, by name with the argument); plain, bigeps, floor, band and cap cases keep it.

THE STRESSES are the forward sweep's (convnext_parity: offset, loweps, bigeps, floor, with its constants and properties), the
backward recomputes the same statistics; and `common`: ln_w = 1 and a pixel's grad_out is a common term of +-512 plus noise of
1 / 8, so that gwv - m1 is a residue of 2^-8 of |gwv| or less (asserted), the place where "gwv - mean(gwv) must see the same
gwv" and the cancellation gwv - m1 - xh m2 matter.

THE CASES.  Head, pass one runs on the forward's tiling: one plain case per (C, TW) class of convnext_parity, th as tall as the
LDS allows -- the narrow tile's from its HEAD_NARROW, the smallest of each C with H >= th; the wide tiles' the smallest map of
the class (B <= 3, th <= H <= 2 th + 1, W < 2200: tests/test_convnext_bwd_parity_cpu.py repeats the search).  A wide tile is
chosen only past 256 workgroups of the narrow one, so the classes <8> at C = 192 and both at C = 384, 768, 1536 have NO map
below 1.5 M input entries; each keeps its one, smallest case (1.5 M to 6.1 M entries).  Maps smaller than the footprint (1 x 1,
3 x 20, 20 x 3), B = 1 and 3, dw_bias given and NULL are among them.  Pass two (8 x 8 tiles, halo 3): EDGE_MAPS, H and W from
{1, 7, 8, 9, 10, 11, 12, 16, 17}, the last tile 1, 2, 3 or 4 wide or tall.  Bands: convnext_train_cases.BAND_HEAD_CASES (bands of
2, 3, 22 with a short last band), BAND_CAP_SHAPE (642 tiles, bands of 64, the last of 2), and C = 1536, 17 x 25: the fewest bands
(6, of 2 tiles, all full) one image reaches with more than a tile a band.  (bands == 1 with per_band > 1 does not exist: the
rule aims at 512 / (C / 32) >= 10 bands, so a band holds more than one tile only past 10 tiles, which then make 6 bands or
more.)  The stresses run on a narrow-tile map at C = 96 (11 x 23), one at C = 768 with th = 6 (6 x 23: the map's height
limits the tile; the LDS-limited th < 8 of C = 768 are the wide classes above, 3.5 M entries and more), and a band case with 2
tiles a band (C = 768, B = 3, 9 x 25).
layernorm_cf: C in CF_CS (fewer channels than the 16 parts, the cached / streamed switch at 512, a streamed odd remainder) x
H W in (1, 63, 64, 65, 131) x B in (1, 3); every stress at C = 512 and 513; reduce_partials at C = 2, B = 1 with 1, 7, 8, 9
partial rows; C = 1 once more with grad_out 512 times as large, so that go lw rounds (see the case).  The tail: TAIL_SIZES squared, B = 3, gamma given / NULL, sample_scale NULL / [1 / 0.3, 0, 1 / 0.3].
"""
import functools
import os
import sys
import zlib

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnext_parity as FP                                                # noqa: E402
import convnext_train_cases as T                                            # noqa: E402
import parity_measure as PM                                                 # noqa: E402
from convnext_parity import TOL, choose_tile, dwconv7_mag, dyadic, fp32, tallest     # noqa: E402,F401
from parity_measure import COMP_MARGIN, SUM_DEPTH, U, entry_bound          # noqa: E402,F401

EPS, BIG_EPS, HEAD_OFFSET, CF_OFFSET = FP.EPS, FP.BIG_EPS, FP.HEAD_OFFSET, FP.CF_OFFSET
STRESSES = FP.STRESSES + ("common",)
COMMON = 512.0                  # the common term of a pixel's grad_out in `common`, over noise of 1 / 8
SIZE_LIMIT = 1500000            # input entries of a case, but for the classes that have no smaller map and the cap case
AUTOGRAD_LIMIT = 300000         # agrees_with_autograd runs on every case up to here
GROUPS = {"head": ("gx", "gw", "gb", "glw", "glb"), "cf": ("gx", "gw", "gb"), "tail": ("gy", "ggamma")}
DROP_SCALE = (fp32(1.0 / 0.3), 0.0, fp32(1.0 / 0.3))       # keep = 0.3, the middle sample dropped


def bands(c, B, H, W):
    return T.head_bands(B, c, H, W)


def head_route(B, C, H, W):
    return "convnext_dwconv_ln_backward<%d>" % choose_tile(B, C, H, W)[1]


def cf_cached(C):
    return C <= 512


def cf_route(C):
    return "layernorm_cf_backward<%s>" % ("cached" if cf_cached(C) else "streamed")


def partial_rows(B, HW):
    """rows reduce_partials adds for layernorm_cf and the tail: one per (image, block of 64 pixels)"""
    return B * -(-HW // 64)


# ------------------------------------------------------------------------------------------------------------------- the cases

CASES = {}


def _add(name, **spec):
    assert name not in CASES, name
    CASES[name] = spec


def _head(group, C, B, H, W, bias, stress="plain"):
    _add("head/C%d_B%d_%dx%d/%s" % (C, B, H, W, stress), kernel="head", group=group, C=C, B=B, H=H, W=W, bias=bias, stress=stress,
         tile=choose_tile(B, C, H, W), bands=bands(C, B, H, W))


# (C, B, H, W, dw_bias given): pass one's classes.  The narrow tile, th = 8 (5 at C = 1536), and the maps below the footprint
TILE_NARROW = [(32, 1, 1, 1, True), (32, 3, 3, 20, True), (32, 1, 17, 9, False), (96, 1, 20, 3, False), (192, 1, 9, 5, False),
               (384, 1, 13, 10, True), (768, 1, 9, 5, True), (1536, 1, 6, 5, True)]
# the wide tiles: (C, B, H, W, dw_bias given, th, TW), the smallest map of each class
TILE_WIDE = [(32, 3, 9, 169, True, 8, 7), (32, 3, 9, 295, False, 8, 8), (96, 3, 9, 169, False, 8, 7), (96, 3, 9, 295, True, 8, 8),
             (192, 3, 9, 169, True, 8, 7), (192, 3, 9, 295, False, 8, 8), (384, 3, 9, 169, False, 8, 7), (384, 3, 9, 295, True, 8, 8),
             (768, 3, 9, 169, True, 6, 7), (768, 3, 9, 295, False, 5, 8), (1536, 3, 6, 169, False, 3, 7), (1536, 3, 2, 596, True, 2, 8)]
# (C, B, H, W, dw_bias given): pass two's last tile 1, 2, 3, 4 (and 7, 8) wide or tall
EDGE_MAPS = [(32, 1, 1, 7, True), (32, 3, 7, 9, False), (32, 1, 8, 10, True), (96, 1, 9, 11, False), (96, 3, 10, 12, True),
             (32, 1, 11, 16, False), (96, 1, 12, 17, True), (96, 3, 16, 8, False), (32, 3, 17, 1, True), (96, 1, 17, 17, False)]
FEW_BANDS = (1536, 1, 17, 25, True)
STRESS_MAPS = [(96, 3, 11, 23, True), (768, 1, 6, 23, True), (768, 3, 9, 25, True)]
for _c in TILE_NARROW:
    _head("tile", *_c)
for _c in TILE_WIDE:
    _head("tile", *_c[:5])
for _c in EDGE_MAPS:
    _head("edge", *_c)
for _c in T.BAND_HEAD_CASES + [FEW_BANDS]:
    _head("band", *_c)
_head("cap", *(T.BAND_CAP_SHAPE + (False,)))
for _c in STRESS_MAPS:
    for _s in STRESSES:
        _head("stress", *_c, stress=_s)

CF_CS = (1, 2, 15, 16, 17, 512, 513, 1025)
CF_HWS = (1, 63, 64, 65, 131)
CF_STRESSED = (512, 513)
CF_REDUCE_HWS = (64, 448, 449, 513)         # at C = 2, B = 1: 1, 7, 8 and 9 partial rows
for _C in CF_CS:
    for _HW in CF_HWS:
        for _B in (1, 3):
            _add("cf/C%d_B%d_HW%d/plain" % (_C, _B, _HW), kernel="cf", group="shape", C=_C, B=_B, H=1, W=_HW, stress="plain")
    if _C in CF_STRESSED:
        for _s in STRESSES[1:]:
            _add("cf/C%d_B3_HW131/%s" % (_C, _s), kernel="cf", group="stress", C=_C, B=3, H=1, W=131, stress=_s)
for _HW in CF_REDUCE_HWS[1:]:                # H W = 64 is among the shapes above
    _add("cf/C2_B1_HW%d/plain" % _HW, kernel="cf", group="reduce", C=2, B=1, H=1, W=_HW, stress="plain")

# grad_out 512 times as large, so that go * lw has more than 24 bits and rounds (products of the other cases' dyadic operands are
# exact): at C = 1 the exact zero of gx holds only if gwv - m1 sees the gwv the mean was taken of
_add("cf/C1_B3_HW65_go512/plain", kernel="cf", group="rounding", C=1, B=3, H=1, W=65, stress="plain", go_scale=512.0)

TAIL_SIZES = T.TAIL_SIZES
for _C in TAIL_SIZES:
    for _HW in TAIL_SIZES:
        for _g in (True, False):
            for _d in (True, False):
                _add("tail/C%d_HW%d/%s_%s" % (_C, _HW, "gamma" if _g else "nogamma", "drop" if _d else "nodrop"), kernel="tail",
                     group="shape", C=_C, B=3, H=1, W=_HW, gamma=_g, drop=_d, stress="plain")


def names(kernel=None, **want):
    return [n for n, c in CASES.items() if (kernel is None or c["kernel"] == kernel) and all(c.get(k) == v for k, v in want.items())]


def entries(name):
    c = CASES[name]
    return c["B"] * c["C"] * c["H"] * c["W"]


# LIFTED: the cases without the project's bound on top, each by name.  The argument is the same for all of them: TOL of a
# tensor's largest value is a statement about fp32 arithmetic only while every entry's own error scale is of the order of
# its value.
#   loweps  a third of the pixels has r = 1000 (variance 0) and a third r of 300 to 1000 (variance near eps): xh there errs by
#           u32 S_xh with S_xh = r (A + ..) of the order of 1e3, and grad_u carries r once more: its error scale s_gu is 1e5 to
#           1e6 u32, a few hundredths, beside values of the tensor that the ordinary third keeps at 1 to 10.  Every group
#           that holds grad_u or xh sums such entries (head gx, gw, gb, glw; cf gx, gw); glb / cf gb hold neither and keep TOL.
#   offset  v = 512 (head) or 1024 (cf) in every channel: A, |v| and |u| are that large while v - u is of the order of 1;
#           S_xh = r (A + mean A + |v| + |u|) is about 1e3 and the cancellation's residue xh is what the gradients are
#           made of.  The same groups as loweps.
#   common  gwv = +-512 + noise: t = gwv - m1 - xh m2 is the residue, 2^-8 of its terms, and s_gu = r (|gwv| + mean |gwv| + ..)
#           is a thousand times |grad_u|.  The groups made of grad_u: head gx, gw, gb; cf gx.  (glw, glb, cf gw, cf gb are
#           plain sums of go and go xh and keep TOL.)
LIFTED_GROUPS = {("head", "loweps"): ("gx", "gw", "gb", "glw"), ("head", "offset"): ("gx", "gw", "gb", "glw"),
                 ("head", "common"): ("gx", "gw", "gb"), ("cf", "loweps"): ("gx", "gw"), ("cf", "offset"): ("gx", "gw"),
                 ("cf", "common"): ("gx",)}
LIFTED = {n: LIFTED_GROUPS[(c["kernel"], c["stress"])] for n, c in CASES.items() if (c["kernel"], c["stress"]) in LIFTED_GROUPS}
# agrees_with_autograd: the same cases' same groups are held to 1e-12 of the group's largest MAGNITUDE, not value -- float64
# autograd and the closed forms are both good to 2^-53 of the uncancelled terms, which is what the magnitude sums.


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(("convnext_bwd/" + name).encode()))


def region(name):
    """loweps: [H, W] of 0 (variance exactly 0), 1 (comparable to eps), 2 (ordinary), as convnext_parity.region: the head splits
    the longer axis into thirds, layernorm_cf takes every third pixel."""
    c = CASES[name]
    H, W = c["H"], c["W"]
    if c["kernel"] == "cf":
        return (torch.arange(H * W) % 3).view(H, W)
    return FP._thirds(W)[None, :].expand(H, W) if W >= H else FP._thirds(H)[:, None].expand(H, W)


@functools.lru_cache(maxsize=2)
def inputs(name):
    """Float64 dyadic inputs of a case from its name (plus eps, the fp32 number as a float); left unchanged.  grad_out `go` is
    [B, H, W, C] for the head and [B, C, H, W] otherwise, as the kernels read it."""
    c = CASES[name]
    g = _gen(name)
    B, C, H, W, stress = c["B"], c["C"], c["H"], c["W"], c["stress"]
    eps = fp32(BIG_EPS if stress == "bigeps" else EPS)
    rn = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    if c["kernel"] == "tail":
        x = dict(go=dyadic(rn(B, C, H, W)), y=dyadic(rn(B, H, W, C)), gamma=dyadic(rn(C)) if c["gamma"] else None,
                 scale=torch.tensor(DROP_SCALE, dtype=torch.float64) if c["drop"] else None)
    else:
        head = c["kernel"] == "head"
        if head:
            xs = dyadic(rn(B, C, H, W), 0.0625 if stress == "floor" else 1.0)
            dw_w = dyadic(rn(C, 1, 7, 7), 0.2)
            dw_b = dyadic(rn(C), 0.03125 if stress == "floor" else 0.5) if c["bias"] else None
            if stress == "offset":
                dw_b = dw_b + HEAD_OFFSET
            elif stress == "loweps":
                reg = region(name)
                tiny = dyadic(rn(B, C, H, W), 2.0 ** -10)
                xs = torch.where(reg == 2, xs, torch.where(reg == 1, tiny, torch.zeros_like(xs)))
                dw_b = torch.full((C,), 0.5, dtype=torch.float64) if c["bias"] else None
            x = dict(x=xs, dw_w=dw_w, dw_b=dw_b)
        else:
            xs = dyadic(rn(B, C, H, W), 0.125) if stress == "floor" else dyadic(2.0 * rn(B, C, H, W) + 0.5)
            if stress == "offset":
                xs = xs + CF_OFFSET
            elif stress == "loweps":
                reg = region(name)
                tiny = 0.5 + dyadic(rn(B, C, H, W), 2.0 ** -10)
                xs = torch.where(reg == 2, xs, torch.where(reg == 1, tiny, torch.full_like(xs, 0.5)))
            x = dict(x=xs)
        x["ln_w"] = torch.ones(C, dtype=torch.float64) if stress == "common" else dyadic(1.0 + 0.25 * rn(C))
        shape = (B, H, W, C) if head else (B, C, H, W)
        if stress == "common":      # one sign per pixel, the same in every channel
            sign = torch.randint(0, 2, (B, H, W), generator=g).double() * 2.0 - 1.0
            x["go"] = (sign.unsqueeze(-1 if head else 1) * COMMON).expand(shape) + dyadic(rn(*shape), 0.125)
        else:
            x["go"] = dyadic(rn(*shape), c.get("go_scale", 1.0))
        x["eps"] = eps
    for key, t in x.items():
        if isinstance(t, torch.Tensor):
            x[key] = t = (t + 0.0).contiguous()                     # rounding to the dyadic grid leaves -0.0 behind: +0.0
            assert torch.equal(t.float().double(), t), (name, key)  # fp32(x) == x
            assert key == "scale" or PM.is_dyadic(t.numpy()), (name, key)
    return x


# ------------------------------------------------------------------------------------------------------------ the restatement

def _m(t):
    return t.mean(1, keepdim=True)


def ln_bwd_mag(v, A, lw, go, eps):
    """The LayerNorm backward over dim 1 of [B, C, H, W] tensors -> a dict of float64 tensors: xh, r, S_xh, gwv, m1, m2, grad_u
    `gu` and its error scale `s_gu`, the sums glw, glb with their magnitudes.  The module docstring derives every line."""
    lw = lw.view(1, -1, 1, 1)
    u = _m(v)
    d = v - u
    r = 1.0 / torch.sqrt(_m(d * d) + eps)
    xh = d * r
    rms = torch.sqrt(_m(A * A))
    S_xh = r * (A + _m(A) + v.abs() + u.abs() + xh.abs() * rms) + xh.abs()
    gwv = go * lw
    m1, m2 = _m(gwv), _m(gwv * xh)
    t = gwv - m1 - xh * m2
    M2 = _m(gwv.abs() * (xh.abs() + S_xh))
    s_gu = r * (gwv.abs() + _m(gwv.abs()) + xh.abs() * M2 + m2.abs() * S_xh + t.abs() * (1.0 + r * rms))
    dims = (0, 2, 3)
    return dict(xh=xh, r=r, S_xh=S_xh, gwv=gwv, m1=m1, m2=m2, gu=r * t, s_gu=s_gu,
                glw=((go * xh).sum(dims), (go.abs() * (S_xh + xh.abs())).sum(dims)), glb=(go.sum(dims), go.abs().sum(dims)))


def pixel_terms(name):
    """ln_bwd_mag of a head or layernorm_cf case"""
    c, x = CASES[name], inputs(name)
    if c["kernel"] == "head":
        v, A = dwconv7_mag(x["x"], x["dw_w"], x["dw_b"])
        return ln_bwd_mag(v, A, x["ln_w"], x["go"].permute(0, 3, 1, 2), x["eps"])
    return ln_bwd_mag(x["x"], x["x"].abs(), x["ln_w"], x["go"], x["eps"])


def restate(name):
    """{group: (value, mag)} float64 numpy, in the kernels' output layouts"""
    c, x = CASES[name], inputs(name)
    B, C, H, W = c["B"], c["C"], c["H"], c["W"]
    if c["kernel"] == "tail":
        s = torch.ones(B, dtype=torch.float64) if x["scale"] is None else x["scale"]
        t = x["go"] * s.view(B, 1, 1, 1)
        gy = (t if x["gamma"] is None else t * x["gamma"].view(1, C, 1, 1)).permute(0, 2, 3, 1)
        out = {"gy": (gy, 2.0 * gy.abs())}
        if x["gamma"] is not None:
            prod = t * x["y"].permute(0, 3, 1, 2)
            out["ggamma"] = (prod.sum((0, 2, 3)), prod.abs().sum((0, 2, 3)))
    else:
        p = pixel_terms(name)
        gu, s = p["gu"], p["s_gu"] + p["gu"].abs()
        if c["kernel"] == "cf":
            out = {"gx": (gu, s), "gw": p["glw"], "gb": p["glb"]}
        else:
            flipped = torch.flip(x["dw_w"], (2, 3))
            gx = dwconv7_mag(gu, flipped, None)[0]
            m_gx = dwconv7_mag(s, flipped.abs(), None)[0]
            xp = F.pad(x["x"], (3, 3, 3, 3))
            gw, m_gw = torch.zeros(C, 1, 7, 7, dtype=torch.float64), torch.zeros(C, 1, 7, 7, dtype=torch.float64)
            for ky in range(7):
                for kx in range(7):
                    win = xp[:, :, ky:ky + H, kx:kx + W]
                    gw[:, 0, ky, kx] = (gu * win).sum((0, 2, 3))
                    m_gw[:, 0, ky, kx] = (s * win.abs()).sum((0, 2, 3))
            out = {"gx": (gx, m_gx), "gw": (gw, m_gw), "glw": p["glw"], "glb": p["glb"]}
            if c["bias"]:
                out["gb"] = (gu.sum((0, 2, 3)), s.sum((0, 2, 3)))
    out = {k: (np.ascontiguousarray(a.numpy()), np.ascontiguousarray(b.numpy())) for k, (a, b) in out.items()}
    for k, (val, mag) in out.items():
        assert np.isfinite(val).all() and np.isfinite(mag).all() and (mag >= 0).all(), (name, k)
        assert (mag[val != 0] > 0).all(), (name, k, "a positive magnitude wherever the value is not zero")
    return out


@functools.lru_cache(maxsize=2)
def reference(name):
    """{group: (value, mag)} of a case: computed once, shared, left unchanged."""
    return restate(name)


def groups_of(name):
    c = CASES[name]
    if c["kernel"] == "head":
        return tuple(g for g in GROUPS["head"] if g != "gb" or c["bias"])
    if c["kernel"] == "tail":
        return ("gy", "ggamma") if c["gamma"] else ("gy",)
    return GROUPS["cf"]


def exactly_zero(name, group):
    """layernorm_cf with one channel: gwv - m1 = 0 and xh = 0 in exact arithmetic"""
    c = CASES[name]
    return c["kernel"] == "cf" and c["C"] == 1 and group in ("gx", "gw")


def _leaf(t, dtype, device):
    return None if t is None else t.detach().to(device=device, dtype=dtype).clone()


def _grads(name, dtype, device="cpu"):
    """{group: tensor} by autograd: float64 through tests/convnext_ref.py, float32 through PyTorch's own composition"""
    c, x = CASES[name], inputs(name)
    C = c["C"]
    zeros = torch.zeros(C, dtype=torch.float64)
    if c["kernel"] == "head":
        leaves = [_leaf(t, dtype, device) for t in (x["x"], x["dw_w"], x["dw_b"], x["ln_w"], zeros)]
        got = T.head_grads(leaves, _leaf(x["go"], dtype, device), dtype, eps=x["eps"])
        keys = {"x": "gx", "dw_weight": "gw", "dw_bias": "gb", "ln_weight": "glw", "ln_bias": "glb"}
    else:
        leaves = [_leaf(t, dtype, device) for t in (x["x"], x["ln_w"], zeros)]
        got = T.cf_grads(leaves, _leaf(x["go"], dtype, device), dtype, eps=x["eps"])
        keys = {"x": "gx", "weight": "gw", "bias": "gb"}
    return {keys[k]: v for k, v in got.items()}


def agrees_with_autograd(name):
    """The closed forms against float64 autograd through tests/convnext_ref.py, to 1e-12 of the group's scale: max(1, the
    largest value), or the largest magnitude for a LIFTED group.  The tail is two products and a sum: nothing to compare."""
    auto = _grads(name, torch.float64)
    mine = reference(name)
    assert sorted(auto) == sorted(mine) == sorted(groups_of(name)), name
    for k, want in auto.items():
        val, mag = mine[k]
        scale = float(mag.max()) if k in LIFTED.get(name, ()) else max(1.0, float(np.abs(val).max()))
        err = float(np.abs(val - want.numpy().reshape(val.shape)).max())
        assert err <= 1e-12 * scale, (name, k, err, scale)


def stress_property(name):
    """Asserts, on float64 quantities, the property that names a stress case (convnext_parity.stress_property's for the forward's)."""
    c, x = CASES[name], inputs(name)
    stress = c["stress"]
    if c["kernel"] == "tail":
        return
    v = dwconv7_mag(x["x"], x["dw_w"], x["dw_b"])[0] if c["kernel"] == "head" else x["x"]
    var = ((v - _m(v)) ** 2).mean(1)
    if stress == "offset":
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
    elif stress == "common":
        assert bool((x["ln_w"] == 1).all()), name
        go = x["go"].permute(0, 3, 1, 2) if c["kernel"] == "head" else x["go"]
        assert float(((go - _m(go)).abs() / go.abs()).max()) <= 2.0 ** -8, name
    else:
        assert stress == "plain" and x["eps"] == fp32(EPS)


def zero_variance_pixels(name):
    """[B, H, W] bool: the pixels whose float64 channel variance is exactly 0; there xh = 0 exactly, in the kernels too"""
    c, x = CASES[name], inputs(name)
    v = dwconv7_mag(x["x"], x["dw_w"], x["dw_b"])[0] if c["kernel"] == "head" else x["x"]
    return (((v - _m(v)) ** 2).mean(1) == 0).numpy()


# ------------------------------------------------------------------------------------------------------------- the composition

def composition(name, device="cpu"):
    """{group: float64 numpy} of the fp32 PyTorch composition on `device`; it never runs the kernels.  The head: autograd of
    F.conv2d + F.layer_norm.  layernorm_cf: autograd of the module's written-out channels-first expressions
    (convnext_train_cases.cf_grads).  The tail: the two products and the sum."""
    c, x = CASES[name], inputs(name)
    if c["kernel"] == "tail":
        dev = lambda t: None if t is None else t.float().to(device)
        go, y, gamma, s = dev(x["go"]), dev(x["y"]), dev(x["gamma"]), dev(x["scale"])
        t = go if s is None else go * s.view(-1, 1, 1, 1)
        got = {"gy": (t if gamma is None else t * gamma.view(1, -1, 1, 1)).permute(0, 2, 3, 1)}
        if gamma is not None:
            got["ggamma"] = (t * y.permute(0, 3, 1, 2)).sum((0, 2, 3))
    else:
        got = _grads(name, torch.float32, device)
    ref = reference(name)
    for k, v in got.items():
        assert v.dtype == torch.float32, (name, k)
    return {k: v.detach().cpu().double().contiguous().numpy().reshape(ref[k][0].shape) for k, v in got.items()}


# ---------------------------------------------------------------------------------------------------------- the error measure

HEAD = "%-34s %-6s %10s %10s %10s %8s" % ("case", "group", "kernel err", "comp err", "bound", "ratio")
_T = PM.Table(HEAD, env="CONVNEXT_BWD_PARITY_TABLE")
TABLE, WORST, report = _T.lines, _T.worst, _T.report        # WORST: (kernel, group) -> (ratio, table line)


def tol(want):
    return TOL * max(1.0, float(np.abs(want).max()) if want.size else 0.0)


def measure(case, what, got, want, mag, comp, check=True):
    """Every entry of `got` within entry_bound(the composition's error at the entry, its magnitude) of `want`, and the project's
    bound on top (TOL of max(1, the group's largest value); none for a LIFTED group).  A group that is exactly zero in float64
    (exactly_zero) must be zero in every entry.  Returns the largest error / bound; check=False only returns it (inf for a
    non-finite entry, or a non-zero one where zero is exact) and adds no line.
    WORST: (kernel, group).  Line: case, group, the worst entry's kernel error, composition error and bound, each relative to
    the entry's MAGNITUDE, and their ratio."""
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    got = got.reshape(want.shape) if got.size == want.size else got
    assert got.shape == want.shape == comp.shape == mag.shape, (case, what, got.shape, want.shape, comp.shape, mag.shape)
    assert np.isfinite(want).all() and np.isfinite(comp).all() and (mag >= 0).all(), (case, what)
    kernel = CASES[case]["kernel"]
    if exactly_zero(case, what):
        assert not want.any(), (case, what, "the restatement is exactly zero")
        bad = np.argwhere(got != 0)
        if check:
            assert bad.size == 0, (case, what, "entries that must be exactly zero", len(bad), bad[:8].tolist())
            _T.add("%-34s %-6s %10s %10s %10s %8s" % (case, what, "0", "-", "exact", "0.000"), (kernel, what), 0.0)
        return float("inf") if bad.size else 0.0
    if not np.isfinite(got).all():
        assert not check, (case, what, "non-finite entries", np.argwhere(~np.isfinite(got))[:8].tolist())
        return float("inf")
    e = PM.errors(got, want, mag, comp)
    if not check:
        return e.worst
    i = e.at
    unit = mag[i] or 1.0
    _T.add("%-34s %-6s %10.2e %10.2e %10.2e %8.3f" % (case, what, e.err[i] / unit, e.cerr[i] / unit, e.bound[i] / unit, e.ratio[i]),
           (kernel, what), e.worst)
    e.check(case, what)
    if what not in LIFTED.get(case, ()):
        assert float(e.err.max()) <= tol(want), (case, what, "the project's bound", float(e.err.max()), tol(want))
    return e.worst


def old_bound_passes(got, want):
    """The one number per tensor of tests/test_convnext_train_gpu.py: max abs error below 1e-4 * max(1, max|ref|)."""
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    return bool(np.isfinite(got).all()) and float(np.abs(got - want).max()) < tol(want)


def worst_table():
    return "\n".join("%-5s %-6s %s" % (k[0], k[1], WORST[k][1]) for k in sorted(WORST))
