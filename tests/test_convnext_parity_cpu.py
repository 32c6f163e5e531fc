"""No GPU: the error measure of tests/convnext_parity.py has teeth.

A fp32 emulation of the kernels' own schemes, written from their description in uninext_amd/csrc/convnext.hip -- dwconv_ln: one
fmaf chain per convolution output, the bias first and the taps in (ky, kx) order, then per pixel the mean and the sum of squared
deviations in two passes with dwconv_ln's grouping (vectors of four channels, (v0 + v1) + (v2 + v3), lane l of 64 adding the
vectors l, l + 64, ... in order, a butterfly over the lanes, times 1 / C); layernorm_cf: 1024 / PX parts, part k adding the
channels k, k + parts, ... in order, the partial sums added in part order, a division by sqrt(var + eps) -- is held to the
measure against the float64 restatement with the fp32 PyTorch composition on the CPU as `comp`.  The correct emulation stays
within the bound on EVERY case of the sweep, with the magnitude as derived (no term had to be added), and each wrong variant
is over it on the case named in WRONG.  The restatements agree with tests/convnext_ref.py to 1e-12 of the output's largest
value, and the restated tile rule reproduces the tiles of the existing HEAD_CASES and WIDE_HEAD_CASES.

Worst error / bound of the correct emulation over the sweep: 0.185 (the head at C = 768, `offset`; head 0.18 at C = 32, 96,
768 and 1536, layernorm_cf 0.079, the tail 0: it is bitwise the composition).  Of each wrong variant on its named cases (inf: NaN
where a number belongs), and whether the OLD one-number bound of tests/test_convnext_gpu.py, max abs error < 1e-4 * max(1,
max|ref|), passes the variant on that case:
    (a) one_pass       head/C96_B3_11x23/offset    37        old bound fails
                       cf/C768_B3_HW67/offset      89        fails
    (b) no_eps         head/C96_B3_11x23/loweps    inf       fails
                       head/C96_B3_11x23/bigeps    5.6e+04   fails
                       cf/C512_B3_HW131/loweps     inf       fails
                       cf/C512_B3_HW131/bigeps     1.8e+04   fails
                       head/C96_B3_11x23/floor     27        fails
                       cf/C512_B3_HW131/floor      9.8       PASSES
    (c) eps_outside    head/C96_B3_11x23/loweps    1.3e+03   fails
                       cf/C512_B3_HW131/bigeps     4.0e+04   fails
                       cf/C512_B3_HW131/floor      7.6       PASSES
    (d) c_minus_1      cf/C2_B3_HW131/plain        6.9e+04   fails
                       cf/C15_B1_HW65/plain        8.4e+03   fails
                       head/C32_B3_3x20/plain      2.8e+03   fails
    (e) miss_tail      head/C96_B3_11x23/plain     2.1e+08   fails
                       head/C384_B1_13x10/plain    4.3e+04   fails
    (f) replicate_pad  head/C32_B3_3x20/plain      5.8e+05   fails
                       head/C192_B1_9x5/plain      5.9e+05   fails
The offsets of the `offset` stress (512 in dw_bias over a sigma of 1.4, 1024 in x over a sigma of 2) are sized so that the
one-pass variance (a) exceeds its bound by more than 10 x on both kernels (37 x and 89 x, asserted), while the correct scheme
still meets the project's bound there.  The old bound is blind to (b) and (c), a dropped or misplaced eps, on layernorm_cf at
the variance floor it allowed (`floor`, C = 512 and C = 768: test_which_wrong_variants_the_old_bound_lets_through); (a), (d),
(e) and (f) it rejects wherever the measure does on the cases searched there -- they were gaps of the old CASES (no offset, no
C = 384 head on its own), not of the old bound.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnext_cases as CC     # noqa: E402
import convnext_parity as P     # noqa: E402

F32 = np.float32
SWITCHES = ("one_pass", "no_eps", "eps_outside", "c_minus_1", "miss_tail", "replicate_pad")

# variant -> the cases of the sweep on which it must exceed the bound
WRONG = {
    "one_pass": ("head/C96_B3_11x23/offset", "cf/C768_B3_HW67/offset"),             # (a)
    "no_eps": ("head/C96_B3_11x23/loweps", "head/C96_B3_11x23/bigeps", "cf/C512_B3_HW131/loweps", "cf/C512_B3_HW131/bigeps",
               "head/C96_B3_11x23/floor", "cf/C512_B3_HW131/floor"),                   # (b)
    "eps_outside": ("head/C96_B3_11x23/loweps", "cf/C512_B3_HW131/bigeps", "cf/C512_B3_HW131/floor"),      # (c)
    "c_minus_1": ("cf/C2_B3_HW131/plain", "cf/C15_B1_HW65/plain", "head/C32_B3_3x20/plain"),                # (d)
    "miss_tail": ("head/C96_B3_11x23/plain", "head/C384_B1_13x10/plain"),           # (e) 24 and 96 vectors: 0 and 1 full trips
    "replicate_pad": ("head/C32_B3_3x20/plain", "head/C192_B1_9x5/plain"),          # (f)
}
# the variants that pass the OLD bound on a case where the measure rejects them, and that case: the gap was real for these
OLD_BOUND_BLIND = {"no_eps": "cf/C512_B3_HW131/floor", "eps_outside": "cf/C512_B3_HW131/floor"}


# ------------------------------------------------------------------------------------------------------------- the emulation

def _f32(t):
    return None if t is None else t.numpy().astype(F32)


def conv_chain(x, w, b, replicate=False):
    """[B, C, H, W] fp32: acc = bias; acc = fmaf(x, w, acc) over the taps in (ky, kx) order.  Inputs are multiples of 2^-10
    below 2^13, so every product and every sum is exact in float64 and the one rounding to fp32 is fmaf's."""
    B, C, H, W = x.shape
    xp = TF.pad(x, (3, 3, 3, 3), mode="replicate") if replicate else TF.pad(x, (3, 3, 3, 3))
    acc = torch.zeros(B, C, H, W, dtype=torch.float32) if b is None else b.float().view(1, C, 1, 1).expand(B, C, H, W).contiguous()
    for ky in range(7):
        for kx in range(7):
            acc = torch.addcmul(acc.double(), xp[:, :, ky:ky + H, kx:kx + W], w[:, 0, ky, kx].view(1, C, 1, 1)).float()
    return acc.numpy()


def wave_sum(a):
    """[N, 64] -> [N]: v += shfl_xor(v, o) for o = 32 .. 1"""
    n = 64
    while n > 1:
        n //= 2
        a = a[:, :n] + a[:, n:2 * n]
    assert a.dtype == F32
    return a[:, 0]


def lane_sums(part, trips):
    """part [N, nvec] -> [N, 64]: lane l adds the vectors l, l + 64, ... of the first `trips` trips, in order"""
    N, nvec = part.shape
    pad = (-nvec) % 64
    t = np.concatenate((part, np.zeros((N, pad), F32)), 1).reshape(N, -1, 64)
    acc = np.zeros((N, 64), F32)
    for k in range(min(trips, t.shape[1])):
        acc = acc + t[:, k]
    return acc


def sd_of(var, eps, sw):
    """sqrt(var + eps), or what a wrong variant makes of it"""
    eps = F32(eps)
    with np.errstate(invalid="ignore"):
        return np.sqrt(var) if "no_eps" in sw else np.sqrt(var) + eps if "eps_outside" in sw else np.sqrt(var + eps)


def head_norm(v, g, b, eps, sw):
    """v [N, C] fp32 (the LDS plane of N pixels) -> [N, C]: dwconv_ln's LayerNorm, one wave per pixel"""
    N, C = v.shape
    q = v.reshape(N, C // 4, 4)
    nvec = C // 4
    trips = nvec // 64 if "miss_tail" in sw else -(-nvec // 64)
    inv_c = F32(1) / F32(C - 1 if "c_minus_1" in sw else C)
    mean = wave_sum(lane_sums((q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3]), trips)) * (F32(1) / F32(C))
    if "one_pass" in sw:
        s = q * q
        var = wave_sum(lane_sums((s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3]), trips)) * inv_c - mean * mean
    else:
        d = q - mean[:, None, None]
        s = d * d
        var = wave_sum(lane_sums((s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3]), trips)) * inv_c
    with np.errstate(invalid="ignore", divide="ignore"):
        rstd = F32(1) / sd_of(var, eps, sw)
        out = (v - mean[:, None]) * rstd[:, None] * g[None, :] + b[None, :]
    assert out.dtype == F32
    return out


def emulate_head(name, sw=()):
    c, x = P.CASES[name], P.inputs(name)
    B, C, H, W = c["B"], c["C"], c["H"], c["W"]
    v = conv_chain(x["x"], x["dw_w"], x["dw_b"], "replicate_pad" in sw)
    plane = np.ascontiguousarray(v.transpose(0, 2, 3, 1)).reshape(B * H * W, C)
    return head_norm(plane, _f32(x["ln_w"]), _f32(x["ln_b"]), x["eps"], sw).reshape(B, H, W, C)


def part_sums(t, parts):
    """t [B, C, N] -> [B, N]: part k adds the channels k, k + parts, ... in order; the parts are added in part order"""
    B, C, N = t.shape
    pad = (-C) % parts
    t = np.concatenate((t, np.zeros((B, pad, N), F32)), 1).reshape(B, -1, parts, N)
    acc = np.zeros((B, parts, N), F32)
    for k in range(t.shape[1]):
        acc = acc + t[:, k]
    tot = np.zeros((B, N), F32)
    for k in range(parts):
        tot = tot + acc[:, k]
    assert tot.dtype == F32
    return tot


def emulate_cf(name, sw=()):
    c, x = P.CASES[name], P.inputs(name)
    B, C, H, W = c["B"], c["C"], c["H"], c["W"]
    parts = 1024 // P.cf_rule(C)[0]
    t = _f32(x["x"]).reshape(B, C, H * W)
    g, b = _f32(x["ln_w"])[None, :, None], _f32(x["ln_b"])[None, :, None]
    div = F32(max(C - 1, 1) if "c_minus_1" in sw else C)
    u = part_sums(t, parts) / F32(C)
    if "one_pass" in sw:
        var = part_sums(t * t, parts) / div - u * u
    else:
        d = t - u[:, None, :]
        var = part_sums(d * d, parts) / div
    with np.errstate(invalid="ignore", divide="ignore"):
        out = g * ((t - u[:, None, :]) / sd_of(var, x["eps"], sw)[:, None, :]) + b
    assert out.dtype == F32
    return out.reshape(B, C, H, W)


def emulate_tail(name, sw=()):
    x = P.inputs(name)
    y, inp, gamma = _f32(x["y"]), _f32(x["inp"]), _f32(x["gamma"])
    return inp + (y if gamma is None else gamma * y).transpose(0, 3, 1, 2)


EMULATE = {"head": emulate_head, "cf": emulate_cf, "tail": emulate_tail}


def run(name, sw=(), check=True):
    """(error / bound of the emulation under the measure, whether the old one-number bound passes it)"""
    want, mag = P.reference(name)
    got = EMULATE[P.CASES[name]["kernel"]](name, sw).astype(np.float64)
    return P.measure(name, got, want, mag, P.composition(name, "cpu"), check=check), P.old_bound_passes(got, want)


def agrees_with_the_existing_restatement(name):
    want = P.reference(name)[0]
    assert np.abs(P.existing_restatement(name) - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), name


def _chunks():
    """the sweep in pieces, so that no test takes long: the head by channel count, layernorm_cf and the tail whole"""
    out = [pytest.param("head", C, id="head-C%d" % C) for C in (32, 96, 192, 384, 768, 1536)]
    return out + [pytest.param("cf", None, id="cf"), pytest.param("tail", None, id="tail")]


# ------------------------------------------------------------------------------------------------------------------ the tests

@pytest.mark.parametrize("kernel,C", _chunks())
def test_correct_emulation_within_the_bound_and_restatements_agree(kernel, C):
    since = len(P.TABLE)
    worst = 0.0
    for name in (P.names(kernel) if C is None else P.names(kernel, C=C)):
        agrees_with_the_existing_restatement(name)
        P.stress_property(name)
        ratio, old = run(name)
        assert old, name
        worst = max(worst, ratio)
        if P.CASES[name]["stress"] == "loweps":                     # variance exactly 0: ln_bias, bitwise
            zero = P.zero_variance_pixels(name)
            assert zero.any()
            got = EMULATE[kernel](name)
            b = P.inputs(name)["ln_b"].numpy().astype(F32)
            rows = got[zero] if kernel == "head" else got.transpose(0, 2, 3, 1)[zero]
            assert np.array_equal(rows.view(np.int32), np.broadcast_to(b, rows.shape).copy().view(np.int32)), name
    P.report(since)
    print("worst error / bound of the correct emulation: %.3f" % worst)
    assert worst <= 1.0


def test_every_case_of_the_issue_is_in_the_sweep():
    classes = set()
    for name in P.names("head"):
        c = P.CASES[name]
        tile = P.choose_tile(c["B"], c["C"], c["H"], c["W"])
        assert tile == c["tile"], (name, tile)
        assert P.head_kernel(c["B"], c["C"], c["H"], c["W"]) == "convnext_dwconv_ln<%d>" % tile[1]
        if tile[0] == P.tallest(c["C"], tile[1]):                   # the tile is as tall as the LDS allows, not as the map does
            classes.add((c["C"], tile[1], tile[0]))
            if tile[1] > 4 and not (c["C"] == 1536 and tile[1] == 8):
                assert c["H"] % tile[0] and c["W"] % tile[1], name
    want = {(C, tw, P.tallest(C, tw)) for C in (32, 96, 192, 384, 768, 1536) for tw in P.WIDTHS}
    assert classes == want, sorted(want - classes)
    assert {(tw, th) for C, tw, th in want if C == 768} == {(4, 8), (7, 6), (8, 5)}
    assert {(tw, th) for C, tw, th in want if C == 1536} == {(4, 5), (7, 3), (8, 2)}
    assert all(th == 8 for C, tw, th in want if C <= 384)
    # <8> at C = 1536 is out of reach of every map taller than 2 (rows up to 40, widths up to 4000 here)
    assert not any(P.choose_tile(1, 1536, H, W) == (2, 8) for H in range(3, 41) for W in range(9, 4000, 7))
    assert P.choose_tile(1, 1536, 2, 1793) == (2, 8) and P.choose_tile(1, 1536, 2, 1785) != (2, 8)      # the smallest W
    for hw in ((1, 1), (3, 20), (20, 3)):
        assert any((P.CASES[n]["H"], P.CASES[n]["W"]) == hw for n in P.names("head"))
    for th in (8, 5):                                               # H = th + 1 with W = TW + 1
        assert any(P.CASES[n]["tile"] == (th, 4) and (P.CASES[n]["H"], P.CASES[n]["W"]) == (th + 1, 5) for n in P.names("head"))
    for flag in (True, False):
        assert {1, 3} <= {P.CASES[n]["B"] for n in P.names("head", bias=flag)}
    for group in ((32, 96, 192, 384), (768,), (1536,)):             # every stress on a narrow and a wide class per C group
        for s in P.STRESSES:
            tws = {P.CASES[n]["tile"][1] for n in P.names("head", stress=s) if P.CASES[n]["C"] in group}
            assert 4 in tws and tws - {4}, (group, s)
    assert [P.cf_rule(C) for C in P.CF_CS] == [(64, True)] * 6 + [(32, True)] * 3 + [(16, True)] * 2 + [(64, False)]
    assert [P.cf_rule(C)[0] for C in P.CF_STRESSED] == [64, 32, 16, 64] and not P.cf_rule(2049)[1]
    for C in P.CF_CS:
        PX = P.cf_rule(C)[0]
        assert {(P.CASES[n]["B"], P.CASES[n]["W"]) for n in P.names("cf", C=C, stress="plain")} == \
            {(B, HW) for B in (1, 3) for HW in (1, PX - 1, PX, PX + 1, 2 * PX + 3)}
    assert len(P.names("tail")) == 50 and "tail/C64_HW64/gamma" in P.CASES and "tail/C65_HW65/nogamma" in P.CASES
    for cases in list(WRONG.values()) + [OLD_BOUND_BLIND.values()]:
        for name in cases:
            assert name in P.CASES, name


def test_tile_rule_reproduces_the_existing_cases():
    """Every HEAD_CASES entry takes <4>, as tests/convnext_cases.py says, and every WIDE_HEAD_CASES entry the kernel it names."""
    for c, B, H, W, _ in CC.HEAD_CASES:
        assert P.head_kernel(B, c, H, W) == "convnext_dwconv_ln<4>", (c, B, H, W)
        assert P.choose_tile(B, c, H, W)[0] == P.tallest(c, 4, H)
    for c, B, H, W, _, kernel in CC.WIDE_HEAD_CASES:
        assert P.head_kernel(B, c, H, W) == kernel, (c, B, H, W)
    assert {(c, P.choose_tile(B, c, H, W)) for c, B, H, W, _, _ in CC.WIDE_HEAD_CASES} >= {(384, (8, 7)), (768, (6, 7))}
    assert [P.choose_tile(2, c, H, W) for c, H, W in CC.LARGE_STAGES] == [(8, 8), (8, 7), (6, 7), (5, 4)]      # DESIGN.md's


@pytest.mark.parametrize("variant", SWITCHES)
def test_wrong_variant_exceeds_the_bound_on_its_named_cases(variant):
    for name in WRONG[variant]:
        assert run(name)[0] <= 1.0                                  # the correct emulation passes the same case
        ratio, old = run(name, (variant,), check=False)
        print("%-14s %-28s error / bound %-9.3g old bound %s" % (variant, name, ratio, "passes" if old else "fails"))
        assert ratio > 1.0, (variant, name, ratio)
        if variant == "one_pass":
            assert ratio > 10.0, (name, ratio)                      # what the offsets are sized for


def test_which_wrong_variants_the_old_bound_lets_through():
    """Over the cases that carry a stress and the named ones: the variants that some case shows to the measure and hides from the
    old one-number bound are exactly those of OLD_BOUND_BLIND, each on the case named there."""
    pool = sorted({n for cases in WRONG.values() for n in cases} | {n for n in P.CASES if P.CASES[n]["stress"] != "plain"
                                                                   and P.CASES[n]["C"] <= (768 if n.startswith("cf/") else 96)})
    blind = {}
    for variant in SWITCHES:
        for name in pool:
            if variant == "replicate_pad" and P.CASES[name]["kernel"] != "head":
                continue
            ratio, old = run(name, (variant,), check=False)
            if ratio > 1.0 and old:
                blind.setdefault(variant, []).append((name, ratio))
    for variant, found in blind.items():
        print("%-14s passes the old bound, error / bound under the measure: %s" % (variant, ", ".join("%s %.3g" % f for f in found)))
    assert set(blind) == set(OLD_BOUND_BLIND), sorted(blind)
    for variant, name in OLD_BOUND_BLIND.items():
        assert name in [n for n, _ in blind[variant]], (variant, name)
