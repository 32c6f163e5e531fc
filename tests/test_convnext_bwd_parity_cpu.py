"""No GPU: the error measure of tests/convnext_bwd_parity.py has teeth.

A numpy fp32 emulation of the backward kernels, written from the header comment of uninext_amd/csrc/convnext_bwd.hip.  The head,
pass one: the forward's fmaf tap chains and two-pass statistics (tests/test_convnext_parity_cpu.py's), gwv = go * lw rounded on
its own, a lane's sums of gwv and gwv * xh over its vectors of four channels in order, a butterfly over the lanes, times 1 / C;
grad_u = rstd * (gwv - m1 - xh * m2); per workgroup (a th x TW tile of the forward's tiling) the fp32 sums of go and go * xh
along a tile row, the rows added in row order.  Pass two: grad_x as a 49-tap fmaf chain over grad_u with the mirrored weights
and a zero halo; per band of 8 x 8 tiles the 49 weight sums and the bias sum of (channel, tile row) as fmaf chains over the
row's eight pixels, tile after tile, then the eight rows in row order.  layernorm_cf: 16 parts of the channels added in part
order, divisions by sd, a butterfly over a block's 64 pixels.  The tail: (go * s) * gamma, and per block of 64 pixels four
fmaf chains of 16 pixels, added in order.  Every family's partial rows are added in float64 in eight interleaved runs, the runs
in order, rounded once (reduce_partials).

The correct emulation stays within the bound on every group of every case of SUBSET (the stress maps with every stress, the
edge maps, the narrow classes, two band cases with more than a tile a band; every layernorm_cf and tail case), with the
magnitudes as derived, no term added: worst error / bound head gx 0.023, gw 0.018, gb 0.013, glw 0.014, glb 0.006; cf gx 0.104,
gw 0.028, gb 0.000; tail gy 0.054, ggamma 0.125.  The closed forms agree with float64 autograd through tests/convnext_ref.py to
1e-12 on every case of at most 300 k input entries, every stress property holds, every case's tile and band triple are as
listed.

Each wrong variant is over the bound on its named cases (WRONG), where the correct emulation passes.  The largest error / bound
over the groups (inf: NaN where a number belongs, or a non-zero entry where zero is exact), the group, and whether the OLD
one-number bound of tests/test_convnext_train_gpu.py (max abs error < 1e-4 * max(1, max|ref|) per tensor) passes every tensor
of the variant on that case:
    no_eps            head/C96_B3_11x23/loweps     inf       gx      old bound fails
                      head/C96_B3_11x23/bigeps     1.9e+04   gx      fails
                      head/C96_B3_11x23/floor      9.1       gx      PASSES
                      cf/C512_B3_HW131/floor       9.3       gx      PASSES
    eps_outside       head/C96_B3_11x23/loweps     2.0e+06   gx      fails
                      cf/C513_B3_HW131/bigeps      3.9e+04   gx      fails
                      cf/C512_B3_HW131/floor       7.2       gx      PASSES
    one_pass          head/C96_B3_11x23/offset     15.6      gx      fails
                      cf/C513_B3_HW131/offset      153       gx      fails
    no_m2             head/C96_B3_11x23/plain      9.0e+03   gx      fails
                      cf/C2_B1_HW513/plain         8.5e+04   gx      fails
    fused_gw          cf/C1_B3_HW65_go512/plain    inf       gx      fails
    no_mirror         head/C32_B3_7x9/plain        1.1e+05   gx      fails
                      head/C96_B3_11x23/plain      1.5e+05   gx      fails
    replicate_halo    head/C32_B3_3x20/plain       3.1e+05   gx      fails
                      head/C96_B1_9x11/plain       2.1e+05   gx      fails
    skip_last_band    head/C768_B3_17x17/plain     1.4e+03   gw      fails
                      head/C768_B3_9x25/plain      3.6e+03   gw      fails
    band_off_by_one   head/C768_B3_17x17/plain     1.0e+04   gw      fails
                      head/C1536_B1_17x25/plain    1.6e+04   gw      fails
    bias_oob_columns  head/C32_B1_8x10/plain       1.0e+04   gb      fails
                      head/C96_B3_11x23/plain      1.7e+03   gb      fails
    reduce_first8     cf/C2_B1_HW513/plain         3.4e+03   gb      fails
                      head/C768_B3_17x17/plain     1.3e+05   glb     fails
    tail_no_scale     tail/C65_HW129/gamma_drop    2.1e+05   ggamma  fails
The old bound is blind to a dropped or misplaced eps at the variance floor it allowed (`floor`: OLD_BOUND_BLIND, asserted both
ways); the other variants it rejects wherever the measure does -- they were gaps of the old CASES (no stress, no band of more
than a tile with a guard behind the workspace, no partial-row counts), not of the old bound.  fused_gw (mean_C taken of the
rounded gwv, the subtraction fed the fused product) cannot show on the sweep's ordinary inputs at all: the product of two
multiples of 2^-10 of this size is exact in fp32, fused or not.  The one case whose grad_out is 512 times as large
(cf/C1_B3_HW65_go512) makes the product round, and C = 1 turns the difference into a non-zero entry where zero is exact.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnext_bwd_parity as P             # noqa: E402
import test_convnext_parity_cpu as FE       # noqa: E402  (the forward's emulation: conv_chain, wave_sum, lane_sums, part_sums, sd_of)

F32, F64 = np.float32, np.float64
SWITCHES = ("no_eps", "eps_outside", "one_pass", "no_m2", "fused_gw", "no_mirror", "replicate_halo", "skip_last_band",
            "band_off_by_one", "bias_oob_columns", "reduce_first8", "tail_no_scale")

# variant -> the cases of the sweep on which it must exceed the bound
WRONG = {
    "no_eps": ("head/C96_B3_11x23/loweps", "head/C96_B3_11x23/bigeps", "head/C96_B3_11x23/floor", "cf/C512_B3_HW131/floor"),
    "eps_outside": ("head/C96_B3_11x23/loweps", "cf/C513_B3_HW131/bigeps", "cf/C512_B3_HW131/floor"),
    "one_pass": ("head/C96_B3_11x23/offset", "cf/C513_B3_HW131/offset"),
    "no_m2": ("head/C96_B3_11x23/plain", "cf/C2_B1_HW513/plain"),
    "fused_gw": ("cf/C1_B3_HW65_go512/plain",),         # C = 1: gwv - m1 is exactly 0 only if both see the same gwv
    "no_mirror": ("head/C32_B3_7x9/plain", "head/C96_B3_11x23/plain"),
    "replicate_halo": ("head/C32_B3_3x20/plain", "head/C96_B1_9x11/plain"),
    "skip_last_band": ("head/C768_B3_17x17/plain", "head/C768_B3_9x25/plain"),
    "band_off_by_one": ("head/C768_B3_17x17/plain", "head/C1536_B1_17x25/plain"),
    "bias_oob_columns": ("head/C32_B1_8x10/plain", "head/C96_B3_11x23/plain"),
    "reduce_first8": ("cf/C2_B1_HW513/plain", "head/C768_B3_17x17/plain"),
    "tail_no_scale": ("tail/C65_HW129/gamma_drop",),
}
# the variants that pass the OLD bound on cases where the measure rejects them, and those cases
OLD_BOUND_BLIND = {"no_eps": ("head/C96_B3_11x23/floor", "cf/C512_B3_HW131/floor"), "eps_outside": ("cf/C512_B3_HW131/floor",)}

SUBSET = (P.names("head", group="stress") + P.names("head", group="edge") +
          ["head/C%d_B%d_%dx%d/plain" % c[:4] for c in P.TILE_NARROW] + ["head/C768_B3_17x17/plain", "head/C1536_B1_17x25/plain"] +
          P.names("cf") + P.names("tail"))


# ------------------------------------------------------------------------------------------------------------- the emulation

def f32(t):
    return None if t is None else t.numpy().astype(F32)


def fma32(a, b, c):
    """a b + c rounded once (the product of two fp32 numbers is exact in float64)"""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def reduce_partials(part, sw=()):
    """part [n, cols] fp32 -> [cols] fp32: run g adds the rows g, g + 8, .. in float64, the runs are added in order"""
    if "reduce_first8" in sw:
        part = part[:8]
    total = np.zeros(part.shape[1], F64)
    for g in range(8):
        run = np.zeros(part.shape[1], F64)
        for row in part[g::8]:
            run = run + row.astype(F64)
        total = total + run if g else run
    return total.astype(F32)


def lane_seq(a):
    """a [N, C] -> [N, 64]: lane l adds the four channels of its vectors l, l + 64, .. one by one"""
    N, C = a.shape
    nvec = C // 4
    pad = (-nvec) % 64
    q = np.concatenate((a.reshape(N, nvec, 4), np.zeros((N, pad, 4), F32)), 1).reshape(N, -1, 64, 4)
    acc = np.zeros((N, 64), F32)
    for k in range(q.shape[1]):
        for e in range(4):
            acc = acc + q[:, k, :, e]
    return acc


def pixel_stats(v, eps, sw):
    """v [N, C] -> (mean, rstd) [N]: convnext_common.hpp's pixel_stats, or what a wrong variant makes of it"""
    N, C = v.shape
    q = v.reshape(N, C // 4, 4)
    trips = -(-(C // 4) // 64)
    inv_c = F32(1) / F32(C)
    quad = lambda s: FE.wave_sum(FE.lane_sums((s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3]), trips)) * inv_c
    mean = quad(q)
    if "one_pass" in sw:
        var = quad(q * q) - mean * mean
    else:
        d = q - mean[:, None, None]
        var = quad(d * d)
    with np.errstate(invalid="ignore", divide="ignore"):
        return mean, F32(1) / FE.sd_of(var, eps, sw)


def grad_u(gwv, go, lw, m1, xh, m2, sw):
    """gwv - m1 - xh * m2 in fp32, or the wrong variants' """
    first = (go.astype(F64) * lw.astype(F64) - m1.astype(F64)).astype(F32) if "fused_gw" in sw else gwv - m1
    with np.errstate(invalid="ignore"):
        return first if "no_m2" in sw else first - xh * m2


def tile_sums(a, th, tw):
    """a [B, H, W, C] -> [workgroups, C]: per th x tw tile, a row's entries added in order, then the rows in order"""
    B, H, W, C = a.shape
    ty, tx = -(-H // th), -(-W // tw)
    p = np.zeros((B, ty * th, tx * tw, C), F32)
    p[:, :H, :W] = a
    p = p.reshape(B, ty, th, tx, tw, C)
    rows = np.zeros((B, ty, th, tx, C), F32)
    for j in range(tw):
        rows = rows + p[:, :, :, :, j]
    out = np.zeros((B, ty, tx, C), F32)
    for r in range(th):
        out = out + rows[:, :, r]
    return out.reshape(B * ty * tx, C)


def band_sums(gu, x, tiles_per_band, sw):
    """gu, x [B, C, H, W] fp32 -> (pw [bands, C, 49], pb [bands, C]): pass two's fp32 sums of a band of 8 x 8 tiles"""
    B, C, H, W = gu.shape
    ty, tx = -(-H // 8), -(-W // 8)
    total = B * ty * tx
    gp = np.zeros((B, C, ty * 8, tx * 8), F32)
    gp[:, :, :H, :W] = gu
    gb = gp
    if "bias_oob_columns" in sw:            # the bias sum reads the columns past W as memory has them: the next row's first ones
        flat = np.concatenate((gu.reshape(B, C, H * W), np.zeros((B, C, tx * 8), F32)), 2)
        gb = np.zeros_like(gp)
        for h in range(H):
            gb[:, :, h] = flat[:, :, h * W:h * W + tx * 8]
    xp = np.zeros((B, C, ty * 8 + 6, tx * 8 + 6), F32)
    xp[:, :, 3:3 + H, 3:3 + W] = x
    cut = lambda a, n: np.stack([a[b, :, y * 8:y * 8 + n, z * 8:z * 8 + n] for b in range(B) for y in range(ty) for z in range(tx)] +
                                [np.zeros((C, n, n), F32)])
    gt, bt, xt = cut(gp, 8), cut(gb, 8), cut(xp, 14)                     # [tiles + 1, C, ..]: the last one is no tile, zeros
    win = np.lib.stride_tricks.sliding_window_view(xt, (7, 7), axis=(2, 3))     # [tiles + 1, C, 8, 8, 7, 7]
    bands = -(-total // tiles_per_band)
    if "skip_last_band" in sw:
        bands -= 1
    start = np.arange(bands) * tiles_per_band
    end = np.minimum(start + tiles_per_band + (1 if "band_off_by_one" in sw else 0), total)
    aw, ab = np.zeros((bands, C, 8, 49), F32), np.zeros((bands, C, 8), F32)
    for p in range(int((end - start).max())):
        idx = np.where(start + p < end, start + p, total)
        for j in range(8):
            ab = ab + bt[idx][:, :, :, j]
        for j in range(8):
            aw = fma32(gt[idx][:, :, :, j, None], win[idx][:, :, :, j].reshape(bands, C, 8, 49), aw)
    pw, pb = np.zeros((bands, C, 49), F32), np.zeros((bands, C), F32)
    for r in range(8):
        pw, pb = pw + aw[:, :, r], pb + ab[:, :, r]
    return pw, pb


def emulate_head(name, sw=(), keep=None):
    """{group: fp32 array}, and "xh" [B, H, W, C]; keep [B, H, W] bool: grad_out is zeroed on the other pixels"""
    c, x = P.CASES[name], P.inputs(name)
    B, C, H, W = c["B"], c["C"], c["H"], c["W"]
    th, tw = c["tile"]
    v = FE.conv_chain(x["x"], x["dw_w"], x["dw_b"])
    plane = np.ascontiguousarray(v.transpose(0, 2, 3, 1)).reshape(B * H * W, C)
    go, lw = f32(x["go"]).reshape(B * H * W, C), f32(x["ln_w"])
    if keep is not None:
        go = go * keep.reshape(-1, 1).astype(F32)
    mean, rstd = pixel_stats(plane, x["eps"], sw)
    inv_c = F32(1) / F32(C)
    with np.errstate(invalid="ignore", over="ignore"):
        xh = (plane - mean[:, None]) * rstd[:, None]
        gwv = go * lw[None]
        m1 = FE.wave_sum(lane_seq(gwv)) * inv_c
        m2 = FE.wave_sum(lane_seq(gwv * xh)) * inv_c
        gu = rstd[:, None] * grad_u(gwv, go, lw[None], m1[:, None], xh, m2[:, None], sw)
        part_b = tile_sums(go.reshape(B, H, W, C), th, tw)
        part_w = tile_sums((go * xh).reshape(B, H, W, C), th, tw)
    assert gu.dtype == F32 and part_w.dtype == F32
    out = {"glb": reduce_partials(part_b, sw), "glw": reduce_partials(part_w, sw), "xh": xh.reshape(B, H, W, C)}
    gu = np.ascontiguousarray(gu.reshape(B, H, W, C).transpose(0, 3, 1, 2))
    weights = x["dw_w"] if "no_mirror" in sw else torch.flip(x["dw_w"], (2, 3))
    with np.errstate(invalid="ignore"):
        out["gx"] = FE.conv_chain(torch.from_numpy(np.nan_to_num(gu, nan=0.0, posinf=0.0, neginf=0.0).astype(F64)), weights, None,
                                  "replicate_halo" in sw)
        if not np.isfinite(gu).all():
            out["gx"] = out["gx"] + np.where(np.isfinite(gu), F32(0), F32("nan"))
        pw, pb = band_sums(gu, f32(x["x"]), c["bands"][1], sw)
    out["gw"] = reduce_partials(pw.reshape(pw.shape[0], -1), sw).reshape(C, 1, 7, 7)
    if c["bias"]:
        out["gb"] = reduce_partials(pb, sw)
    return out


def emulate_cf(name, sw=(), keep=None):
    c, x = P.CASES[name], P.inputs(name)
    B, C, HW = c["B"], c["C"], c["H"] * c["W"]
    t, go, w = f32(x["x"]).reshape(B, C, HW), f32(x["go"]).reshape(B, C, HW), f32(x["ln_w"])[None, :, None]
    if keep is not None:
        go = go * keep.reshape(B, 1, HW).astype(F32)
    cf = F32(C)
    u = FE.part_sums(t, 16) / cf
    d = t - u[:, None, :]
    var = FE.part_sums(t * t, 16) / cf - u * u if "one_pass" in sw else FE.part_sums(d * d, 16) / cf
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        sd = FE.sd_of(var, x["eps"], sw)[:, None, :]
        xh = d / sd
        gwv = go * w
        m1, m2 = FE.part_sums(gwv, 16) / cf, FE.part_sums(gwv * xh, 16) / cf
        gx = grad_u(gwv, go, w, m1[:, None, :], xh, m2[:, None, :], sw) / sd
        blocks = -(-HW // 64)

        def wave(a):                                                    # [B, C, HW] -> [B * blocks, C]
            p = np.concatenate((a, np.zeros((B, C, blocks * 64 - HW), F32)), 2).reshape(B * C * blocks, 64)
            return FE.wave_sum(p).reshape(B, C, blocks).transpose(0, 2, 1).reshape(B * blocks, C)
        out = {"gx": gx.reshape(B, C, c["H"], c["W"]), "gb": reduce_partials(wave(go), sw), "gw": reduce_partials(wave(go * xh), sw),
               "xh": xh}
    assert gx.dtype == F32
    return out


def emulate_tail(name, sw=(), keep=None):
    c, x = P.CASES[name], P.inputs(name)
    B, C, HW = c["B"], c["C"], c["H"] * c["W"]
    go, y, gamma = f32(x["go"]).reshape(B, C, HW), f32(x["y"]).reshape(B, HW, C), f32(x["gamma"])
    t = go if x["scale"] is None else go * f32(x["scale"])[:, None, None]
    out = {"gy": (t if gamma is None else t * gamma[None, :, None]).transpose(0, 2, 1).reshape(B, c["H"], c["W"], C)}
    if gamma is not None:
        blocks = -(-HW // 64)
        pad = lambda a: np.concatenate((a, np.zeros((B, C, blocks * 64 - HW), F32)), 2).reshape(B, C, blocks, 16, 4)
        tt, yy = pad(go if "tail_no_scale" in sw else t), pad(np.ascontiguousarray(y.transpose(0, 2, 1)))
        acc = np.zeros((B, C, blocks, 4), F32)
        for k in range(16):
            acc = fma32(tt[:, :, :, k], yy[:, :, :, k], acc)
        s = acc[..., 0]
        for g in range(1, 4):
            s = s + acc[..., g]
        out["ggamma"] = reduce_partials(s.transpose(0, 2, 1).reshape(B * blocks, C), sw)
    return out


EMULATE = {"head": emulate_head, "cf": emulate_cf, "tail": emulate_tail}


def run(name, sw=(), check=True):
    """{group: (error / bound of the emulation under the measure, whether the old one-number bound passes it)}"""
    ref, comp = P.reference(name), P.composition(name, "cpu")
    got = EMULATE[P.CASES[name]["kernel"]](name, sw)
    assert sorted(k for k in got if k != "xh") == sorted(ref) == sorted(comp) == sorted(P.groups_of(name)), name
    return {k: (P.measure(name, k, got[k].astype(F64), want, mag, comp[k], check=check), P.old_bound_passes(got[k], want))
            for k, (want, mag) in ref.items()}


def worst(res):
    k = max(res, key=lambda g: res[g][0])
    return res[k][0], k, all(old for _, old in res.values())


# ------------------------------------------------------------------------------------------------------------------ the tests

def _chunks():
    out = [pytest.param("head", g, id="head-" + g) for g in ("stress", "edge", "tile", "band")]
    return out + [pytest.param("cf", None, id="cf"), pytest.param("tail", None, id="tail")]


@pytest.mark.parametrize("kernel,group", _chunks())
def test_correct_emulation_within_the_bound(kernel, group):
    since = len(P.TABLE)
    top = {}
    cases = [n for n in SUBSET if P.CASES[n]["kernel"] == kernel and (group is None or P.CASES[n]["group"] == group)]
    assert cases
    for name in cases:
        P.stress_property(name)
        for k, (ratio, old) in run(name).items():
            assert old or k in P.LIFTED.get(name, ()), (name, k)
            top[k] = max(top.get(k, 0.0), ratio)
        if P.CASES[name]["stress"] == "loweps":
            # variance exactly 0: xh is exactly 0 there, so grad_u = r (gwv - m1) and glw takes nothing from these pixels -- with
            # grad_out kept on them alone, glw (cf: gw) is exactly zero
            zero = P.zero_variance_pixels(name)
            assert zero.any() and not zero.all()
            got = EMULATE[kernel](name, keep=zero)
            xh = got["xh"][zero] if kernel == "head" else got["xh"].transpose(0, 2, 1).reshape(zero.shape + (-1,))[zero]
            assert not xh.any(), name
            assert not got["glw" if kernel == "head" else "gw"].any(), name
            assert got["glb" if kernel == "head" else "gb"].any(), name
    P.report(since)
    print("worst error / bound of the correct emulation: " + ", ".join("%s %.3f" % kv for kv in sorted(top.items())))
    assert max(top.values()) <= 1.0


def test_restatement_agrees_with_float64_autograd():
    ran = 0
    for name in P.names("head") + P.names("cf"):
        if P.entries(name) <= P.AUTOGRAD_LIMIT:
            P.agrees_with_autograd(name)
            ran += 1
    assert ran >= 93 + 30, ran
    for stress in P.STRESSES:       # every stress of both kernels is among them
        assert any(P.entries(n) <= P.AUTOGRAD_LIMIT for n in P.names("head", stress=stress)), stress
        assert any(P.entries(n) <= P.AUTOGRAD_LIMIT for n in P.names("cf", stress=stress)), stress


def test_every_case_of_the_issue_is_in_the_sweep():
    # pass one: every (C, TW) class at its tallest tile, the wide ones on the smallest map there is
    classes = {}
    for name in P.names("head"):
        c = P.CASES[name]
        assert c["tile"] == P.choose_tile(c["B"], c["C"], c["H"], c["W"]) and c["bands"] == P.T.head_bands(c["B"], c["C"], c["H"], c["W"]), name
        assert P.head_route(c["B"], c["C"], c["H"], c["W"]) == "convnext_dwconv_ln_backward<%d>" % c["tile"][1]
        if c["group"] == "tile" and c["tile"][0] == P.tallest(c["C"], c["tile"][1]):
            classes.setdefault((c["C"], c["tile"][1], c["tile"][0]), []).append(name)
    want = {(C, tw, P.tallest(C, tw)) for C in (32, 96, 192, 384, 768, 1536) for tw in P.FP.WIDTHS}
    assert set(classes) == want, sorted(want - set(classes))
    over = []
    for C, B, H, W, _, th, tw in P.TILE_WIDE:
        assert P.choose_tile(B, C, H, W) == (th, tw) == (P.tallest(C, tw), tw)
        best = B * C * H * W
        for b in (1, 2, 3):
            for h in range(th, 2 * th + 2):
                for w in range(9, 2200):
                    if b * C * h * w >= best:
                        break
                    assert P.choose_tile(b, C, h, w) != (th, tw), ("a smaller map of the class", C, b, h, w)
        if best > P.SIZE_LIMIT:
            over.append((C, tw))
    assert over == [(192, 8), (384, 7), (384, 8), (768, 7), (768, 8), (1536, 7), (1536, 8)]
    for name in P.CASES:
        assert P.entries(name) <= P.SIZE_LIMIT or P.CASES[name]["group"] in ("tile", "cap"), name
    for hw in ((1, 1), (3, 20), (20, 3)):
        assert any((P.CASES[n]["H"], P.CASES[n]["W"]) == hw for n in P.names("head", group="tile"))
    for flag in (True, False):
        assert {1, 3} <= {P.CASES[n]["B"] for n in P.names("head", bias=flag)}
    # pass two: the last 8 x 8 tile 1, 2, 3 and 4 pixels wide and tall, at both channel counts, one and three images
    edge = [P.CASES[n] for n in P.names("head", group="edge")]
    assert len(edge) >= 6 and {c["C"] for c in edge} == {32, 96} and {c["B"] for c in edge} == {1, 3}
    assert all(c["H"] in (1, 7, 8, 9, 10, 11, 12, 16, 17) and c["W"] in (1, 7, 8, 9, 10, 11, 12, 16, 17) for c in edge)
    for axis in ("H", "W"):
        assert {(c[axis] - 1) % 8 + 1 for c in edge} >= {1, 2, 3, 4, 8}
    # the bands
    triples = {n: P.CASES[n]["bands"] for n in P.names("head", group="band") + P.names("head", group="cap")}
    assert triples == {"head/C768_B3_17x17/plain": (27, 2, 14), "head/C1536_B7_9x9/plain": (28, 3, 10), "head/C1536_B107_1x9/plain": (214, 22, 10),
                       "head/C1536_B1_17x25/plain": (12, 2, 6), "head/C1536_B321_1x9/plain": (642, 64, 11)}
    assert 642 - 10 * 64 == 2 and 214 - 9 * 22 == 16 and 28 - 9 * 3 == 1 and 27 - 13 * 2 == 1      # the last bands
    # bands == 1 with more than a tile a band does not exist for any supported C
    for C in range(32, 1537, 32):
        for tiles in range(1, 700):
            per = max(1, min(64, -(-tiles // max(1, 512 // (C // 32)))))
            assert per == 1 or -(-tiles // per) >= 6
    # the stresses: a narrow tile at C = 96, th < 8 at C = 768, a band case with more than a tile a band
    stress = {(c["C"], c["B"], c["H"], c["W"]): c for c in (P.CASES[n] for n in P.names("head", group="stress"))}
    assert len(P.names("head", group="stress")) == 3 * len(P.STRESSES) and len(stress) == 3
    assert stress[(96, 3, 11, 23)]["tile"] == (8, 4) and stress[(768, 1, 6, 23)]["tile"] == (6, 4) and stress[(768, 3, 9, 25)]["bands"] == (24, 2, 12)
    assert all(max(c["H"], c["W"]) >= 21 for c in stress.values())
    # layernorm_cf and the tail
    for C in P.CF_CS:
        assert {(P.CASES[n]["B"], P.CASES[n]["W"]) for n in P.names("cf", C=C, group="shape")} == {(B, HW) for B in (1, 3) for HW in P.CF_HWS}
    assert [P.cf_cached(C) for C in P.CF_CS] == [True] * 6 + [False] * 2 and P.cf_route(512).endswith("<cached>") and P.cf_route(513).endswith("<streamed>")
    assert [P.partial_rows(1, HW) for HW in P.CF_REDUCE_HWS] == [1, 7, 8, 9]
    assert all("cf/C2_B1_HW%d/plain" % HW in P.CASES for HW in P.CF_REDUCE_HWS)
    for C in P.CF_STRESSED:
        assert sorted(P.CASES[n]["stress"] for n in P.names("cf", C=C, B=3, W=131)) == sorted(P.STRESSES)
    assert len(P.names("tail")) == 100 and all(P.CASES[n]["B"] == 3 for n in P.names("tail"))
    assert P.DROP_SCALE[1] == 0.0 and P.DROP_SCALE[0] == float(np.float32(1.0 / 0.3))
    for cases in list(WRONG.values()) + list(OLD_BOUND_BLIND.values()):
        for name in cases:
            assert name in P.CASES and name in SUBSET, name
    # only loweps, offset and common cases are without the project's bound
    assert {P.CASES[n]["stress"] for n in P.LIFTED} == {"loweps", "offset", "common"}
    assert not any(g in ("glb",) for gs in P.LIFTED.values() for g in gs)


@pytest.mark.parametrize("variant", SWITCHES)
def test_wrong_variant_exceeds_the_bound_on_its_named_cases(variant):
    for name in WRONG[variant]:
        assert worst(run(name))[0] <= 1.0                           # the correct emulation passes the same case
        ratio, group, old = worst(run(name, (variant,), check=False))
        print("%-17s %-30s error / bound %-9.3g (%s) old bound %s" % (variant, name, ratio, group, "passes" if old else "fails"))
        assert ratio > 1.0, (variant, name, ratio)
        assert old == (name in OLD_BOUND_BLIND.get(variant, ())), (variant, name, "which variants the old bound lets through")
