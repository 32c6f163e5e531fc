"""GPU: the three fused attention cores through the C ABI (biattn_hip_self_forward_f32, patch_embed_hip_vit_attn_f32,
biattn_hip_forward_f32) against the float64 restatements of tests/attn_parity.py, entry by entry, on seeded dyadic inputs at the
shapes where the 32-token tile, the key ranges, the biattn_image instantiations and the running softmax's rescale can go wrong.

Every output is handed over filled with NaN and followed by 64 sentinel floats, every workspace is exactly as large as its
query answers, filled with NaN and followed by the same sentinel: afterwards no NaN is left in an output (outside the rows of
dec_attn that must be NaN) and every sentinel is bitwise untouched.  Every entry is held to max(8 x the fp32 PyTorch
composition's error of the same entry on the same case, 16 x 2^-24 x s), s the restatement's magnitude of the entry
(attn_parity's docstring); the project's bound (TOL of the tensor's largest value) is asserted on top.  The composition never
runs the kernels.  The tables are printed; with ATTN_PARITY_TABLE set they are appended to that file.

Largest kernel error / bound seen on an MI355X, per core and output over every case of this file (the entry's kernel error, the
composition's error and the bound are relative to the entry's own magnitude):
    dec_attn  out     0.104   dec/L130/ascending/2x3        7.67e-06   7.79e-06   7.38e-05
    vit_attn  out     0.163   vit/D64/20x23/ascending/2x3   1.27e-04   6.79e-05   7.81e-04
    biattn    out_v   0.175   bi/S1065_T65/ascending/2x3    3.71e-04   2.64e-04   2.11e-03
    biattn    out_l   0.213   bi/S1065_T65/ascending/2x3    1.66e-04   9.71e-05   7.77e-04
Every entry of every case met its bound with the magnitude as derived: no term had to be added, and the sweep found no kernel bug.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_parity as P     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAIL = 64
MASK_NONE, MASK_INT64, MASK_F32, MASK_BOOL = 0, 1, 2, 3         # include/biattn_hip.h
DEC_NAME = {MASK_NONE: "dec_attn<none>", MASK_BOOL: "dec_attn<bool>", MASK_F32: "dec_attn<f32>"}
BI_NAME = "biattn_image+biattn_text+biattn_combine"


# ---------------------------------------------------------------------------------------------------------------- the C ABI

def _sentinel():
    return (torch.arange(TAIL, dtype=torch.float32, device=DEV) * -3.0 - 0.625)


def guarded(n):
    buf = torch.full((n + TAIL,), float("nan"), dtype=torch.float32, device=DEV)
    buf[n:] = _sentinel()
    return buf


def intact(buf, n, what):
    assert buf.numel() == n + TAIL
    assert torch.equal(buf[n:].view(torch.int32), _sentinel().view(torch.int32)), what + ": written past the end"


def written(buf, shape, what, nan_rows=None):
    """The output of a guarded buffer: every entry written (no NaN left outside `nan_rows`, a bool array over all but the last
    axis), nothing written behind it."""
    n = int(np.prod(shape))
    intact(buf, n, what)
    out = buf[:n].view(*shape).clone()
    left = torch.isnan(out)
    if nan_rows is None:
        assert not bool(left.any()), what + ": entries left unwritten"
    else:
        must = torch.from_numpy(nan_rows).to(DEV)[..., None].expand_as(left)
        assert torch.equal(left, must), what + ": NaN outside the rows that must be NaN, or entries left unwritten"
    return out


def dev32(t):
    return t.float().to(DEV).contiguous()


def run_dec(name, strides=None):
    """strides: (q, k, v) row strides in floats; the floats between the rows are NaN."""
    from uninext_amd import _lib
    c, x = P.CASES[name], P.inputs(name)
    B, L, heads = c["B"], c["L"], c["heads"]
    E = heads * P.DEC_D
    rows = []
    for t, stride in zip((x["q"], x["k"], x["v"]), strides or (E, E, E)):
        buf = torch.full((B, L, stride), float("nan"), dtype=torch.float32, device=DEV)
        buf[..., :E] = dev32(t)
        rows.append(buf)
    mask, kind = x["mask"], MASK_NONE
    if mask is not None:
        kind = MASK_BOOL if mask.dtype == torch.bool else MASK_F32
        mask = mask.to(DEV).contiguous() if kind == MASK_BOOL else dev32(mask)
        assert mask.element_size() == (1 if kind == MASK_BOOL else 4)
    out = guarded(B * L * E)
    rc = _lib.load().biattn_hip_self_forward_f32(*(r.data_ptr() for r in rows), *(r.stride(1) for r in rows),
                                                 mask.data_ptr() if mask is not None else None, kind, B, heads, L, P.DEC_D,
                                                 x["scale"], out.data_ptr(), None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert _lib.last_kernel("dec_attn") == DEC_NAME[kind]
    return written(out, (B, L, E), name, np.isnan(P.reference(name)["out"][0]).all(-1))


def run_vit(name):
    from uninext_amd import _lib
    c, x = P.CASES[name], P.inputs(name)
    B, heads, D, (Hq, Wq) = c["B"], c["heads"], c["D"], c["hw"]
    S = Hq * Wq
    lib = _lib.load()
    qkv = dev32(x["qkv"])
    th, tw = (dev32(x["th"]), dev32(x["tw"])) if c["rel"] else (None, None)
    nbytes = lib.patch_embed_hip_vit_attn_workspace_bytes(B, heads, Hq, Wq, D)
    assert nbytes == max(256, B * heads * (Hq + Wq) * (-(-S // P.TILE) * P.TILE) * 4)
    ws, out = guarded(nbytes // 4), guarded(B * S * heads * D)
    rc = lib.patch_embed_hip_vit_attn_f32(qkv.data_ptr(), th.data_ptr() if c["rel"] else None, tw.data_ptr() if c["rel"] else None,
                                          B, heads, Hq, Wq, D, x["scale"], out.data_ptr(), ws.data_ptr(), nbytes, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert _lib.last_kernel("vit_attn") == ("vit_rel<%d>+vit_attn<%d,rel>" % (D, D) if c["rel"] else "vit_attn<%d>" % D)
    intact(ws, nbytes // 4, name + " workspace")
    return written(out, (B, S, heads * D), name)


def run_bi(name):
    from uninext_amd import _lib
    c, x = P.CASES[name], P.inputs(name)
    B, heads, S, T = c["B"], c["heads"], c["S"], c["T"]
    E = heads * P.BI_D
    lib = _lib.load()
    q, k, vv, vl = (dev32(x[n]) for n in ("q", "k", "vv", "vl"))
    mask, kind = x["mask"], MASK_NONE
    if mask is not None:
        kind = MASK_INT64 if mask.dtype == torch.int64 else MASK_F32
        mask = mask.to(DEV).contiguous() if kind == MASK_INT64 else dev32(mask)
    TP, NC = P.bi_ranges(B * heads, S, T)
    nbytes = lib.biattn_hip_workspace_bytes(B, heads, S, T, P.BI_D)
    assert nbytes == max(256, B * heads * NC * (P.BI_D + 2) * TP * 4), (name, nbytes, TP, NC)
    ws, out_v, out_l = guarded(nbytes // 4), guarded(B * S * E), guarded(B * T * E)
    rc = lib.biattn_hip_forward_f32(q.data_ptr(), k.data_ptr(), vv.data_ptr(), vl.data_ptr(), mask.data_ptr() if mask is not None else None,
                                    kind, B, heads, S, T, P.BI_D, x["scale"], out_v.data_ptr(), out_l.data_ptr(), ws.data_ptr(),
                                    nbytes, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert _lib.last_kernel("biattn") == BI_NAME
    intact(ws, nbytes // 4, name + " workspace")
    return {"out_v": written(out_v, (B, S, E), name + " out_v"), "out_l": written(out_l, (B, T, E), name + " out_l")}


def check(name, got):
    """`got` {output: tensor} of a case under the measure; the property that names a stress case first."""
    if P.CASES[name]["stress"]:
        P.stress_property(name)
    ref, comp = P.reference(name), P.composition(name, DEV)
    for what, (want, mag) in ref.items():
        P.measure(name, what, got[what], want, mag, comp[what])


# --------------------------------------------------------------------------------------------------------------------- dec_attn

@pytest.mark.parametrize("L", P.DEC_LENS)
def test_dec_attn(L):
    since = len(P.TABLE)
    cases = P.names("dec", L=L)
    assert {P.CASES[n]["mask"] for n in cases} == {"none", "bool", "f32"}
    assert {(P.CASES[n]["B"], P.CASES[n]["heads"]) for n in cases} == set(P.BHS)
    for name in cases:
        c, x = P.CASES[name], P.inputs(name)
        want = P.reference(name)["out"][0]
        nan_rows = np.isnan(want).all(-1)
        if c["pattern"] == "row45":                                 # one fully excluded row: NaN in that row only
            assert nan_rows[:, 45].all() and nan_rows.sum() == c["B"]
        else:
            assert not nan_rows.any()
        if c["pattern"] == "dn":                                    # leading tiles wholly excluded for the later queries
            m = x["mask"] if x["mask"].dtype == torch.bool else torch.isinf(x["mask"])
            first = L // 2 // P.TILE * P.TILE
            assert first >= P.TILE and bool(m[first:, :first].all()) and not bool(m.all(1).any())
        if c["pattern"] == "last_open":
            m = x["mask"] if x["mask"].dtype == torch.bool else torch.isinf(x["mask"])
            assert bool(m[:, :L - 1].all()) and not bool(m[:, L - 1].any())
        check(name, {"out": run_dec(name)})
    P.report(since)


@pytest.mark.parametrize("name", ["dec/L97/none/2x3", "dec/L97/bool/2x3", "dec/L33/f32/1x1"])
def test_dec_attn_row_strides_with_nan_between_the_rows(name):
    """q rows E + 4 floats apart, k and v rows E + 8, NaN in the floats between: bitwise the contiguous call's output."""
    E = P.CASES[name]["heads"] * P.DEC_D
    plain = run_dec(name)
    strided = run_dec(name, (E + 4, E + 8, E + 8))
    assert torch.equal(strided.view(torch.int32), plain.view(torch.int32))


# --------------------------------------------------------------------------------------------------------------------- vit_attn

@pytest.mark.parametrize("D", P.VIT_DS)
@pytest.mark.parametrize("hw", P.VIT_SHAPES, ids=lambda hw: "%dx%d" % hw)
def test_vit_attn(hw, D):
    since = len(P.TABLE)
    cases = P.names("vit", hw=hw, D=D)
    assert len([n for n in cases if P.CASES[n]["stress"] is None]) == 4          # tables and none, both batch x heads
    assert len(cases) == (4 + 2 * len(P.STRESS) if hw == (20, 23) else 4)
    for name in cases:
        c = P.CASES[name]
        if c["rel"] and c["stress"] is None:
            assert P.swapped_tables_differ(name) == (hw[0] != hw[1])
        check(name, {"out": run_vit(name)})
    P.report(since)


# ----------------------------------------------------------------------------------------------------------------------- biattn

NJ = {1: 1, 32: 1, 33: 2, 65: 4, 96: 4, 97: 4, 129: 8, 224: 8, 256: 8}      # the biattn_image instantiation each T is to reach


def _bi(cases, T):
    nj = P.bi_nj(T)
    assert nj == NJ[T] and 32 * nj >= T
    assert (32 * nj - T >= 32) == (T in (65, 96, 129, 224))         # a tile with no row
    for name in cases:
        c, x = P.CASES[name], P.inputs(name)
        if c["mask"] == "allmasked":
            assert not bool(x["mask"][c["B"] - 1].any())
        elif c["mask"] != "none":
            assert bool((x["mask"] != 0).any(1).all()) and (T == 1 or bool((x["mask"] == 0).any()))
        check(name, run_bi(name))


@pytest.mark.parametrize("T", P.BI_TS)
def test_biattn_text_lengths(T):
    since = len(P.TABLE)
    cases = [n for n in P.names("bi", T=T, stress=None) if P.CASES[n]["S"] in (1, 33, 129)]
    assert len(cases) == 3 * len(P.BI_MASKS) * len(P.BHS)
    _bi(cases, T)
    P.report(since)


@pytest.mark.parametrize("T", [65, 129])
@pytest.mark.parametrize("S", [32, 128, 1065])
def test_biattn_image_lengths(S, T):
    since = len(P.TABLE)
    cases = P.names("bi", S=S, T=T)
    stress = [n for n in cases if P.CASES[n]["stress"]]
    assert len(cases) - len(stress) == len(P.BI_MASKS) * len(P.BHS)
    if S == 1065:
        assert P.bi_ranges(1, S, T)[1] == 34 == -(-S // 32)         # one tile per range
        assert len(stress) == (2 * len(P.STRESS) if T == 65 else 2)
        if T == 129:
            assert P.bi_ranges(6, S, T)[1] == 22                    # neither 64 nor the tile count
    _bi(cases, T)
    P.report(since)
