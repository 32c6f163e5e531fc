"""GPU: the ConvNeXt backward kernels through the C ABI (patch_embed_hip_convnext_dwconv_ln_backward_f32,
patch_embed_hip_convnext_scale_residual_backward_f32, patch_embed_hip_layernorm_cf_backward_f32) against the float64
restatement of tests/convnext_bwd_parity.py, entry by entry, on seeded dyadic inputs at the shapes where the forward's tiling,
the 8 x 8 tiles and bands of pass two, the partial-row reduction, the cached / streamed switch and the statistics' eps can go
wrong.

The workspace is exactly the *_backward_workspace_bytes answer; it and every output are NaN-filled and followed by 64 sentinel
floats.  Afterwards no NaN is left in a requested output, every sentinel is bitwise intact, every input is bitwise unchanged,
and the last_kernel query names the route the restated rules expect (<4|7|8> for the head, <cached|streamed> for
layernorm_cf).  Every entry of every group is held to max(8 x the fp32 PyTorch composition's error of the same entry, computed
on the device, 16 x 2^-24 x the entry's magnitude); the project's bound sits on top but for the cases convnext_bwd_parity.LIFTED
names.  On the `loweps` cases the kernels are run once more with grad_out kept on the zero-variance pixels alone: glw (cf: gw)
is then exactly zero, because xh is exactly zero there.  The tables are printed; with CONVNEXT_BWD_PARITY_TABLE set they are
appended to that file.

Largest kernel error / bound seen on an MI355X, per (kernel, group) over every case of this file (the entry's kernel error, the
composition's error and the bound are relative to the entry's magnitude; profiles/r33_convnext_bwd_parity.txt has every line):
    cf    gb     cf/C1_B1_HW1/plain                 gb       0.00e+00   0.00e+00   9.54e-07    0.000
    cf    gw     cf/C512_B3_HW1/plain               gw       2.64e-08   7.88e-09   9.54e-07    0.028
    cf    gx     cf/C513_B3_HW131/common            gx       9.96e-08   2.01e-08   9.54e-07    0.104
    head  gb     head/C32_B1_1x7/plain              gb       1.21e-08   5.06e-09   9.54e-07    0.013
    head  glb    head/C768_B3_9x25/common           glb      5.65e-09   5.65e-09   9.54e-07    0.006
    head  glw    head/C32_B1_1x1/plain              glw      1.38e-08   1.55e-09   9.54e-07    0.014
    head  gw     head/C1536_B1_6x5/plain            gw       1.61e-08   1.27e-09   9.54e-07    0.017
    head  gx     head/C1536_B321_1x9/plain          gx       4.57e-08   9.55e-09   9.54e-07    0.048
    tail  ggamma tail/C63_HW1/gamma_drop            ggamma   1.23e-07   1.23e-07   9.81e-07    0.125
    tail  gy     tail/C129_HW129/gamma_drop         gy       5.15e-08   5.15e-08   9.54e-07    0.054
Every entry of every case met its bound with the magnitudes as derived in convnext_bwd_parity's docstring: no term had to be
added after the run, and the sweep found no kernel bug.  The file takes 20 s on the MI355X, tests/test_convnext_parity_gpu.py 9 s
in the same process.
"""
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnext_bwd_parity as P     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAIL = 64
STARTED = []                    # the time of the first launch of this file


def _sentinel():
    return (torch.arange(TAIL, dtype=torch.float32, device=DEV) * -3.0 - 0.625)


def guarded(n):
    buf = torch.full((n + TAIL,), float("nan"), dtype=torch.float32, device=DEV)
    buf[n:] = _sentinel()
    return buf


def intact(buf, n, what):
    assert buf.numel() == n + TAIL
    assert torch.equal(buf[n:].view(torch.int32), _sentinel().view(torch.int32)), what + ": written past the end"


def written(buf, shape, what):
    """The output of a guarded buffer: every entry written (no NaN left), nothing written behind it."""
    n = int(np.prod(shape))
    intact(buf, n, what)
    out = buf[:n].view(*shape).clone()
    assert not bool(torch.isnan(out).any()), what + ": entries left unwritten"
    return out


def dev32(t):
    return None if t is None else t.float().to(DEV).contiguous()


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def ptr(t):
    return None if t is None else t.data_ptr()


def out_shapes(name):
    c = P.CASES[name]
    B, C, H, W = c["B"], c["C"], c["H"], c["W"]
    if c["kernel"] == "head":
        return {"gx": (B, C, H, W), "gw": (C, 1, 7, 7), "gb": (C,), "glw": (C,), "glb": (C,)}
    if c["kernel"] == "cf":
        return {"gx": (B, C, H, W), "gw": (C,), "gb": (C,)}
    return {"gy": (B, H, W, C), "ggamma": (C,)}


def run(name, want=None, keep=None):
    """{group: tensor} of the case's C entry for the groups in `want` (default: all the case has), the others' pointers NULL;
    every contract of the C ABI asserted on the way.  keep [B, H, W] bool: grad_out is zeroed on the other pixels."""
    from uninext_amd import _lib
    lib = _lib.load()
    STARTED.append(time.time()) if not STARTED else None
    c, x = P.CASES[name], P.inputs(name)
    B, C, H, W = c["B"], c["C"], c["H"], c["W"]
    want = P.groups_of(name) if want is None else want
    assert want and set(want) <= set(P.groups_of(name))
    shapes = out_shapes(name)
    bufs = {g: guarded(int(np.prod(shapes[g]))) for g in want}
    o = lambda g: ptr(bufs.get(g))
    go = dev32(x["go"])
    if keep is not None:
        mask = torch.from_numpy(keep).to(DEV)
        go = go * (mask.unsqueeze(-1) if c["kernel"] == "head" else mask.unsqueeze(1)).float()
    if c["kernel"] == "head":
        ins = [dev32(x["x"]), dev32(x["dw_w"]), dev32(x["dw_b"]), dev32(x["ln_w"]), go]
        nbytes = lib.patch_embed_hip_convnext_dwconv_ln_backward_workspace_bytes(B, C, H, W)
        tiles, per, nbands = c["bands"]
        th, tw = c["tile"]
        wgs = B * -(-H // th) * -(-W // tw)
        a256 = lambda n: -(-n // 256) * 256
        assert nbytes == a256(4 * B * C * H * W) + a256(4 * wgs * 2 * C) + a256(4 * nbands * C * 49) + a256(4 * nbands * C), (name, nbytes)
        route = P.head_route(B, C, H, W)
    elif c["kernel"] == "cf":
        ins = [dev32(x["x"]), dev32(x["ln_w"]), go]
        nbytes = lib.patch_embed_hip_layernorm_cf_backward_workspace_bytes(B, C, H, W)
        assert nbytes == -(-(4 * P.partial_rows(B, H * W) * 2 * C) // 256) * 256
        route = P.cf_route(C)
    else:
        ins = [go, dev32(x["y"]), dev32(x["gamma"]), dev32(x["scale"])]
        nbytes = lib.patch_embed_hip_convnext_scale_residual_backward_workspace_bytes(B, C, H, W)
        assert nbytes == -(-(4 * P.partial_rows(B, H * W) * C) // 256) * 256
        route = "convnext_scale_residual_backward"
    assert nbytes > 0 and nbytes % 256 == 0
    ws = guarded(nbytes // 4)
    before = [None if t is None else t.clone() for t in ins]
    if c["kernel"] == "head":
        xs, dw_w, dw_b, ln_w, go = ins
        rc = lib.patch_embed_hip_convnext_dwconv_ln_backward_f32(xs.data_ptr(), dw_w.data_ptr(), ptr(dw_b), ln_w.data_ptr(), x["eps"], go.data_ptr(),
                                                                 B, C, H, W, o("gx"), o("gw"), o("gb"), o("glw"), o("glb"), ws.data_ptr(), nbytes, None)
    elif c["kernel"] == "cf":
        xs, ln_w, go = ins
        rc = lib.patch_embed_hip_layernorm_cf_backward_f32(xs.data_ptr(), ln_w.data_ptr(), x["eps"], go.data_ptr(), B, C, H, W, o("gx"), o("gw"),
                                                           o("gb"), ws.data_ptr(), nbytes, None)
    else:
        go, y, gamma, scale = ins
        rc = lib.patch_embed_hip_convnext_scale_residual_backward_f32(go.data_ptr(), y.data_ptr(), ptr(gamma), ptr(scale), B, C, H, W, o("gy"),
                                                                      o("ggamma"), ws.data_ptr(), nbytes, None)
    assert rc == 0, (name, _lib.last_error())
    torch.cuda.synchronize()
    assert _lib.last_kernel("convnext") == route, (name, _lib.last_kernel("convnext"), route)
    intact(ws, nbytes // 4, name + " workspace")
    for was, now in zip(before, ins):
        assert was is None or same_bits(was, now), name + ": an input was written"
    return {g: written(bufs[g], shapes[g], "%s %s" % (name, g)) for g in want}


def check(name):
    if P.CASES[name]["stress"] != "plain":
        P.stress_property(name)
    got = run(name)
    ref, comp = P.reference(name), P.composition(name, DEV)
    assert sorted(got) == sorted(ref) == sorted(comp) == sorted(P.groups_of(name)), name
    for what, (want, mag) in ref.items():
        P.measure(name, what, got[what], want, mag, comp[what])
    if P.CASES[name]["stress"] == "loweps":     # xh is exactly zero on the zero-variance pixels: they give glw nothing
        zero = P.zero_variance_pixels(name)
        assert zero.any() and not zero.all()
        lw, lb = ("glw", "glb") if P.CASES[name]["kernel"] == "head" else ("gw", "gb")
        only = run(name, want=(lw, lb), keep=zero)
        assert not bool(only[lw].any()) and bool(only[lb].any()), name
    return got


def sweep(cases):
    since = len(P.TABLE)
    assert cases
    for name in cases:
        check(name)
    P.report(since)


@pytest.mark.parametrize("C", (32, 96, 192, 384, 768, 1536))
@pytest.mark.parametrize("tw", (4, 7, 8))
def test_head_pass_one_classes(tw, C):
    cases = [n for n in P.names("head", group="tile", C=C) if P.CASES[n]["tile"][1] == tw]
    assert any(P.CASES[n]["tile"] == (P.tallest(C, tw), tw) for n in cases)
    sweep(cases)


@pytest.mark.parametrize("name", P.names("head", group="edge"))
def test_head_pass_two_edges(name):
    sweep([name])


@pytest.mark.parametrize("name", P.names("head", group="band"))
def test_head_bands(name):
    assert P.CASES[name]["bands"][1] > 1
    sweep([name])


def test_head_band_cap():
    (name,) = P.names("head", group="cap")
    assert P.CASES[name]["bands"] == (642, 64, 11)
    sweep([name])


@pytest.mark.parametrize("hw", sorted({(P.CASES[n]["C"], P.CASES[n]["H"], P.CASES[n]["W"]) for n in P.names("head", group="stress")}),
                         ids=lambda t: "C%d_%dx%d" % t)
def test_head_stresses(hw):
    cases = P.names("head", group="stress", C=hw[0], H=hw[1], W=hw[2])
    assert sorted(P.CASES[n]["stress"] for n in cases) == sorted(P.STRESSES)
    sweep(cases)


@pytest.mark.parametrize("C", P.CF_CS)
def test_layernorm_cf_shapes(C):
    cases = P.names("cf", C=C, group="shape") + (P.names("cf", group="rounding") if C == 1 else [])
    assert len(cases) == 10 + (C == 1)
    sweep(cases)


def test_layernorm_cf_partial_rows():
    cases = ["cf/C2_B1_HW%d/plain" % HW for HW in P.CF_REDUCE_HWS]
    assert [P.partial_rows(1, P.CASES[n]["W"]) for n in cases] == [1, 7, 8, 9]
    sweep(cases)


@pytest.mark.parametrize("C", P.CF_STRESSED)
def test_layernorm_cf_stresses(C):
    sweep(P.names("cf", C=C, group="stress"))


@pytest.mark.parametrize("C", P.TAIL_SIZES)
def test_tail(C):
    since = len(P.TABLE)
    cases = P.names("tail", C=C)
    assert len(cases) == 20
    for name in cases:
        got = check(name)
        if P.CASES[name]["drop"]:
            assert not bool(got["gy"][1].any()), name                   # the dropped sample
    P.report(since)


@pytest.mark.parametrize("name", ["head/C768_B3_17x17/plain", "cf/C512_B3_HW131/plain", "cf/C513_B3_HW131/plain", "tail/C65_HW129/gamma_drop"])
def test_null_pointer_subsets_leave_the_rest_bitwise(name):
    """Each single output NULL in turn, and all outputs but one NULL: what remains is bitwise the full run's.  On the head (a
    band case with two tiles a band) this reaches head_bwd_xw<true, false> and <false, true>, pass one without grad_u and
    without partial sums."""
    if name.startswith("head/"):
        assert P.CASES[name]["bands"][1] > 1
    groups = P.groups_of(name)
    full = run(name)
    for g in groups:
        for want in ([k for k in groups if k != g], [g]):
            if want:
                got = run(name, want=tuple(want))
                for k in want:
                    assert same_bits(got[k], full[k]), (name, "without" if len(want) > 1 else "only", g, k)


def test_worst_ratio_per_kernel_and_group():
    """Runs last: the worst line per (kernel, group) of this process, and the file's wall time."""
    assert {k for k, _ in P.WORST} == {"head", "cf", "tail"}
    assert {g for k, g in P.WORST if k == "head"} == set(P.GROUPS["head"])
    print("largest kernel error / bound per (kernel, group):\n" + P.worst_table())
    print("wall time of tests/test_convnext_bwd_parity_gpu.py: %.1f s" % (time.time() - STARTED[0]))
    path = os.environ.get("CONVNEXT_BWD_PARITY_TABLE")
    if path:
        with open(path, "a") as f:
            f.write("WORST\n" + P.worst_table() + "\nwall time %.1f s\n" % (time.time() - STARTED[0]))
    assert all(r <= 1.0 for r, _ in P.WORST.values())
