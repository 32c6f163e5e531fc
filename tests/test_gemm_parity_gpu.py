"""GPU: the GEMM family through its `ext` entry points (linear_pack_weight, linear_packed_forward, linear_packed_ln,
linear_packed_split_forward, ffn_packed; patch_embed_pack_weight, patch_embed_packed_forward, patch_embed_forward;
conv3x3_pack_weight, conv3x3_packed_forward, conv3x3_forward) against tests/gemm_parity.py, entry by entry.

Exact tiers (E8, EX, EW): every output entry equals the float64 sum bit for bit, on the split paths and the exact-fp32 paths.
Bounded tiers (dy10, dy20) on the packed paths: entry_bound(error of the fp32 CPU composition of the three split products, s)
against the restated split, and that + SPLIT_EPS s against the true product; on the exact-fp32 paths entry_bound against
float64.  The packed weights are compared byte for byte with the restated layout.  gemm_parity's docstring derives every form.
_lib.last_kernel has no entry for this family: the tiling a shape takes is restated in gemm_parity (linear_tiling,
conv_exact_unit, ...) from the inequalities of the launch code, and asserted on the case tables here and in the CPU test.
The table is printed; with GEMM_PARITY_TABLE set it is appended to that file.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_parity as P     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bytes(t):
    return t.cpu().numpy()


def check_linear_pack(packed, w):
    want = P.packed_layout(w)
    assert np.array_equal(_bytes(packed).view(np.uint16).reshape(want.shape), want), "linear_pack_weight: bytes"


def run(name):
    """(entry point, {output: fp32 tensor}) of a case; the packed weights are checked byte for byte on the way."""
    from uninext_amd import ext
    c, i = P.CASES[name], P.inputs(name)
    kind = c["kind"]
    if kind == "lin":
        packed = ext.linear_pack_weight(dev(i["w"]))
        check_linear_pack(packed, i["w"])
        x, xa, b, m = dev(i["x"]), dev(i["x_add"]), dev(i["bias"]), dev(i["mask"])
        if c["split_col"]:
            a, b2 = ext.linear_packed_split_forward(x, packed, c["split_col"], c["N"], b, xa)
            return "linear_packed_split_forward", {"out_a": a, "out_b": b2}
        if c["hm"]:
            out = ext.linear_packed_forward(x.view(-1, c["hm"], c["K"]), packed, c["N"], b, None if m is None else m.view(-1, c["hm"]),
                                            head_major_rows=c["hm"])
            return "linear_packed_forward<hm>", {"out": out}
        out = ext.linear_packed_forward(x, packed, c["N"], b, m, x_add=xa, relu=c["relu"])
        return "linear_packed_forward" + ("<ex>" if (xa is not None or c["relu"]) else ""), {"out": out}
    if kind == "ln":
        packed = ext.linear_pack_weight(dev(i["w"]))
        out = ext.linear_packed_ln(dev(i["x"]), packed, dev(i["bias"]), dev(i["residual"]), dev(i["gamma"]), dev(i["beta"]), P.LN_EPS)
        return "linear_packed_ln", {"out": out}
    if kind == "ffn":
        p1, p2 = ext.linear_pack_weight(dev(i["w1"])), ext.linear_pack_weight(dev(i["w2"]))
        out = ext.ffn_packed(dev(i["x"]), p1, dev(i["b1"]), p2, dev(i["b2"]), c["F"], dev(i["residual"]), dev(i["gamma"]), dev(i["beta"]),
                             P.LN_EPS, layer_norm=c["layer_norm"])
        return "ffn_packed<%d waves>" % (8 if c["F"] % 256 == 0 else 4), {"out": out}
    if kind == "pe":
        if c["path"] == "exact":
            return "patch_embed_forward", {"out": ext.patch_embed_forward(dev(i["x"]), dev(i["w"]), dev(i["bias"]), c["cl"])}
        packed = ext.patch_embed_pack_weight(dev(i["w"]))
        want = P.packed_layout(i["w"].reshape(c["E"], -1))
        assert np.array_equal(_bytes(packed).view(np.uint16).reshape(want.shape), want), "patch_embed_pack_weight: bytes"
        return "patch_embed_packed_forward", {"out": ext.patch_embed_packed_forward(dev(i["x"]), packed, c["E"], c["k"], dev(i["bias"]), c["cl"])}
    assert kind == "conv"
    x, w, b = dev(i["x"]), dev(i["w"]), dev(i["bias"])
    if c["prec"] in (0, 1):
        return "conv3x3_forward<%d>" % c["prec"], {"out": ext.conv3x3_forward(x, w, b, relu=c["relu"], precision=c["prec"])}
    exact = c["prec"] == 3
    packed = ext.conv3x3_pack_weight(w, exact=exact)
    if exact:
        want = P.packed_exact_layout(i["w"])
        assert np.array_equal(_bytes(packed).view(np.uint32).reshape(want.shape), want.view(np.uint32)), "conv3x3_pack_weight(exact): bytes"
    else:
        want = P.packed_layout(i["w"].reshape(c["cout"], -1), taps=9)
        assert np.array_equal(_bytes(packed).view(np.uint16).reshape(want.shape), want), "conv3x3_pack_weight: bytes"
    out = ext.conv3x3_packed_forward(x, packed, c["cout"], b, relu=c["relu"], exact=exact)
    return "conv3x3_packed_forward" + ("<exact>" if exact else ""), {"out": out}


def sweep(group):
    since = len(P.TABLE)
    for name in P.names(group):
        if P.CASES[name]["tier"] in P.EXACT:
            P.exact_condition(name)
        entry, got = run(name)
        P.hold(name, entry, got)
    P.report(since)


# ------------------------------------------------------------------------------------------------------------------- linear

@pytest.mark.parametrize("group", P.groups("lin/"))
def test_linear(group):
    sweep(group)
    if group.startswith("lin/tiling/"):
        n = int(group.rsplit("n", 1)[1])
        rows, tiling, below = next((r, t, b) for nn, r, t, b in P.LIN_TILINGS if nn == n)
        took = {P.CASES[c]["rows"]: P.linear_tiling(P.CASES[c]["rows"], n) for c in P.names(group)}
        assert took[rows] == took[rows + 62] == tiling and took[rows - 1] == below, took


@pytest.mark.parametrize("tier", P.TIERS)
def test_linear_masked_rows_are_exact_zeros_and_relu_is_non_negative(tier):
    for name in P.names("lin/opt/%s" % tier):
        c, i = P.CASES[name], P.inputs(name)
        if not (c["mask"] or c["relu"]):
            continue
        out = run(name)[1]["out"]
        if c["mask"]:
            rows = torch.from_numpy(i["mask"]).to(DEV)
            assert bool(rows[-1]) and (c["rows"] < 129 or bool(rows[64:128].all())), "a masked tail row and a fully masked tile"
            assert int((out[rows].view(torch.int32) & 0x7fffffff).max()) == 0, name
        if c["relu"]:
            assert float(out.min()) >= 0.0, name


@pytest.mark.parametrize("group", P.groups("ln/"))
def test_linear_layernorm(group):
    sweep(group)
    for name in P.names(group):
        c, i = P.CASES[name], P.inputs(name)
        if c["rows"] > 1 and (c["residual"] or not c["bias"]):       # row 0 has variance 0: beta, bit for bit
            out = run(name)[1]["out"][0].cpu().numpy()
            beta = np.zeros(256, dtype=np.float32) if i["beta"] is None else i["beta"]
            assert np.array_equal((out + np.float32(0)).view(np.uint32), (beta + np.float32(0)).view(np.uint32)), name


@pytest.mark.parametrize("group", P.groups("ffn/"))
def test_ffn(group):
    sweep(group)
    for name in P.names(group):
        c, i = P.CASES[name], P.inputs(name)
        if c["negative"]:                                            # no hidden unit is active: bias2 + residual alone
            want = (i["b2"][None, :] + i["residual"]).astype(np.float64)
            assert len(P.bit_mismatches(run(name)[1]["out"], want)) == 0, name


# -------------------------------------------------------------------------------------------------------------- patch_embed

@pytest.mark.parametrize("group", P.groups("pe/"))
def test_patch_embed(group):
    sweep(group)


# ------------------------------------------------------------------------------------------------------------------ conv3x3

@pytest.mark.parametrize("group", P.groups("conv/"))
def test_conv3x3(group):
    sweep(group)


# ------------------------------------------------------------------------------------------------------------ repeatability

REPEAT = ("lin/dy20/k320/r129/n384", "lin/dy20/k64/r10881/n384/tiling", "lin/dy20/k64/r32705/n256/tiling",
          "lin/dy20/k128/r195/n128/hm65/b1m1", "lin/dy20/k128/r129/n384/sc256/a1", "ln/dy20/k256/r65/all",
          "ffn/dy20/f384/r65/ln1", "ffn/dy20/f1024/r65/ln1", "pe/packed/dy20/k16c3/e130/p1x3x43/nchw",
          "pe/exact/dy20/k16c3/e130/p1x3x43/nhwc", "conv/p0/dy20/b1/c48/33x47/o130/b1r0", "conv/p1/dy20/b1/c48/33x47/o130/b1r0",
          "conv/p2/dy20/b1/c48/33x47/o130/b1r0", "conv/p3/dy20/b1/c48/33x47/o130/b1r0")


@pytest.mark.parametrize("name", REPEAT)
def test_two_runs_give_the_same_bits(name):
    a, b = run(name)[1], run(name)[1]
    for what in a:
        assert torch.equal(a[what].view(torch.int32), b[what].view(torch.int32)), (name, what)


def test_table():
    """The worst line per entry point and reference of everything this process measured."""
    print(P.HEAD)
    lines = ["%-28s %-8s %s" % (k[0], k[1], line) for k, (_, line) in sorted(P.WORST.items())]
    print("\n".join(lines))
    path = os.environ.get("GEMM_PARITY_TABLE")
    if path:
        with open(path, "a") as f:
            f.write("worst per entry point and reference\n" + P.HEAD + "\n" + "\n".join(lines) + "\n")
