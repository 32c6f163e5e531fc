"""GPU: the three ConvNeXt entry points through the C ABI (patch_embed_hip_convnext_dwconv_ln_f32,
patch_embed_hip_convnext_scale_residual_f32, patch_embed_hip_layernorm_cf_f32) against the float64 restatements of
tests/convnext_parity.py, entry by entry, on seeded dyadic inputs: every (TW, th) tile class of dwconv_ln, every
pixels-per-workgroup class of layernorm_cf and its boundaries, the 64 x 64 tile edges of scale_residual, and the stresses that
make eps, the two-pass variance and the zero padding visible (offset, loweps, bigeps, floor: convnext_parity's docstring).

Every output is handed over filled with NaN and followed by 64 sentinel floats: afterwards no NaN is left and every sentinel is
bitwise untouched.  ln_weight, ln_bias and out are 16-byte aligned, as the header requires.  Each case asserts the kernel name
the Python restatement of the host's rule predicts, every entry within max(8 x the fp32 PyTorch composition's error of the same
entry on the same case, 16 x 2^-24 x s), s the restatement's magnitude of the entry, and the project's bound (1e-4 of the
tensor's largest value, at least 1e-4) on top.  On the variance-0 pixels of `loweps` the output is ln_bias, bitwise; the tail is
bitwise PyTorch's inp + (gamma * y).permute.  The composition never runs the kernels.  The tables are printed; with
CONVNEXT_PARITY_TABLE set they are appended to that file.

Largest kernel error / bound seen on an MI355X, per kernel and stress over every case of this file (the entry's kernel error,
the composition's error and the bound are relative to the entry's own magnitude):
    dwconv_ln     plain    0.039   head/C1536_B1_2x1793/plain   2.26e-07   6.85e-08   5.78e-06
    dwconv_ln     offset   0.265   head/C768_B3_9x169/offset    1.26e-03   1.28e-04   4.76e-03
    dwconv_ln     loweps   0.047   head/C768_B3_9x169/loweps    3.84e-03   1.28e-03   8.22e-02
    dwconv_ln     bigeps   0.031   head/C1536_B3_7x169/bigeps   2.28e-07   5.76e-08   7.43e-06
    dwconv_ln     floor    0.033   head/C768_B3_9x169/floor     2.32e-07   5.94e-09   7.06e-06
    layernorm_cf  plain    0.068   cf/C1025_B3_HW15/plain       3.23e-07   2.57e-08   4.77e-06
    layernorm_cf  offset   0.073   cf/C2048_B3_HW35/offset      1.98e-03   2.82e-04   2.72e-02
    layernorm_cf  loweps   0.063   cf/C768_B3_HW67/loweps       2.56e-07   2.12e-09   4.09e-06
    layernorm_cf  bigeps   0.060   cf/C768_B3_HW67/bigeps       2.35e-07   5.13e-08   3.90e-06
    layernorm_cf  floor    0.075   cf/C512_B3_HW131/floor       4.02e-07   5.43e-08   5.38e-06
    scale_residual         0       bitwise the composition on all 50 cases
Every entry of every case met its bound with the magnitude as derived: no term had to be added, every kernel name was the
one the restated rule predicts, and the sweep found no kernel bug.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnext_parity as P     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAIL = 64


# ---------------------------------------------------------------------------------------------------------------- the C ABI

def _sentinel():
    return (torch.arange(TAIL, dtype=torch.float32, device=DEV) * -3.0 - 0.625)


def guarded(n):
    buf = torch.full((n + TAIL,), float("nan"), dtype=torch.float32, device=DEV)
    buf[n:] = _sentinel()
    assert buf.data_ptr() % 16 == 0
    return buf


def written(buf, shape, what):
    """The output of a guarded buffer: every entry written (no NaN left), nothing written behind it."""
    n = int(np.prod(shape))
    assert buf.numel() == n + TAIL
    assert torch.equal(buf[n:].view(torch.int32), _sentinel().view(torch.int32)), what + ": written past the end"
    out = buf[:n].view(*shape).clone()
    assert not bool(torch.isnan(out).any()), what + ": entries left unwritten"
    return out


def dev32(t):
    if t is None:
        return None
    t = t.float().to(DEV).contiguous()
    assert t.data_ptr() % 16 == 0
    return t


def ptr(t):
    return None if t is None else t.data_ptr()


def last():
    from uninext_amd import _lib
    return _lib.last_kernel("convnext")


def run_head(name):
    from uninext_amd import _lib
    c, x = P.CASES[name], P.inputs(name)
    B, C, H, W = c["B"], c["C"], c["H"], c["W"]
    xs, dw_w, dw_b, ln_w, ln_b = (dev32(x[k]) for k in ("x", "dw_w", "dw_b", "ln_w", "ln_b"))
    assert (dw_b is not None) == c["bias"]
    out = guarded(B * H * W * C)
    rc = _lib.load().patch_embed_hip_convnext_dwconv_ln_f32(ptr(xs), ptr(dw_w), ptr(dw_b), ptr(ln_w), ptr(ln_b), x["eps"], B, C, H, W,
                                                            out.data_ptr(), None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert last() == P.head_kernel(B, C, H, W) == "convnext_dwconv_ln<%d>" % c["tile"][1], (name, last())
    return written(out, (B, H, W, C), name)


def run_cf(name):
    from uninext_amd import _lib
    c, x = P.CASES[name], P.inputs(name)
    B, C, H, W = c["B"], c["C"], c["H"], c["W"]
    xs, ln_w, ln_b = (dev32(x[k]) for k in ("x", "ln_w", "ln_b"))
    out = guarded(B * C * H * W)
    rc = _lib.load().patch_embed_hip_layernorm_cf_f32(ptr(xs), ptr(ln_w), ptr(ln_b), x["eps"], B, C, H, W, out.data_ptr(), None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert last() == P.cf_kernel(C), (name, last())
    return written(out, (B, C, H, W), name)


def run_tail(name):
    from uninext_amd import _lib
    c, x = P.CASES[name], P.inputs(name)
    B, C, H, W = c["B"], c["C"], c["H"], c["W"]
    y, gamma, inp = (dev32(x[k]) for k in ("y", "gamma", "inp"))
    out = guarded(B * C * H * W)
    rc = _lib.load().patch_embed_hip_convnext_scale_residual_f32(ptr(y), ptr(gamma), ptr(inp), B, C, H, W, out.data_ptr(), None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert last() == "convnext_scale_residual"
    got = written(out, (B, C, H, W), name)
    want = inp + (y if gamma is None else gamma * y).permute(0, 3, 1, 2)
    assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32)), name + ": not bitwise PyTorch's"
    return got


def check(name, got):
    """`got` under the measure; the property that names the stress first; ln_bias bitwise where the variance is exactly 0."""
    c = P.CASES[name]
    P.stress_property(name)
    want, mag = P.reference(name)
    P.measure(name, got, want, mag, P.composition(name, DEV))
    if c["stress"] == "loweps":
        zero = torch.from_numpy(P.zero_variance_pixels(name)).to(DEV)
        assert bool(zero.any())
        rows = (got if c["kernel"] == "head" else got.permute(0, 2, 3, 1))[zero]
        b = dev32(P.inputs(name)["ln_b"]).expand_as(rows).contiguous()
        assert torch.equal(rows.contiguous().view(torch.int32), b.view(torch.int32)), name + ": ln_bias where the variance is 0"


# ------------------------------------------------------------------------------------------------------------------- the tests

@pytest.mark.parametrize("name", P.names("head"))
def test_dwconv_ln(name):
    since = len(P.TABLE)
    c = P.CASES[name]
    assert P.choose_tile(c["B"], c["C"], c["H"], c["W"]) == c["tile"]
    check(name, run_head(name))
    P.report(since)


@pytest.mark.parametrize("C", P.CF_CS)
def test_layernorm_cf(C):
    since = len(P.TABLE)
    cases = P.names("cf", C=C)
    assert len(cases) == 10 + (len(P.STRESSES) - 1 if C in P.CF_STRESSED else 0)
    for name in cases:
        check(name, run_cf(name))
    P.report(since)


def test_scale_residual():
    since = len(P.TABLE)
    cases = P.names("tail")
    assert len(cases) == 2 * len(P.TAIL_SIZES) ** 2
    for name in cases:
        check(name, run_tail(name))
    P.report(since)


def test_worst_ratio_per_kernel_and_stress():
    """Prints what the sweep above measured (this test runs last in the file); nothing over 1 got here."""
    print(P.worst_table())
    path = os.environ.get("CONVNEXT_PARITY_TABLE")
    if path:
        with open(path, "a") as f:
            f.write("WORST\n" + P.worst_table() + "\n")
    assert all(w[0] <= 1.0 for w in P.WORST.values())
