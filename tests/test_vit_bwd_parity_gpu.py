"""GPU: the ViT attention core's training route through the C ABI (patch_embed_hip_vit_attn_train_f32,
patch_embed_hip_vit_attn_backward_f32) against the float64 restatement of tests/vit_bwd_parity.py, entry by entry, on seeded
dyadic inputs at the shapes where the 32-token tile, the height and width bins, the dtables chunks and the large-LDS opt-in of
the query pass can go wrong.

The train entry gets a workspace of exactly patch_embed_hip_vit_attn_workspace_bytes, filled with NaN, and NaN-filled `out`
and `lse`, each followed by 64 sentinel floats: `out` is bitwise the inference entry's, every one of the B' heads SP lse entries
is written and finite, the entries below S are under the measure.  The backward entry is fed the kernel's own out and lse; its
workspace is exactly the backward_workspace_bytes answer, which is the layout rel | drel | delta | part of the kernel file's
header (vit_bwd_parity.workspace_layout), NaN-filled with a sentinel behind it; grad_qkv and the two table gradients are
NaN-filled and guarded: afterwards no NaN is left, every sentinel is bitwise intact, every input is bitwise unchanged, and the
last_kernel query names the route.  Every entry of lse, dq, dk, dv, dth, dtw is held to max(8 x the fp32 PyTorch composition's
error of the same entry, computed on the device, 16 x 2^-24 x the entry's magnitude); the project's bound sits on top
(vit_bwd_parity's docstring).  The tables are printed; with VIT_BWD_PARITY_TABLE set they are appended to that file.

Largest kernel error / bound seen on an MI355X, per group over every case of this file (the entry's kernel error, the
composition's error and the bound are relative to the entry's magnitude):
    lse   0.129   D64/20x23/ascending/2x3    1.23e-07   8.02e-08   9.54e-07
    dq    0.023   D80/20x23/ascending/2x3    2.15e-08   2.08e-08   9.54e-07
    dk    0.033   D80/20x23/sharp/2x3        3.11e-08   2.52e-08   9.54e-07
    dv    0.062   D80/20x23/sharp/2x3        5.96e-08   4.76e-08   9.54e-07
    dth   0.007   D80/20x23/descending/1x1   7.08e-09   7.35e-09   9.54e-07
    dtw   0.012   D64/1x3/rel/1x1            1.15e-08   3.49e-09   9.54e-07
Every entry of every case met its bound with the magnitudes as derived in vit_bwd_parity's docstring: no term had to be added
after the run, and the sweep found no kernel bug.  The launches at exactly 64 KiB of LDS (q_w = 94 / 78) are accepted.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vit_bwd_parity as P     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAIL = 64


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


def run(name):
    """{group: tensor} of the two entries on a case, every contract of the C ABI asserted on the way."""
    from uninext_amd import _lib
    c, x = P.CASES[name], P.inputs(name)
    B, heads, D, (Hq, Wq), rel, scale = c["B"], c["heads"], c["D"], c["hw"], c["rel"], x["scale"]
    S, BH, E = Hq * Wq, B * heads, heads * D
    SP = -(-S // P.TILE) * P.TILE
    lib = _lib.load()
    qkv, th, tw, g = dev32(x["qkv"]), dev32(x["th"]), dev32(x["tw"]), dev32(x["g"])
    ptr = lambda t: None if t is None else t.data_ptr()

    # ---- the train entry
    nbytes = lib.patch_embed_hip_vit_attn_workspace_bytes(B, heads, Hq, Wq, D)
    assert nbytes == max(256, BH * (Hq + Wq) * SP * 4)
    ws, out, lse = guarded(nbytes // 4), guarded(B * S * E), guarded(BH * SP)
    rc = lib.patch_embed_hip_vit_attn_train_f32(qkv.data_ptr(), ptr(th), ptr(tw), B, heads, Hq, Wq, D, scale, out.data_ptr(),
                                                lse.data_ptr(), ws.data_ptr(), nbytes, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    intact(ws, nbytes // 4, name + " train workspace")
    out, lse = written(out, (B, S, E), name + " out"), written(lse, (BH, SP), name + " lse")
    assert bool(torch.isfinite(lse).all()) and bool(torch.isfinite(out).all()), name
    ws2, out2 = guarded(nbytes // 4), guarded(B * S * E)
    rc = lib.patch_embed_hip_vit_attn_f32(qkv.data_ptr(), ptr(th), ptr(tw), B, heads, Hq, Wq, D, scale, out2.data_ptr(), ws2.data_ptr(),
                                          nbytes, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert same_bits(out, written(out2, (B, S, E), name + " inference out")), name + ": out is not the inference entry's"

    # ---- the backward entry
    nb = lib.patch_embed_hip_vit_attn_backward_workspace_bytes(B, heads, Hq, Wq, D)
    assert nb == P.workspace_layout(B, heads, Hq, Wq, D)[1] and nb % 256 == 0, (name, nb)
    wsb, gq = guarded(nb // 4), guarded(B * S * 3 * E)
    gth, gtw = (guarded((2 * Hq - 1) * D), guarded((2 * Wq - 1) * D)) if rel else (None, None)
    before = [t.clone() for t in (qkv, th, tw, out, lse, g) if t is not None]
    rc = lib.patch_embed_hip_vit_attn_backward_f32(qkv.data_ptr(), ptr(th), ptr(tw), out.data_ptr(), lse.data_ptr(), g.data_ptr(), B, heads,
                                                   Hq, Wq, D, scale, gq.data_ptr(), ptr(gth), ptr(gtw), wsb.data_ptr(), nb, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    route = "vit_rel<%d>+vit_bwd_q<%d,rel>+vit_bwd_kv<%d,rel>+vit_bwd_tables<%d>" % (D, D, D, D) if rel else "vit_bwd_q<%d>+vit_bwd_kv<%d>" % (D, D)
    assert _lib.last_kernel("vit_attn_bwd") == route
    intact(wsb, nb // 4, name + " backward workspace")
    for was, now in zip(before, [t for t in (qkv, th, tw, out, lse, g) if t is not None]):
        assert same_bits(was, now), name + ": an input was written"
    t = written(gq, (B, S, 3, heads, D), name + " grad_qkv")
    got = {"lse": lse[:, :S], "dq": t[:, :, 0].reshape(B, S, E), "dk": t[:, :, 1].reshape(B, S, E), "dv": t[:, :, 2].reshape(B, S, E)}
    if rel:
        got["dth"] = written(gth, (2 * Hq - 1, D), name + " grad_rel_h_table")
        got["dtw"] = written(gtw, (2 * Wq - 1, D), name + " grad_rel_w_table")
    return got


def check(name):
    if P.CASES[name]["stress"]:
        P.stress_property(name)
    got = run(name)
    ref, comp = P.reference(name), P.composition(name, DEV)
    assert sorted(got) == sorted(ref) == sorted(comp) == sorted(P.groups_of(name)), name
    for what, (want, mag) in ref.items():
        P.measure(name, what, got[what], want, mag, comp[what])


@pytest.mark.parametrize("D", P.DS)
@pytest.mark.parametrize("hw", P.SHAPES, ids=lambda hw: "%dx%d" % hw)
def test_shapes(hw, D):
    since = len(P.TABLE)
    cases = P.names(group="shape", hw=hw, D=D)
    assert len(cases) == 4                                          # tables and none, both batch x heads
    for name in cases:
        if P.CASES[name]["rel"]:
            assert P.swapped_tables_differ(name) == (hw[0] != hw[1])
        check(name)
    P.report(since)


@pytest.mark.parametrize("D", P.DS)
def test_both_sides_of_the_large_lds_opt_in(D):
    """q_w = 94 (D = 64) / 78 (D = 80) is the last launch of the query pass inside the static 64 KiB, exactly; the next q_w is
    the first that opts in; 2 x 256 is the route's limit."""
    since = len(P.TABLE)
    w = P.last_static_w(D)
    assert P.bwd_q_lds_bytes(D, w) == 64 * 1024
    cases = P.names(group="lds", D=D)
    assert sorted({P.CASES[n]["hw"] for n in cases}) == [(1, w), (1, w + 1), (2, 256)] and len(cases) == 5
    for name in cases:
        check(name)
    P.report(since)


@pytest.mark.parametrize("D", P.DS)
def test_dtables_chunks(D):
    since = len(P.TABLE)
    cases = P.names(group="chunk", D=D)
    assert [P.chunks(P.CASES[n]["B"] * P.CASES[n]["heads"]) for n in cases] == [16, 16, 16, 16] and len(cases) == 4
    for name in cases:
        check(name)
    P.report(since)


@pytest.mark.parametrize("D", P.DS)
@pytest.mark.parametrize("hw", [(20, 23), (9, 15)], ids=lambda hw: "%dx%d" % hw)
def test_stress(hw, D):
    since = len(P.TABLE)
    cases = P.names(group="stress", hw=hw, D=D)
    assert len(cases) == len(P.BHS) * len(P.STRESS if hw == (20, 23) else P.STRESS_9X15)
    for name in cases:
        check(name)
    P.report(since)
