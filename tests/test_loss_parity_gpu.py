"""GPU: the loss kernels (uninext_amd/csrc/criterion.hip, uninext_amd/csrc/boxinst.hip) against the float64 restatements of
tests/loss_parity.py at the slice, band, halo and tile edges its case tables list.

Per entry and per gradient group: |got - ref64| <= max(8 x the fp32 PyTorch composition's error at the entry on this GPU,
16 x 2^-24 x s) with s as derived in tests/loss_parity.py, and the project's 1e-4 of the tensor's scale on top; an entry with
reference 0 and s = 0 must be exactly 0; pos, tmax, sum w, sum t and the bitmasks are equal exactly; the float64 sums are held to
the derived term alone.  Every output and workspace is carved out of a sentinel-filled buffer whose guard bands must come back
untouched; `last_kernel` names the path taken; a second call gives the same bits.  Every test prints, per group, the worst
|error| / bound and the worst relative error of the kernel, and the composition's against the derived term alone.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import loss_parity as P     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 256
SENTINEL = {torch.float32: 12345.0, torch.uint8: 0x5A, torch.int32: 0x5A5A5A5A, torch.float64: 12345.0}


class Guarded:
    """Outputs carved out of larger buffers filled with a sentinel; check() asserts the bands are as they were.  shift: the view
    starts that many elements later (a base that is not 16-byte aligned)."""

    def __init__(self):
        self.bufs = []

    def __call__(self, shape, dtype=torch.float32, shift=0):
        n = int(np.prod(shape))
        buf = torch.full((BAND + shift + n + BAND,), SENTINEL[dtype], dtype=dtype, device=DEV)
        self.bufs.append((buf, n, shift))
        return buf[BAND + shift:BAND + shift + n].view(shape)

    def check(self):
        for buf, n, shift in self.bufs:
            assert bool((buf[:BAND + shift] == SENTINEL[buf.dtype]).all()) and bool((buf[BAND + shift + n:] == SENTINEL[buf.dtype]).all())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def workspace(guard, which, count, per):
    from uninext_amd import _lib
    nbytes = _lib.load().criterion_hip_workspace_bytes(which, count, per)
    assert nbytes > 0 and nbytes % 8 == 0
    return guard((nbytes,), torch.uint8)               # 256 guard bytes in front: the carved workspace stays 16-byte aligned


report = P.report


# ---------------------------------------------------------------------------------------------------------------- token focal

@pytest.mark.parametrize("name", list(P.TOKEN))
def test_token_focal_per_entry(name):
    from uninext_amd import _lib, ext
    p, since = P.token_inputs(name), len(P.TABLE)
    ref = P.token64(p)
    B, Q, T = p["logits"].shape
    guard = Guarded()
    shift = 1 if p["misaligned"] else 0
    x = guard((B, Q, T), shift=shift)
    x.copy_(dev(p["logits"]))
    assert (x.data_ptr() % 16 != 0) == bool(shift)
    m = None if p["mask"] is None else dev(p["mask"]).to(torch.bool if p["mask_kind"] == "bool" else torch.int64)
    rt, pm, scale = dev(p["row_target"]), dev(p["pm"]), torch.full((1,), p["scale"], device=DEV)
    out, grad = guard((1,)), guard((B, Q, T))
    ws = workspace(guard, _lib.CRITERION_TOKEN_FOCAL, B * Q, T)
    path = "<vec4>" if T % 4 == 0 and not shift else "<scalar>"
    loss = ext.token_focal_loss_forward(x, m, rt, pm, p["alpha"], out=out, workspace=ws)
    assert _lib.last_kernel("criterion") == "token_focal_fwd" + path
    ext.token_focal_loss_backward(x, m, rt, pm, p["alpha"], scale, out=grad)
    assert _lib.last_kernel("criterion") == "token_focal_bwd" + path
    torch.cuda.synchronize()
    guard.check()
    comp = P.token_composition(p, DEV)
    got = host(grad).astype(np.float64)
    worst = [P.measure("token", "loss", name, host(loss)[0], ref["loss"], ref["mag_loss"], comp["loss"])]
    for sl, where in P.token_slices(p, ref).items():
        worst.append(P.measure("token", sl, name, got, ref["grad"], ref["mag_grad"], comp["grad"], where))
    report(since)
    assert not got[~ref["counted"]].any()                       # exactly 0.0 at masked tokens
    assert max(worst) <= 1.0
    assert torch.equal(ext.token_focal_loss_forward(x, m, rt, pm, p["alpha"]), loss)
    assert torch.equal(ext.token_focal_loss_backward(x, m, rt, pm, p["alpha"], scale), grad)


# ---------------------------------------------------------------------------------------------------------------- mask losses

@pytest.mark.parametrize("name", list(P.MASK))
def test_mask_losses_per_entry(name):
    from uninext_amd import _lib, ext
    p, since = P.mask_inputs(name), len(P.TABLE)
    focal, dice = P.mask64(p, (1.0, 0.0)), P.mask64(p, (0.0, 1.0))
    n, F, h, w = p["src"].shape
    guard = Guarded()
    x, gt, rows = dev(p["src"]), dev(p["gt"]), dev(p["gt_row"])
    losses, sums = guard((2,)), guard((n, 4))
    g_focal, g_dice = guard((n, F, h, w)), guard((n, F, h, w))
    ws = workspace(guard, _lib.CRITERION_MASK_LOSSES, n, F * h * w)
    path = "<vec4>" if w % 4 == 0 else "<scalar>"
    ext.mask_losses_forward(x, gt, rows, p["stride"], p["num_boxes"], out=(losses, sums), workspace=ws)
    assert _lib.last_kernel("criterion") == "mask_losses_fwd" + path
    one, zero = torch.ones(1, device=DEV), torch.zeros(1, device=DEV)
    ext.mask_losses_backward(x, gt, rows, p["stride"], p["num_boxes"], sums, one, zero, out=g_focal)
    ext.mask_losses_backward(x, gt, rows, p["stride"], p["num_boxes"], sums, zero, one, out=g_dice)
    assert _lib.last_kernel("criterion") == "mask_losses_bwd" + path
    torch.cuda.synchronize()
    guard.check()
    comp = P.mask_composition(p, focal["t"], DEV)
    got_sums = host(sums).astype(np.float64)
    assert np.array_equal(got_sums[:, 3], focal["sums"][:, 3])                  # sum t, exactly
    worst = [P.measure("mask", "sums", name, got_sums, focal["sums"], focal["mag_sums"]),
             P.measure("mask", "losses", name, host(losses), focal["losses"], focal["mag_losses"], comp["losses"]),
             P.measure("mask", "focal", name, host(g_focal), focal["grad"], focal["mag_grad"], comp["grad_focal"]),
             P.measure("mask", "dice", name, host(g_dice), dice["grad"], dice["mag_grad"], comp["grad_dice"])]
    report(since)
    assert max(worst) <= 1.0
    again, sums2 = ext.mask_losses_forward(x, gt, rows, p["stride"], p["num_boxes"])
    assert torch.equal(again, losses) and torch.equal(sums2, sums)
    assert torch.equal(ext.mask_losses_backward(x, gt, rows, p["stride"], p["num_boxes"], sums, zero, one), g_dice)


# -------------------------------------------------------------------------------------------------------------------- BoxInst

def box_tensors(p):
    h, w = p["src"].shape[2:]
    return (dev(p["src"]), dev(p["inst"]), dev(p["gt"]), dev(p["gt_row"]), p["stride"], dev(p["sim"]), dev(p["img"]), float(p["thresh"]), p["d"],
            torch.full((1,), p["warmup"], device=DEV))


@pytest.mark.parametrize("name", list(P.BOX))
def test_boxinst_losses_per_entry(name):
    from uninext_amd import _lib, ext
    p, since = P.box_inputs(name), len(P.TABLE)
    ref = P.box64(p)
    N, _, h, w = p["src"].shape
    n = len(p["inst"])
    args = box_tensors(p)
    assert ext.boxinst_losses_supported(args[0], args[2], args[5], p["d"])
    guard = Guarded()
    out = (guard((2,)), guard((n, h + w), torch.int32), guard((n, h + w), torch.uint8), guard((n, 4), torch.float64), guard((2,), torch.float64))
    g_prj, g_pair = guard((N, 1, h, w)), guard((N, 1, h, w))
    ws = workspace(guard, _lib.CRITERION_BOXINST, n, h * w)
    path = "<vec4>" if w % 4 == 0 else "<scalar>"
    losses, saved = ext.boxinst_losses_forward(*args, out=out, workspace=ws)
    assert _lib.last_kernel("criterion") == "boxinst_fwd" + path
    one, zero = torch.ones(1, device=DEV), torch.zeros(1, device=DEV)
    ext.boxinst_losses_backward(*args, saved, one, zero, out=g_prj)
    ext.boxinst_losses_backward(*args, saved, zero, one, out=g_pair)
    assert _lib.last_kernel("criterion") == "boxinst_bwd" + path
    torch.cuda.synchronize()
    guard.check()
    pos, tmax, sums, totals = (host(t) for t in saved)
    bad = np.argwhere(pos != ref["pos"])
    assert not len(bad), (name, "pos: first (instance, row or h + column)", bad[:4].tolist())
    assert np.array_equal(tmax, ref["tmax"]) and totals[1] == ref["totals"][1]                 # the targets' maxima and sum w, exactly
    comp = P.box_composition(p, ref, DEV)
    got_prj, got_pair = host(g_prj).astype(np.float64), host(g_pair).astype(np.float64)
    worst = [P.measure("boxinst", "sums", name, sums, ref["sums"], ref["mag_sums"]),
             P.measure("boxinst", "totals", name, totals, ref["totals"], ref["mag_totals"]),
             P.measure("boxinst", "losses", name, host(losses), ref["losses"], ref["mag_losses"], comp["losses"]),
             P.measure("boxinst", "pairwise", name, got_pair, ref["grad_pair"], ref["mag_grad_pair"], comp["grad_pair"])]
    for sl, where in P.box_slices(ref).items():
        worst.append(P.measure("boxinst", "prj." + sl, name, got_prj, ref["grad_prj"], ref["mag_grad_prj"], comp["grad_prj"], where))
    report(since)
    assert max(worst) <= 1.0
    if ref["totals"][1] == 0:                                   # no weight: the clamp to 1 applies, the pairwise gradient is exactly 0
        assert not got_pair.any() and float(losses[1]) == 0.0
    unread = sorted(set(range(N)) - set(int(r) for r in p["inst"]))
    assert not got_prj[unread].any() and not got_pair[unread].any()             # exactly 0.0 in the rows no instance reads
    again, saved2 = ext.boxinst_losses_forward(*args)
    assert torch.equal(again, losses) and all(torch.equal(a, b) for a, b in zip(saved2, saved))
    assert torch.equal(ext.boxinst_losses_backward(*args, saved, zero, one), g_pair)
    assert torch.equal(ext.boxinst_losses_backward(*args, saved, one, zero), g_prj)


@pytest.mark.parametrize("d", [1, 8])
def test_one_column_past_the_lds_limit_is_refused(d):
    from uninext_amd import ext
    w = P.widest(d) + 1
    assert P.tile_bytes(w, d) > P.LDS_BYTES >= P.tile_bytes(w - 1, d)
    src = torch.zeros(1, 1, 2, w, device=DEV)
    gt, sim = torch.zeros(1, 2, w, dtype=torch.uint8, device=DEV), torch.zeros(1, 8, 2, w, device=DEV)
    zero = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert not ext.boxinst_losses_supported(src, gt, sim, d)
    assert ext.boxinst_losses_supported(src[..., :w - 1].contiguous(), gt, sim[..., :w - 1].contiguous(), d)
    with pytest.raises(RuntimeError, match=r"code -5"):
        ext.boxinst_losses_forward(src, zero, gt, zero, 1, sim, zero, 0.3, d, torch.ones(1, device=DEV))


# ----------------------------------------------------------------------------------------------------------- colour similarity

@pytest.mark.parametrize("name", list(P.COLOR))
def test_colour_similarity_per_entry(name):
    from uninext_amd import _lib, ext
    since = len(P.TABLE)
    worst = []
    for kind in ("u8", "f32"):
        p = P.color_inputs(name, kind)
        ref = P.color64(p)
        bs, _, h, w = ref["lab"].shape
        guard = Guarded()
        out, lab = guard((bs, 8, h, w)), guard((bs, 3, h, w))
        images, keep = dev(p["images"]), dev(p["keep"])
        ext.color_similarity(images, keep, p["stride"], p["d"], out=out, lab=lab)
        assert _lib.last_kernel("criterion") == "color_similarity<%s>" % kind
        torch.cuda.synchronize()
        guard.check()
        comp = P.color_composition(p, DEV)
        got = host(out).astype(np.float64)
        worst.append(P.measure("color." + kind, "lab", name, host(lab), ref["lab"], ref["mag_lab"], comp["lab"]))
        worst.append(P.measure("color." + kind, "sim", name, got, ref["sim"], ref["mag_sim"], comp["sim"]))
        assert not got[ref["sim"] == 0].any()                   # outside the image or not kept: exactly 0.0
        assert torch.equal(ext.color_similarity(images, keep, p["stride"], p["d"]), out)
        if kind == "u8":                                        # the two kernels on the same integer image: bit for bit
            lab2 = torch.empty_like(lab)
            same = ext.color_similarity(images.float(), keep, p["stride"], p["d"], lab=lab2)
            assert torch.equal(same, out) and torch.equal(lab2, lab)
    report(since)
    assert max(worst) <= 1.0


# ---------------------------------------------------------------------------------------------------------------- box bitmasks

@pytest.mark.parametrize("W", P.BITMASK_WS)
def test_box_bitmasks_exactly(W):
    from uninext_amd import _lib, ext
    boxes = P.bitmask_boxes(W)
    want = P.bitmasks_exact(boxes, P.BITMASK_H, W)
    guard = Guarded()
    out = guard((len(boxes), P.BITMASK_H, W), torch.uint8)
    ext.box_bitmasks(dev(boxes), P.BITMASK_H, W, out=out)
    assert _lib.last_kernel("criterion") == ("box_bitmasks<vec4>" if W % 16 == 0 else "box_bitmasks<scalar>")
    torch.cuda.synchronize()
    guard.check()
    bad = np.argwhere(host(out) != want)
    assert not len(bad), (W, "first (box, y, x)", bad[:4].tolist())
    assert torch.equal(ext.box_bitmasks(dev(boxes), P.BITMASK_H, W).to(torch.uint8), out)


def test_print_the_worst_ratios():
    """Prints the largest |error| / bound and relative error per kernel and group over the tests of this file that ran before it
    in the same process, and the composition's against the derived term; it asserts nothing (every test above asserts its own)."""
    print(P.worst_table())
