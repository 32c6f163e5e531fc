"""Shared helpers of tests/test_vit_train_cpu.py and tests/test_vit_train_gpu.py: the fixtures of tests/golden/vit_train/ (minted by
tests/golden/make_vit_train_golden.py with the reference's code), modules built from them, and the float64 autograd reference of
the attention core's gradients (tests/vit_ref.py)."""
import functools
import glob
import os

import numpy as np
import torch

import vit_cases as C
import vit_ref as R

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vit_train")
NAMES = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(HERE, "*.npz")))
EXPECTED = ["attn_global_interp_grad", "attn_win_d80_grad", "block_win_padded_grad", "net_small_grad"]
GROUPS = ("dq", "dk", "dv", "dth", "dtw")
# the forward's shapes, and a one-row and a one-column grid
SHAPES = C.SHAPES + [(1, 9), (5, 1)]


def load(name):
    z = np.load(os.path.join(HERE, name + ".npz"))
    fx = {k: z[k] for k in z.files}
    fx["state"] = {k[len("state."):]: torch.from_numpy(fx.pop(k).astype(np.float64)) for k in list(fx) if k.startswith("state.")}
    fx["grad"] = {k[len("grad."):]: torch.from_numpy(fx.pop(k)) for k in list(fx) if k.startswith("grad.")}
    if "x" not in fx:     # the network's image is stored as its two factors
        fx["x"] = fx["x_rows"][..., None] + fx["x_cols"][..., None, :]
    return fx


def module_from(name, fx, dtype, device="cpu"):
    return C.module_from(name[:-len("_grad")], fx, dtype, device)


def loss_of(out, fx, device="cpu"):
    """sum(out . G): G is stored per output as its two factors, G[..., r, c] = G_rows[..., r] + G_cols[..., c] over the last two axes."""
    outs = out if isinstance(out, dict) else {"out": out}
    total = 0
    for k in sorted(outs):
        g = torch.from_numpy(fx["G_rows." + k])[..., None] + torch.from_numpy(fx["G_cols." + k])[..., None, :]
        total = total + (outs[k] * g.to(outs[k].dtype).to(device)).sum()
    return total


def gradients(m, fx, dtype, device="cpu"):
    """{"x": d loss / d input, parameter name: its gradient} of the fixture's loss on module m."""
    x = torch.from_numpy(fx["x"]).to(dtype).to(device).requires_grad_(True)
    for p in m.parameters():
        p.grad = None
    loss_of(m(x), fx, device).backward()
    got = {"x": x.grad}
    got.update({n: p.grad for n, p in m.named_parameters()})
    return got


def stored_view(fx, key, got):
    """`got` cut down to what the fixture stores under grad.<key>: the rows of `rows.<key>` of the flattened leading axes."""
    if "rows." + key in fx:
        return got.reshape(-1, got.shape[-1])[torch.from_numpy(fx["rows." + key])]
    return got


def split_qkv_grad(grad_qkv, heads):
    B, S, E3 = grad_qkv.shape
    t = grad_qkv.reshape(B, S, 3, heads, E3 // (3 * heads))
    return t[:, :, 0], t[:, :, 1], t[:, :, 2]


def upstream(seed, B, S, E):
    return torch.randn(B, S, E, generator=torch.Generator().manual_seed(1000 + seed))


def _grads_of(core, qkv, th, tw, heads, hw, scale, G, table_dtype):
    q = qkv.clone().requires_grad_(True)
    th = None if th is None else th.to(table_dtype).clone().requires_grad_(True)
    tw = None if tw is None else tw.to(table_dtype).clone().requires_grad_(True)
    out = core(q, th, tw, heads, hw, scale)
    (out * G.to(out.dtype)).sum().backward()
    dq, dk, dv = split_qkv_grad(q.grad, heads)
    got = {"dq": dq, "dk": dk, "dv": dv}
    if th is not None:
        got.update(dth=th.grad, dtw=tw.grad)
    return {k: v.detach() for k, v in got.items()}, out.detach()


def reference_grads(qkv, th, tw, heads, hw, scale, G):
    """Float64 autograd of vit_ref.core on an fp32 qkv (the scaled q is rounded in fp32, as the module does)."""
    return _grads_of(R.core, qkv, th, tw, heads, hw, scale, G, torch.float64)


def composition_grads(qkv, th, tw, heads, hw, scale, G):
    """fp32 autograd of the module's PyTorch composition, on the CPU."""
    return _grads_of(R.composition_fp32, qkv, th, tw, heads, hw, scale, G, torch.float32)[0]


@functools.lru_cache(maxsize=None)
def random_reference(seed, B, heads, hw, D, rel=True):
    """(inputs, upstream gradient, float64 gradients, fp32 composition's gradients) of vit_cases.random_case: computed once."""
    qkv, th, tw, scale = C.random_case(seed, B, heads, hw, D, rel=rel)
    G = upstream(seed, B, hw[0] * hw[1], heads * D)
    want, out = reference_grads(qkv, th, tw, heads, hw, scale, G)
    return (qkv, th, tw, scale), G, want, composition_grads(qkv, th, tw, heads, hw, scale, G), out


def group_err(got, want):
    """Per group: max abs error over the group's max abs.  A group that is exactly zero in float64 (one key: the softmax is
    constant, dq = dk = 0; a table of one row: it shifts every score of a query alike, its gradient is float64's rounding noise,
    below 1e-12 of dv) has no scale of its own; its error is held to dv's scale, the product of the same g, p and unit-variance
    rows without the cancellation."""
    errs = {}
    dv = float(want["dv"].abs().max())
    for k in want:
        scale = float(want[k].abs().max())
        scale = scale if scale > 1e-12 * dv else dv
        errs[k] = float((got[k].detach().cpu().double() - want[k].double()).abs().max() / scale)
    return errs
