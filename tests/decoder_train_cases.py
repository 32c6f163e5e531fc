"""Shared helpers of tests/test_decoder_train_cpu.py, tests/test_decoder_train_gpu.py and
tests/golden/make_decoder_train_golden.py: the fixtures of tests/golden/decoder_train/ (minted with the reference's code), the
float64 autograd reference of the self-attention core's gradients written out from the formula in include/biattn_hip.h, the
fp32 composition's gradients on the CPU, and the error measure."""
import functools
import os

import numpy as np
import torch

import decoder_cases as C

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_train")
EXPECTED = ["layer_plain", "layer_dn_mask", "layer_float_mask", "decoder_2layers"]     # files <name>_grad.npz
GROUPS = ("dq", "dk", "dv")
G_BITS = 6            # the fixtures' upstream gradient is a multiple of 2 ** -6: exact in float16
INPUT_KEYS = {"layer": ("tgt", "query_pos", "ref", "src"), "decoder": ("tgt", "ref", "src")}


# ---- the core -------------------------------------------------------------------------------------------------------------
def core64(q, k, v, heads, mask=None, scale=None):
    """include/biattn_hip.h in float64: s[i, j] = sum_d (q[i, d] * q_scale) * k[j, d] + m[i, j], with q scaled AND ROUNDED in
    fp32 first; out = softmax_j(s) v.  q, k, v [B, L, E] (fp32 values; q may carry a float64 autograd leaf) -> [B, L, E]."""
    B, L, E = q.shape
    D = E // heads
    scale = D ** -0.5 if scale is None else scale
    s32 = np.float32(scale)
    # the fp32 product q * scale, as a float64 function of q whose derivative is the scale: value rounded, gradient straight
    qd = q.double()
    rounded = (q.detach().float() * s32).double()
    qs = rounded + (qd - qd.detach()) * float(s32)
    split = lambda t: t.double().reshape(B, L, heads, D).permute(0, 2, 1, 3)
    s = split(qs) @ split(k).transpose(-1, -2)
    if mask is not None:
        s = s.masked_fill(mask, float("-inf")) if mask.dtype == torch.bool else s + mask.double()
    return (torch.softmax(s, -1) @ split(v)).permute(0, 2, 1, 3).reshape(B, L, E)


def composition32(q, k, v, heads, mask=None, scale=None):
    """The PyTorch composition of F.multi_head_attention_forward between the projections, in fp32: q scaled first, baddbmm with
    the mask (bool: -inf filled), softmax, bmm."""
    B, L, E = q.shape
    D = E // heads
    scale = D ** -0.5 if scale is None else scale
    split = lambda t: t.reshape(B, L, heads, D).permute(0, 2, 1, 3).reshape(B * heads, L, D)
    qh, kh, vh = split(q * scale), split(k), split(v)
    if mask is None:
        s = torch.bmm(qh, kh.transpose(1, 2))
    else:
        m = torch.zeros(L, L).masked_fill(mask, float("-inf")) if mask.dtype == torch.bool else mask
        s = torch.baddbmm(m, qh, kh.transpose(1, 2))
    return torch.bmm(torch.softmax(s, -1), vh).reshape(B, heads, L, D).permute(0, 2, 1, 3).reshape(B, L, E)


def _grads_of(core, qk, v, heads, mask, scale, G, dtype):
    E = v.shape[-1]
    qk = qk.to(dtype).clone().requires_grad_(True)
    v = v.to(dtype).clone().requires_grad_(True)
    out = core(qk[..., :E], qk[..., E:], v, heads, mask, scale)
    (out * G.to(out.dtype)).sum().backward()
    return {"dq": qk.grad[..., :E].detach(), "dk": qk.grad[..., E:].detach(), "dv": v.grad.detach()}, out.detach()


def reference_grads(qk, v, heads, mask, G, scale=None, dead=()):
    """Float64 autograd of core64 on fp32 qk [B, L, 2 E] (q | k) and v: ({"dq", "dk", "dv"}, out).  dead: queries whose keys are
    all excluded.  What the kernels define for them (include/biattn_hip.h) is that they contribute nothing to dk and dv: the
    reference is computed with their upstream gradient set to zero (and their mask rows opened, so that float64 autograd has a
    finite row to multiply the zero with); their own dq rows are zero here and NaN in the kernels."""
    if dead:
        G = G.clone()
        G[:, list(dead)] = 0.0
        mask = mask.clone()
        mask[list(dead)] = False if mask.dtype == torch.bool else 0.0
    return _grads_of(core64, qk, v, heads, mask, scale, G, torch.float64)


def composition_grads(qk, v, heads, mask, G, scale=None):
    """fp32 autograd of the PyTorch composition, on the CPU."""
    return _grads_of(composition32, qk, v, heads, mask, scale, G, torch.float32)[0]


def upstream(seed, B, L, E):
    return torch.randn(B, L, E, generator=torch.Generator().manual_seed(1000 + seed))


def bool_mask(seed, L):
    m = torch.rand(L, L, generator=torch.Generator().manual_seed(seed)) < 0.3
    m[:, 0] = False                                    # no row is empty
    return m


def mask_of(kind, seed, L):
    """None, a bool mask (0.3 excluded, column 0 open) or decoder_cases.float_mask (a quarter -inf, column 0 open)."""
    if kind == "none":
        return None
    return bool_mask(seed, L) if kind == "bool" else C.float_mask(torch.Generator().manual_seed(seed), L).float()


@functools.lru_cache(maxsize=None)
def random_reference(seed, B, L, heads, kind):
    """(qk, v, mask, upstream gradient, float64 gradients, fp32 composition's gradients, float64 out): computed once."""
    qk, v = C.kernel_case(seed, B, L, heads)
    mask = mask_of(kind, seed, L)
    G = upstream(seed, B, L, heads * 32)
    want, out = reference_grads(qk, v, heads, mask, G)
    return qk, v, mask, G, want, composition_grads(qk, v, heads, mask, G), out


def group_err(got, want):
    """Per group: max abs error over the group's max abs, every entry compared.  A group that is exactly zero in float64 (one
    key: the softmax is constant, dq = dk = 0) has no scale of its own; its error is held to dv's scale, the product of the
    same g, p and unit-variance rows without the cancellation (tests/vit_train_cases.py)."""
    errs = {}
    dv = float(want["dv"].abs().max())
    for k in want:
        scale = float(want[k].abs().max())
        scale = scale if scale > 1e-12 * dv else dv
        errs[k] = float((got[k].detach().cpu().double() - want[k].double()).abs().max() / scale)
    return errs


# ---- the fixtures ---------------------------------------------------------------------------------------------------------
def fixture_upstream(name):
    """The seeded G of a fixture's loss, one per output, multiples of 2 ** -G_BITS: (G,) for a layer's output [B, Lq, d]; for
    the decoder (built with look_forward_twice, so that the box heads' points come out undetached and every parameter has a
    gradient) the stack of the layers' outputs [layers, B, Lq, d] and the stack of the points [layers, B, Lq, 4]."""
    cfg = C.FIXTURES[name]
    g = torch.Generator().manual_seed(cfg["seed"] + 5000)
    step = float(1 << G_BITS)
    draw = lambda *shape: torch.round(torch.randn(*shape, generator=g, dtype=torch.float64) * 0.5 * step) / step
    if cfg["kind"] == "layer":
        return (draw(2, cfg["lq"], cfg["d_model"]),)
    return draw(cfg["layers"], 2, cfg["lq"], cfg["d_model"]), draw(cfg["layers"], 2, cfg["lq"], 4)


def stored_rows(name, key, rows, keep):
    """The seeded subset of `keep` of a large parameter's `rows` rows that the fixture stores (sorted)."""
    g = torch.Generator().manual_seed(C.FIXTURES[name]["seed"] + sum(ord(c) for c in key))
    return torch.sort(torch.randperm(rows, generator=g)[:keep])[0]


def load(name):
    z = np.load(os.path.join(HERE, name + "_grad.npz"))
    fx = {k: z[k] for k in z.files}
    fx["grad"] = {k[len("grad."):]: torch.from_numpy(fx.pop(k)) for k in list(fx) if k.startswith("grad.")}
    fx["G"] = tuple(torch.from_numpy(fx.pop(k).astype(np.float64)) for k in ("G", "G_points") if k in fx)
    return fx


def stored_view(fx, key, got):
    """`got` cut down to what the fixture stores under grad.<key>: the rows of `rows.<key>` of the flattened leading axes."""
    if "rows." + key in fx:
        return got.reshape(-1, got.shape[-1])[torch.from_numpy(fx["rows." + key]).to(got.device)]
    return got


def gradients(cfg, m, x, G, dtype, device="cpu"):
    """({input key or parameter name: gradient} of sum_n sum(out_n . G_n) on module m (a layer or a decoder, from
    decoder_cases.build or the reference's classes), the outputs); G as fixture_upstream gives it."""
    t = lambda k: None if k not in x else (x[k].to(device) if x[k].dtype in (torch.bool, torch.long) else x[k].to(dtype).to(device))
    leaves = {k: t(k).clone().requires_grad_(True) for k in INPUT_KEYS[cfg["kind"]]}
    for p in m.parameters():
        p.grad = None
    with torch.enable_grad():
        if cfg["kind"] == "layer":
            outs = (m(leaves["tgt"], leaves["query_pos"], leaves["ref"], leaves["src"], t("shapes"), t("lsi"), t("padding_mask"),
                      t("attn_mask")),)
        else:
            outs = m(leaves["tgt"], leaves["ref"], leaves["src"], t("shapes"), t("lsi"), t("valid_ratios"), None, t("padding_mask"),
                     None)
        assert len(outs) == len(G)
        sum((o * g.to(o.dtype).to(device)).sum() for o, g in zip(outs, G)).backward()
    got = {k: v.grad for k, v in leaves.items()}
    got.update({n: p.grad for n, p in m.named_parameters()})
    return got, tuple(o.detach() for o in outs)
