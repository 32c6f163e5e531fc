"""Mint fixtures for the ViT backbone blocks with the REFERENCE's own code (build container only).

    UNINEXT_REFERENCE=<checkout of the reference> python tests/golden/make_vit_golden.py

Loads projects/UNINEXT/uninext/backbone/utils.py as it is (it imports only torch) and backbone/vit.py with stubs of this file for
its foreign imports: fvcore.nn.weight_init, detectron2.layers, detectron2.modeling[.backbone.fpn] and timm.models.layers
(DropPath: never constructed, drop_path = 0 is nn.Identity there; Mlp: fc1 -> GELU -> fc2).  Everything runs in float64 in eval().

Every file of tests/golden/vit/ holds data only: the input, the state_dict (stored as float16 or float32, whichever is exact: every parameter and
input is a multiple of 2^-STEP_BITS of small magnitude, the relative-position tables -- zero in the reference -- and the biases
included), the list of state-dict keys, the module's output, the attention core's output (the input of `proj`, taken by a hook on
the FIRST Attention of the module) and score_absmax.  To keep each file under 500 KB, outputs are stored in float64 at the token
(or channel) subset `rows` (`chans`) only, and the core's input (3 x as wide) is stored rounded to float32 at every second of those rows
(`core_in_rows`): the tests recompute it in float64 as `qkv(x)` of the stored input and parameters and hold it to these.  The weights of q and k are scaled up so that the scores reach a few tens:
a softmax that is neither flat nor one-hot (asserted: the median over rows of the largest probability lies in [0.05, 0.9]),
inside the range where the reference's own fp32 run stays within 3e-5 of its float64 run (asserted on every file).
"""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

REF = os.environ.get("UNINEXT_REFERENCE")
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vit")
STEP_BITS = 6


def load_reference():
    class DropPath(nn.Module):
        def __init__(self, p=0.0):
            super().__init__()
            raise RuntimeError("DropPath stub: drop_path > 0 is not part of these fixtures")

    class Mlp(nn.Module):
        def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU):
            super().__init__()
            self.fc1 = nn.Linear(in_features, hidden_features or in_features)
            self.act = act_layer()
            self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)

        def forward(self, x):
            return self.fc2(self.act(self.fc1(x)))

    class Registry:
        def register(self):
            return lambda cls: cls

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    mod("fvcore"), mod("fvcore.nn"), mod("fvcore.nn.weight_init")
    sys.modules["fvcore.nn"].weight_init = sys.modules["fvcore.nn.weight_init"]
    mod("detectron2")
    mod("detectron2.layers", CNNBlockBase=nn.Module, Conv2d=nn.Conv2d, get_norm=None)
    mod("detectron2.modeling", BACKBONE_REGISTRY=Registry(), Backbone=nn.Module, ShapeSpec=dict)
    mod("detectron2.modeling.backbone")
    mod("detectron2.modeling.backbone.fpn", _assert_strides_are_log2_contiguous=None)
    mod("timm"), mod("timm.models"), mod("timm.models.layers", DropPath=DropPath, Mlp=Mlp)
    pkg = mod("ref_backbone")
    pkg.__path__ = [os.path.join(REF, "projects/UNINEXT/uninext/backbone")]
    return importlib.import_module("ref_backbone.vit")


def dyadic(t, scale=1.0):
    step = float(1 << STEP_BITS)
    return torch.round(t * scale * step) / step


def fill(module, gain, dim):
    """Non-trivial dyadic parameters everywhere; the q and k rows of every qkv weight carry `gain`."""
    with torch.no_grad():
        for n, p in module.named_parameters():
            if n.endswith("rel_pos_h") or n.endswith("rel_pos_w"):
                p.copy_(dyadic(torch.randn_like(p), 0.25))
            elif n.endswith("pos_embed"):
                p.copy_(dyadic(torch.randn_like(p), 0.5))
            elif n.endswith(".bias"):
                p.copy_(dyadic(torch.rand_like(p) - 0.5, 0.5))
            elif n.endswith("norm1.weight") or n.endswith("norm2.weight"):
                p.copy_(dyadic(1.0 + 0.25 * (torch.rand_like(p) - 0.5)))
            elif n.endswith("qkv.weight"):
                w = torch.randn_like(p) * dim ** -0.5
                w[:2 * dim] *= gain
                p.copy_(dyadic(w))
            else:
                p.copy_(dyadic(torch.randn_like(p) * p.shape[-1] ** -0.5 if p.dim() > 1 else torch.randn_like(p)))


def first_attention(module):
    for m in module.modules():
        if type(m).__name__ == "Attention":
            return m
    raise RuntimeError("no Attention")


def run(module, x, name, extra=None, subset=None, store_x=True, row_step=10):
    module = module.double().eval()
    attn = first_attention(module)
    seen = {}
    hooks = [attn.proj.register_forward_hook(lambda m, i, o: seen.__setitem__("core_out", i[0].detach())),
             attn.qkv.register_forward_hook(lambda m, i, o: seen.__setitem__("core_in", o.detach()))]
    with torch.no_grad():
        out = module(x)
        core_in, core_out = seen["core_in"], seen["core_out"]
        m32 = module.float()
        out32 = m32(x.float())
        core_out32 = seen["core_out"]
        module.double()
    for h in hooks:
        h.remove()
    outs = out if isinstance(out, dict) else {"out": out}
    outs32 = out32 if isinstance(out32, dict) else {"out": out32}
    rel = lambda a, b: float((a.double() - b).abs().max() / b.abs().max())
    fp32_err = max([rel(outs32[k], outs[k]) for k in outs] + [rel(core_out32, core_out)])
    assert fp32_err < 3e-5, (name, fp32_err)

    # the softmax of the first Attention, restated from its stored input: neither flat nor one-hot
    Bp, H, W, E3 = core_in.shape
    heads, S = attn.num_heads, H * W
    t = core_in.reshape(Bp, S, 3, heads, -1).permute(2, 0, 3, 1, 4).reshape(3, Bp * heads, S, -1)
    s = (t[0] * attn.scale) @ t[1].transpose(-2, -1)
    if attn.use_rel_pos:
        s = sys.modules["ref_backbone.utils"].add_decomposed_rel_pos(s, t[0], attn.rel_pos_h, attn.rel_pos_w, (H, W), (H, W))
    # (over the rows of the first window: it holds no padded token, whose query is the bias alone and whose row is flat)
    pmax = float(s.detach()[:heads].softmax(-1).max(-1)[0].median())
    assert 0.05 <= pmax <= 0.9, (name, pmax)
    smax = float(s.detach().abs().max())

    f64 = lambda a: a.detach().contiguous().numpy().astype(np.float64)
    f32 = lambda a: a.detach().contiguous().numpy().astype(np.float32)
    S_tokens = core_out.shape[1] * core_out.shape[2]
    rows = np.unique(np.concatenate([np.arange(0, S_tokens, row_step), [S_tokens - 1]]))
    data = dict(score_absmax=np.array(smax), softmax_median_max=np.array(pmax), fp32_err=np.array(fp32_err),
                num_heads=np.array(heads), rows=rows, core_out=f64(core_out.reshape(Bp, S_tokens, -1)[:, rows]),
                keys=np.array(list(module.state_dict().keys())),
                core_in_rows=rows[::2], core_in=f32(core_in.reshape(Bp, S_tokens, -1)[:, rows[::2]]))
    assert float((x.float().double() - x).abs().max()) == 0
    if store_x:
        data["x"] = f32(x)
    for k, v in outs.items():
        if subset and k in subset:
            data[k] = f64(v[:, ::subset[k]])
            data[k + "_step"] = np.array(subset[k])
        elif v.dim() == 4 and not isinstance(out, dict):
            Bo, Ho, Wo, _ = v.shape
            orow = np.unique(np.concatenate([np.arange(0, Ho * Wo, 10), [Ho * Wo - 1]]))
            data["out_rows"] = orow
            data[k] = f64(v.reshape(Bo, Ho * Wo, -1)[:, orow])
        else:
            data[k] = f64(v)
    for n, p in module.state_dict().items():
        assert float((p.float().double() - p).abs().max()) == 0, n
        half = p.detach().numpy().astype(np.float16)      # exact for the coarse steps: half the bytes
        data["state." + n] = half if float(np.abs(half.astype(np.float64) - p.detach().numpy()).max()) == 0 else f32(p)
    data.update(extra or {})
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **data)
    print("%-20s core %s max |score| %.1f median max p %.3f fp32 err %.1e %d bytes" % (
        name, tuple(core_in.shape), smax, pmax, fp32_err, os.path.getsize(path)))
    assert os.path.getsize(path) < 500000, name


def main():
    if not REF:
        raise SystemExit("set UNINEXT_REFERENCE to a checkout of the reference project")
    ref = load_reference()
    utils = sys.modules["ref_backbone.utils"]
    os.makedirs(HERE, exist_ok=True)
    torch.manual_seed(31)
    torch.set_default_dtype(torch.float64)
    inp = lambda *shape: dyadic(torch.randn(*shape))

    for name, D in (("attn_win_d80", 80), ("attn_win_d64", 64)):
        a = ref.Attention(2 * D, num_heads=2, use_rel_pos=True, input_size=(14, 14))
        fill(a, 2.0, 2 * D)
        run(a, inp(3, 14, 14, 2 * D), name)

    a = ref.Attention(128, num_heads=2, use_rel_pos=True, input_size=(64, 64))
    fill(a, 2.0, 128)
    # get_rel_pos(n, n, t)[i, 0] is row i + n - 1 of the resized table: rows n - 1 .. 2n - 2; [0, j] is row n - 1 - j
    full = lambda n, t: torch.cat([utils.get_rel_pos(n, n, t)[0].flip(0), utils.get_rel_pos(n, n, t)[1:, 0]]).numpy()
    tabs = dict(rel_h_resized=full(17, a.rel_pos_h.detach()), rel_w_resized=full(20, a.rel_pos_w.detach()))
    run(a, inp(2, 17, 20, 128), "attn_global_interp", extra=tabs)

    b = ref.Block(128, 2, use_rel_pos=True, window_size=14, input_size=(64, 64))
    fill(b, 2.0, 128)
    run(b, inp(1, 17, 20, 128), "block_win_padded")

    b = ref.Block(128, 2, use_rel_pos=True, window_size=0, input_size=(17, 20))
    fill(b, 2.0, 128)
    run(b, inp(1, 17, 20, 128), "block_global")

    global STEP_BITS
    STEP_BITS = 4          # the network's 0.6 M parameters at a coarser step, to stay under the size limit
    net = ref.ViT(img_size=1024, embed_dim=128, depth=4, num_heads=2, mlp_ratio=1.0, use_rel_pos=True, window_size=14,
                  window_block_indexes=(0, 1, 3),
                  pretrain_img_size=224, pretrain_use_cls_token=True)
    fill(net, 1.5, 128)
    with torch.no_grad():
        net.patch_embed.proj.weight.copy_(dyadic(torch.randn_like(net.patch_embed.proj.weight) * 768 ** -0.5))
        net.fpn1[0].weight.copy_(dyadic(torch.randn_like(net.fpn1[0].weight) * 128 ** -0.5))
    # the image is stored as its two factors: x[b, c, y, x] = x_rows[b, c, y] + x_cols[b, c, x]
    rows, cols = inp(2, 3, 272), inp(2, 3, 320)
    run(net, rows[..., None] + cols[..., None, :], "net_small", subset={"res3": 64, "res4": 32, "res5": 8}, store_x=False, row_step=40,
        extra=dict(x_rows=rows.numpy().astype(np.float32), x_cols=cols.numpy().astype(np.float32), mlp_ratio=np.array(1.0)))


if __name__ == "__main__":
    main()
