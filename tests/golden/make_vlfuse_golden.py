"""Mint fixtures for the early vision-language fusion layer with the REFERENCE's own code (build container only).

    UNINEXT_REFERENCE=<checkout of the reference> python tests/golden/make_vlfuse_golden.py

Loads projects/UNINEXT/uninext/models/deformable_detr/fuse_helper.py as it is (its one foreign import, timm's DropPath, is
replaced by a stub of this file: VLFuse passes drop_path = 0, which is nn.Identity there), builds
BiAttentionBlockForCheckpoint the way VLFuse does (vlfusion.py:78-86: 8 -> here 2 heads, dropout 0.1, drop_path 0,
init_values 1 / ENC_LAYERS) with small v_dim / l_dim and embed_dim = heads * 256, and runs it in float64 in eval().  vlfusion.py
itself imports `transformers` for the BERT layer and cannot be loaded; VLFuse.forward only wraps the block's call in the
features dict (vlfusion.py:100-120), which tests/test_vlfuse_*.py restate.

Every file of tests/golden/vlfuse/ holds data only: inputs (visual, hidden, masks), the block's state_dict, the block's outputs
and BiMultiHeadAttention's outputs on the normalised inputs (float64), and the inputs of out_v_proj / out_l_proj -- the
attention core's outputs -- rounded to float32 (2^-24 relative, far inside the 1e-4 bound) to keep each file under 1 MB.
Inputs and parameters are multiples of 2^-10, exact in fp32.  The projections of q and k are scaled up so that the scores reach
a few tens to hundreds: a softmax that is far from uniform, inside the range where fp32 itself stays within 3e-5 of float64.
"""
import importlib.util
import os
import sys
import types
from types import SimpleNamespace as NS

import numpy as np
import torch
import torch.nn as nn

REF = os.environ.get("UNINEXT_REFERENCE")
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vlfuse")
HEADS, HEAD_DIM, V_DIM, L_DIM, ENC_LAYERS = 2, 256, 16, 24, 6


def load_reference_fuse_helper():
    class DropPath(nn.Module):          # never constructed: drop_path = 0 takes nn.Identity in the reference
        def __init__(self, p=0.0):
            super().__init__()
            raise RuntimeError("DropPath stub: drop_path > 0 is not part of these fixtures")
    timm = types.ModuleType("timm")
    timm.models = types.ModuleType("timm.models")
    timm.models.layers = types.ModuleType("timm.models.layers")
    timm.models.layers.DropPath = DropPath
    for name, mod in (("timm", timm), ("timm.models", timm.models), ("timm.models.layers", timm.models.layers)):
        sys.modules.setdefault(name, mod)
    path = os.path.join(REF, "projects/UNINEXT/uninext/models/deformable_detr/fuse_helper.py")
    spec = importlib.util.spec_from_file_location("ref_fuse_helper", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_cfg():
    fuse = NS(STABLE_SOFTMAX_2D=False, CLAMP_MIN_FOR_UNDERFLOW=True, CLAMP_MAX_FOR_OVERFLOW=True)
    return NS(MODEL=NS(DYHEAD=NS(FUSE_CONFIG=fuse)))


def dyadic(t, scale=1.0):
    return torch.round(t * scale * 1024.0) / 1024.0


def run(ref, name, B, S, T, mask_kind, gain):
    block = ref.BiAttentionBlockForCheckpoint(v_dim=V_DIM, l_dim=L_DIM, embed_dim=HEADS * HEAD_DIM, num_heads=HEADS, dropout=0.1,
                                              drop_path=.0, init_values=1.0 / ENC_LAYERS, cfg=make_cfg()).double().eval()
    with torch.no_grad():
        for n, p in block.named_parameters():
            g = gain if n in ("attn.v_proj.weight", "attn.l_proj.weight") else 1.0
            if n.endswith(".bias"):
                p.copy_(dyadic(torch.rand_like(p) - 0.5, 0.25))      # make the biases count
            else:
                p.copy_(dyadic(p, g))
    visual = dyadic(torch.randn(B, S, V_DIM, dtype=torch.float64))
    hidden = dyadic(torch.randn(B, T, L_DIM, dtype=torch.float64))
    masks = None
    if mask_kind != "none":
        masks = (torch.rand(B, T) > 0.35).long()
        masks[:, 0] = 1
        if mask_kind == "full":
            masks[B - 1] = 0                                          # every token of the last image is masked
    seen = {}
    hooks = [block.attn.out_v_proj.register_forward_hook(lambda m, i, o: seen.__setitem__("core_v", i[0].detach())),
             block.attn.out_l_proj.register_forward_hook(lambda m, i, o: seen.__setitem__("core_l", i[0].detach()))]
    with torch.no_grad():
        out_v, out_l = block(visual, hidden, masks, None)
        core_v, core_l = seen["core_v"], seen["core_l"]
        nv, nl = block.layer_norm_v(visual), block.layer_norm_l(hidden)
        attn_v, attn_l = block.attn(nv, nl, attention_mask_l=masks)
        q = block.attn.v_proj(nv) * block.attn.scale
        k = block.attn.l_proj(nl)
        smax = float(torch.einsum("bshd,bthd->bhst", q.view(B, S, HEADS, HEAD_DIM), k.view(B, T, HEADS, HEAD_DIM)).abs().max())
    for h in hooks:
        h.remove()
    f64 = lambda t: t.detach().contiguous().numpy().astype(np.float64)
    f32 = lambda t: t.detach().contiguous().numpy().astype(np.float32)
    data = dict(visual=f64(visual), hidden=f64(hidden), out_visual=f64(out_v), out_hidden=f64(out_l), attn_out_v=f64(attn_v),
                attn_out_l=f64(attn_l), core_out_v=f32(core_v), core_out_l=f32(core_l), num_heads=np.array(HEADS),
                init_values=np.array(1.0 / ENC_LAYERS), score_absmax=np.array(smax))
    if masks is not None:
        data["masks"] = masks.numpy().astype(np.int64)
    for n, t in block.state_dict().items():
        data["state." + n] = f64(t)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **data)
    print(name, (B, S, T), mask_kind, "max |score| %.1f" % smax, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


def main():
    if not REF:
        raise SystemExit("set UNINEXT_REFERENCE to a checkout of the reference project")
    ref = load_reference_fuse_helper()
    os.makedirs(HERE, exist_ok=True)
    torch.manual_seed(23)
    run(ref, "t1_nomask", 2, 200, 1, "none", 24.0)
    run(ref, "t37_partial", 2, 160, 37, "partial", 24.0)
    run(ref, "t37_fullmask", 2, 160, 37, "full", 24.0)
    run(ref, "t256_partial", 1, 100, 256, "partial", 32.0)


if __name__ == "__main__":
    main()
