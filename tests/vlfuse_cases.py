"""Shared helpers of tests/test_vlfuse_cpu.py and tests/test_vlfuse_gpu.py: the fixtures of tests/golden/vlfuse/ (minted by
tests/golden/make_vlfuse_golden.py with the reference's code) and modules built from them."""
import glob
import os
from types import SimpleNamespace as NS

import numpy as np
import torch

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vlfuse")
NAMES = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(HERE, "*.npz")))
EXPECTED = ["t1_nomask", "t256_partial", "t37_fullmask", "t37_partial"]
TOL = 1e-4            # the project's bound: max abs error <= 1e-4 of the output's max abs, against float64 (README)
TOL_REFERENCE_FP32 = 3e-5   # what the fp32 PyTorch composition itself must keep on every fixture (|score| <~ 500)
TOL_EXACT = 1e-6      # exact-score family: only exp and the final fp32 sums differ


def load(name):
    z = np.load(os.path.join(HERE, name + ".npz"))
    fx = {k: z[k] for k in z.files}
    fx["state"] = {k[len("state."):]: torch.from_numpy(fx.pop(k)) for k in list(fx) if k.startswith("state.")}
    return fx


def fuse_cfg(stable=False, clamp_min=True, clamp_max=True):
    return NS(STABLE_SOFTMAX_2D=stable, CLAMP_MIN_FOR_UNDERFLOW=clamp_min, CLAMP_MAX_FOR_OVERFLOW=clamp_max)


def vlfuse_cfg(img_dim, lang_dim, embed_dim, enc_layers=6, checkpoint=False):
    """The cfg fields VLFuse reads (vlfusion.py:88-103)."""
    return NS(MODEL=NS(VL_FUSION_USE_CHECKPOINT=checkpoint,
                       LANGUAGE_BACKBONE=NS(MODEL_TYPE="bert-base-uncased", MAX_QUERY_LEN=256, N_LAYERS=1, LANG_DIM=lang_dim),
                       DDETRS=NS(HIDDEN_DIM=img_dim, VL_HIDDEN_DIM=embed_dim, ENC_LAYERS=enc_layers),
                       DYHEAD=NS(FUSE_CONFIG=fuse_cfg())))


def block_from(fx, dtype, device="cpu"):
    from uninext_amd.modules import BiAttentionBlockForCheckpoint
    st = fx["state"]
    v_dim, l_dim = st["layer_norm_v.weight"].numel(), st["layer_norm_l.weight"].numel()
    embed = st["attn.v_proj.weight"].shape[0]
    blk = BiAttentionBlockForCheckpoint(v_dim=v_dim, l_dim=l_dim, embed_dim=embed, num_heads=int(fx["num_heads"]), dropout=0.1,
                                        drop_path=.0, init_values=float(fx["init_values"]),
                                        cfg=NS(MODEL=NS(DYHEAD=NS(FUSE_CONFIG=fuse_cfg()))))
    blk.load_state_dict(st, strict=True)
    return blk.to(dtype).to(device).eval()


def vlfuse_from(fx, dtype, device="cpu"):
    from uninext_amd.modules import VLFuse
    st = fx["state"]
    v_dim, l_dim = st["layer_norm_v.weight"].numel(), st["layer_norm_l.weight"].numel()
    embed = st["attn.v_proj.weight"].shape[0]
    m = VLFuse(vlfuse_cfg(v_dim, l_dim, embed))
    m.b_attn.attn.num_heads = int(fx["num_heads"])          # VLFuse fixes 8 heads; the fixtures use fewer of 256 each
    m.b_attn.attn.head_dim = embed // int(fx["num_heads"])
    m.b_attn.attn.scale = m.b_attn.attn.head_dim ** (-0.5)
    m.load_state_dict({"b_attn." + k: v for k, v in st.items()}, strict=True)
    return m.to(dtype).to(device).eval()


def inputs(fx, dtype, device="cpu"):
    v = torch.from_numpy(fx["visual"]).to(dtype).to(device)
    l = torch.from_numpy(fx["hidden"]).to(dtype).to(device)
    m = torch.from_numpy(fx["masks"]).to(device) if "masks" in fx else None
    return v, l, m


def core_inputs(fx, dtype, device="cpu"):
    """q (unscaled), k, vv, vl of the attention core, recomputed from the stored inputs and parameters in `dtype`."""
    blk = block_from(fx, dtype, device)
    v, l, m = inputs(fx, dtype, device)
    with torch.no_grad():
        nv, nl = blk.layer_norm_v(v), blk.layer_norm_l(l)
        a = blk.attn
        return a.v_proj(nv), a.l_proj(nl), a.values_v_proj(nv), a.values_l_proj(nl), m, a.num_heads, a.scale


def fully_masked_images(fx):
    """Batch indices whose text tokens are all masked: the float64 reference keeps the scores there (module docstring of
    tests/vlfuse_ref.py), fp32 gives the uniform row; they stay out of comparisons of the image side against float64."""
    if "masks" not in fx:
        return []
    return [b for b in range(fx["masks"].shape[0]) if not fx["masks"][b].any()]


def rel_err(got, want):
    want = want.double()
    return float((got.double() - want).abs().max() / want.abs().max())
