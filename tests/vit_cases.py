"""Shared helpers of tests/test_vit_cpu.py and tests/test_vit_gpu.py: the fixtures of tests/golden/vit/ (minted by
tests/golden/make_vit_golden.py with the reference's code) and modules built from them."""
import glob
import os

import numpy as np
import torch

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vit")
NAMES = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(HERE, "*.npz")))
EXPECTED = ["attn_global_interp", "attn_win_d64", "attn_win_d80", "block_global", "block_win_padded", "net_small"]
TOL = 1e-4            # the project's bound: max abs error <= 1e-4 of the output's max abs, against float64 (tests/vlfuse_cases.py)
TOL_EXACT = 1e-6      # exact-score family: only exp and the final fp32 sums differ

# kernel shapes (q_h, q_w) and the hazard each is the smallest to reach
SHAPES = [(1, 1), (2, 7), (3, 5),     # less than one tile
          (14, 14),                   # key tail of 4 in the 7th tile; query tail in the second workgroup
          (9, 15),                    # 135: crosses a 128-query workgroup by 7
          (20, 23),                   # 460: many key tiles, q_w not dividing 32
          (37, 61)]                   # 2257: many workgroups per head; long running-max chain


def load(name):
    z = np.load(os.path.join(HERE, name + ".npz"))
    fx = {k: z[k] for k in z.files}
    fx["state"] = {k[len("state."):]: torch.from_numpy(fx.pop(k).astype(np.float64)) for k in list(fx) if k.startswith("state.")}
    if "x" not in fx:     # the network's image is stored as its two factors
        fx["x"] = fx["x_rows"][..., None] + fx["x_cols"][..., None, :]
    return fx


def module_from(name, fx, dtype, device="cpu"):
    from uninext_amd import vit
    st = fx["state"]
    heads = int(fx["num_heads"])
    if name.startswith("attn_"):
        dim = st["proj.weight"].shape[0]
        m = vit.Attention(dim, num_heads=heads, use_rel_pos=True, input_size=((st["rel_pos_h"].shape[0] + 1) // 2,
                                                                              (st["rel_pos_w"].shape[0] + 1) // 2))
    elif name.startswith("block_"):
        dim = st["attn.proj.weight"].shape[0]
        window = 14 if name == "block_win_padded" else 0
        m = vit.Block(dim, heads, use_rel_pos=True, window_size=window, input_size=(64, 64) if window else (17, 20))
    else:
        m = vit.ViT(img_size=1024, embed_dim=128, depth=4, num_heads=heads, mlp_ratio=float(fx["mlp_ratio"]), use_rel_pos=True,
                    window_size=14, window_block_indexes=(0, 1, 3), pretrain_img_size=224, pretrain_use_cls_token=True)
    m.load_state_dict(st, strict=True)
    return m.to(dtype).to(device).eval()


def first_attention(m):
    from uninext_amd import vit
    return next(a for a in m.modules() if isinstance(a, vit.Attention))


def run_with_core(m, x):
    """(module output, input of the first Attention's qkv-to-proj core [B', S, 3 E], its output [B', S, E])."""
    a, seen = first_attention(m), {}
    def keep(key, t):      # a hook that returns a tensor would replace the layer's output
        seen.setdefault(key, t.detach())
    hooks = [a.qkv.register_forward_hook(lambda mod, i, o: keep("core_in", o)),
             a.proj.register_forward_hook(lambda mod, i, o: keep("core_out", i[0]))]
    try:
        with torch.no_grad():
            out = m(x)
    finally:
        for h in hooks:
            h.remove()
    ci, co = seen["core_in"], seen["core_out"]
    return out, ci.reshape(ci.shape[0], -1, ci.shape[-1]), co.reshape(co.shape[0], -1, co.shape[-1])


def stored_view(fx, key, got):
    """`got` cut down to what the fixture stores under `key` (token rows of [B, H, W, C] outputs, channel steps of NCHW maps)."""
    if key + "_step" in fx:
        return got[:, ::int(fx[key + "_step"])]
    if key == "out" and "out_rows" in fx:
        return got.reshape(got.shape[0], -1, got.shape[-1])[:, torch.from_numpy(fx["out_rows"])]
    if key == "core_out":
        return got[:, torch.from_numpy(fx["rows"])]
    return got


def output_keys(fx):
    return [k for k in ("out", "res3", "res4", "res5") if k in fx]


def rel_err(got, want):
    want = torch.as_tensor(want).double()
    return float((got.detach().cpu().double() - want).abs().max() / want.abs().max())


def random_case(seed, B, heads, q_hw, D, rel=True, table_gain=0.3):
    g = torch.Generator().manual_seed(seed)
    S = q_hw[0] * q_hw[1]
    qkv = torch.randn(B, S, 3 * heads * D, generator=g)
    th = torch.randn(2 * q_hw[0] - 1, D, generator=g) * table_gain if rel else None
    tw = torch.randn(2 * q_hw[1] - 1, D, generator=g) * table_gain if rel else None
    return qkv, th, tw, D ** -0.5
