"""Mint gradient fixtures for the ViT backbone blocks with the REFERENCE's own code (build container only).

    UNINEXT_REFERENCE=<checkout of the reference> python tests/golden/make_vit_train_golden.py

The reference's backbone/vit.py and backbone/utils.py are loaded as tests/golden/make_vit_golden.py loads them (same stubs), the
modules are filled with the same dyadic parameters and run in float64 in eval().  The loss is sum(out . G) with a stored G per
output, G[..., r, c] = G_rows[..., r] + G_cols[..., c] over the output's last two axes (two small dyadic factors instead of a
tensor of the output's size).  Every file of tests/golden/vit_train/ holds data only: the input, the state_dict (float16 or
float32, whichever is exact), the key list, the factors of G, and the float64 gradients of the input ("grad.x") and of every
parameter ("grad.<name>"), stored rounded to float32, large ones at a subset of the rows of their flattened leading axes
("rows.<name>") to keep each file under 500 KB.

The relative-position tables are non-zero in the attn and block files and ZERO in the net file, the reference's initial state: their
gradients are non-zero there all the same (asserted).  Per gradient the reference's own fp32 run stays within 3e-5 of its float64
run (asserted; the margin of make_vit_golden.py) -- a case that fails it gets a lower score gain.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_vit_golden as M   # noqa: E402

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vit_train")
CAP = 2048          # stored elements of one gradient (the network, with its 60 parameters: 512)


def factors(out):
    return M.dyadic(torch.randn(out.shape[:-1]), 0.5), M.dyadic(torch.randn(out.shape[:-2] + out.shape[-1:]), 0.5)


def gradients(module, x, G):
    x = x.clone().requires_grad_(True)
    for p in module.parameters():
        p.grad = None
    out = module(x)
    outs = out if isinstance(out, dict) else {"out": out}
    sum((outs[k] * (G[k][0][..., None] + G[k][1][..., None, :]).to(outs[k].dtype)).sum() for k in sorted(outs)).backward()
    got = {"x": x.grad.detach().clone()}
    got.update({n: p.grad.detach().clone() for n, p in module.named_parameters()})
    return got, outs


def run(module, x, name, extra=None, store_x=True, cap=CAP):
    module = module.double().eval()
    with torch.no_grad():
        outs = module(x)
    outs = outs if isinstance(outs, dict) else {"out": outs}
    G = {k: factors(v) for k, v in sorted(outs.items())}
    want, _ = gradients(module, x, G)
    got32, _ = gradients(module.float(), x.float(), G)
    module.double()
    errs = {k: float((got32[k].double() - want[k]).abs().max() / want[k].abs().max()) for k in want}
    worst = max(errs, key=errs.get)
    assert errs[worst] < 3e-5, (name, worst, errs[worst])
    for k, g in want.items():
        assert float(g.abs().max()) > 0, (name, k)

    f32 = lambda a: a.detach().contiguous().numpy().astype(np.float32)
    data = dict(fp32_err=np.array(errs[worst]), num_heads=np.array(M.first_attention(module).num_heads),
                keys=np.array(list(module.state_dict().keys())))
    assert float((x.float().double() - x).abs().max()) == 0
    if store_x:
        data["x"] = f32(x)
    for k, (gr, gc) in G.items():
        data["G_rows." + k], data["G_cols." + k] = f32(gr), f32(gc)
    for k, g in want.items():
        flat = g.reshape(-1, g.shape[-1])
        if flat.numel() > cap:
            step = -(-flat.numel() // cap)
            rows = np.unique(np.concatenate([np.arange(0, flat.shape[0], step), [flat.shape[0] - 1]]))
            data["rows." + k] = rows
            flat = flat[torch.from_numpy(rows)]
            data["grad." + k] = f32(flat)
        else:
            data["grad." + k] = f32(g)
    for n, p in module.state_dict().items():
        assert float((p.float().double() - p).abs().max()) == 0, n
        half = p.detach().numpy().astype(np.float16)
        data["state." + n] = half if float(np.abs(half.astype(np.float64) - p.detach().numpy()).max()) == 0 else f32(p)
    data.update(extra or {})
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **data)
    print("%-26s %d gradients, worst fp32 err %.1e (%s) %d bytes" % (name, len(want), errs[worst], worst, os.path.getsize(path)))
    assert os.path.getsize(path) < 500000, name


def main():
    if not M.REF:
        raise SystemExit("set UNINEXT_REFERENCE to a checkout of the reference project")
    ref = M.load_reference()
    os.makedirs(HERE, exist_ok=True)
    torch.manual_seed(47)
    torch.set_default_dtype(torch.float64)
    inp = lambda *shape: M.dyadic(torch.randn(*shape))

    a = ref.Attention(160, num_heads=2, use_rel_pos=True, input_size=(14, 14))
    M.fill(a, 2.0, 160)
    run(a, inp(2, 14, 14, 160), "attn_win_d80_grad")

    a = ref.Attention(128, num_heads=2, use_rel_pos=True, input_size=(64, 64))      # tables of 127 rows, interpolated to 33 and 39
    M.fill(a, 2.0, 128)
    run(a, inp(2, 17, 20, 128), "attn_global_interp_grad")

    b = ref.Block(128, 2, use_rel_pos=True, window_size=14, input_size=(64, 64))    # 17 x 20 tokens padded to 28 x 28
    M.fill(b, 2.0, 128)
    run(b, inp(1, 17, 20, 128), "block_win_padded_grad")

    M.STEP_BITS = 4        # the network's 0.6 M parameters at a coarser step, to stay under the size limit
    net = ref.ViT(img_size=1024, embed_dim=128, depth=4, num_heads=2, mlp_ratio=1.0, use_rel_pos=True, window_size=14,
                  window_block_indexes=(0, 1, 3), pretrain_img_size=224, pretrain_use_cls_token=True)
    M.fill(net, 1.5, 128)
    with torch.no_grad():
        net.patch_embed.proj.weight.copy_(M.dyadic(torch.randn_like(net.patch_embed.proj.weight) * 768 ** -0.5))
        net.fpn1[0].weight.copy_(M.dyadic(torch.randn_like(net.fpn1[0].weight) * 128 ** -0.5))
        for n, p in net.named_parameters():
            if n.endswith("rel_pos_h") or n.endswith("rel_pos_w"):
                p.zero_()
    rows, cols = inp(2, 3, 272), inp(2, 3, 320)
    run(net, rows[..., None] + cols[..., None, :], "net_small_grad", store_x=False, cap=512,
        extra=dict(x_rows=rows.numpy().astype(np.float32), x_cols=cols.numpy().astype(np.float32), mlp_ratio=np.array(1.0)))


if __name__ == "__main__":
    main()
