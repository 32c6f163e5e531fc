"""Mint training fixtures for the early vision-language fusion layer with the REFERENCE's own code under autograd (build
container only).

    UNINEXT_REFERENCE=<checkout of the reference> python tests/golden/make_vlfuse_train_golden.py

Loads the reference's fuse_helper.py the way make_vlfuse_golden.py does (its loader, cfg and dyadic rounding are reused), builds
BiAttentionBlockForCheckpoint as VLFuse does (2 heads of 256 here, dropout 0.1, drop_path 0, init_values 1 / ENC_LAYERS) and runs
it in float64 in eval() -- dropout inactive, the condition of the own training route -- with the inputs and every parameter
requiring a gradient.  The loss is sum(out_visual * w_v) + sum(out_hidden * w_l) with stored dyadic weights.

Every file of tests/golden/vlfuse_train/ holds data only: inputs (visual, hidden, masks), the loss weights, the block's
state_dict, its two outputs, and the gradients of the two inputs ("grad.visual", "grad.hidden") and of every parameter
("grad.<name>"), all float64.  Inputs and parameters are multiples of 2^-10, exact in fp32.  The q and k projections are scaled
up so that the scores reach some tens: a softmax far from uniform, inside the range where fp32 stays well within 1e-4 of
float64.

No fixture has an image whose tokens are ALL masked: there float64 is a different function.  In fp32 the add of -9e15 absorbs
the score and the row is uniform over T (include/biattn_hip.h); in float64 it does not, and the row is softmax(s).  That case is
held against the float64 restatement that reproduces the fp32 add (tests/vlfuse_train_cases.py) in the C ABI's sweep.
"""
import os

import numpy as np
import torch

import make_vlfuse_golden as G

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vlfuse_train")


def run(ref, name, B, S, T, mask_kind, gain):
    block = ref.BiAttentionBlockForCheckpoint(v_dim=G.V_DIM, l_dim=G.L_DIM, embed_dim=G.HEADS * G.HEAD_DIM, num_heads=G.HEADS,
                                              dropout=0.1, drop_path=.0, init_values=1.0 / G.ENC_LAYERS, cfg=G.make_cfg()).double().eval()
    with torch.no_grad():
        for n, p in block.named_parameters():
            g = gain if n in ("attn.v_proj.weight", "attn.l_proj.weight") else 1.0
            if n.endswith(".bias"):
                p.copy_(G.dyadic(torch.rand_like(p) - 0.5, 0.25))
            else:
                p.copy_(G.dyadic(p, g))
    visual = G.dyadic(torch.randn(B, S, G.V_DIM, dtype=torch.float64)).requires_grad_()
    hidden = G.dyadic(torch.randn(B, T, G.L_DIM, dtype=torch.float64)).requires_grad_()
    w_v = G.dyadic(torch.randn(B, S, G.V_DIM, dtype=torch.float64))
    w_l = G.dyadic(torch.randn(B, T, G.L_DIM, dtype=torch.float64))
    masks = None
    if mask_kind != "none":
        masks = (torch.rand(B, T) > 0.35).long()
        masks[:, 0] = 1
    out_v, out_l = block(visual, hidden, masks, None)
    ((out_v * w_v).sum() + (out_l * w_l).sum()).backward()
    with torch.no_grad():
        nv, nl = block.layer_norm_v(visual), block.layer_norm_l(hidden)
        q, k = block.attn.v_proj(nv) * block.attn.scale, block.attn.l_proj(nl)
        smax = float(torch.einsum("bshd,bthd->bhst", q.view(B, S, G.HEADS, G.HEAD_DIM), k.view(B, T, G.HEADS, G.HEAD_DIM)).abs().max())
    f64 = lambda t: t.detach().contiguous().numpy().astype(np.float64)
    data = dict(visual=f64(visual), hidden=f64(hidden), w_visual=f64(w_v), w_hidden=f64(w_l), out_visual=f64(out_v),
                out_hidden=f64(out_l), num_heads=np.array(G.HEADS), init_values=np.array(1.0 / G.ENC_LAYERS),
                score_absmax=np.array(smax))
    data["grad.visual"], data["grad.hidden"] = f64(visual.grad), f64(hidden.grad)
    if masks is not None:
        data["masks"] = masks.numpy().astype(np.int64)
    for n, t in block.state_dict().items():
        data["state." + n] = f64(t)
    for n, p in block.named_parameters():
        data["grad." + n] = f64(p.grad)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **data)
    print(name, (B, S, T), mask_kind, "max |score| %.1f" % smax, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


def main():
    if not G.REF:
        raise SystemExit("set UNINEXT_REFERENCE to a checkout of the reference project")
    ref = G.load_reference_fuse_helper()
    os.makedirs(HERE, exist_ok=True)
    torch.manual_seed(36)
    run(ref, "t1_nomask", 2, 130, 1, "none", 8.0)
    run(ref, "t37_partial", 2, 161, 37, "partial", 8.0)
    run(ref, "t33_nomask", 2, 129, 33, "none", 8.0)
    run(ref, "t256_partial", 1, 70, 256, "partial", 8.0)


if __name__ == "__main__":
    main()
