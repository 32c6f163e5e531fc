"""Mint gradient fixtures for the decoder layer and the decoder with the REFERENCE's own code (build container only).

    python tests/golden/make_decoder_train_golden.py

The reference's classes are loaded as tests/golden/make_decoder_golden.py loads them and run in float64 on the CPU in eval()
(dropout is the identity) under autograd, on the seeds, shapes, dyadic parameters and inputs of tests/decoder_cases.py; the
denoising mask of layer_dn_mask is checked against the reference's own construction there.  The loss is sum(out . G) with the
seeded G of tests/decoder_train_cases.py (the decoder, with look_forward_twice so that every box head has a gradient: over the
stack of its layers' outputs and the stack of its points, "G" and "G_points").  Every file of
tests/golden/decoder_train/ holds data only: the inputs, G, the digest of the parameters (which are re-drawn from the seeds,
not stored), and the float64 gradients of the inputs ("grad.tgt", "grad.query_pos", "grad.ref", "grad.src") and of every
parameter ("grad.<name>"), stored rounded to float32.  In the d_model-256 fixture a parameter of more than CAP elements is
stored at a seeded subset of its rows ("rows.<name>", decoder_train_cases.stored_rows).

Per gradient the reference's own fp32 run stays within 3e-5 of its float64 run (asserted and recorded as fp32_err; the margin
of make_vit_train_golden.py).
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import decoder_cases as C                      # noqa: E402
import decoder_train_cases as T                # noqa: E402
import make_decoder_golden as M                # noqa: E402

CAP = 1024          # stored elements of one large parameter's gradient (d_model 256)


def reference_module(ns, cfg, state):
    layer = ns["DeformableTransformerDecoderLayer"](d_model=cfg["d_model"], d_ffn=cfg["d_ffn"], dropout=0.1, activation="relu",
                                                    n_levels=C.N_LEVELS, n_heads=cfg["heads"], n_points=C.N_POINTS)
    if cfg["kind"] == "layer":
        m = layer
    else:
        m = ns["DeformableTransformerDecoder"](cfg["d_model"], layer, cfg["layers"], return_intermediate=True, look_forward_twice=True)
        m.bbox_embed = nn.ModuleList(ns["MLP"](cfg["d_model"], cfg["d_model"], 4, 3) for _ in range(cfg["layers"]))
    m = m.double().eval()
    m.load_state_dict(state, strict=True)
    return m


def main():
    ns = M.load_reference()
    os.makedirs(T.HERE, exist_ok=True)
    for name in T.EXPECTED:
        cfg, state, x = C.make_case(name)
        if cfg["mask"] == "dn":
            assert torch.equal(M.reference_dn_mask(cfg["lq"], C.DN_PAD, C.DN_NUMBER), x["attn_mask"])
        m = reference_module(ns, cfg, state)
        G = T.fixture_upstream(name)
        want, out = T.gradients(cfg, m, x, G, torch.float64)
        want = {k: v.detach().clone() for k, v in want.items()}
        got32, _ = T.gradients(cfg, m.float(), x, G, torch.float32)
        errs = {k: C.rel_err(got32[k], want[k]) for k in want}
        worst = max(errs, key=errs.get)
        assert errs[worst] < 3e-5, (name, worst, errs[worst])
        assert sorted(want) == sorted(list(T.INPUT_KEYS[cfg["kind"]]) + list(state))
        for k, g in want.items():
            assert float(g.abs().max()) > 0, (name, k)

        f32 = lambda a: a.detach().contiguous().numpy().astype(np.float32)
        data = {k: v.numpy() for k, v in x.items()}
        for k in ("tgt", "src", "query_pos", "ref", "valid_ratios"):
            if k in data:
                assert float(np.abs(data[k].astype(np.float32).astype(np.float64) - data[k]).max()) == 0
                data[k] = data[k].astype(np.float32)
        if "attn_mask" in data and data["attn_mask"].dtype != np.bool_:
            data["attn_mask"] = data["attn_mask"].astype(np.float32)
        for key, g in zip(("G", "G_points"), G):
            data[key] = g.numpy().astype(np.float16)
            assert float(np.abs(data[key].astype(np.float64) - g.numpy()).max()) == 0
        data.update(digest=np.float64(C.digest(state)), fp32_err=np.array(errs[worst]))
        for k, g in want.items():
            flat = g.reshape(-1, g.shape[-1])
            if cfg["d_model"] == 256 and k in state and g.numel() > CAP:
                rows = T.stored_rows(name, k, flat.shape[0], max(1, CAP // flat.shape[1]))
                data["rows." + k] = rows.numpy()
                data["grad." + k] = f32(flat[rows])
            else:
                data["grad." + k] = f32(g)
        path = os.path.join(T.HERE, name + "_grad.npz")
        np.savez_compressed(path, **data)
        print("%-18s %d gradients, worst fp32 err %.1e (%s) %d bytes" % (name, len(want), errs[worst], worst, os.path.getsize(path)))
        assert os.path.getsize(path) < 500 * 1024, name


if __name__ == "__main__":
    main()
