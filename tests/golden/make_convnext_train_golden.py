"""Mint the gradient fixtures of the ConvNeXt training tests with the REFERENCE's own code (build container only).

    UNINEXT_REFERENCE=<checkout of the reference> python tests/golden/make_convnext_train_golden.py

Loads projects/UNINEXT/uninext/backbone/convnext.py through tests/convnext_cases.py::load_reference (stubs for timm and detectron2),
builds the reference's Block / ConvNeXt in float64 from the state dicts and inputs of the forward fixtures block_c32,
block_c96_noscale and net_small (tests/golden/convnext/, made by make_convnext_golden.py, which this script leaves alone), and
backpropagates a seeded grad_out (multiples of 2^-12, exact in fp32; for the network one per output, res2..res5).

Every file of tests/golden/convnext_train/ holds data only: `grad_out` (`grad_out.res2` ...), `grad.x` and one `grad.<parameter>`
per parameter, float64.  (A directory of its own: tests/test_convnext_cpu.py holds the list of files in tests/golden/convnext/.)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import convnext_cases as C         # noqa: E402
import convnext_train_cases as T   # noqa: E402


def save(name, arrays):
    path = os.path.join(T.HERE, name + "_grad.npz")
    np.savez_compressed(path, **{k: v.detach().contiguous().numpy().astype(np.float64) for k, v in arrays.items()})
    print(name, len(arrays), "arrays", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20          # the size limit of a committed file


def gradients(module, x, outs, grad_outs):
    torch.autograd.backward(outs, grad_outs)
    arrays = {"grad.x": x.grad}
    for n, p in module.named_parameters():
        assert p.grad is not None, n
        arrays["grad." + n] = p.grad
    return arrays


def block(ref, name, seed):
    fx = C.load(name)
    blk = ref.Block(fx["x"].shape[1], layer_scale_init_value=1.0 if "gamma.weight" in fx["state"] else 0.0).double().eval()
    blk.load_state_dict(fx["state"], strict=True)
    x = fx["x"].clone().requires_grad_(True)
    out = blk(x)
    assert C.max_err(out, fx["out"]) < 1e-12
    grad_out = T.grad_out_for(out.shape, seed)
    arrays = gradients(blk, x, [out], [grad_out])
    assert len(arrays) == (10 if "gamma.weight" in fx["state"] else 9)
    save(name, dict(grad_out=grad_out, **arrays))


def net(ref, name, seed):
    fx = C.load(name)
    m = ref.ConvNeXt(in_chans=3, depths=list(C.NET_DEPTHS), dims=list(C.NET_DIMS), drop_path_rate=0.0, layer_scale_init_value=1.0).double().eval()
    m.load_state_dict(fx["state"], strict=True)
    x = fx["x"].clone().requires_grad_(True)
    out = m(x)
    keys = sorted(out)
    grad_outs = {k: T.grad_out_for(out[k].shape, seed + i) for i, k in enumerate(keys)}
    arrays = gradients(m, x, [out[k] for k in keys], [grad_outs[k] for k in keys])
    save(name, dict(**{"grad_out." + k: v for k, v in grad_outs.items()}, **arrays))


def main():
    if not C.reference_available():
        raise SystemExit("set UNINEXT_REFERENCE to a checkout of the reference project")
    ref = C.load_reference()
    os.makedirs(T.HERE, exist_ok=True)
    block(ref, "block_c32", 41)
    block(ref, "block_c96_noscale", 42)
    net(ref, "net_small", 43)


if __name__ == "__main__":
    main()
