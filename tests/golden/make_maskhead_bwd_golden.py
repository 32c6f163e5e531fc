"""Mint gradient fixtures for the static mask head with the REFERENCE's own code (build container only).

    python tests/golden/make_maskhead_bwd_golden.py

As make_maskhead_golden.py, the class MaskHeadSmallConv (projects/UNINEXT/uninext/models/ddetrs_dn.py:923-1031) and _expand
(:1112-1113) are cut out of the reference source with `ast` and executed as they are, in float64 under autograd.  dim = 64, so
every 3x3 layer has a multiple of 16 input channels (lay1 64 -> 16, lay2 16 -> 2: the padded grad-input of a cout below 16).
Two cases, `nofpn` and `fpn` (tests/golden/maskhead_bwd/*.npz): the inputs, the parameters, a fixed upstream gradient and the
gradients of the inputs and of every parameter.  Inputs and parameters are multiples of 2^-10 (exact in fp32, and they compress);
the float64 gradients are stored rounded to float32 (2^-24 relative, far inside the 1e-4 bound of the tests) to keep each file small.
"""
import ast
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

REF = os.environ.get("UNINEXT_REFERENCE", "/root/reference")
SRC = os.path.join(REF, "projects/UNINEXT/uninext/models/ddetrs_dn.py")
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "maskhead_bwd")


def load_reference_class():
    tree = ast.parse(open(SRC).read())
    body = [n for n in tree.body if (isinstance(n, ast.ClassDef) and n.name == "MaskHeadSmallConv")
            or (isinstance(n, ast.FunctionDef) and n.name == "_expand")]
    assert len(body) == 2
    ns = {"torch": torch, "nn": nn, "F": F}
    exec(compile(ast.Module(body=body, type_ignores=[]), SRC, "exec"), ns)
    return ns["MaskHeadSmallConv"]


def dyadic(t, scale):
    """`t * scale` rounded to a multiple of 2^-10."""
    return torch.round(t * scale * 1024.0) / 1024.0


def main():
    cls = load_reference_class()
    os.makedirs(HERE, exist_ok=True)
    torch.manual_seed(23)
    dim = 64
    for name, fpn_dims in (("nofpn", None), ("fpn", [16, 24, 8])):
        head = cls(dim, fpn_dims, dim).double()
        with torch.no_grad():
            for p in head.parameters():
                if p.dim() == 1:                   # the reference zero-initialises the biases: make them count
                    p.copy_(dyadic(torch.rand_like(p) - 0.5, 0.4))
                else:
                    p.copy_(dyadic(p, 1.0))
        sizes = [(13, 18), (7, 9), (4, 5)]         # stride 8 / 16 / 32 of a 100 x 140 image
        x = [dyadic(torch.randn(2, dim, h, w, dtype=torch.float64), 1.0).requires_grad_(True) for h, w in sizes]
        fpns = None
        if fpn_dims is not None:
            fpns = [dyadic(torch.randn(1, fpn_dims[i], *sizes[2 - i], dtype=torch.float64), 1.0).requires_grad_(True)
                    for i in range(3)]
        out = head(x, fpns)
        grad_out = dyadic(torch.randn(out.shape, dtype=torch.float64), 1.0)
        out.backward(grad_out)
        f32 = lambda t: t.detach().numpy().astype(np.float32)
        arrays = {"x%d" % i: f32(t) for i, t in enumerate(x)}
        arrays.update({"gx%d" % i: f32(t.grad) for i, t in enumerate(x)})
        if fpns is not None:
            arrays.update({"fpn%d" % i: f32(t) for i, t in enumerate(fpns)})
            arrays.update({"gfpn%d" % i: f32(t.grad) for i, t in enumerate(fpns)})
        for k, p in head.named_parameters():
            arrays["p:" + k] = f32(p)
            arrays["g:" + k] = f32(p.grad)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), out=f32(out), grad_out=f32(grad_out), **arrays)
        print(name, [tuple(t.shape) for t in x], "->", tuple(out.shape),
              os.path.getsize(os.path.join(HERE, name + ".npz")), "bytes")


if __name__ == "__main__":
    main()
