"""Mint gradient fixtures for the patch-embedding convolutions with the REFERENCE's own code (build container only).

    python tests/golden/make_patch_embed_bwd_golden.py

As make_patch_embed_golden.py: `vit_*` run the reference class PatchEmbed (projects/UNINEXT/uninext/backbone/utils.py:160-186,
loaded as it is; output after its permute, B H W C), `convnext_*` repeat the two literal nn.Conv2d constructor calls of
backbone/convnext.py (:80 stem, :87 downsample).  Each case runs in float64 under autograd with a seeded upstream gradient and
stores x, weight, bias, grad_out, out and the gradients gx, gw, gb (tests/golden/patch_bwd/*.npz).  Inputs, parameters and
grad_out are multiples of 2^-10 (exact in fp32, so an fp32 run sees the same numbers); the float64 output and gradients are
stored rounded to float32 (2^-24 relative, far inside the 1e-4 bound of the tests) to keep each file small.
"""
import importlib.util
import os

import numpy as np
import torch
import torch.nn as nn

REF = os.environ.get("UNINEXT_REFERENCE", "/root/reference")
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "patch_bwd")


def load_reference_utils():
    path = os.path.join(REF, "projects/UNINEXT/uninext/backbone/utils.py")
    spec = importlib.util.spec_from_file_location("ref_backbone_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def dyadic(t, scale=1.0):
    """`t * scale` rounded to a multiple of 2^-10."""
    return torch.round(t * scale * 1024.0) / 1024.0


def run(name, module, conv, x_shape, channels_last):
    with torch.no_grad():
        conv.weight.copy_(dyadic(conv.weight))
        conv.bias.copy_(dyadic(torch.rand_like(conv.bias) - 0.5, 0.4))   # make the bias count
    x = dyadic(torch.randn(x_shape, dtype=torch.float64)).requires_grad_(True)
    out = module(x)
    grad_out = dyadic(torch.randn(out.shape, dtype=torch.float64))
    out.backward(grad_out)
    path = os.path.join(HERE, name + ".npz")
    f32 = lambda t: t.detach().contiguous().numpy().astype(np.float32)
    np.savez_compressed(path, x=f32(x), weight=f32(conv.weight), bias=f32(conv.bias), grad_out=f32(grad_out), out=f32(out),
                        gx=f32(x.grad), gw=f32(conv.weight.grad), gb=f32(conv.bias.grad), channels_last=np.array(int(channels_last)))
    print(name, tuple(x.shape), "->", tuple(out.shape), os.path.getsize(path), "bytes")


def main():
    ref = load_reference_utils()
    os.makedirs(HERE, exist_ok=True)
    torch.manual_seed(17)
    # ViT, 16 x 16 patches: an image size with remainders (37 x 50), an E that leaves a partial 128-column tile (136)
    for name, (B, H, W, E) in {"vit_remainder": (2, 37, 50, 40), "vit_tiles": (1, 64, 160, 136)}.items():
        pe = ref.PatchEmbed(kernel_size=(16, 16), stride=(16, 16), padding=(0, 0), in_chans=3, embed_dim=E).double()
        run(name, pe, pe.proj, (B, 3, H, W), True)
    # ConvNeXt stem (convnext.py:80; k = 4, K = 48) and a downsample convolution (convnext.py:87; k = 2, odd H x W)
    stem = nn.Conv2d(3, 24, kernel_size=4, stride=4).double()
    run("convnext_stem", stem, stem, (2, 3, 22, 35), False)
    down = nn.Conv2d(12, 24, kernel_size=2, stride=2).double()
    run("convnext_down", down, down, (2, 12, 13, 19), False)


if __name__ == "__main__":
    main()
