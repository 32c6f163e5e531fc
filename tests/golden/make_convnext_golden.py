"""Mint fixtures for the ConvNeXt block, its channels-first LayerNorm and a small backbone with the REFERENCE's own code (build
container only).

    UNINEXT_REFERENCE=<checkout of the reference> python tests/golden/make_convnext_golden.py

Loads projects/UNINEXT/uninext/backbone/convnext.py as it is; what it imports from timm and detectron2 (trunc_normal_, DropPath,
BACKBONE_REGISTRY, Backbone, ShapeSpec) is replaced by the stubs of tests/convnext_cases.py.  The modules run in float64 in
eval() on seeded inputs, with non-trivial values in every parameter (LayerNorm weights and biases, layer scales and convolution
biases included), all multiples of 2^-12 and therefore exact in fp32.

Every file of tests/golden/convnext/ holds data only: the input, the state dict, the intermediate after `norm` (blocks) and the
outputs.  Every pixel's channel variance of every depthwise convolution's output, and of every channels-first LayerNorm's input,
is asserted to be above 1e-2: LayerNorm amplifies a rounding of the mean by 1 / sqrt(var + eps), and a tolerance means nothing on
a nearly constant pixel.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import convnext_cases as C   # noqa: E402
import convnext_ref as R     # noqa: E402


def save(name, data, state):
    f64 = lambda t: t.detach().contiguous().numpy().astype(np.float64)
    out = {k: f64(v) for k, v in data.items()}
    for n, t in state.items():
        out["state." + n] = t.detach().contiguous().numpy().astype(np.float32)     # dyadic: nothing is lost
        assert np.array_equal(out["state." + n].astype(np.float64), f64(t)), n
    path = os.path.join(C.HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, {k: tuple(v.shape) for k, v in data.items()}, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 500000


def watch_variances(module, ref):
    """Forward hooks that check the variance floor where a LayerNorm follows: after every dwconv, before every channels_first norm."""
    seen, hooks = [], []
    for name, m in module.named_modules():
        if name.endswith("dwconv") or name == "dwconv":
            hooks.append(m.register_forward_hook(lambda mod, i, o, n=name: seen.append((n, float(R.channel_variance(o, 1).min())))))
        elif isinstance(m, ref.LayerNorm) and m.data_format == "channels_first":
            hooks.append(m.register_forward_hook(lambda mod, i, o, n=name: seen.append((n, float(R.channel_variance(i[0], 1).min())))))
    return seen, hooks


def checked(seen, hooks):
    for h in hooks:
        h.remove()
    assert seen
    for name, v in seen:
        assert v > C.VARIANCE_FLOOR, (name, v)
    return min(v for _, v in seen)


def block(ref, name, gen, B, dim, H, W, scale):
    blk = ref.Block(dim, layer_scale_init_value=1.0 if scale else 0.0).double().eval()
    C.randomise(blk, gen)
    x = C.dyadic(torch.randn(B, dim, H, W, generator=gen, dtype=torch.float64))
    seen, hooks = watch_variances(blk, ref)
    with torch.no_grad():
        out = blk(x)
        normed = blk.norm(blk.dwconv(x).permute(0, 2, 3, 1))
    print(name, "min channel variance %.3f" % checked(seen, hooks))
    save(name, dict(x=x, normed=normed, out=out), blk.state_dict())


def ln_cf(ref, name, gen, B, dim, H, W):
    ln = ref.LayerNorm(dim, eps=C.EPS, data_format="channels_first").double().eval()
    C.randomise(ln, gen)
    x = C.dyadic(torch.randn(B, dim, H, W, generator=gen, dtype=torch.float64) * 2.0 + 0.5)
    seen, hooks = watch_variances(ln, ref)
    with torch.no_grad():
        out = ln(x)
    checked(seen, hooks)
    save(name, dict(x=x, out=out), ln.state_dict())


def net(ref, name, gen, B, H, W):
    m = ref.ConvNeXt(in_chans=3, depths=list(C.NET_DEPTHS), dims=list(C.NET_DIMS), drop_path_rate=0.0, layer_scale_init_value=1.0).double().eval()
    C.randomise(m, gen)
    x = C.dyadic(torch.randn(B, 3, H, W, generator=gen, dtype=torch.float64))
    seen, hooks = watch_variances(m, ref)
    with torch.no_grad():
        out = m(x)
    print(name, "min channel variance %.3f over %d LayerNorm inputs" % (checked(seen, hooks), len(seen)))
    save(name, dict(x=x, **out), m.state_dict())


def main():
    if not C.reference_available():
        raise SystemExit("set UNINEXT_REFERENCE to a checkout of the reference project")
    ref = C.load_reference()
    os.makedirs(C.HERE, exist_ok=True)
    gen = torch.Generator().manual_seed(31)
    block(ref, "block_c32", gen, 2, 32, 9, 13, True)
    block(ref, "block_c96_noscale", gen, 1, 96, 11, 7, False)
    ln_cf(ref, "ln_cf_c48", gen, 2, 48, 9, 13)
    net(ref, "net_small", gen, 2, 48, 64)


if __name__ == "__main__":
    main()
