"""What the ConvNeXt tests share: the fixtures of tests/golden/convnext/ (tests/golden/make_convnext_golden.py), the reference's
module loaded behind test-side stubs, and the seeded cases of the kernels with their variance floor."""
import glob
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convnext")
REF = os.environ.get("UNINEXT_REFERENCE", "/root/reference")
REF_FILE = os.path.join(REF, "projects/UNINEXT/uninext/backbone/convnext.py")
EXPECTED = ["block_c32", "block_c96_noscale", "ln_cf_c48", "net_small"]
NAMES = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(HERE, "*.npz")))
EPS = 1e-6
# LayerNorm multiplies a rounding of the mean by 1 / sqrt(var + eps), up to 1000 x: a tolerance says nothing on a pixel whose
# channels are nearly constant.  Fixtures and seeded cases keep every pixel's channel variance above this floor.
VARIANCE_FLOOR = 1e-2
NET_DEPTHS, NET_DIMS = (1, 1, 1, 1), (32, 32, 32, 64)


def tol(ref):
    """The project's parity bound (tests/test_conv3x3_gpu.py): 1e-4 of the output scale, at least 1e-4."""
    return 1e-4 * max(1.0, float(ref.abs().max()))


def max_err(got, ref):
    return float((got.detach().to("cpu", torch.float64) - ref.detach().to("cpu", torch.float64)).abs().max()) if ref.numel() else 0.0


def load(name):
    with np.load(os.path.join(HERE, name + ".npz")) as z:
        d = {k: z[k] for k in z.files}
    state = {k[len("state."):]: torch.from_numpy(v) for k, v in d.items() if k.startswith("state.")}
    rest = {k: torch.from_numpy(v) for k, v in d.items() if not k.startswith("state.")}
    rest["state"] = state
    return rest


def reference_available():
    return os.path.exists(REF_FILE)


def load_reference():
    """The reference's backbone/convnext.py as it is, behind stubs for what it imports from timm and detectron2."""
    class DropPath(nn.Module):
        def __init__(self, p=0.0):
            super().__init__()
            raise RuntimeError("DropPath stub: the tests build the reference with drop_path_rate = 0")

    class Registry:
        def register(self, obj=None):
            return obj if obj is not None else (lambda o: o)

    def module(name, **attrs):
        m = sys.modules.get(name) or types.ModuleType(name)
        for k, v in attrs.items():
            if not hasattr(m, k):
                setattr(m, k, v)
        sys.modules.setdefault(name, m)
        return m

    module("timm")
    module("timm.models")
    module("timm.models.layers", trunc_normal_=nn.init.trunc_normal_, DropPath=DropPath)
    module("detectron2")
    module("detectron2.modeling", BACKBONE_REGISTRY=Registry(), Backbone=type("Backbone", (nn.Module,), {}),
           ShapeSpec=type("ShapeSpec", (), {}))
    spec = importlib.util.spec_from_file_location("ref_convnext", REF_FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def dyadic(t, step=4096.0):
    """Rounded to multiples of 2^-12: exact in fp32, and the files compress."""
    return torch.round(t * step) / step


def randomise(module, gen):
    """Non-trivial values for every parameter: weights ~ N(0, 1 / fan_in) (the depthwise taps ~ N(0, 0.2^2)), biases in
    [-0.25, 0.25], LayerNorm weights around 1, layer scales in [0.5, 1.5]."""
    with torch.no_grad():
        for name, p in module.named_parameters():
            r = lambda: torch.randn(p.shape, generator=gen, dtype=torch.float64)
            u = lambda: torch.rand(p.shape, generator=gen, dtype=torch.float64)
            leaf = name.rsplit(".", 2)
            if "gamma" in name:
                v = 0.5 + u()
            elif len(leaf) >= 2 and leaf[-2] in ("weight", "bias") and leaf[-1] == "weight" and p.shape[0] == 1:   # LayerNorm's embeddings
                v = 1.0 + 0.5 * (u() - 0.5) if leaf[-2] == "weight" else 0.5 * (u() - 0.5)
            elif name.endswith("dwconv.weight"):
                v = 0.2 * r()
            elif name.endswith(".bias"):
                v = 0.5 * (u() - 0.5)
            else:
                v = r() / float(np.prod(p.shape[1:])) ** 0.5
            p.copy_(dyadic(v).to(p.dtype))


# (C, B, H, W, dw_bias given): every supported class of C, maps smaller than the 7 x 7 footprint in one or both directions, sizes
# that are multiples of no tile, one and three images, no convolution bias
HEAD_CASES = [(32, 1, 1, 1, True), (32, 3, 3, 20, True), (96, 1, 20, 3, True), (96, 3, 11, 23, True), (192, 1, 37, 29, True),
              (192, 3, 9, 13, False), (768, 1, 13, 19, True), (768, 3, 6, 9, True), (1536, 1, 11, 10, True), (1536, 3, 5, 7, False),
              (64, 1, 17, 41, False)]
# maps large enough for the wider tiles, with the kernel the library's tile rule must pick for them (the cases above all take <4>)
WIDE_HEAD_CASES = [(32, 2, 71, 116, True, "convnext_dwconv_ln<7>"), (64, 2, 50, 120, False, "convnext_dwconv_ln<7>"),
                   (192, 3, 85, 106, True, "convnext_dwconv_ln<8>"),
                   # 8 x 7 at C = 384 and 6 x 7 at C = 768, where the LDS plane cuts the tile's height (tests/convnext_parity.py)
                   (384, 1, 65, 113, True, "convnext_dwconv_ln<7>"), (768, 1, 65, 113, True, "convnext_dwconv_ln<7>")]
TAIL_CASES = [(1, 1, 7, 9), (32, 2, 5, 11), (100, 3, 13, 7), (1536, 1, 9, 5), (70, 2, 1, 1)]           # (C, B, H, W)
CF_CASES = [(1, 2, 7, 9), (3, 1, 5, 7), (192, 3, 13, 9), (1536, 1, 7, 11), (2100, 1, 3, 5)]            # 2100: past the LDS-resident block
LARGE_STAGES = [(192, 200, 336), (384, 100, 168), (768, 50, 84), (1536, 25, 42)]                       # ConvNeXt-L at 800 x 1344, bs 2


def head_case(seed, B, C, H, W, bias=True):
    """Seeded inputs of the block's head (float32 CPU tensors) whose convolution output clears the variance floor at every pixel."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g)
    dw_w = 0.2 * torch.randn(C, 1, 7, 7, generator=g)
    dw_b = 0.5 * torch.randn(C, generator=g) if bias else None
    ln_w = 1.0 + 0.25 * torch.randn(C, generator=g)
    ln_b = 0.25 * torch.randn(C, generator=g)
    return x, dw_w, dw_b, ln_w, ln_b


def cf_case(seed, B, C, H, W):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g) * 2.0 + 0.5
    return x, 1.0 + 0.25 * torch.randn(C, generator=g), 0.25 * torch.randn(C, generator=g)


def our_block(fx, dtype, device="cpu"):
    from uninext_amd.backbone import Block
    dim = fx["x"].shape[1]
    blk = Block(dim, layer_scale_init_value=1.0 if "gamma.weight" in fx["state"] else 0.0)
    blk.load_state_dict(fx["state"], strict=True)
    return blk.to(device=device, dtype=dtype).eval()


def our_net(fx, dtype, device="cpu"):
    from uninext_amd.backbone import ConvNeXt
    net = ConvNeXt(in_chans=3, depths=NET_DEPTHS, dims=NET_DIMS, layer_scale_init_value=1.0)
    net.load_state_dict(fx["state"], strict=True)
    return net.to(device=device, dtype=dtype).eval()
