"""What the ConvNeXt training tests share: the gradient fixtures of tests/golden/convnext_train/
(tests/golden/make_convnext_train_golden.py), the cases of the backward kernels, and float64 autograd through the restatement of
tests/convnext_ref.py, computed once per case."""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnext_cases as C   # noqa: E402
import convnext_ref as R     # noqa: E402

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convnext_train")
GRAD_NAMES = ["block_c32", "block_c96_noscale", "net_small"]

# (C, B, H, W, dw_bias given): a 1 x 1 map, maps narrower than the footprint either way, three chunks on no tile multiple with three
# images, no convolution bias, the largest C, a wider map
HEAD_CASES = [(32, 1, 1, 1, True), (32, 3, 3, 20, True), (96, 1, 20, 3, True), (96, 3, 11, 23, True), (192, 3, 9, 13, False),
              (1536, 3, 5, 7, False), (64, 1, 17, 41, False)]
for _case in HEAD_CASES:
    assert _case in C.HEAD_CASES
WIDE_HEAD_CASE = C.WIDE_HEAD_CASES[0][:5]                       # (32, 2, 71, 116, True): many workgroups, 270 bands of one tile
# Pass two sums a band of 8 x 8 tiles per workgroup (head_bands below).  Bands of more than one tile and a shorter last band: bands
# of 2 over 3 x 3 tiles an image (they cross tile rows and images), bands of 3 over 2 x 2 tiles an image, and bands of 22 over two
# tiles an image, the second one pixel wide
BAND_HEAD_CASES = [(768, 3, 17, 17, True), (1536, 7, 9, 9, False), (1536, 107, 1, 9, False)]
# (C, B, H, W) at which the rule's cap of 64 tiles a band holds: 642 tiles.  tests/test_convnext_train_cpu.py reads the cap off the
# workspace size; the kernel runs the shape in tests/test_convnext_bwd_parity_gpu.py, against a float64 reference of 4.4 M entries
BAND_CAP_SHAPE = (1536, 321, 1, 9)
TAIL_SIZES = (1, 63, 64, 65, 129)                               # C and H * W
CF_CASES = [(1, 2, 7, 9), (3, 1, 5, 7), (192, 3, 13, 9), (2100, 1, 3, 5)]
for _case in CF_CASES:
    assert _case in C.CF_CASES


def grad_out_for(shape, seed):
    """A seeded gradient of the output, multiples of 2^-12."""
    return C.dyadic(torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed), dtype=torch.float64))


def load_grads(name):
    with np.load(os.path.join(HERE, name + "_grad.npz")) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


def head_seed(case):
    """The seed tests/test_convnext_gpu.py gives this case: the same inputs, whose variance floor tests/test_convnext_cpu.py checks;
    the band cases have seeds of their own (tests/test_convnext_train_cpu.py checks their floor)."""
    case = tuple(case)
    if case == WIDE_HEAD_CASE:
        return 300
    if case in BAND_HEAD_CASES:
        return 400 + BAND_HEAD_CASES.index(case)
    return 100 + C.HEAD_CASES.index(case)


def head_bands(B, c, H, W):
    """(tiles, tiles per band, bands) of the head backward's pass two, as include/patch_embed_hip.h states the rule: 8 x 8 tiles,
    about 512 / (C / 32) bands, never more than 64 tiles each."""
    tiles = B * (-(-H // 8)) * (-(-W // 8))
    per = max(1, min(64, -(-tiles // max(1, 512 // (c // 32)))))
    return tiles, per, -(-tiles // per)


def grads_of(out, grad_out, named):
    """{name: gradient} of sum(out * grad_out) with respect to the named leaves (None leaves are left out)."""
    out.backward(grad_out.to(out.dtype))
    return {n: t.grad.detach() for n, t in named if t is not None}


@functools.lru_cache(maxsize=None)
def head_reference(case):
    """Inputs (float32, CPU), grad_out and the float64 gradients of the head for one case."""
    c, B, H, W, bias = case
    inputs = C.head_case(head_seed(case), B, c, H, W, bias)
    assert float(R.channel_variance(R.dwconv7(inputs[0], inputs[1], inputs[2]), 1).min()) > C.VARIANCE_FLOOR
    grad_out = grad_out_for((B, H, W, c), 7000 + c + H).float()
    ref = head_grads(inputs, grad_out, torch.float64)
    return inputs, grad_out, ref


def head_grads(inputs, grad_out, dtype, eps=C.EPS):
    """Autograd through the restatement (float64) or through PyTorch's own fp32 composition (float32)."""
    import torch.nn.functional as F
    x, dw_w, dw_b, ln_w, ln_b = [None if t is None else t.detach().to(dtype).clone().requires_grad_(True) for t in inputs]
    if dtype == torch.float64:
        out = _with_grad(lambda: R.dwconv_ln(x, dw_w, dw_b, ln_w, ln_b, eps))
    else:
        u = F.conv2d(x, dw_w, dw_b, padding=3, groups=x.shape[1]).permute(0, 2, 3, 1)
        out = F.layer_norm(u, (x.shape[1],), ln_w, ln_b, eps)
    return grads_of(out, grad_out, (("x", x), ("dw_weight", dw_w), ("dw_bias", dw_b), ("ln_weight", ln_w), ("ln_bias", ln_b)))


@functools.lru_cache(maxsize=None)
def cf_reference(case_index):
    c, B, H, W = CF_CASES[case_index]
    inputs = C.cf_case(200 + C.CF_CASES.index(CF_CASES[case_index]), B, c, H, W)
    if c > 1:
        assert float(R.channel_variance(inputs[0], 1).min()) > C.VARIANCE_FLOOR
    grad_out = grad_out_for((B, c, H, W), 7100 + c).float()
    return inputs, grad_out, cf_grads(inputs, grad_out, torch.float64)


def cf_grads(inputs, grad_out, dtype, eps=C.EPS):
    x, w, b = [t.detach().to(dtype).clone().requires_grad_(True) for t in inputs]
    if dtype == torch.float64:
        out = _with_grad(lambda: R.layernorm_cf(x, w, b, eps))
    else:                                                       # the module's PyTorch expressions
        m = x.mean(1, keepdim=True)
        s = ((x - m) * (x - m)).mean(1, keepdim=True)
        out = w.view(-1, 1, 1) * ((x - m) / torch.sqrt(s + eps)) + b.view(-1, 1, 1)
    return grads_of(out, grad_out, (("x", x), ("weight", w), ("bias", b)))


def restatement_block_grads(fx, grad_out):
    """Float64 autograd through tests/convnext_ref.py::block on leaves made from a block fixture's x and state."""
    x = fx["x"].detach().to(torch.float64).clone().requires_grad_(True)
    state = {k: v.detach().to(torch.float64).clone().requires_grad_(True) for k, v in fx["state"].items()}
    out = _with_grad(lambda: R.block(x, state))
    out.backward(grad_out)
    return dict({"grad.x": x.grad}, **{"grad." + k: v.grad for k, v in state.items()})


def restatement_net_grads(fx, grad_outs):
    x = fx["x"].detach().to(torch.float64).clone().requires_grad_(True)
    state = {k: v.detach().to(torch.float64).clone().requires_grad_(True) for k, v in fx["state"].items()}
    out = _with_grad(lambda: R.convnext(x, state, C.NET_DEPTHS))
    keys = sorted(out)
    torch.autograd.backward([out[k] for k in keys], [grad_outs[k] for k in keys])
    return dict({"grad.x": x.grad}, **{"grad." + k: v.grad for k, v in state.items()})


def _with_grad(fn):
    """tests/convnext_ref.py detaches what it is given (its f64 helper); for autograd the helper keeps float64 tensors as they are."""
    old = R.f64
    R.f64 = lambda t: None if t is None else (t if (torch.is_tensor(t) and t.dtype == torch.float64) else old(t))
    try:
        return fn()
    finally:
        R.f64 = old
