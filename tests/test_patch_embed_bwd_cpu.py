"""CPU tests of the patch-embedding training route: the C ABI of patch_embed_hip_backward_f32 (include/patch_embed_hip.h;
exports, argument checks and the workspace query, no GPU work), the scratch budget of the new kernels, the gradient fixtures
(tests/golden/patch_bwd, minted from the reference's PatchEmbed and ConvNeXt's literal nn.Conv2d calls) against PyTorch's float64
autograd, and the default of the opt-in."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = os.path.join(ROOT, "tests", "golden", "patch_bwd")
NAMES = ["vit_remainder", "vit_tiles", "convnext_stem", "convnext_down"]


def test_backward_symbols_are_exported():
    from uninext_amd import _lib
    for sym in ("patch_embed_hip_backward_workspace_bytes", "patch_embed_hip_backward_f32"):
        assert sym in _lib.PATCH_EMBED_EXPORTS
        assert hasattr(_lib.load(), sym)


def test_backward_argument_errors_need_no_gpu():
    from uninext_amd import _lib
    lib = _lib.load()
    one = 16   # dummy non-null pointer value; rejected calls never dereference
    ws = lib.patch_embed_hip_backward_workspace_bytes(2, 3, 64, 64, 32, 16)
    call = lambda *a: lib.patch_embed_hip_backward_f32(*a)
    # bad dimensions
    assert call(one, one, one, 1, 3, 0, 64, 32, 16, 1, one, one, one, one, ws, None) == -2
    assert "bad dimensions" in _lib.last_error()
    assert call(one, one, one, -1, 3, 64, 64, 32, 16, 1, one, one, one, one, ws, None) == -2
    assert call(one, one, one, 1, 3, 64, 64, 0, 16, 1, one, one, one, one, ws, None) == -2
    assert call(one, one, one, 1, 0, 64, 64, 32, 16, 1, one, one, one, one, ws, None) == -2
    # unsupported geometry: patch 3, K = C k^2 not a multiple of 16
    assert call(one, one, one, 1, 3, 64, 64, 32, 3, 1, one, one, one, one, ws, None) == -5
    assert "patch size" in _lib.last_error()
    assert call(one, one, one, 1, 1, 64, 64, 32, 2, 1, one, one, one, one, ws, None) == -5
    # null pointers: grad_out, x for grad-weight, weight for grad-input, the workspace for grad-weight / grad-bias
    assert call(one, one, None, 2, 3, 64, 64, 32, 16, 1, one, one, one, one, ws, None) == -1
    assert "null pointer" in _lib.last_error()
    assert call(None, one, one, 2, 3, 64, 64, 32, 16, 1, None, one, None, one, ws, None) == -1
    assert call(one, None, one, 2, 3, 64, 64, 32, 16, 1, one, None, None, one, ws, None) == -1
    assert call(one, one, one, 2, 3, 64, 64, 32, 16, 1, None, None, one, None, ws, None) == -1
    # a workspace smaller than the query
    assert call(one, one, one, 2, 3, 64, 64, 32, 16, 1, one, one, one, one, ws - 1, None) == -6
    assert "workspace" in _lib.last_error()
    # nothing requested: nothing to enqueue; x may be NULL without grad-weight, weight without grad-input
    assert call(one, one, one, 2, 3, 64, 64, 32, 16, 1, None, None, None, one, ws, None) == 0
    assert call(None, None, None, 2, 3, 64, 64, 32, 16, 0, None, None, None, None, 0, None) == 0


def test_workspace_size_is_a_function_of_the_shape():
    from uninext_amd import _lib
    q = _lib.load().patch_embed_hip_backward_workspace_bytes
    # bad dimensions / unsupported geometry: 0
    assert q(2, 3, 0, 64, 32, 16) == 0 and q(-1, 3, 64, 64, 32, 16) == 0 and q(2, 3, 64, 64, 0, 16) == 0
    assert q(2, 3, 64, 64, 32, 3) == 0 and q(2, 1, 64, 64, 32, 2) == 0 and q(2, 0, 64, 64, 32, 2) == 0
    # valid shapes: at least 256 bytes (an empty batch included), a multiple of 256, repeatable
    assert q(0, 3, 64, 64, 32, 16) >= 256
    shapes = [(2, 3, 800, 1333, 1280, 16), (2, 3, 800, 1333, 192, 4), (2, 192, 200, 333, 384, 2), (2, 768, 50, 83, 1536, 2),
              (2, 3, 37, 50, 40, 16), (1, 12, 13, 19, 24, 2)]
    for s in shapes:
        assert q(*s) >= 256 and q(*s) % 256 == 0 and q(*s) == q(*s)
    # the split partials of the large shapes hold at least one [E, K] slab plus bias partials, and stay bounded
    B, C, H, W, E, k = shapes[0]
    assert E * C * k * k * 4 < q(*shapes[0]) < 256 << 20
    assert q(2, 3, 800, 1333, 192, 4) < 64 << 20
    # the image size, not only the patch count, is part of the shape: a remainder changes nothing
    assert q(2, 3, 800, 1333, 1280, 16) == q(2, 3, 815, 1343, 1280, 16)


# kernel prefix -> max VGPRs; every kernel: no scratch, no spills
LIMITS = {
    "patch_embed_bwd::patch_wgrad<": 256,
    "patch_embed_bwd::patch_dgrad<": 256,
    "patch_embed_bwd::patch_colsum<": 64,
    "patch_embed_bwd::wgrad_reduce": 64,
    "patch_embed_bwd::zero_remainder": 64,
}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_backward_kernels_compile_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    got = kernel_resources.resources(os.path.join(ROOT, "uninext_amd", "csrc", "patch_embed_bwd.hip"))
    for prefix, max_vgprs in LIMITS.items():
        found = [k for k in got if k.startswith(prefix)]
        assert found, (prefix, sorted(got))
        for k in found:
            r = got[k]
            assert r["vgprs"] <= max_vgprs, (k, r)
            assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0, (k, r)
    assert len([k for k in got if k.startswith("patch_embed_bwd::patch_wgrad<")]) == 16   # 4 patch sizes x 2 layouts x 2 tiles


def _fixture(name):
    with np.load(os.path.join(FIXTURES, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", NAMES)
def test_fixtures_reproduced_by_conv2d_autograd_on_cpu(name):
    g = _fixture(name)
    w = torch.from_numpy(g["weight"]).double()
    E, C, k, _ = w.shape
    conv = torch.nn.Conv2d(C, E, kernel_size=k, stride=k).double()
    conv.load_state_dict({"weight": w, "bias": torch.from_numpy(g["bias"]).double()})
    x = torch.from_numpy(g["x"]).double().requires_grad_(True)
    out = conv(x)
    if int(g["channels_last"]):
        out = out.permute(0, 2, 3, 1)
    out.backward(torch.from_numpy(g["grad_out"]).double())
    rel = lambda a, b: float(np.abs(a.detach().numpy() - b).max()) / max(1e-30, float(np.abs(b).max()))
    assert rel(out, g["out"]) < 1e-6
    assert rel(x.grad, g["gx"]) < 1e-6 and rel(conv.weight.grad, g["gw"]) < 1e-6 and rel(conv.bias.grad, g["gb"]) < 1e-6
    for key in ("gx", "gw", "gb"):
        assert float(np.abs(g[key]).max()) > 0, key


def test_fixtures_cover_the_issue_shapes():
    shapes = {n: (_fixture(n)["x"].shape, _fixture(n)["weight"].shape) for n in NAMES}
    assert shapes["vit_remainder"][0][2:] == (37, 50)
    assert shapes["vit_tiles"][1][0] == 136
    assert shapes["convnext_stem"][1][2] == 4 and np.prod(shapes["convnext_stem"][1][1:]) == 48
    (_, _, H, W), wshape = shapes["convnext_down"]
    assert wshape[2] == 2 and H % 2 == 1 and W % 2 == 1


def test_fixtures_stay_small():
    for f in os.listdir(FIXTURES):
        assert os.path.getsize(os.path.join(FIXTURES, f)) < 1 << 20, f


def test_own_exact_training_is_off_by_default():
    import inspect
    from uninext_amd import backbone
    assert backbone.PatchEmbed.own_exact_training is False
    assert backbone.PatchEmbed(embed_dim=32).own_exact_training is False
    assert inspect.signature(backbone.patch_conv2d).parameters["own_training"].default is False


def test_training_route_stays_with_pytorch_on_cpu():
    from uninext_amd.backbone import PatchEmbed, patch_conv2d
    pe = PatchEmbed(embed_dim=32)
    pe.own_exact_training = True
    x = torch.randn(1, 3, 40, 48, requires_grad=True)
    out = pe(x)
    assert type(out.grad_fn).__name__ == "PermuteBackward0"
    conv = torch.nn.Conv2d(8, 16, kernel_size=2, stride=2)
    assert type(patch_conv2d(torch.randn(1, 8, 6, 6), conv, own_training=True).grad_fn).__name__ == "ConvolutionBackward0"
