"""CPU tests of the static mask head's training route: the C ABI of conv3x3_hip_backward_exact_f32 and its helpers
(include/conv3x3_hip.h; argument checks and size queries, no GPU work), the register budgets of the new kernels, the gradient
fixtures (tests/golden/maskhead_bwd, minted from the reference class) against the module's PyTorch path in float64, and the
default of the opt-in."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = os.path.join(ROOT, "tests", "golden", "maskhead_bwd")


def test_backward_argument_errors_need_no_gpu():
    from uninext_amd import _lib
    lib = _lib.load()
    one = 16
    ws = lib.conv3x3_hip_backward_workspace_bytes(1, 16, 4, 4, 8)
    call = lambda *a: lib.conv3x3_hip_backward_exact_f32(*a)
    # bad dimensions
    assert call(one, one, one, one, 1, 16, 0, 4, 8, 1, one, one, one, one, ws, None) == -2
    assert "bad dimensions" in _lib.last_error()
    assert call(one, one, one, one, -1, 16, 4, 4, 8, 1, one, one, one, one, ws, None) == -2
    assert call(one, one, one, one, 1, 16, 4, 4, 0, 1, one, one, one, one, ws, None) == -2
    # null pointers: grad_out, out under relu, the workspace, the packed weights for grad-input, the input for grad-weight
    assert call(one, one, one, None, 1, 16, 4, 4, 8, 1, one, one, one, one, ws, None) == -1
    assert call(one, one, None, one, 1, 16, 4, 4, 8, 1, one, one, one, one, ws, None) == -1
    assert call(one, one, one, one, 1, 16, 4, 4, 8, 1, one, one, one, None, ws, None) == -1
    assert call(one, None, one, one, 1, 16, 4, 4, 8, 1, one, None, None, one, ws, None) == -1
    assert call(None, one, one, one, 1, 16, 4, 4, 8, 1, None, one, None, one, ws, None) == -1
    assert "null pointer" in _lib.last_error()
    # a workspace smaller than the query
    assert call(one, one, one, one, 1, 16, 4, 4, 8, 1, one, one, one, one, ws - 1, None) == -2
    assert "workspace" in _lib.last_error()
    # nothing requested, or an empty batch without parameter gradients: nothing to enqueue
    assert call(one, one, one, one, 1, 16, 4, 4, 8, 1, None, None, None, one, ws, None) == 0
    assert call(None, None, None, None, 0, 16, 4, 4, 8, 1, None, None, None, None, 0, None) == 0
    assert lib.conv3x3_hip_pack_weight_exact_dgrad_f32(one, 0, 16, one, None) == -2
    assert lib.conv3x3_hip_pack_weight_exact_dgrad_f32(None, 8, 16, one, None) == -1


def test_workspace_and_packing_sizes():
    from uninext_amd import _lib
    lib = _lib.load()
    q = lib.conv3x3_hip_backward_workspace_bytes
    assert q(1, 16, 0, 4, 8) == 0 and q(-1, 16, 4, 4, 8) == 0 and q(0, 16, 4, 4, 8) == 0
    # at least the ReLU-masked gradient with its channels padded to 16, the per-split partials of grad-weight and the bias partials
    for B, cin, cout, H, W in ((1, 16, 8, 5, 7), (2, 64, 8, 100, 168), (2, 256, 256, 100, 168), (3, 48, 130, 9, 31)):
        cp = (cout + 15) // 16 * 16
        assert q(B, cin, H, W, cout) >= 4 * (B * cp * H * W + cout * cin * 9 + B * cout)
        assert q(B, cin, H, W, cout) % 256 == 0
        assert q(B, cin, H, W, cout) == q(B, cin, H, W, cout)          # a function of the shape only
    assert q(2, 256, 100, 168, 256) < 128 << 20                       # jia_dcn at the training shapes: bounded split count
    d = lib.conv3x3_hip_packed_exact_dgrad_weight_bytes
    assert d(8, 64) == lib.conv3x3_hip_packed_exact_weight_bytes(64, 16)     # cout 8 -> 16 input channels of the transposed conv
    assert d(256, 256) == lib.conv3x3_hip_packed_exact_weight_bytes(256, 256)
    assert d(2, 16) == lib.conv3x3_hip_packed_exact_weight_bytes(16, 16)
    assert d(0, 16) == 0 and d(8, 0) == 0


# kernel -> (max VGPRs, max scratch bytes per lane).  conv3x3_wgrad holds 9 x 16 accumulator registers per lane and runs two
# workgroups per CU: at most 256 registers.
LIMITS = {
    "conv3x3_bwd::conv3x3_wgrad": (256, 0),
    "conv3x3_bwd::relu_bias_kernel": (32, 0),
    "conv3x3_bwd::pack_weight_dgrad_kernel": (32, 0),
    "conv3x3_bwd::wgrad_reduce_kernel": (32, 0),
}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_backward_kernels_compile_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    got = kernel_resources.resources(os.path.join(ROOT, "uninext_amd", "csrc", "conv3x3_bwd.hip"))
    for kernel, (max_vgprs, max_scratch) in LIMITS.items():
        assert kernel in got, (kernel, sorted(got))
        r = got[kernel]
        assert r["vgprs"] <= max_vgprs, (kernel, r)
        assert r["scratch"] <= max_scratch and r.get("vgpr_spill", 0) == 0, (kernel, r)


def _fixture(name):
    with np.load(os.path.join(FIXTURES, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", ["nofpn", "fpn"])
def test_fixtures_reproduced_by_module_on_cpu(name):
    from uninext_amd.mask_head import MaskHeadSmallConv
    g = _fixture(name)
    fpn_dims = [g["fpn%d" % i].shape[1] for i in range(3)] if "fpn0" in g else None
    dim = g["x0"].shape[1]
    assert dim == 64
    head = MaskHeadSmallConv(dim, fpn_dims, dim).double()
    params = {k[2:]: torch.from_numpy(v).double() for k, v in g.items() if k.startswith("p:")}
    assert sorted(head.state_dict()) == sorted(params)
    head.load_state_dict(params)
    x = [torch.from_numpy(g["x%d" % i]).double().requires_grad_(True) for i in range(3)]
    fpns = [torch.from_numpy(g["fpn%d" % i]).double().requires_grad_(True) for i in range(3)] if fpn_dims else None
    out = head(x, fpns)
    out.backward(torch.from_numpy(g["grad_out"]).double())
    rel = lambda a, b: float(np.abs(a.detach().numpy() - b).max()) / max(1e-30, float(np.abs(b).max()))
    assert rel(out, g["out"]) < 1e-6
    for i, t in enumerate(x):
        assert rel(t.grad, g["gx%d" % i]) < 1e-6
    for i, t in enumerate(fpns or ()):
        assert rel(t.grad, g["gfpn%d" % i]) < 1e-6
    for k, p in head.named_parameters():
        assert float(np.abs(g["g:" + k]).max()) > 0, k                 # every parameter's gradient is exercised
        assert rel(p.grad, g["g:" + k]) < 1e-6, k


def test_fixtures_stay_small():
    for f in os.listdir(FIXTURES):
        assert os.path.getsize(os.path.join(FIXTURES, f)) < 1 << 20, f


def test_own_exact_training_is_off_by_default():
    from uninext_amd import mask_head
    assert mask_head.MaskHeadSmallConv.own_exact_training is False
    assert mask_head.MaskHeadSmallConv(64, None, 64).own_exact_training is False
    import inspect
    assert inspect.signature(mask_head.conv3x3_relu).parameters["own_training"].default is False
