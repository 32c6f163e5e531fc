"""The ViT attention core's training route (Attention.own_training, patch_embed_hip_vit_attn_train_f32 /
patch_embed_hip_vit_attn_backward_f32 in include/patch_embed_hip.h): everything that needs no GPU."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vit_cases as C          # noqa: E402
import vit_train_cases as T    # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# as shipped: a regression pin, not an acceptance number.  The key passes and bwd_q<80, true> add accumulation registers on top
# and run at one wave per SIMD.
MAX_VGPRS = {"vit_attn_bwd::attn_lse<64, true>": 181, "vit_attn_bwd::attn_lse<64, false>": 178,
             "vit_attn_bwd::attn_lse<80, true>": 187, "vit_attn_bwd::attn_lse<80, false>": 165,
             "vit_attn_bwd::bwd_q<64, true>": 196, "vit_attn_bwd::bwd_q<64, false>": 150,
             "vit_attn_bwd::bwd_q<80, true>": 247, "vit_attn_bwd::bwd_q<80, false>": 201,
             "vit_attn_bwd::bwd_kv<64, true>": 254, "vit_attn_bwd::bwd_kv<64, false>": 242,
             "vit_attn_bwd::bwd_kv<80, true>": 256, "vit_attn_bwd::bwd_kv<80, false>": 256,
             "vit_attn_bwd::dtables<64>": 28, "vit_attn_bwd::dtables<80>": 28, "vit_attn_bwd::dtables_reduce": 8}


def test_fixtures_load():
    assert T.NAMES == T.EXPECTED
    for name in T.NAMES:
        fx = T.load(name)
        assert list(fx["keys"]) == list(fx["state"]) and float(fx["fp32_err"]) < 3e-5
        assert sorted(fx["grad"]) == sorted(["x"] + [k for k in fx["state"]])
        tables = [k for k in fx["state"] if k.endswith("rel_pos_h") or k.endswith("rel_pos_w")]
        assert tables and all(float(fx["grad"][k].abs().max()) > 0 for k in tables)
        zero = all(float(fx["state"][k].abs().max()) == 0 for k in tables)
        assert zero == (name == "net_small_grad")                # the reference's initial state in the net file only
        assert os.path.getsize(os.path.join(T.HERE, name + ".npz")) < 500000


@pytest.mark.parametrize("name", T.EXPECTED)
def test_float64_torch_route_reproduces_the_fixtures(name):
    fx = T.load(name)
    m = T.module_from(name, fx, torch.float64)
    got = T.gradients(m, fx, torch.float64)
    for k, want in fx["grad"].items():
        assert C.rel_err(T.stored_view(fx, k, got[k]), want) < 1e-6, k      # stored rounded to float32


def test_error_codes_without_a_device():
    from uninext_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(1 << 20)      # never dereferenced: every check runs before the device is touched
    off = ctypes.c_void_p((1 << 20) + 4)
    big = 1 << 40

    def train(qkv=fake, th=fake, tw=fake, dims=(1, 2, 14, 14, 80), out=fake, lse=fake, ws=fake, ws_bytes=big):
        return lib.patch_embed_hip_vit_attn_train_f32(qkv, th, tw, *dims, 0.125, out, lse, ws, ws_bytes, None)

    def back(qkv=fake, th=fake, tw=fake, out=fake, lse=fake, g=fake, dims=(1, 2, 14, 14, 80), gq=fake, gth=fake, gtw=fake, ws=fake,
             ws_bytes=big):
        return lib.patch_embed_hip_vit_attn_backward_f32(qkv, th, tw, out, lse, g, *dims, 0.125, gq, gth, gtw, ws, ws_bytes, None)

    for call in (train, back):
        assert call(qkv=None) == -1 and "null" in _lib.last_error()
        assert call(out=None) == -1 and call(lse=None) == -1 and call(ws=None) == -1
        assert call(tw=None) == -1 and "both or neither" in _lib.last_error()
        assert call(th=None) == -1
        assert call(dims=(1, 2, 0, 14, 80)) == -2 and "dimensions" in _lib.last_error()
        assert call(dims=(1, 0, 14, 14, 80)) == -2 and call(dims=(-1, 2, 14, 14, 80)) == -2 and call(dims=(1, 2, 14, -3, 80)) == -2
        assert call(dims=(1, 2, 5000, 2, 80)) == -2 and "large" in _lib.last_error()
        assert call(dims=(1, 2, 14, 14, 48)) == -5 and "head_dim" in _lib.last_error()
        assert call(dims=(1, 2, 2, 257, 80)) == -5 and "q_w" in _lib.last_error()
        assert call(qkv=off) == -5 and "aligned" in _lib.last_error()
        assert call(lse=off) == -5
        assert call(ws_bytes=16) == -6
        assert call(dims=(0, 2, 14, 14, 80)) == 0                # an empty batch enqueues nothing
        assert call(dims=(0, 2, 14, 14, 48)) == -5               # the geometry is still checked
    assert back(g=None) == -1 and back(gq=None) == -1 and back(gth=None) == -1 and back(gtw=None) == -1
    assert back(g=off) == -5 and back(gq=off) == -5 and back(gtw=off) == -5
    assert train(ws_bytes=lib.patch_embed_hip_vit_attn_workspace_bytes(1, 2, 14, 14, 80) - 1) == -6
    assert back(ws_bytes=lib.patch_embed_hip_vit_attn_backward_workspace_bytes(1, 2, 14, 14, 80) - 1) == -6
    assert back(qkv=None, th=None, tw=None, out=None, lse=None, g=None, dims=(0, 2, 14, 14, 64), gq=None, gth=None, gtw=None, ws=None,
                ws_bytes=0) == 0                                  # and needs no buffer
    assert _lib.last_kernel("vit_attn_bwd") == "" or _lib.last_kernel("vit_attn_bwd").startswith("vit_")
    for n in ("patch_embed_hip_vit_attn_train_f32", "patch_embed_hip_vit_attn_backward_workspace_bytes",
              "patch_embed_hip_vit_attn_backward_f32", "patch_embed_hip_vit_attn_backward_last_kernel"):
        assert n in _lib.PATCH_EMBED_EXPORTS and hasattr(lib, n)


def test_workspace_query_is_monotone_and_small():
    from uninext_amd import _lib
    q = _lib.load().patch_embed_hip_vit_attn_backward_workspace_bytes
    base = (2, 4, 14, 20, 64)
    assert q(*base) > 0 and q(0, 2, 14, 14, 64) > 0 and q(1, 1, 1, 1, 64) > 0
    for axis in range(4):
        grown = list(base)
        grown[axis] += 3
        assert q(*grown) >= q(*base), axis
    assert q(2, 4, 14, 20, 80) >= q(*base)
    for B, heads, qh, qw, D in ((48, 16, 14, 14, 80), (2, 16, 64, 64, 80), (1, 2, 37, 61, 64)):
        assert q(B, heads, qh, qw, D) < B * heads * (qh * qw) ** 2 * 4 // 2       # next to one fp32 score matrix
    for bad in ((1, 2, 14, 14, 48), (1, 2, 0, 14, 80), (1, 2, 4096, 2, 80), (1, 2, 2, 257, 64)):
        assert q(*bad) == 0, bad


def test_own_training_takes_the_torch_route_where_the_kernels_do_not_apply():
    """CPU tensors, fp64, autocast, head sizes the kernels lack: with own_training on, the gradients are the flag-off ones."""
    from uninext_amd import vit

    class OnGpu:
        def __init__(self, *shape, dtype=torch.float32, requires_grad=False):
            self.shape, self.dtype, self.is_cuda, self.device, self.requires_grad = torch.Size(shape), dtype, True, torch.device("cpu"), requires_grad

        def dim(self):
            return len(self.shape)

    def grads(m, x):
        x = x.clone().requires_grad_(True)
        for p in m.parameters():
            p.grad = None
        m(x).square().sum().backward()
        return [x.grad] + [p.grad for p in m.parameters()]

    torch.manual_seed(3)
    a = vit.Attention(128, num_heads=2, use_rel_pos=True, rel_pos_zero_init=False, input_size=(5, 6))
    small = vit.Attention(96, num_heads=2, use_rel_pos=True, rel_pos_zero_init=False, input_size=(5, 6))       # head_dim 48
    x, xs = torch.randn(2, 5, 6, 128), torch.randn(2, 5, 6, 96)
    assert vit.Attention.own_training is False
    import copy
    cases = [(a, x), (small, xs), (copy.deepcopy(a).double(), x.double())]
    off = [grads(m, t) for m, t in cases]
    entered = []
    old_apply = vit.ViTAttentionFunction.apply
    vit.ViTAttentionFunction.apply = lambda *args: entered.append(1) or old_apply(*args)
    vit.Attention.own_training = True
    try:
        for (m, t), want in zip(cases, off):
            assert not m._use_hip_training(t)
            for g, w in zip(grads(m, t), want):
                assert torch.equal(g, w)
        assert a._use_hip_training(OnGpu(1, 5, 6, 128))                                 # what the route takes ...
        assert not a._use_hip_training(OnGpu(1, 5, 6, 128, dtype=torch.float64))       # ... and what it leaves
        assert not a._use_hip_training(OnGpu(1, 5, 6, 64)) and not small._use_hip_training(OnGpu(1, 5, 6, 96))
        is_autocast = torch.is_autocast_enabled
        torch.is_autocast_enabled = lambda *args: True                                  # autocast on the GPU, which is not here
        try:
            assert not a._use_hip_training(OnGpu(1, 5, 6, 128))
        finally:
            torch.is_autocast_enabled = is_autocast
        with torch.no_grad():
            assert not a._use_hip_training(OnGpu(1, 5, 6, 128))                         # autograd does not record
        vit.Attention.own_training = False
        assert not a._use_hip_training(OnGpu(1, 5, 6, 128))
        assert not entered
    finally:
        vit.Attention.own_training = False
        vit.ViTAttentionFunction.apply = old_apply
    net = vit.ViT(img_size=64, embed_dim=128, depth=2, num_heads=2, use_rel_pos=True, window_size=2, window_block_indexes=(0,))
    assert net.set_own_training(True) is net and all(b.attn.own_training for b in net.blocks) and net.patch_embed.own_exact_training
    net.set_own_training(False)
    assert not any(b.attn.own_training for b in net.blocks) and not net.patch_embed.own_exact_training


def test_kernel_resources():
    import shutil
    if shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None:
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    got = kernel_resources.resources(os.path.join(ROOT, "uninext_amd", "csrc", "vit_attn_bwd.hip"))
    for kernel, max_vgprs in MAX_VGPRS.items():
        assert kernel in got, (kernel, sorted(got))
        r = got[kernel]
        print("%-36s vgprs %d agprs %d scratch %d B/lane lds %d occupancy %d" % (kernel, r["vgprs"], r.get("agprs", -1), r["scratch"],
                                                                               r.get("lds", -1), r["occupancy"]))
        assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0, (kernel, r)
        assert r["vgprs"] <= max_vgprs, (kernel, r)
