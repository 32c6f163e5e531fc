"""ViT backbone blocks (uninext_amd/vit.py, patch_embed_hip_vit_attn_f32 in include/patch_embed_hip.h): everything that needs no GPU."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vit_cases as C   # noqa: E402
import vit_ref as R     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_VGPRS = {"vit_attn::attn<64, true>": 180, "vit_attn::attn<64, false>": 177, "vit_attn::attn<80, true>": 186,
             "vit_attn::attn<80, false>": 164, "vit_attn::rel_terms<64>": 84, "vit_attn::rel_terms<80>": 100}   # as shipped


def test_fixtures_load():
    assert C.NAMES == C.EXPECTED
    for name in C.NAMES:
        fx = C.load(name)
        assert list(fx["keys"]) == list(fx["state"])
        assert 1.0 < float(fx["score_absmax"]) < 110.0 and float(fx["fp32_err"]) < 3e-5
        assert 0.05 <= float(fx["softmax_median_max"]) <= 0.9
        assert os.path.getsize(os.path.join(C.HERE, name + ".npz")) < 500000


@pytest.mark.parametrize("name", C.EXPECTED)
def test_modules_float64_and_restatement_match_the_fixtures(name):
    """The modules in float64 against the reference's outputs, and tests/vit_ref.py on the core's input against the core's
    output; state-dict keys in the reference's order, strict load (inside module_from)."""
    fx = C.load(name)
    m = C.module_from(name, fx, torch.float64)
    assert list(m.state_dict()) == list(fx["keys"])
    out, core_in, core_out = C.run_with_core(m, torch.from_numpy(fx["x"]).double())
    outs = out if isinstance(out, dict) else {"out": out}
    assert sorted(outs) == sorted(C.output_keys(fx))
    for k in outs:
        assert C.rel_err(C.stored_view(fx, k, outs[k]), fx[k]) < 1e-11, k
    assert C.rel_err(C.stored_view(fx, "core_out", core_out), fx["core_out"]) < 1e-11
    assert C.rel_err(core_in[:, torch.from_numpy(fx["core_in_rows"])], fx["core_in"]) < 1e-6      # stored rounded to float32
    a = C.first_attention(m)
    S = core_in.shape[1]
    hw = (14, 14) if S == 196 else (17, 20)
    th, tw = R.resize_table(a.rel_pos_h.detach(), 2 * hw[0] - 1), R.resize_table(a.rel_pos_w.detach(), 2 * hw[1] - 1)
    got = R.core(core_in, th, tw, a.num_heads, hw, a.scale)
    assert C.rel_err(C.stored_view(fx, "core_out", got), fx["core_out"]) < 1e-11


def test_padded_tokens_are_keys():
    """block_win_padded: 17 x 20 tokens in windows of 14 are padded to 28 x 28; dropping the padded keys changes the output."""
    fx = C.load("block_win_padded")
    m = C.module_from("block_win_padded", fx, torch.float64)
    _, core_in, core_out = C.run_with_core(m, torch.from_numpy(fx["x"]).double())
    assert core_in.shape[:2] == (4, 196)
    a = m.attn
    w = 3                                                      # the last window: 3 x 6 real tokens
    keep = torch.zeros(14, 14, dtype=torch.bool)
    keep[:3, :6] = True
    t = core_in[w:w + 1].reshape(1, 196, 3, a.num_heads, -1)
    q, k, v = (t[:, :, j].permute(0, 2, 1, 3) for j in range(3))
    s = R.scores(core_in[w:w + 1], a.rel_pos_h.detach(), a.rel_pos_w.detach(), a.num_heads, (14, 14), a.scale)
    s_real = s.masked_fill(~keep.reshape(1, 1, 1, 196), float("-inf"))
    out_real = torch.matmul(s_real.softmax(-1), v).permute(0, 2, 1, 3).reshape(1, 196, -1)
    assert C.rel_err(out_real, core_out[w:w + 1]) > 1e-3


def test_exact_family_is_exact():
    """Scores are the same numbers in fp32 and float64, and the fp32 PyTorch composition keeps TOL_EXACT on every exact case the
    GPU tests use."""
    from uninext_amd.vit import add_decomposed_rel_pos
    for D, hw in ((64, (9, 15)), (80, (14, 14))):
        qkv, th, tw, scale = R.exact_case(5, 2, 2, hw, D)
        s64 = R.scores(qkv, th, tw, 2, hw, scale)
        S = hw[0] * hw[1]
        t = qkv.reshape(2, S, 3, 2, D).permute(2, 0, 3, 1, 4).reshape(3, 4, S, D)
        s32 = add_decomposed_rel_pos((t[0] * scale) @ t[1].transpose(-2, -1), t[0], th, tw, hw, hw)
        assert torch.equal(s32.double().reshape(s64.shape), s64)
        p = s64.softmax(-1).max(-1)[0]
        assert 0.05 < float(p.median()) < 0.9
        assert C.rel_err(R.composition_fp32(qkv, th, tw, 2, hw, scale), R.core(qkv, th, tw, 2, hw, scale)) < C.TOL_EXACT


def test_window_round_trip_with_padding():
    from uninext_amd.vit import window_partition, window_unpartition
    x = torch.arange(2 * 17 * 20 * 3, dtype=torch.float64).reshape(2, 17, 20, 3) + 1
    w, pad_hw = window_partition(x, 14)
    assert w.shape == (8, 14, 14, 3) and pad_hw == (28, 28)
    want, _ = R.window_partition(x, 14)
    assert torch.equal(w, want)
    assert torch.equal(w[1, :, 6:], torch.zeros(14, 8, 3, dtype=torch.float64)) and float(w[1, 0, 5, 0]) == float(x[0, 0, 19, 0])
    assert torch.equal(window_unpartition(w, 14, pad_hw, (17, 20)), x)
    w, pad_hw = window_partition(x[:, :14, :14], 14)           # no padding: a view round trip
    assert pad_hw == (14, 14) and torch.equal(window_unpartition(w, 14, pad_hw, (14, 14)), x[:, :14, :14])


def test_get_rel_pos_interpolates_like_the_reference():
    from uninext_amd.vit import get_rel_pos, resize_rel_pos
    fx = C.load("attn_global_interp")
    for key, n in (("rel_pos_h", 17), ("rel_pos_w", 20)):
        table = fx["state"][key]
        assert table.shape[0] == 127
        stored = torch.from_numpy(fx[key.replace("pos_", "") + "_resized"])
        assert stored.shape == (2 * n - 1, table.shape[1])
        assert float((resize_rel_pos(table, 2 * n - 1) - stored).abs().max()) < 1e-12
        assert float((R.resize_table(table, 2 * n - 1) - stored).abs().max()) < 1e-12
        got = get_rel_pos(n, n, table)
        idx = torch.arange(n)[:, None] - torch.arange(n)[None, :] + n - 1
        assert got.shape == (n, n, table.shape[1]) and float((got - stored[idx]).abs().max()) < 1e-12
    assert resize_rel_pos(fx["state"]["rel_pos_h"], 127) is fx["state"]["rel_pos_h"]


def test_constructors_follow_the_reference():
    from uninext_amd import vit
    from uninext_amd.backbone import PatchEmbed
    with pytest.raises(ValueError, match="use_residual_block"):
        vit.Block(128, 2, use_residual_block=True)
    with pytest.raises(ValueError):
        vit.ViT(embed_dim=128, depth=2, num_heads=2, residual_block_indexes=(1,))
    with pytest.raises(ValueError):
        vit.vit_kwargs("ViT-Tiny")
    kw = vit.vit_kwargs("ViT-huge")
    assert (kw["embed_dim"], kw["depth"], kw["num_heads"], kw["drop_path_rate"], kw["window_size"]) == (1280, 32, 16, 0.5, 14)
    assert [vit.vit_kwargs(n)["embed_dim"] // vit.vit_kwargs(n)["num_heads"] for n in ("ViT-Base", "ViT-Large", "ViT-huge")] == [64, 64, 80]
    kw = dict(vit.vit_kwargs("ViT-Base"), depth=3, embed_dim=128, num_heads=2)
    m = vit.ViT(**kw)
    assert isinstance(m.patch_embed, PatchEmbed) and m.pos_embed.shape == (1, 197, 128)
    assert [b.window_size for b in m.blocks] == [14, 14, 0] and m.blocks[0].attn.rel_pos_h.shape == (27, 64)
    assert m.blocks[2].attn.rel_pos_w.shape == (127, 64) and m.blocks[0].norm1.eps == 1e-6
    assert isinstance(m.blocks[0].drop_path, torch.nn.Identity) and abs(m.blocks[2].drop_path.drop_prob - 0.1) < 1e-7
    assert float(m.blocks[0].attn.rel_pos_h.abs().max()) == 0 and isinstance(m.fpn1[0], torch.nn.ConvTranspose2d)
    assert vit.Attention.fused_core in (True, False)
    x = torch.randn(1, 3, 64, 96)
    m.eval()
    with torch.no_grad():
        out = m(x)
    assert {k: tuple(v.shape) for k, v in out.items()} == {"res3": (1, 64, 8, 12), "res4": (1, 128, 4, 6), "res5": (1, 128, 2, 3)}
    ck = vit.ViT(**dict(kw, use_act_checkpoint=True, drop_path_rate=0.0))
    ck.load_state_dict(m.state_dict(), strict=True)
    y = ck(x.requires_grad_(True))["res4"]
    y.sum().backward()
    assert x.grad is not None and float(x.grad.abs().max()) > 0


def test_routing_predicate():
    """Everything that must go to PyTorch does: CPU tensors, other dtypes, autograd recording, head sizes the kernel lacks,
    the switch off.  (A tensor stand-in says it is on the GPU; the parameters stay where they are, so _fp32_on is patched.)"""
    from uninext_amd import vit

    class OnGpu:
        def __init__(self, *shape, dtype=torch.float32, requires_grad=False):
            self.shape, self.dtype, self.is_cuda, self.device, self.requires_grad = torch.Size(shape), dtype, True, torch.device("cpu"), requires_grad

        def dim(self):
            return len(self.shape)

    a = vit.Attention(128, num_heads=2, use_rel_pos=True, input_size=(14, 14)).eval()
    small = vit.Attention(96, num_heads=2, use_rel_pos=True, input_size=(14, 14)).eval()       # head_dim 48
    old = vit.Attention.fused_core
    try:
        vit.Attention.fused_core = True
        with torch.no_grad():
            assert not a._use_hip(torch.zeros(1, 14, 14, 128))                                 # a CPU tensor
            assert a._use_hip(OnGpu(1, 14, 14, 128))
            assert not a._use_hip(OnGpu(1, 14, 14, 128, dtype=torch.float64))
            assert not a._use_hip(OnGpu(1, 14, 14, 64))
            assert not small._use_hip(OnGpu(1, 14, 14, 96))
            vit.Attention.fused_core = False
            assert not a._use_hip(OnGpu(1, 14, 14, 128))
            vit.Attention.fused_core = True
        assert not a._use_hip(OnGpu(1, 14, 14, 128))                                           # autograd records: the parameters
        for p in a.parameters():
            p.requires_grad_(False)
        assert a._use_hip(OnGpu(1, 14, 14, 128))
        assert not a._use_hip(OnGpu(1, 14, 14, 128, requires_grad=True))                       # autograd records: the input
        # the last (H, W) only is kept of the interpolated tables
        b = vit.Attention(128, num_heads=2, use_rel_pos=True, rel_pos_zero_init=False, input_size=(64, 64))
        t1 = b._resized_tables(17, 20)
        assert b._resized_tables(17, 20)[0] is t1[0] and t1[0].shape == (33, 64) and t1[1].shape == (39, 64)
        assert b._resized_tables(9, 9)[0].shape == (17, 64) and b._tables[0][:2] == (9, 9)
        with torch.no_grad():
            b.rel_pos_h.add_(1.0)
        assert b._resized_tables(9, 9)[0] is not t1[0] and float(b._resized_tables(9, 9)[0].mean()) > 0.5
    finally:
        vit.Attention.fused_core = old


def test_error_codes_without_a_device():
    from uninext_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(1 << 20)      # never dereferenced: every check runs before the device is touched
    call = lambda qkv, th, tw, B, H, qh, qw, D, out=fake, ws=fake, ws_bytes=1 << 40: lib.patch_embed_hip_vit_attn_f32(
        qkv, th, tw, B, H, qh, qw, D, 0.125, out, ws, ws_bytes, None)
    assert call(None, fake, fake, 1, 2, 14, 14, 80) == -1 and "null" in _lib.last_error()
    assert call(fake, fake, fake, 1, 2, 14, 14, 80, out=None) == -1
    assert call(fake, fake, None, 1, 2, 14, 14, 80) == -1 and "both or neither" in _lib.last_error()
    assert call(fake, None, fake, 1, 2, 14, 14, 80) == -1
    assert call(fake, fake, fake, 1, 2, 0, 14, 80) == -2 and "dimensions" in _lib.last_error()
    assert call(fake, fake, fake, 1, 0, 14, 14, 80) == -2
    assert call(fake, fake, fake, -1, 2, 14, 14, 80) == -2
    assert call(fake, fake, fake, 1, 2, 14, -3, 80) == -2
    assert call(fake, fake, fake, 1, 2, 5000, 2, 80) == -2 and "large" in _lib.last_error()
    assert call(fake, fake, fake, 1, 2, 14, 14, 48) == -5 and "head_dim" in _lib.last_error()
    assert call(ctypes.c_void_p((1 << 20) + 4), fake, fake, 1, 2, 14, 14, 80) == -5 and "aligned" in _lib.last_error()
    assert call(fake, fake, fake, 1, 2, 14, 14, 80, ws_bytes=16) == -6
    need = lib.patch_embed_hip_vit_attn_workspace_bytes(1, 2, 14, 14, 80)
    assert call(fake, fake, fake, 1, 2, 14, 14, 80, ws_bytes=need - 1) == -6
    assert call(fake, fake, fake, 0, 2, 14, 14, 80) == 0          # an empty batch enqueues nothing
    assert call(fake, None, None, 0, 2, 14, 14, 64) == 0
    assert call(None, None, None, 0, 2, 14, 14, 64, out=None, ws=None, ws_bytes=0) == 0     # and needs no buffer
    assert call(None, None, None, 0, 2, 14, 14, 48, out=None, ws=None, ws_bytes=0) == -5    # the geometry is still checked
    assert _lib.last_kernel("vit_attn") == "" or _lib.last_kernel("vit_attn").startswith("vit_")


def test_workspace_is_small_next_to_the_scores():
    from uninext_amd import _lib
    lib = _lib.load()
    for B, heads, qh, qw, D in ((48, 16, 14, 14, 80), (2, 16, 50, 84, 80), (48, 12, 14, 14, 64), (2, 12, 50, 84, 64)):
        S = qh * qw
        ws = lib.patch_embed_hip_vit_attn_workspace_bytes(B, heads, qh, qw, D)
        assert ws == B * heads * (qh + qw) * ((S + 31) // 32 * 32) * 4           # a function of the shapes only
        assert 0 < ws < B * heads * S * S * 4 // 4
    assert lib.patch_embed_hip_vit_attn_workspace_bytes(1, 1, 1, 1, 64) > 0
    assert lib.patch_embed_hip_vit_attn_workspace_bytes(0, 2, 14, 14, 64) > 0
    for bad in ((1, 2, 14, 14, 48), (1, 2, 0, 14, 80), (1, 0, 14, 14, 80), (1, 2, 4096, 2, 80), (1, 2, 2048, 1024, 80)):
        assert lib.patch_embed_hip_vit_attn_workspace_bytes(*bad) == 0, bad


def test_supported_agrees_with_the_c_side():
    """vit_attention_supported on stand-ins for GPU tensors against the workspace query (0 = the C side refuses the shape)."""
    from uninext_amd import _lib, ext
    lib = _lib.load()

    class OnGpu:
        def __init__(self, *shape, dtype=torch.float32, contiguous=True):
            self.shape, self.dtype, self.is_cuda, self.device, self._c = torch.Size(shape), dtype, True, "gpu", contiguous

        def dim(self):
            return len(self.shape)

        def is_contiguous(self):
            return self._c

        def data_ptr(self):
            return 1 << 20

    class Misaligned(OnGpu):
        def data_ptr(self):
            return (1 << 20) + 8

    for B, heads, qh, qw, D in ((1, 2, 14, 14, 80), (3, 1, 1, 1, 64), (2, 2, 9, 15, 64), (1, 2, 14, 14, 48), (1, 2, 14, 14, 96),
                                (1, 1, 4096, 2, 64), (1, 1, 2, 4095, 80), (0, 2, 5, 5, 64)):
        qkv, th, tw = OnGpu(B, qh * qw, 3 * heads * D), OnGpu(2 * qh - 1, D), OnGpu(2 * qw - 1, D)
        c_side = lib.patch_embed_hip_vit_attn_workspace_bytes(B, heads, qh, qw, D) > 0
        assert ext.vit_attention_supported(qkv, th, tw, heads, (qh, qw)) == c_side, (B, heads, qh, qw, D)
        assert ext.vit_attention_supported(qkv, None, None, heads, (qh, qw)) == c_side
    qkv, th, tw = OnGpu(1, 196, 480), OnGpu(27, 80), OnGpu(27, 80)
    assert ext.vit_attention_supported(qkv, th, tw, 2, (14, 14))
    assert not ext.vit_attention_supported(qkv, th, None, 2, (14, 14))                       # one table without the other
    assert not ext.vit_attention_supported(qkv, OnGpu(28, 80), tw, 2, (14, 14))              # a table of another length
    assert not ext.vit_attention_supported(qkv, th, tw, 2, (14, 13))
    assert not ext.vit_attention_supported(OnGpu(1, 196, 480, dtype=torch.float64), th, tw, 2, (14, 14))
    assert not ext.vit_attention_supported(OnGpu(1, 196, 480, contiguous=False), th, tw, 2, (14, 14))
    assert not ext.vit_attention_supported(torch.zeros(1, 196, 480), None, None, 2, (14, 14))  # a CPU tensor
    assert not ext.vit_attention_supported(Misaligned(1, 196, 480), th, tw, 2, (14, 14))
    assert not ext.vit_attention_supported(qkv, Misaligned(27, 80), tw, 2, (14, 14))


def test_header_and_table_carry_the_new_names():
    from uninext_amd import _lib
    names = ("patch_embed_hip_vit_attn_workspace_bytes", "patch_embed_hip_vit_attn_f32", "patch_embed_hip_vit_attn_last_kernel")
    lib = _lib.load()
    for n in names:
        assert n in _lib.PATCH_EMBED_EXPORTS and hasattr(lib, n)
    assert _lib.load().msda_hip_abi_version() == 2


def test_kernel_resources():
    import shutil
    if shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None:
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    got = kernel_resources.resources(os.path.join(ROOT, "uninext_amd", "csrc", "vit_attn.hip"))
    for kernel, max_vgprs in MAX_VGPRS.items():
        assert kernel in got, (kernel, sorted(got))
        r = got[kernel]
        print("%-28s vgprs %d scratch %d B/lane lds %d occupancy %d" % (kernel, r["vgprs"], r["scratch"], r.get("lds", -1), r["occupancy"]))
        assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0, (kernel, r)
        assert r["vgprs"] <= max_vgprs, (kernel, r)
