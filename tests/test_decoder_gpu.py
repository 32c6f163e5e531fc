"""The decoder's self-attention core on the GPU (biattn_hip_self_forward_f32) against the float64 restatement, and the
decoder modules of uninext_amd/modules/decoder_layer.py on it against the fixtures of tests/golden/decoder/."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_cases as C   # noqa: E402
import decoder_ref as R     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME = {None: "dec_attn<none>", torch.bool: "dec_attn<bool>", torch.float32: "dec_attn<f32>"}
# lengths and the hazard each is the smallest to reach (tiles of 32 keys, 32 queries per workgroup, two key ranges per workgroup)
LENS = [1,      # one key, one query
        31,     # a tail in the only tile; the second key range is empty
        33,     # a tail of 1 in the second tile and the second workgroup; one tile per range
        97,     # four tiles, two per range; more than one workgroup per (b, h)
        130]    # five tiles: ranges of 3 and 2


def gpu(t):
    return None if t is None else t.to(DEV)


def run_kernel(q, k, v, heads, mask=None, scale=None):
    from uninext_amd import _lib, ext
    out = ext.decoder_self_attention(gpu(q), gpu(k), gpu(v), heads, gpu(mask), scale)
    torch.cuda.synchronize()
    assert _lib.last_kernel("dec_attn") == NAME[None if mask is None else mask.dtype]
    return out


def check(q, k, v, heads, mask=None, scale=None, nan_rows=()):
    want = R.core(q, k, v, heads, mask, scale)
    got = run_kernel(q, k, v, heads, mask, scale).cpu()
    keep = [i for i in range(q.shape[1]) if i not in nan_rows]
    assert torch.isfinite(got[:, keep]).all()
    for i in nan_rows:
        assert torch.isnan(got[:, i]).all() and torch.isnan(want[:, i]).all()
    err = C.rel_err(got[:, keep], want[:, keep])
    print("B %d L %d heads %d mask %s: err %.2e" % (q.shape[0], q.shape[1], heads, None if mask is None else mask.dtype, err))
    assert err < C.TOL, err
    return got, want


def halves(qk):
    E = qk.shape[-1] // 2
    return qk[..., :E], qk[..., E:]


def random_bool_mask(seed, L):
    m = torch.rand(L, L, generator=torch.Generator().manual_seed(seed)) < 0.3
    m[:, 0] = False                                    # no row is empty
    return m


@pytest.mark.parametrize("L", LENS)
@pytest.mark.parametrize("kind", ["none", "bool", "float"])
def test_kernel_matches_the_restatement(L, kind):
    qk, v = C.kernel_case(20 + L, 2, L, 2)
    mask = None if kind == "none" else random_bool_mask(L, L)
    if kind == "float":
        mask = torch.randn(L, L, generator=torch.Generator().manual_seed(L)) * 2.0
    check(*halves(qk), v, 2, mask)


@pytest.mark.parametrize("B,heads", [(1, 1), (7, 1), (1, 7), (2, 8)])
def test_batch_and_head_counts(B, heads):
    qk, v = C.kernel_case(40 + B, B, 33, heads)
    check(*halves(qk), v, heads, random_bool_mask(3, 33))


def test_strided_views_and_separate_tensors_agree():
    from uninext_amd import ext
    qk, v = C.kernel_case(51, 2, 97, 2)
    q, k = halves(qk)
    assert not q.is_contiguous()
    got_views, _ = check(q, k, v, 2)
    qk_d = gpu(qk)
    qd, kd = halves(qk_d)
    assert qd.stride(1) == 128 and kd.data_ptr() == qk_d.data_ptr() + 64 * 4          # read in place
    assert ext.decoder_self_attention_supported(qd, kd, gpu(v), 2, None)
    got_sep = run_kernel(q.contiguous(), k.contiguous(), v, 2).cpu()
    assert torch.equal(got_views, got_sep)
    got_scaled = run_kernel(q * 0.5, k, v, 2, scale=2 * 32 ** -0.5).cpu()             # q_scale is applied to q: exact for 2
    assert torch.equal(got_views, got_scaled)
    # what the predicate refuses
    assert not ext.decoder_self_attention_supported(qd, kd, gpu(v), 4, None)          # head_dim 16
    assert not ext.decoder_self_attention_supported(qd, kd, gpu(v), 2, torch.zeros(2, 97, 97, dtype=torch.bool, device=DEV))
    assert not ext.decoder_self_attention_supported(qd, kd, gpu(v), 2, torch.zeros(97, 97, dtype=torch.float64, device=DEV))
    assert not ext.decoder_self_attention_supported(qd, kd, gpu(v), 2, torch.zeros(97, 97, dtype=torch.bool))
    assert not ext.decoder_self_attention_supported(qd.double(), kd.double(), gpu(v).double(), 2, None)
    assert not ext.decoder_self_attention_supported(qk_d[..., 1:65], kd, gpu(v), 2, None)   # 4-byte aligned only
    assert ext.decoder_self_attention(qd[:0], kd[:0], gpu(v)[:0], 2).shape == (0, 97, 64)    # an empty batch


def test_denoising_mask_with_wholly_excluded_leading_tiles():
    """len 130, pad_size 64: every query >= 64 has its first two key tiles wholly excluded (its running max is still -inf after
    them), and the two groups of 32 exclude each other's tile."""
    L, pad = 130, 64
    qk, v = C.kernel_case(61, 2, L, 2)
    q, k = halves(qk)
    m = C.dn_mask(L, pad, 2)
    assert bool(m[pad:, :pad].all()) and bool(m[:32, 32:64].all()) and not bool(m.all(1).any())
    got_bool, _ = check(q, k, v, 2, m)
    f = torch.zeros(L, L).masked_fill(m, float("-inf"))
    got_f, _ = check(q, k, v, 2, f)
    assert C.rel_err(got_bool, got_f) < C.TOL_SAME
    # the same exclusions as very negative finite numbers: no tile can be skipped, the probabilities underflow to 0
    got_big, _ = check(q, k, v, 2, torch.zeros(L, L).masked_fill(m, -1e30))
    assert C.rel_err(got_bool, got_big) < C.TOL_SAME


def test_exclusions_at_the_far_end():
    L = 130
    qk, v = C.kernel_case(62, 1, L, 2)
    q, k = halves(qk)
    m = torch.zeros(L, L, dtype=torch.bool)
    m[:, 64:] = True                                   # the last three key tiles (all of the second range, one of the first)
    got, _ = check(q, k, v, 2, m)
    short = R.core(q[:, :64], k[:, :64], v[:, :64], 2)
    assert C.rel_err(got[:, :64], short) < C.TOL       # the same as attention over the first 64 keys alone
    m = torch.ones(L, L, dtype=torch.bool)
    m[:, 129] = False                                  # a single open key in the last tile
    got, _ = check(q, k, v, 2, m)
    assert C.rel_err(got, v[:, 129:130].expand(1, L, -1)) < C.TOL_SAME
    m[:, 129] = True
    m[:, 40] = False                                   # ... and in the first range, with every later tile excluded
    got, _ = check(q, k, v, 2, m)
    assert C.rel_err(got, v[:, 40:41].expand(1, L, -1)) < C.TOL_SAME


def test_one_fully_excluded_row_is_nan_and_nothing_else():
    L = 97
    qk, v = C.kernel_case(63, 2, L, 2)
    for mask in (random_bool_mask(5, L), torch.randn(L, L, generator=torch.Generator().manual_seed(6))):
        mask[45] = True if mask.dtype == torch.bool else float("-inf")
        check(*halves(qk), v, 2, mask, nan_rows=(45,))


def test_late_maximum_flat_and_large_scores():
    L, heads = 130, 2
    # late maximum: q = 4 e0; k[:, 0] = 8 on key 0, 40 on the last key, 0 elsewhere: every row's largest score sits in the last key
    # tile (the second range), the second largest (far below) in the first
    q = torch.zeros(1, L, heads, 32)
    k = torch.zeros(1, L, heads, 32)
    q[..., 0] = 4.0
    k[:, 0, :, 0] = 8.0
    k[:, L - 1, :, 0] = 40.0
    v = torch.randn(1, L, heads * 32, generator=torch.Generator().manual_seed(3))
    flat = lambda t: t.reshape(1, L, -1)
    got, _ = check(flat(q), flat(k), v, heads, scale=0.125)
    assert C.rel_err(got, v[:, L - 1:L].expand(1, L, -1)) < 1e-3        # nearly one-hot on the last key
    k[:, L - 1, :, 0], k[:, 70, :, 0] = 0.0, 40.0                       # ... and in the first range's last tile
    got, _ = check(flat(q), flat(k), v, heads, scale=0.125)
    assert C.rel_err(got, v[:, 70:71].expand(1, L, -1)) < 1e-3
    # flat: all scores equal, the output is the mean of v
    k.zero_()
    got, _ = check(flat(q), flat(k), v, heads, scale=0.125)
    assert C.rel_err(got, v.mean(dim=1, keepdim=True).expand(1, L, -1)) < 1e-5
    # scores of +-1e4: finite and within the bound
    q.zero_()
    q[..., 0] = 100.0
    k[..., 0] = (torch.randint(0, 2, (1, L, heads), generator=torch.Generator().manual_seed(4)) * 2 - 1).float() * 100.0
    s = torch.einsum("blhd,bmhd->bhlm", q, k)
    assert float(s.abs().max()) == 1e4
    check(flat(q), flat(k), v, heads, scale=1.0)


def test_bitwise_repeatable_across_runs_and_streams_and_leaves_biattn_alone():
    from uninext_amd import _lib, ext
    before = _lib.last_kernel("biattn")
    qk, v = C.kernel_case(71, 2, 130, 2)
    q, k = halves(gpu(qk))
    v, m = gpu(v), gpu(C.dn_mask(130, 64, 2))
    a = ext.decoder_self_attention(q, k, v, 2, m)
    b = ext.decoder_self_attention(q, k, v, 2, m)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = ext.decoder_self_attention(q, k, v, 2, m)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)
    assert _lib.last_kernel("dec_attn") == "dec_attn<bool>" and _lib.last_kernel("biattn") == before


@pytest.mark.parametrize("name", sorted(C.FIXTURES))
def test_modules_fp32_match_the_fixtures(name):
    from uninext_amd import _lib, ext
    from uninext_amd.modules import DeformableTransformerDecoderLayer as Layer
    cfg, st, x = C.make_case(name)
    fx = C.load(name)
    assert C.digest(st) == float(fx["digest"])
    wants = (fx["out"], fx["points"]) if cfg["kind"] == "decoder" else (fx["out"],)
    mask = x.get("attn_mask")
    # the kind the layer hands the kernel: make_case's float mask is float64, C.run casts it to the module's fp32
    kind = None if mask is None else torch.bool if mask.dtype == torch.bool else torch.float32
    marker = torch.zeros(1, 1, 32, device=DEV)
    old = Layer.fused_self_attn
    try:
        for fused in (True, False):
            Layer.fused_self_attn = fused
            m = C.build(name, cfg, st, torch.float32, DEV)
            # a call of another kind first: last_kernel must change when the module runs the kernel, and only then
            other = None if kind == torch.float32 else torch.zeros(1, 1, device=DEV)
            ext.decoder_self_attention(marker, marker, marker, 1, other)
            outs = C.run(cfg, m, x, DEV, torch.float32)
            torch.cuda.synchronize()
            for got, want in zip(outs, wants):
                err = C.rel_err(got, want)
                print(name, "fused" if fused else "torch", "%.2e" % err)
                assert err < C.TOL, (fused, err)
            assert _lib.last_kernel("dec_attn") == NAME[kind if fused else None if other is None else torch.float32]
    finally:
        Layer.fused_self_attn = old


def test_a_3d_mask_takes_the_composition_and_still_matches():
    from uninext_amd import _lib, ext
    from uninext_amd.modules import DeformableTransformerDecoderLayer as Layer
    cfg, st, x = C.make_case("layer_dn_mask")
    fx = C.load("layer_dn_mask")
    x = dict(x)
    x["attn_mask"] = x["attn_mask"][None].expand(2 * cfg["heads"], -1, -1).contiguous()     # [B * heads, L, L]
    marker = torch.zeros(1, 1, 32, device=DEV)
    old = Layer.fused_self_attn
    try:
        Layer.fused_self_attn = True
        m = C.build("layer_dn_mask", cfg, st, torch.float32, DEV)
        ext.decoder_self_attention(marker, marker, marker, 1)
        (out,) = C.run(cfg, m, x, DEV, torch.float32)
        assert C.rel_err(out, fx["out"]) < C.TOL
        assert _lib.last_kernel("dec_attn") == "dec_attn<none>"          # the marker's: the layer did not call the kernel
    finally:
        Layer.fused_self_attn = old
