"""The encoder's input preparation on the GPU (include/dynmask_hip.h: encprep_hip_*; uninext_amd.modules.prepare_encoder_inputs
with fused = True) against the reference's record (tests/golden/encoder_input/) and the CPU composition, at the smallest shapes
where a kernel can still go wrong: the pixel tile's and the wave's edges, 1 x 1 and H = 1 levels, every kind of mask, the chained
mask source and the NCHW fallback of a fifth level, GroupNorm's hard inputs, repeatability, and the launch / host-copy count.

Bounds (tests/encoder_input_cases.py): mask_flatten, spatial_shapes, level_start_index and valid_ratios bit for bit;
reference_points equal to the CPU's fp32 composition (two correctly rounded operations in the same order: equality is expected,
holds, and is asserted); the position embedding within 4 fp32 ulp at max(1, |expected|) of float64 sin / cos of torch's fp32
argument; GroupNorm within twice torch's own fp32 CPU error against float64 on the same input, never below 4 fp32 ulp of the
largest |output|."""
import os
import sys
import warnings

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import encoder_input_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = 32      # the kernels' pixel tile (ENCPREP_HIP_PIXEL_TILE)


def make_direct(levels, sources, kind, seed, image=None, bs=2, mean=0.0, spread=1.0, constant=None, zero_weight=False):
    """Inputs of ext.encoder_input_prepare on the CPU: convolution outputs per level, the image mask, GroupNorm parameters."""
    g = torch.Generator().manual_seed(seed)
    image = image or (levels[0][0] * 8 - 3, levels[0][1] * 8 - 5)
    convs = [mean + spread * torch.randn((bs, C.D_MODEL, h, w), generator=g) for h, w in levels]
    if constant is not None:
        convs = [torch.full_like(c, constant) for c in convs]
    weights = [torch.zeros(C.D_MODEL) if zero_weight else 1.0 + 0.5 * torch.randn(C.D_MODEL, generator=g) for _ in levels]
    biases = [0.3 * torch.randn(C.D_MODEL, generator=g) for _ in levels]
    return dict(convs=convs, image_mask=C.image_mask(kind, seed + 1, bs=bs, size=image), sources=list(sources), weights=weights,
                biases=biases, eps=[1e-5] * len(levels), level_embed=torch.randn((len(levels), C.D_MODEL), generator=g))


def run_direct(x):
    from uninext_amd import ext
    from uninext_amd.modules import PositionEmbeddingSine
    embed = PositionEmbeddingSine(128, normalize=True)
    to = lambda ts: [t.to(DEV) for t in ts]
    return ext.encoder_input_prepare(to(x["convs"]), x["image_mask"].to(DEV), x["sources"], to(x["weights"]), to(x["biases"]), x["eps"],
                                     x["level_embed"].to(DEV), embed.dim_t(DEV), embed.scale, return_stats=True)


def check(tag, got, convs, image_mask, sources, weights, biases, eps, level_embed):
    """Every output of the fused route against the CPU composition of the same inputs; returns the largest errors."""
    from uninext_amd.modules import get_reference_points, get_valid_ratio
    src, mask_flatten, pos, valid_ratios, reference_points = [t.cpu() for t in got[:5]]
    shapes = [tuple(c.shape[-2:]) for c in convs]
    masks = C.level_masks(image_mask.cpu(), shapes, sum(s < 0 for s in sources))
    assert mask_flatten.dtype == torch.bool and torch.equal(mask_flatten, torch.cat([m.flatten(1) for m in masks], 1)), tag
    want_ratios = torch.stack([get_valid_ratio(m) for m in masks], 1)
    assert torch.equal(valid_ratios, want_ratios), tag
    want_points = get_reference_points(torch.tensor(shapes), want_ratios, "cpu")
    points_ulp = C.refpoint_error_ulp(reference_points, want_points)
    pos_ulp = C.pos_error_ulp(pos, C.pos_expected(masks, level_embed))
    figures = {"reference_points_ulp": points_ulp, "pos_ulp": pos_ulp, "groupnorm": []}
    start = 0
    for l, conv in enumerate(convs):
        n = shapes[l][0] * shapes[l][1]
        expected = C.groupnorm64(conv, weights[l], biases[l], eps[l])
        bound, own = C.groupnorm_bound(conv, weights[l], biases[l], eps[l], expected)
        err = float((src[:, start:start + n].double() - expected).abs().max())
        figures["groupnorm"].append((shapes[l], err, own, bound))
        start += n
    print(tag, "reference_points %.2f ulp, pos %.3f ulp, groupnorm (shape, error, torch's own, bound): %s" % (
        points_ulp, pos_ulp, ["%s %.3e %.3e %.3e" % f for f in figures["groupnorm"]]))
    assert points_ulp == 0.0, (tag, points_ulp)
    assert pos_ulp <= 4.0, (tag, pos_ulp)
    for shape, err, own, bound in figures["groupnorm"]:
        assert err <= bound, (tag, shape, err, own, bound)
    return figures


def check_direct(tag, x):
    from uninext_amd import _lib
    got = run_direct(x)
    assert _lib.last_kernel("encprep") == "encprep_gn_apply"
    check(tag, got, x["convs"], x["image_mask"], x["sources"], x["weights"], x["biases"], x["eps"], x["level_embed"])
    return got


def same_bits(a, b):
    """torch.equal on the bits: a NaN (a reference point of a level whose first row or column is all padding) equals itself."""
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return torch.equal(a, b)


class recorded_call(object):
    """Records the arguments prepare_encoder_inputs hands to ext.encoder_input_prepare: the convolution outputs the kernels
    normalise are the device's own (a convolution may round differently from call to call while its library tunes itself)."""

    def __enter__(self):
        from uninext_amd import ext
        self.ext, self.real, self.args = ext, ext.encoder_input_prepare, None
        ext.encoder_input_prepare = self
        return self

    def __call__(self, *args, **kwargs):
        self.args = (args, kwargs)
        return self.real(*args, **kwargs)

    def __exit__(self, *exc):
        self.ext.encoder_input_prepare = self.real

    def convs(self):
        return [c.cpu() for c in self.args[0][0]]

    def again(self):
        return self.real(*self.args[0], **self.args[1])


@pytest.mark.parametrize("name", C.FIXTURES)
def test_fused_reproduces_the_fixture(name):
    from uninext_amd import _lib
    from uninext_amd.modules import prepare_encoder_inputs
    case, gold = C.make_case(name), C.golden(name)
    feats, mask, proj, level_embed, embed = C.build(case, DEV)
    with torch.no_grad(), recorded_call() as call:
        got = prepare_encoder_inputs(feats, mask, proj, level_embed, embed, fused=True)
    torch.cuda.synchronize()
    assert _lib.last_kernel("encprep") == "encprep_gn_apply"
    for key in C.EXACT_KEYS:
        assert getattr(got, key).dtype == gold[key].dtype and torch.equal(getattr(got, key).cpu(), gold[key]), key
    assert C.refpoint_error_ulp(got.reference_points, gold["reference_points"]) == 0.0
    convs = call.convs()
    check(name, (got.src_flatten, got.mask_flatten, got.lvl_pos_embed_flatten, got.valid_ratios, got.reference_points), convs,
          mask, [-1, -1, -1, 0], [p[1].weight.detach().cpu() for p in proj], [p[1].bias.detach().cpu() for p in proj],
          [p[1].eps for p in proj], level_embed)
    # and against the record's float64 convolutions too, with the CPU test's derived bound for the fp32 convolutions before it
    err = float((got.src_flatten.cpu().double() - gold["src_flatten"]).abs().max())
    assert err <= 64 * float(C.spacing(gold["src_flatten"].abs().max().reshape(1))[0]), err


@pytest.mark.parametrize("hw", [(1, P - 1), (P, 1), (3, 11), (5, 13)])
def test_pixel_tile_edges_with_unaligned_channel_rows(hw):
    assert hw[0] * hw[1] in (P - 1, P, P + 1, 2 * P + 1) and hw[1] % 2 == 1
    check_direct("tile %dx%d" % hw, make_direct([hw], [-1], "padding", 7 + hw[0]))


@pytest.mark.parametrize("hw", [(1, 1), (1, 9)])
def test_one_pixel_and_one_row_levels(hw):
    check_direct("level %dx%d" % hw, make_direct([hw], [-1], "holes", 11 + hw[1], image=(9, 31)))


@pytest.mark.parametrize("h", [1, 2])
@pytest.mark.parametrize("w", [63, 64, 65])
def test_mask_scan_at_the_wave_edges(h, w):
    check_direct("scan %dx%d" % (h, w), make_direct([(h, w)], [-1], "holes", 20 + w + h, image=(h * 3 + 1, w * 2 + 3), bs=1))


@pytest.mark.parametrize("kind", ["none", "padding", "holes", "one_valid", "all_masked"])
def test_every_kind_of_mask(kind):
    """A fully masked image (and every padded column and row of the others) has total 0: the arguments are about -3.1e6, and
    an argument that is not bit-identical to torch's misses by O(1) there."""
    x = make_direct([(6, 9), (3, 5), (2, 3)], [-1, -1, 0], kind, 31, image=(45, 70))
    got = check_direct("mask " + kind, x)
    if kind == "all_masked":
        assert bool(got[1].all()) and float(got[3].abs().max()) == 0.0 and bool(torch.isnan(got[4]).all())


def test_five_levels_over_three_backbone_outputs():
    from uninext_amd.modules import PositionEmbeddingSine, build_input_proj, prepare_encoder_inputs
    g = torch.Generator().manual_seed(5)
    shapes = ((9, 13), (5, 7), (3, 4))
    feats = [torch.randn((2, c, h, w), generator=g).to(DEV) for c, (h, w) in zip(C.IN_CHANNELS, shapes)]
    proj = build_input_proj(C.IN_CHANNELS, C.D_MODEL, 5)
    proj.load_state_dict(C.make_proj_state(C.IN_CHANNELS, 5, 6), strict=True)
    proj = proj.to(DEV).eval()
    level_embed = torch.randn((5, C.D_MODEL), generator=g).to(DEV)
    mask = C.image_mask("holes", 8, size=(70, 100)).to(DEV)
    embed = PositionEmbeddingSine(128, normalize=True)
    with torch.no_grad(), recorded_call() as call:
        got = prepare_encoder_inputs(feats, mask, proj, level_embed, embed, fused=True)
        again = call.again()
        plain = prepare_encoder_inputs([f.cpu() for f in feats], mask.cpu(), proj.cpu(), level_embed.cpu(), embed, fused=False)
    proj.to(DEV)
    assert tuple(map(tuple, got.spatial_shapes.tolist())) == ((9, 13), (5, 7), (3, 4), (2, 2), (1, 1))
    for a, b in zip((got.src_flatten, got.mask_flatten, got.lvl_pos_embed_flatten, got.valid_ratios, got.reference_points), again):
        assert same_bits(a, b)
    for key in C.EXACT_KEYS:
        assert torch.equal(getattr(got, key).cpu(), getattr(plain, key)), key
    assert C.refpoint_error_ulp(got.reference_points, plain.reference_points) == 0.0
    convs = call.convs()
    assert [tuple(c.shape[-2:]) for c in convs] == [(9, 13), (5, 7), (3, 4), (2, 2), (1, 1)] and call.args[0][2] == [-1, -1, -1, 0, 0]
    check("five levels", (got.src_flatten, got.mask_flatten, got.lvl_pos_embed_flatten, got.valid_ratios, got.reference_points), convs,
          mask, [-1, -1, -1, 0, 0], [p[1].weight.detach().cpu() for p in proj], [p[1].bias.detach().cpu() for p in proj],
          [p[1].eps for p in proj], level_embed)
    # the whole route against the CPU composition: fp32 convolutions on both sides, so only a sanity bound (1e-4 of the range)
    assert float((got.src_flatten.cpu() - plain.src_flatten).abs().max()) <= 1e-4 * float(plain.src_flatten.abs().max())


@pytest.mark.parametrize("stress", ["mean_100", "constant", "zero_weight", "several_partials"])
def test_groupnorm_stresses(stress):
    kw = {"mean_100": dict(mean=100.0), "constant": dict(constant=3.25), "zero_weight": dict(zero_weight=True), "several_partials": {}}[stress]
    levels = [(40, 67)] if stress == "several_partials" else [(7, 9), (3, 3)]
    x = make_direct(levels, [-1] * len(levels), "padding", 40, **kw)
    got = check_direct("groupnorm " + stress, x)
    src, mean, rstd = got[0].cpu(), got[5].cpu(), got[6].cpu()
    for l, conv in enumerate(x["convs"]):
        groups = conv.double().view(conv.shape[0], 32, -1)
        want_mean, want_var = groups.mean(-1), groups.var(-1, unbiased=False)
        torch.testing.assert_close(mean[:, l].double(), want_mean, rtol=2 ** -23, atol=1e-30)
        torch.testing.assert_close(rstd[:, l].double(), 1 / torch.sqrt(want_var + 1e-5), rtol=2 ** -22, atol=0)
    if stress == "constant":
        assert float((rstd.double() - 1e-5 ** -0.5).abs().max()) <= 2 ** -22 * 1e-5 ** -0.5
    if stress in ("constant", "zero_weight"):       # the bias alone
        start = 0
        for l, (h, w) in enumerate(levels):
            assert torch.equal(src[:, start:start + h * w], x["biases"][l].expand(src.shape[0], h * w, -1)), stress
            start += h * w
    if stress == "several_partials":
        assert all(same_bits(a, b) for a, b in zip(got, run_direct(x)))


def test_four_launches_and_no_copy_to_the_host(monkeypatch):
    from uninext_amd import ext
    from uninext_amd.modules import prepare_encoder_inputs
    feats, mask, proj, level_embed, embed = C.build(C.make_case("holes"), DEV)
    launched = []
    launch = ext._launch
    monkeypatch.setattr(ext, "_launch", lambda dev, fn, *args: (launched.append(fn.__name__), launch(dev, fn, *args))[1])
    with torch.no_grad():
        prepare_encoder_inputs(feats, mask, proj, level_embed, embed, fused=True)      # warm: the dim_t table, the allocator
        del launched[:]
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                got = prepare_encoder_inputs(feats, mask, proj, level_embed, embed, fused=True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    syncs = [str(w.message) for w in seen if "synchroniz" in str(w.message).lower()]
    print("launches:", launched, "synchronising calls:", syncs)
    assert launched == ["encprep_hip_masks_u8", "encprep_hip_pos_f32", "encprep_hip_gn_stats_f32", "encprep_hip_gn_apply_f32"]
    assert syncs == []
    assert got.src_flatten.is_cuda and got.spatial_shapes.is_cuda and got.level_start_index.tolist() == [0, 35, 47, 51]


def test_unsupported_requests_take_the_composition():
    from uninext_amd import _lib
    from uninext_amd.modules import PositionEmbeddingSine, prepare_encoder_inputs
    feats, mask, proj, level_embed, embed = C.build(C.make_case("padding"), DEV)
    with torch.no_grad():
        fused = prepare_encoder_inputs(feats, mask, proj, level_embed, embed, fused=True)
        ext_calls = []
        import uninext_amd.ext as ext
        real = ext.encoder_input_prepare
        ext.encoder_input_prepare = lambda *a, **k: (ext_calls.append(1), real(*a, **k))[1]
        try:
            plain = prepare_encoder_inputs(feats, mask, proj, level_embed, PositionEmbeddingSine(128, normalize=True, scale=3.0), fused=False)
            half = prepare_encoder_inputs([f.double() for f in feats], mask, proj.double(), level_embed.double(), embed, fused=True)
        finally:
            ext.encoder_input_prepare = real
            proj.float()
    assert ext_calls == [] and half.src_flatten.dtype == torch.float64 and plain.src_flatten.shape == fused.src_flatten.shape
    feats[0].requires_grad_(True)
    with_grad = prepare_encoder_inputs(feats, mask, proj, level_embed, embed, fused=True)
    assert with_grad.src_flatten.requires_grad and _lib.last_kernel("encprep") == "encprep_gn_apply"
