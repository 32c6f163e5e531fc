"""CPU: the encoder's input preparation (uninext_amd/modules/encoder_input.py, uninext_amd/modules/encoder.py and the
encprep_hip_* entry points of include/dynmask_hip.h) without a GPU: the composition against the reference's record
(tests/golden/encoder_input/), state-dict keys, the nearest-index rule, the C ABI's names and refusals, the kernels' resources,
and the order in which DeformableTransformerEncoderVL visits its layers."""
import ctypes
import json
import math
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import encoder_input_cases as C  # noqa: E402

NAMES = ("encprep_hip_workspace_bytes", "encprep_hip_masks_u8", "encprep_hip_pos_f32", "encprep_hip_gn_stats_f32",
         "encprep_hip_gn_apply_f32", "encprep_hip_last_kernel")


@pytest.mark.parametrize("name", C.FIXTURES)
def test_composition_reproduces_the_fixture(name):
    from uninext_amd.modules import prepare_encoder_inputs
    case, gold = C.make_case(name), C.golden(name)
    feats, mask, proj, level_embed, embed = C.build(case)
    with torch.no_grad():
        got = prepare_encoder_inputs(feats, mask, proj, level_embed, embed, fused=False)
    for key in C.EXACT_KEYS:
        assert getattr(got, key).dtype == gold[key].dtype and torch.equal(getattr(got, key), gold[key]), key
    # reference_points: two correctly rounded fp32 operations in the reference's order -- equality holds
    assert C.refpoint_error_ulp(got.reference_points, gold["reference_points"]) == 0.0
    # position embedding: the bound of the GPU tests, for the composition and for the record alike
    masks = C.level_masks(mask, C.LEVELS, len(feats))
    expected = C.pos_expected(masks, level_embed)
    for what, pos in (("composition", got.lvl_pos_embed_flatten), ("golden", gold["lvl_pos_embed_flatten"])):
        err = C.pos_error_ulp(pos, expected)
        print(name, what, "position embedding: %.3f ulp" % err)
        assert err <= 4.0, (what, err)
    # src_flatten: fp32 convolutions (at most 144 products) and torch's own fp32 GroupNorm against the float64 record: 64 fp32
    # ulp of the largest |output| covers the dot products' rounding (~ sqrt(144) / 2 ulp of their size) through a normalisation
    # whose gain |weight| * rstd * |x| stays below ~5 here.  (The GroupNorm bound proper, twice torch's own error, is what this
    # composition defines: tests/test_encoder_input_gpu.py.)
    err = float((got.src_flatten.double() - gold["src_flatten"]).abs().max())
    bound = 64 * float(C.spacing(gold["src_flatten"].abs().max().reshape(1))[0])
    print(name, "src_flatten: error %.3e, bound %.3e" % (err, bound))
    assert got.src_flatten.dtype == torch.float32 and err <= bound


def test_state_dict_keys_and_shapes_equal_the_recorded_ones():
    from uninext_amd.modules import DeformableTransformerEncoderVL, build_input_proj
    want = json.load(open(os.path.join(C.HERE, "state_dict_keys.json")))
    proj = build_input_proj(C.IN_CHANNELS, C.D_MODEL, len(C.LEVELS))
    assert [[k, list(v.shape)] for k, v in proj.state_dict().items()] == want["input_proj"]
    assert all(float(p[0].bias.detach().abs().max()) == 0.0 for p in proj)
    assert proj[3][0].kernel_size == (3, 3) and proj[3][0].stride == (2, 2) and proj[3][0].padding == (1, 1)
    assert len(build_input_proj(C.IN_CHANNELS, C.D_MODEL, 5)) == 5 and build_input_proj(C.IN_CHANNELS, C.D_MODEL, 5)[4][0].in_channels == 256
    assert len(build_input_proj((7,), C.D_MODEL, 1)) == 1
    enc = DeformableTransformerEncoderVL(nn.Linear(2, 2), nn.Linear(3, 3), nn.Identity(), C.ENCODER_VL_STUB["num_layers"],
                                         num_vl_layers=C.ENCODER_VL_STUB["num_vl_layers"])
    assert [[k, list(v.shape)] for k, v in enc.state_dict().items()] == want["DeformableTransformerEncoderVL"]
    assert [[n, type(m).__name__, [type(c).__name__ for c in m]] for n, m in enc.named_children()] == want["DeformableTransformerEncoderVL.children"]
    with pytest.raises(ValueError, match="NOT supported for now"):
        DeformableTransformerEncoderVL(nn.Identity(), nn.Linear(3, 3), nn.Identity(), 2, use_checkpoint=True)
    with pytest.raises(ValueError, match="nn.Identity"):
        DeformableTransformerEncoderVL(nn.Identity(), nn.Linear(3, 3), nn.Linear(3, 3), 2)


def test_position_embedding_class_is_the_references():
    from uninext_amd.modules import NestedTensor, PositionEmbeddingSine
    with pytest.raises(ValueError, match="normalize should be True if scale is passed"):
        PositionEmbeddingSine(64, scale=1.0)
    embed = PositionEmbeddingSine(128, normalize=True)
    assert embed.scale == 2 * math.pi and embed.temperature == 10000
    mask = C.image_mask("holes", 3, size=(6, 9))
    nested = NestedTensor(torch.zeros((C.BS, 4, 6, 9), dtype=torch.float64), mask)
    assert nested.decompose()[1] is mask
    pos = embed(nested)
    assert pos.shape == (C.BS, 256, 6, 9) and pos.dtype == torch.float32
    dim_t = torch.arange(128, dtype=torch.float32)
    assert torch.equal(embed.dim_t("cpu"), 10000 ** (2 * (dim_t // 2) / 128)) and embed.dim_t("cpu") is embed.dim_t("cpu")
    plain = PositionEmbeddingSine(64)(nested)       # not normalised: the counts themselves
    assert plain.shape == (C.BS, 128, 6, 9)


def nearest_index(dst, size_in, size_out):
    """The kernels' rule: min(int(floorf(dst * (float(in) / out))), in - 1), every step in fp32."""
    scale = np.float32(size_in) / np.float32(size_out)
    return min(int(np.floor(np.float32(dst) * scale)), size_in - 1)


def test_nearest_rule_equals_interpolate_for_every_pair_up_to_70_and_chained():
    sizes = range(1, 71)
    table = {}
    for n_in in sizes:
        src = torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in)
        for n_out in sizes:
            want = F.interpolate(src, size=(1, n_out))[0, 0, 0].long().tolist()
            got = [nearest_index(d, n_in, n_out) for d in range(n_out)]
            assert got == want, (n_in, n_out)
            table[n_in, n_out] = got
    for n_img in (13, 40, 56, 70):       # image -> level 0 -> a further level, as the reference resizes masks[0]
        src = torch.arange(n_img, dtype=torch.float32).view(1, 1, 1, n_img)
        for n0 in (1, 5, 7, 34, 69):
            for n1 in (1, 2, 3, 17, 70):
                want = F.interpolate(F.interpolate(src, size=(1, n0)), size=(1, n1))[0, 0, 0].long().tolist()
                assert [table[n_img, n0][table[n0, n1][d]] for d in range(n1)] == want, (n_img, n0, n1)


def test_interpolate_mask_and_valid_ratio_helpers():
    from uninext_amd.modules import get_reference_points, get_valid_ratio, interpolate_mask
    mask = C.image_mask("padding", 0)
    small = interpolate_mask(mask, (5, 7))
    assert small.dtype == torch.bool and small.shape == (C.BS, 5, 7)
    rows = [nearest_index(y, 40, 5) for y in range(5)]
    cols = [nearest_index(x, 56, 7) for x in range(7)]
    assert torch.equal(small, mask[:, rows][:, :, cols])
    ratio = get_valid_ratio(small)
    assert ratio.shape == (C.BS, 2) and torch.equal(ratio[:, 0], (~small[:, 0, :]).sum(1).float() / 7)
    points = get_reference_points(torch.tensor([[5, 7]]), ratio[:, None], "cpu")
    assert points.shape == (C.BS, 35, 1, 2)


def test_every_export_is_in_the_header_the_table_and_the_library():
    from uninext_amd import _lib
    text = open(os.path.join(ROOT, "include", "dynmask_hip.h")).read()
    declared = set(re.findall(r"\b(encprep_hip_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(NAMES)
    assert {n for n in _lib.DYNMASK_EXPORTS if n.startswith("encprep_")} == set(NAMES)
    lib = _lib.load()
    for n in NAMES:
        assert getattr(lib, n).argtypes is not None
    assert (_lib.ENCPREP_MAX_LEVELS, _lib.ENCPREP_CHANNELS, _lib.ENCPREP_GROUPS, _lib.ENCPREP_PIXEL_TILE) == tuple(
        int(re.search(r"#define ENCPREP_HIP_%s (\d+)" % k, text).group(1)) for k in ("MAX_LEVELS", "CHANNELS", "GROUPS", "PIXEL_TILE"))
    assert _lib.last_kernel("encprep") in ("", "encprep_masks", "encprep_pos", "encprep_gn_stats", "encprep_gn_apply")


def levels_of(rows):
    flat = [v for row in rows for v in row]
    return (ctypes.c_int * len(flat))(*flat), len(rows)


def test_launchers_refuse_before_any_runtime_call():
    from uninext_amd import _lib
    lib = _lib.load()
    one, odd, null = ctypes.c_void_p(64), ctypes.c_void_p(68), ctypes.c_void_p(0)
    ptrs = lambda v, n=1: (ctypes.c_void_p * n)(*([v] * n))
    eps = (ctypes.c_float * 8)(*([1e-5] * 8))
    lv, n = levels_of([(5, 7, -1), (3, 4, -1), (2, 2, 0)])
    masks = lambda m=one, B=2, Hi=40, Wi=56, lv=lv, n=n, out=one: lib.encprep_hip_masks_u8(m, B, Hi, Wi, lv, n, out, one, one, one, null)
    pos = lambda a=one, le=one, out=one, B=2, lv=lv, n=n, ch=256: lib.encprep_hip_pos_f32(a, one, one, le, one, B, lv, n, ch, 6.28, 1e-6, out, one, null)
    stats = lambda x=ptrs(one, 3), B=2, lv=lv, n=n, ch=256, g=32, ws=one, nb=1 << 20: lib.encprep_hip_gn_stats_f32(x, B, lv, n, ch, g, ws, nb, null)
    apply_ = lambda x=ptrs(one, 3), w=ptrs(one, 3), e=eps, B=2, lv=lv, n=n, ch=256, g=32, out=one, nb=1 << 20: lib.encprep_hip_gn_apply_f32(
        x, w, w, e, one, nb, B, lv, n, ch, g, out, one, one, null)

    def refused(rc, code, text):
        assert rc == code and text in _lib.last_error(), (rc, _lib.last_error())

    # empty problems: 0, nothing launched, whatever the pointers
    assert masks(m=null, B=0) == 0 and pos(a=null, B=0) == 0 and stats(x=null, B=0) == 0 and apply_(x=null, B=0) == 0
    assert masks(m=null, lv=null, n=0) == 0 and lib.encprep_hip_workspace_bytes(0, lv, n) == 0
    nine, n9 = levels_of([(2, 2, -1)] * 9)
    for call in (masks, pos, stats, apply_):
        refused(call(lv=nine, n=n9), -5, "at most 8 levels")
        refused(call(B=-1), -2, "bad dimensions")
        refused(call(lv=levels_of([(5, 0, -1)])[0], n=1), -2, "bad dimensions")
        refused(call(lv=levels_of([(5, 7, -1), (3, 4, 1)])[0], n=2), -2, "mask source")
        refused(call(lv=levels_of([(5, 7, -1), (3, 4, 0), (2, 2, 1)])[0], n=3), -2, "mask source")
        refused(call(lv=null), -1, "null pointer")
    refused(masks(m=null), -1, "encprep_masks: null pointer argument")
    refused(masks(out=null), -1, "encprep_masks: null pointer argument")
    refused(masks(Hi=0), -2, "encprep_masks: bad dimensions")
    refused(pos(a=null), -1, "encprep_pos: null pointer argument")
    refused(pos(ch=128), -5, "encprep_pos: 256 channels (num_pos_feats 128) only")
    refused(pos(le=odd), -5, "encprep_pos: level_embed and lvl_pos_embed must be 16-byte aligned")
    refused(pos(out=odd), -5, "encprep_pos: level_embed and lvl_pos_embed must be 16-byte aligned")
    refused(stats(ch=128), -5, "encprep_gn_stats: GroupNorm(32, 256) only")
    refused(stats(g=16), -5, "encprep_gn_stats: GroupNorm(32, 256) only")
    refused(stats(x=null), -1, "encprep_gn_stats: null pointer argument")
    refused(stats(x=ptrs(null, 3)), -1, "encprep_gn_stats: null pointer argument")
    refused(stats(x=ptrs(odd, 3)), -5, "encprep_gn_stats: x must be 16-byte aligned")
    refused(stats(nb=16), -2, "encprep_gn_stats: partials below encprep_hip_workspace_bytes or not 16-byte aligned")
    refused(stats(ws=ctypes.c_void_p(72)), -2, "encprep_gn_stats: partials below encprep_hip_workspace_bytes or not 16-byte aligned")
    refused(apply_(ch=512), -5, "encprep_gn_apply: GroupNorm(32, 256) only")
    refused(apply_(w=ptrs(null, 3)), -1, "encprep_gn_apply: null pointer argument")
    refused(apply_(e=null), -1, "encprep_gn_apply: null pointer argument")
    refused(apply_(out=odd), -5, "encprep_gn_apply: src_flatten and partials must be 16-byte aligned")
    refused(apply_(nb=16), -2, "encprep_gn_apply: partials below encprep_hip_workspace_bytes")
    refused(apply_(e=(ctypes.c_float * 8)()), -2, "encprep_gn_apply: eps must be positive")
    # the workspace: 16 bytes per (image, level, group, slice); (5, 7), (3, 4) and (2, 2) are one slice each
    assert lib.encprep_hip_workspace_bytes(2, lv, n) == 2 * 3 * 32 * 16
    big, nb = levels_of([(40, 67, -1)])
    assert lib.encprep_hip_workspace_bytes(1, big, nb) == 32 * 5 * 16       # 5360 float4 a group: five slices of >= 1024


def test_launchers_refuse_cpu_tensors_and_other_geometries():
    from uninext_amd import ext
    convs = [torch.zeros((2, 256, 3, 4))]
    assert not ext.encoder_input_supported(convs, torch.zeros((2, 8, 8), dtype=torch.bool))
    with pytest.raises(RuntimeError, match="encoder_input_prepare"):
        ext.encoder_input_prepare(convs, torch.zeros((2, 8, 8), dtype=torch.bool), [-1], [torch.ones(256)], [torch.zeros(256)], [1e-5],
                                  torch.zeros((1, 256)), torch.ones(128), 6.28)


def test_fused_request_on_the_cpu_runs_the_composition():
    from uninext_amd.modules import prepare_encoder_inputs
    case = C.make_case("padding")
    feats, mask, proj, level_embed, embed = C.build(case)
    with torch.no_grad():
        a = prepare_encoder_inputs(feats, mask, proj, level_embed, embed, fused=True)
        b = prepare_encoder_inputs(feats, mask, proj, level_embed, embed, fused=False)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert a._fields == ("src_flatten", "mask_flatten", "lvl_pos_embed_flatten", "spatial_shapes", "level_start_index", "valid_ratios",
                         "reference_points")


def test_kernels_compile_for_gfx950_without_scratch():
    import kernel_resources
    got = kernel_resources.resources(os.path.join(ROOT, "uninext_amd", "csrc", "enc_prep.hip"))
    assert set(got) == {"encprep::masks", "encprep::pos", "encprep::gn_stats", "encprep::gn_apply"}
    for name, r in got.items():
        print(name, r)
        assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, (name, r)
    # LDS does not grow with the level: only gn_apply's tile (32 pixels x 260 floats) and the two small reduction arrays
    assert got["encprep::masks"]["lds"] == 0 and got["encprep::pos"]["lds"] == 0
    assert got["encprep::gn_stats"]["lds"] == 64 and got["encprep::gn_apply"]["lds"] == 32 * 260 * 4 + 512


def test_encoder_vl_visits_its_layers_in_the_references_order():
    from uninext_amd.modules import DeformableTransformerEncoderVL
    log = []

    class VL(nn.Module):
        def forward(self, output, task=None):
            log.append(("vl", task, float(output["visual"].sum())))
            return {"visual": output["visual"] + 1, "lang": output["lang"]}

    class Layer(nn.Module):
        def forward(self, src, pos, reference_points, spatial_shapes, level_start_index, padding_mask):
            log.append(("layer", tuple(reference_points.shape), float(src.sum())))
            return src * 2

    enc = DeformableTransformerEncoderVL(VL(), Layer(), nn.Identity(), 3, num_vl_layers=2)
    assert [type(m).__name__ for m in enc.vl_layers] == ["VL", "VL", "Identity"]
    shapes = torch.tensor([[2, 3], [1, 2]])
    ratios = torch.ones((1, 2, 2))
    src = torch.ones((1, 8, 1))
    lang = {"hidden": torch.zeros(1), "masks": torch.ones(1)}
    out = enc(src, shapes, torch.tensor([0, 6]), ratios, pos=None, padding_mask=None, language_dict_features=lang, task="detection")
    assert set(out) == {"visual", "lang"} and out["lang"] is lang
    assert log == [("vl", "detection", 8.0), ("layer", (1, 8, 2, 2), 16.0), ("vl", "detection", 32.0), ("layer", (1, 8, 2, 2), 40.0),
                   ("layer", (1, 8, 2, 2), 80.0)]
    assert float(out["visual"].sum()) == 160.0
    want = DeformableTransformerEncoderVL.get_reference_points(shapes, ratios, "cpu")
    assert want.shape == (1, 8, 2, 2) and float(want[0, 0, 0, 0]) == float(np.float32(0.5) / np.float32(3))
