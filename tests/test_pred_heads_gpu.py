"""Decoder prediction heads on the GPU: the HIP route (pred_heads_hip_f32) against the reference's float64 fixtures, and the
kernel's own contracts (repeatability, row-position independence, strides, NULL scale, clamp, optional outputs, the two grids,
error codes)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pred_heads_cases as C   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LVL = C.LEVELS - 1
KERNEL = "pred_heads<split>"


@functools.lru_cache(maxsize=None)
def case(name):
    """(fixture, cfg, fp32 GPU heads, float64 CPU heads, inputs), built once per fixture and left unchanged."""
    fx = C.load(name)
    cfg, states, x = C.make_case(name)
    assert int(fx["seed"]) == cfg["seed"] and C.digest(states) == float(fx["digest"])
    return fx, cfg, C.build(cfg, states, torch.float32, DEV), C.build(cfg, states, torch.float64), x


def flat(mlp):
    return [t.detach() for l in mlp.layers for t in (l.weight, l.bias)]


def kernel_args(name, rows=slice(None)):
    """The arguments of ext.pred_heads for the last level of a fixture, as DetectionHeads passes them; rows: a slice of Q."""
    fx, cfg, heads, _, x = case(name)
    hs, _, inter_references, text = C.inputs(x, torch.float32, DEV)
    text = text["hidden"]
    if cfg["task"] == "grounding":
        from uninext_amd.modules import agg_lang_feat
        text = agg_lang_feat(text, x["masks"].to(DEV)).unsqueeze(1)
    with torch.no_grad():
        tokens, bias, scale, clamp = heads.class_terms(LVL, text)
    iou = (heads.iou_head[LVL].weight.detach(), heads.iou_head[LVL].bias.detach()) if cfg["iou"] else None
    return dict(hs=hs[LVL][:, rows].contiguous(), tokens=tokens.detach(), token_bias=bias.detach(),
                scale=None if scale is None else scale.detach(), clamp=clamp,
                reference=inter_references[LVL - 1][:, rows].contiguous(), box_mlp=flat(heads.bbox_embed[LVL]), iou=iou,
                controller=flat(heads.controller))


def logits64(name, gain=1.0, scale=True, clamp=0.0):
    """Float64 logits of a VL_Align fixture from the float64 modules, its tokens multiplied by gain."""
    fx, cfg, _, heads64, x = case(name)
    head = heads64.class_embed[LVL]
    with torch.no_grad():
        tokens, bias = head.token_terms(x["hidden"])
        want = torch.matmul(x["hs"][LVL], (tokens * gain).transpose(-1, -2)) / (head.log_scale.exp() if scale else 1.0)
    want = want + bias.unsqueeze(1)
    return want.clamp(-clamp, clamp) if clamp else want


def close(got, want, what):
    got, want = got.detach().cpu().double().numpy(), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert np.isfinite(got).all(), what
    err, bound = float(np.abs(got - want).max()), C.TOL * float(np.abs(want).max())
    print("%-28s max abs error %.3e, bound %.3e" % (what, err, bound))
    assert err <= bound, (what, err, bound)


def equal(a, b):
    return all((s is None and t is None) or torch.equal(s, t) for s, t in zip(a, b))


def last():
    from uninext_amd import _lib
    return _lib.last_kernel("pred_heads")


@pytest.mark.parametrize("name", list(C.FIXTURES))
def test_fused_route_matches_the_reference(name):
    fx, cfg, heads, _, x = case(name)
    out = C.run(cfg, heads, x, DEV, torch.float32, fused=True)
    assert last() == KERNEL
    assert set(out) == {k for k in C.OUTPUTS if k in fx}
    for k, v in out.items():
        close(v, fx[k], k)
    if cfg["iou"]:
        assert tuple(out["pred_boxious"].shape) == (C.B, C.Q, 1)
    if name == "detection":                  # level 0 with its own heads and init_reference, without the controller
        hs, init_reference, _, text = C.inputs(x, torch.float32, DEV)
        with torch.no_grad():
            got = heads.forward_level(0, hs[0], init_reference, text["hidden"], want_controller=False)
            want = case(name)[3].forward_level(0, x["hs"][0], x["init_reference"], x["hidden"], want_controller=False)
        assert got[3] is None and want[3] is None
        for g, w, k in zip(got[:3], want[:3], C.OUTPUTS):
            close(g, w, "level 0 " + k)


def test_bitwise_repeatable():
    from uninext_amd import ext
    for name in ("detection", "ref2_plain"):
        args = kernel_args(name)
        assert equal(ext.pred_heads(**args), ext.pred_heads(**args))


def test_a_rows_result_does_not_depend_on_its_place_in_a_tile():
    """Rows 5..36 alone fill one tile from its row 0; in the whole batch they are rows 5..31 of one tile and 0..4 of the next."""
    from uninext_amd import ext
    both, alone = ext.pred_heads(**kernel_args("detection")), ext.pred_heads(**kernel_args("detection", slice(5, None)))
    assert alone[0].shape[1] == 32
    assert equal([t[:, 5:] for t in both], alone)


def test_one_text_for_every_image_has_batch_stride_0():
    from uninext_amd import ext
    args = kernel_args("detection")
    one = dict(args, tokens=args["tokens"][1:].contiguous(), token_bias=args["token_bias"][1:].contiguous())
    every = dict(args, tokens=one["tokens"].expand(C.B, -1, -1).contiguous(), token_bias=one["token_bias"].expand(C.B, -1).contiguous())
    shared, per_image = ext.pred_heads(**one), ext.pred_heads(**every)
    assert equal(shared, per_image)
    assert not torch.equal(shared[0][0], ext.pred_heads(**args)[0][0])       # image 0 did read image 1's text
    # a Still_Classifier is one token with stride 0
    still = kernel_args("ref2_plain")
    assert tuple(still["tokens"].shape) == (1, 1, C.D_MODEL) and still["scale"] is None and still["clamp"] == 0.0


def test_null_scale_means_1():
    from uninext_amd import ext
    args = kernel_args("detection")
    assert args["scale"] is not None
    close(ext.pred_heads(**dict(args, scale=None, clamp=0.0))[0], logits64("detection", scale=False), "scale NULL")
    close(ext.pred_heads(**dict(args, clamp=0.0))[0], logits64("detection"), "scale given")


def test_clamp_clamps():
    from uninext_amd import ext
    args = kernel_args("detection")
    clamp, gain = args["clamp"], 65536.0
    assert clamp == 50000.0
    free = logits64("detection", gain)
    assert bool((free > clamp).any()) and bool((free < -clamp).any()) and bool((free.abs() < clamp).any())   # of the fixture
    got = ext.pred_heads(**dict(args, tokens=args["tokens"] * gain))[0]
    assert bool((got == clamp).any()) and bool((got == -clamp).any()) and float(got.abs().max()) == clamp
    assert bool((got.abs() < clamp).any())
    close(got, logits64("detection", gain, clamp=clamp), "clamped")
    close(ext.pred_heads(**dict(args, tokens=args["tokens"] * gain, clamp=0.0))[0], free, "not clamped")


def test_optional_outputs_off_leave_the_others_unchanged():
    from uninext_amd import ext
    args = kernel_args("detection")
    full = ext.pred_heads(**args)
    assert all(t is not None for t in full)
    for off in ({"iou": None}, {"controller": None}, {"iou": None, "controller": None}):
        part = ext.pred_heads(**dict(args, **off))
        assert last() == KERNEL
        for k, (p, f) in enumerate(zip(part, full)):
            if (k == 2 and "iou" in off) or (k == 3 and "controller" in off):
                assert p is None
            else:
                assert torch.equal(p, f), (off, k)


def test_both_grids_give_the_same_bits():
    from uninext_amd import ext
    try:
        for name in ("detection", "ref2_plain"):
            args = kernel_args(name)
            ext.pred_heads_set_variant("split")
            split = ext.pred_heads(**args)
            assert last() == "pred_heads<split>"
            ext.pred_heads_set_variant("tile")
            tile = ext.pred_heads(**args)
            assert last() == "pred_heads<tile>"
            assert equal(split, tile)
            assert equal(split[:3], ext.pred_heads(**dict(args, controller=None))[:3])
    finally:
        ext.pred_heads_set_variant("auto")


@pytest.mark.parametrize("how", ["requires_grad", "non_contiguous"])
def test_other_inputs_take_the_composition_and_still_match(how):
    from uninext_amd import ext
    fx, cfg, heads, _, x = case("detection")
    try:
        ext.pred_heads_set_variant("tile")
        ext.pred_heads(**kernel_args("detection"))           # the marker
    finally:
        ext.pred_heads_set_variant("auto")
    assert last() == "pred_heads<tile>"
    hs, init_reference, inter_references, text = C.inputs(x, torch.float32, DEV)
    heads.fused = True
    if how == "requires_grad":
        out = heads.inference(hs.requires_grad_(True), init_reference, inter_references, text, cfg["task"], x["image_sizes"])
        assert out["pred_boxes"].requires_grad
    else:
        hs = hs.transpose(1, 2).contiguous().transpose(1, 2)
        assert not hs[LVL].is_contiguous()
        with torch.no_grad():
            out = heads.inference(hs, init_reference, inter_references, text, cfg["task"], x["image_sizes"])
    assert last() == "pred_heads<tile>"                    # the marker's: the kernel did not run
    for k, v in out.items():
        close(v, fx[k], "composition " + k)
    with torch.no_grad():                                   # and the same object does run the kernel when it may
        heads.inference(hs.detach().contiguous(), init_reference, inter_references, text, cfg["task"], x["image_sizes"])
    assert last() == KERNEL


def test_error_codes():
    from uninext_amd import _lib, ext
    lib = _lib.load()
    a = kernel_args("detection")
    Bn, Qn, d = a["hs"].shape
    T, P = a["tokens"].shape[1], a["controller"][4].shape[0]
    out = [torch.empty(Bn, Qn, T, device=DEV), torch.empty(Bn, Qn, 4, device=DEV), torch.empty(Bn, Qn, device=DEV),
           torch.empty(Bn, Qn, P, device=DEV)]
    p = lambda t: t.data_ptr()

    def call(hs=p(a["hs"]), T=T, P=P, ref_dim=4, d_model=d, box_w3=p(a["box_mlp"][4]), params=p(out[3])):
        box = [p(t) for t in a["box_mlp"]]
        box[4] = box_w3
        return lib.pred_heads_hip_f32(hs, p(a["tokens"]), T * d, p(a["token_bias"]), T, p(a["scale"]), a["clamp"], p(a["reference"]),
                                      ref_dim, *box, *[p(t) for t in a["iou"]], *[p(t) for t in a["controller"]], P, Bn, Qn, T,
                                      d_model, p(out[0]), p(out[1]), p(out[2]), params, None)

    ext.pred_heads(**a)
    torch.cuda.synchronize()
    before = last()
    for t in out:
        t.fill_(-7.0)
    assert call(hs=None) == -1 and "null pointer" in _lib.last_error()
    assert call(box_w3=None) == -1
    assert call(d_model=128) == -5 and "d_model must be 256" in _lib.last_error()
    assert call(T=0) == -2 and call(T=257) == -5 and "T must be at most 256" in _lib.last_error()
    assert call(P=0) == -2 and call(P=257) == -5 and "P must be at most 256" in _lib.last_error()
    for ref_dim in (0, 1, 3, 5):
        assert call(ref_dim=ref_dim) == -2 and "ref_dim must be 2 or 4" in _lib.last_error()
    assert lib.pred_heads_hip_set_variant(3) == -2
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in out)       # a refused call enqueues nothing
    assert last() == before
    assert call(P=257, params=None) == 0                   # without the output P is not read
    torch.cuda.synchronize()
    assert bool((out[0] != -7.0).all()) and bool((out[3] == -7.0).all())
    with pytest.raises(RuntimeError, match="d_model must be 256"):
        half = lambda t: t[..., :128].contiguous()
        box = a["box_mlp"]
        ext.pred_heads(half(a["hs"]), half(a["tokens"]), a["token_bias"], a["scale"], a["clamp"], a["reference"],
                       [box[0][:128, :128].contiguous(), box[1][:128].contiguous(), box[2][:128, :128].contiguous(),
                        box[3][:128].contiguous(), half(box[4]), box[5]])
    with pytest.raises(RuntimeError, match="reference must be float32"):
        ext.pred_heads(**dict(a, reference=a["reference"][..., :3].contiguous()))
    torch.cuda.synchronize()
