"""Two-stage query selection on the GPU: the HIP route (qsel_scores_hip_f32 + torch.topk + qsel_boxes_hip_f32) against the
reference's float64 fixtures, and the kernels' own contracts (repeatability, row-position independence, strides, NULL scale,
clamp, optional output, error codes)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import query_selection_cases as C   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def case(name):
    """(fixture, cfg, fp32 GPU modules, float64 CPU modules, inputs), built once per fixture and left unchanged."""
    fx = C.load(name)
    cfg, states, x = C.make_case(name, int(fx["seed"]))
    assert C.digest(states) == float(fx["digest"])
    return fx, cfg, C.build(cfg, states, torch.float32, DEV), C.build(cfg, states, torch.float64), x


def geometry(mods, x, image=None):
    """The leading arguments of ext.qsel_scores / qsel_boxes; image: one image alone (B = 1)."""
    from uninext_amd.modules.query_selection import valid_sizes
    pick = (lambda t: t) if image is None else (lambda t: t[image:image + 1].contiguous())
    memory, mask = pick(x["memory"].float().to(DEV)), pick(x["mask"].to(DEV))
    shapes = x["shapes"].to(DEV)
    n = mods["enc_output_norm"]
    return (memory, mask, shapes, valid_sizes(mask, shapes), mods["enc_output"].weight.detach(), mods["enc_output"].bias.detach(),
            n.weight.detach(), n.bias.detach(), n.eps)


def class_terms(mods, x, image=None):
    from uninext_amd.modules import TwoStageQuerySelection as Sel
    pool = x["lang_feat_pool"].float().to(DEV)
    with torch.no_grad():
        return Sel.class_terms(mods["class_embed"], pool if image is None else pool[image:image + 1].contiguous())


def mlp_terms(mods):
    return [t.detach() for l in mods["bbox_embed"].layers for t in (l.weight, l.bias)]


def close(got, want, what):
    """Identical infinities; finite entries within TOL of the reference's largest finite magnitude."""
    got, want = got.detach().cpu().double().numpy(), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), what
    assert not np.isnan(got).any(), what
    err, bound = float(np.abs(got[~inf] - want[~inf]).max()), C.TOL * float(np.abs(want[~inf]).max())
    print("%-28s max abs error %.3e, bound %.3e" % (what, err, bound))
    assert err <= bound, (what, err, bound)


def last():
    from uninext_amd import _lib
    return _lib.last_kernel("qsel")


@pytest.mark.parametrize("name", list(C.FIXTURES))
def test_fused_route_matches_the_reference(name):
    from uninext_amd import ext
    fx, cfg, mods, _, x = case(name)
    for all_coords in (False, True):
        points, coords, idx, logits, every = C.run(cfg, mods, x, DEV, torch.float32, fused=True, all_coords=all_coords)
        assert last() == "qsel_boxes"
        assert idx.dtype == torch.long and np.array_equal(idx.cpu().numpy(), fx["topk_proposals"])      # exactly, in order
        close(logits, fx["enc_outputs_class"], "logits")
        close(coords, fx["topk_coords_unact"], "topk_coords_unact")
        close(points, fx["reference_points"], "reference_points")
        assert bool((points[torch.isinf(coords)] == 1.0).all())
        if all_coords:
            close(every, fx["enc_outputs_coord_unact"], "enc_outputs_coord_unact")
        else:
            assert every is None
    # the box kernel over every row, called directly: the reference's whole enc_outputs_coord_unact and its sigmoid
    B, S = x["mask"].shape
    rows = torch.arange(S, device=DEV).unsqueeze(0).expand(B, S).contiguous()
    coords, points = ext.qsel_boxes(*geometry(mods, x), rows, *mlp_terms(mods))
    close(coords, fx["enc_outputs_coord_unact"], "qsel_boxes over arange(S)")
    close(points, torch.from_numpy(fx["enc_outputs_coord_unact"]).sigmoid(), "its sigmoid")
    dead = np.isinf(fx["output_proposals"]).any(-1)
    assert np.array_equal(torch.isinf(coords).any(-1).cpu().numpy(), dead)                  # validity, row by row


@pytest.mark.parametrize("name", ["vl_align", "one_level"])
def test_optional_output_memory(name):
    from uninext_amd import ext
    fx, cfg, mods, _, x = case(name)
    vec, bias, scale, clamp = class_terms(mods, x)
    plain = ext.qsel_scores(*geometry(mods, x), vec, bias, scale, clamp)
    assert last() == "qsel_scores"
    logits, memory = ext.qsel_scores(*geometry(mods, x), vec, bias, scale, clamp, want_memory=True)
    assert last() == "qsel_scores<memory>"
    assert torch.equal(plain, logits)
    close(memory[:, torch.as_tensor(fx["memory_rows"], device=DEV)], fx["output_memory"], "output_memory")


def test_bitwise_repeatable():
    from uninext_amd import ext
    fx, cfg, mods, _, x = case("vl_align")
    vec, bias, scale, clamp = class_terms(mods, x)
    idx = torch.from_numpy(fx["topk_proposals"]).to(DEV)
    first = ext.qsel_scores(*geometry(mods, x), vec, bias, scale, clamp, want_memory=True) \
        + ext.qsel_boxes(*geometry(mods, x), idx, *mlp_terms(mods))
    again = ext.qsel_scores(*geometry(mods, x), vec, bias, scale, clamp, want_memory=True) \
        + ext.qsel_boxes(*geometry(mods, x), idx, *mlp_terms(mods))
    for a, b in zip(first, again):
        assert torch.equal(a, b)


def test_a_rows_result_does_not_depend_on_its_place_in_a_tile():
    """Image 1 alone starts its rows at tile row 0; in the batch of two they start at row 233 % 32 = 9 of a shared tile."""
    from uninext_amd import ext
    fx, cfg, mods, _, x = case("vl_align")
    vec, bias, scale, clamp = class_terms(mods, x)
    both = ext.qsel_scores(*geometry(mods, x), vec, bias, scale, clamp, want_memory=True)
    v1, b1, _, _ = class_terms(mods, x, image=1)
    alone = ext.qsel_scores(*geometry(mods, x, image=1), v1, b1, scale, clamp, want_memory=True)
    assert torch.equal(both[0][1:], alone[0]) and torch.equal(both[1][1:], alone[1])
    idx = torch.from_numpy(fx["topk_proposals"]).to(DEV)
    boxes = ext.qsel_boxes(*geometry(mods, x), idx, *mlp_terms(mods))
    boxes1 = ext.qsel_boxes(*geometry(mods, x, image=1), idx[1:].contiguous(), *mlp_terms(mods))
    assert torch.equal(boxes[0][1:], boxes1[0]) and torch.equal(boxes[1][1:], boxes1[1])


def test_one_head_for_every_image_has_batch_stride_0():
    from uninext_amd import ext
    fx, cfg, mods, _, x = case("still")
    vec, bias, scale, clamp = class_terms(mods, x)
    assert tuple(vec.shape) == (1, C.D_MODEL) and tuple(bias.shape) == (1,) and scale is None and clamp == 0.0
    shared = ext.qsel_scores(*geometry(mods, x), vec, bias)
    close(shared.unsqueeze(-1), fx["enc_outputs_class"], "still logits")
    per_image = ext.qsel_scores(*geometry(mods, x), vec.expand(2, -1).contiguous(), bias.expand(2).contiguous())
    assert torch.equal(shared, per_image)


def recorded_rows_logits(fx, mods64, x, gain=1.0, scale=True, clamp=0.0):
    """Float64 logits of the rows whose output_memory the fixture records, from the reference's output_memory."""
    with torch.no_grad():
        tokens, bias = mods64["class_embed"].token_terms(x["lang_feat_pool"].unsqueeze(1))
        s = mods64["class_embed"].log_scale.exp() if scale else 1.0
    want = (torch.from_numpy(fx["output_memory"]) * (tokens * gain)).sum(-1) / s + bias
    return want.clamp(-clamp, clamp) if clamp else want


def test_null_scale_means_1():
    from uninext_amd import ext
    fx, cfg, mods, mods64, x = case("vl_align")
    vec, bias, _, _ = class_terms(mods, x)
    got = ext.qsel_scores(*geometry(mods, x), vec, bias, None, 0.0)
    close(got[:, torch.as_tensor(fx["memory_rows"], device=DEV)], recorded_rows_logits(fx, mods64, x, scale=False), "scale NULL")


def test_clamp_clamps():
    from uninext_amd import ext
    fx, cfg, mods, mods64, x = case("vl_align")
    vec, bias, scale, clamp = class_terms(mods, x)
    assert clamp == 50000.0
    gain = 65536.0
    free = recorded_rows_logits(fx, mods64, x, gain)
    assert bool((free.abs() > clamp).any()) and bool((free.abs() < clamp).any())      # a property of the fixture
    rows = torch.as_tensor(fx["memory_rows"], device=DEV)
    got = ext.qsel_scores(*geometry(mods, x), vec * gain, bias, scale, clamp)
    assert float(got.abs().max()) == clamp
    close(got[:, rows], recorded_rows_logits(fx, mods64, x, gain, clamp=clamp), "clamped")
    close(ext.qsel_scores(*geometry(mods, x), vec * gain, bias, scale, 0.0)[:, rows], free, "not clamped")


@pytest.mark.parametrize("how", ["requires_grad", "non_contiguous"])
def test_other_inputs_take_the_composition_and_still_match(how):
    from uninext_amd import ext
    from uninext_amd.modules import TwoStageQuerySelection
    fx, cfg, mods, _, x = case("vl_align")
    vec, bias, scale, clamp = class_terms(mods, x)
    ext.qsel_scores(*geometry(mods, x), vec, bias, scale, clamp, want_memory=True)      # the marker
    assert last() == "qsel_scores<memory>"
    memory = x["memory"].float().to(DEV)
    sel = TwoStageQuerySelection()
    sel.fused = True
    args = (x["mask"].to(DEV), x["shapes"].to(DEV), mods["enc_output"], mods["enc_output_norm"], mods["class_embed"],
            mods["bbox_embed"], x["lang_feat_pool"].float().to(DEV), cfg["topk"])
    if how == "requires_grad":
        out = sel(memory.requires_grad_(True), *args)
        assert out[0].requires_grad
    else:
        memory = memory.transpose(0, 1).contiguous().transpose(0, 1)
        assert not memory.is_contiguous()
        with torch.no_grad():
            out = sel(memory, *args)
    assert last() == "qsel_scores<memory>"                 # the marker's: no kernel of this file's ran
    assert np.array_equal(out[2].cpu().numpy(), fx["topk_proposals"])
    close(out[3], fx["enc_outputs_class"], "composition logits")
    close(out[1], fx["topk_coords_unact"], "composition coords")
    close(out[0], fx["reference_points"], "composition points")
    with torch.no_grad():                                   # and the same object does run the kernels when it may
        sel(x["memory"].float().to(DEV), *args)
    assert last() == "qsel_boxes"


def test_error_codes():
    from uninext_amd import _lib, ext
    fx, cfg, mods, _, x = case("one_level")
    lib = _lib.load()
    memory, mask, shapes, valid_wh, w, b, g, beta, eps = geometry(mods, x)
    vec, bias, scale, clamp = class_terms(mods, x)
    B, S, d = memory.shape
    logits = torch.empty(B, S, device=DEV)
    p = lambda t: t.data_ptr()
    scores = lambda mem, dm: lib.qsel_scores_hip_f32(mem, p(mask), p(shapes), 1, p(valid_wh), p(w), p(b), p(g), p(beta), eps, p(vec), d,
                                                     p(bias), 1, None, 0.0, B, S, dm, p(logits), None, None)
    before = last()
    assert scores(None, d) == -1 and "null pointer" in _lib.last_error()
    assert scores(p(memory), 128) == -5 and "d_model must be 256" in _lib.last_error()
    idx = torch.zeros(B, 2, dtype=torch.long, device=DEV)
    m = [p(t) for t in mlp_terms(mods)]
    out = torch.empty(B, 2, 4, device=DEV)
    boxes = lambda index, dm: lib.qsel_boxes_hip_f32(p(memory), p(mask), p(shapes), 1, p(valid_wh), p(w), p(b), p(g), p(beta), eps,
                                                     index, 2, *m, B, S, dm, p(out), p(out), None)
    assert boxes(None, d) == -1 and boxes(p(idx), 512) == -5
    assert last() == before                                # a refused call enqueues nothing
    with pytest.raises(RuntimeError, match="d_model must be 256"):
        ext.qsel_scores(memory[..., :128].contiguous(), mask, shapes, valid_wh, w[:128, :128].contiguous(), b[:128].contiguous(),
                        g[:128].contiguous(), beta[:128].contiguous(), eps, vec[:, :128].contiguous(), bias)
    torch.cuda.synchronize()
