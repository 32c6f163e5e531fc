"""CPU: everything about the dynamic mask head's float64 parity sweep (tests/dynmask_cases.py) that needs no GPU.

The float64 restatement is pinned to the reference-minted gradient fixtures; every recorded seed satisfies the kink condition
and exercises every gradient group; the float32 PyTorch composition's error per group -- the yardstick of the GPU test's
bounds -- is measured against float64; and the per-group measure with its bound is shown to reject what the whole-tensor
measure of tests/test_dynmask_gpu.py lets through."""
import numpy as np
import pytest
import torch

import dynmask_cases as dc
from golden_util import dynmask_bwd_names, load_golden

CASES = dc.case_names()
# Restatement against the fixtures, both float64: measured 2.6e-16 of the tensor's maximum at worst (out of dynmask_bwd_norel_up2;
# every gradient but one agrees to the last bit); 100 x that, rounded up to a power of ten.
PIN_TOL = 1e-13


def test_groups_partition_a_parameter_row():
    for rel, n in ((True, 169), (False, 153)):
        g = dc.groups(rel)
        assert list(g) == ["w0_rel", "w0_feat", "w1", "w2", "b0", "b1", "b2"] and dc.num_params(rel) == n
        assert sorted(i for idx in g.values() for i in idx) == list(range(n))
        assert [len(g[k]) for k in g] == [16 if rel else 0, 64, 64, 8, 8, 8, 1]
    g = dc.groups(True)          # w0 is [out][in] with the two relative coordinates first (ddetrs_dn.py:53-66, :786-808)
    assert g["w0_rel"][:4] == [0, 1, 10, 11] and g["w0_feat"][:9] == [2, 3, 4, 5, 6, 7, 8, 9, 12]


def test_sweep_reaches_the_kernels_edges():
    """The shapes are the smallest that reach what their names say (include/dynmask_hip.h: dynmask_hip_backward_parts; 256-thread
    slices of dynmask_bwd_params, 128-pixel chunks of dynmask_bwd_feats)."""
    def parts(shape):
        H, W, num_insts, _, _ = dc.SHAPES[shape]
        return max(1, min(1024 // sum(num_insts), (H * W + 255) // 256))
    hw = lambda s: dc.SHAPES[s][0] * dc.SHAPES[s][1]
    assert [parts(s) for s in ("one_slice_tail", "two_slices", "three_slices_uneven", "many_instances")] == [1, 2, 3, 1]
    assert hw("three_slices_uneven") == 529 and -(-529 // 3) == 177 and 529 - 2 * 177 == 175
    assert (hw("one_slice_tail"), hw("feats_chunk_128"), hw("feats_chunk_129"), hw("two_slices")) == (126, 128, 129, 272)
    assert 1024 // sum(dc.SHAPES["many_instances"][2]) == 0
    assert len(CASES) == 27 and len(set(CASES)) == 27


@pytest.mark.parametrize("name", dynmask_bwd_names())
def test_restatement_reproduces_the_reference_fixtures_in_float64(name):
    g = load_golden(name)
    f, r, p = (torch.from_numpy(g[k]).double().requires_grad_(True) for k in ("mask_feats", "reference_points", "mask_head_params"))
    out, _ = dc.head(f, r, p, g["num_insts"].tolist(), dc.STRIDE, bool(g["rel_coord"]), dc.STRIDE // int(g["mask_out_stride"]))
    assert out.dtype == torch.float64 and out.shape == g["out"].shape
    gf, gr, gp = torch.autograd.grad((out * torch.from_numpy(g["upstream"]).double()).sum(), (f, r, p), allow_unused=True)
    gr = gr if gr is not None else torch.zeros_like(r)
    for got, key in ((out.detach(), "out"), (gf, "grad_mask_feats"), (gr, "grad_reference_points"), (gp, "grad_mask_head_params")):
        want = g[key]
        assert want.dtype == np.float64 and tuple(got.shape) == want.shape
        scale = float(np.abs(want).max())
        err = float(np.abs(got.numpy() - want).max())
        print("%s %s: max |err| %.2e of max %.2e" % (name, key, err, scale))
        assert err <= PIN_TOL * scale, key


def test_float32_inputs_reach_the_reference_exactly():
    c = dc.case("three_slices_uneven-rel-up2")
    for t in (c.feats, c.ref, c.params, c.upstream):
        assert t.dtype == torch.float32 and torch.equal(t.double().float(), t)
    assert bool((c.ref[..., 0] >= 0).all() and (c.ref[..., 0] <= c.W * dc.STRIDE).all() and (c.ref[..., 1] <= c.H * dc.STRIDE).all())
    far = dc.case("far_reference-rel-up2")
    assert far.ref.reshape(-1, 2).tolist() == [[0.0, 0.0], [112.0, 0.0], [112.0, 72.0]]


@pytest.mark.parametrize("name", CASES)
def test_kink_condition_and_group_scales(name):
    """Every pre-activation a of the float64 restatement has |a| >= 64 * 2^-24 * (|b| + sum |w_i x_i|), so no ReLU unit can
    switch under float32 rounding; and no group's reference gradient vanishes unless it is zero by structure."""
    c = dc.case(name)
    want, mags, margin = dc.reference(name)
    print("%s: min |a| / (|b| + sum |w x|) = %.3e = %.1f x the condition" % (name, margin, margin / dc.KINK))
    assert margin >= dc.KINK
    assert dc.unexercised(name) == []
    for e, key, idx in dc.entries(c.num_insts, c.rel):
        if dc.structurally_zero(e, c.num_insts, c.rel):
            assert float(want[key][idx].abs().max()) == 0.0, e
    # the magnitudes are the same backward with absolute values: they dominate the values they bound
    for key in want:
        assert bool((mags[key] >= want[key].abs() * (1 - 1e-12)).all()), key


def test_composition_errors_per_group():
    """The float32 PyTorch composition (mask_head._dynamic_convs_torch + _aligned_bilinear_torch, the fallback route) under autograd
    on the CPU against float64, per group: the yardsticks of tests/test_dynmask_parity_gpu.py.  Each lies inside the summand
    bound SUM_DEPTH u s on its own, so the composition is a sane yardstick."""
    lines = ["# dynamic mask head, float64 parity per gradient group (tests/dynmask_cases.py)",
             "# float32 PyTorch composition on the CPU against the float64 restatement; per case and group the entry with the",
             "# largest error / bound; bound = max(%g x composition error, %g x 2^-24 x s), s = sum |summand| / max |want|" % (dc.COMP_MARGIN, dc.SUM_DEPTH),
             "%-32s %-15s %-22s %10s %8s %10s" % ("case", "group", "entry", "comp err", "s", "bound")]
    for name in CASES:
        comp, bound, s = dc.composition_errors(name), dc.bounds(name), dc.summand_ratios(name)
        for e, err in comp.items():
            assert np.isfinite(err) and err <= dc.SUM_DEPTH * dc.U * s[e], (name, e, err, s[e])
            assert s[e] >= 1.0 or s[e] == 0.0, (name, e, s[e])
        for group, e, err, _, b, _ in dc.worst_by_group(name, comp, bound):
            lines.append("%-32s %-15s %-22s %10.2e %8.1f %10.2e" % (name, group, e, err, s[e], b))
    print("\n".join(lines))
    if dc.table_path():
        with open(dc.table_path(), "w") as f:
            f.write("\n".join(lines) + "\n")


def _old_measure_accepts(got, want):
    """tests/test_dynmask_gpu.py: the whole tensor against 2e-5 * max(1, max |want|)."""
    return float((got.double() - want).abs().max()) < 2e-5 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("group", ["w1", "w0_feat"])
@pytest.mark.parametrize("name", ["many_instances-rel-up1", "many_instances-norel-up1"])
def test_group_errors_reject_what_the_whole_tensor_measure_accepts(name, group):
    """One gradient entry of the composition, of the instance whose `group` is smallest, moved by 1e-3 of that group's own scale:
    the whole-tensor measure cannot see it, the per-group measure with its bound does.  (On the few-instance shapes w1's
    gradient is as large as the relative-coordinate columns' -- h0 grows with |rel| too -- so the shadow that hides a w1 block is
    the one cast by the other instances; a feature column of w0 sits in the shadow on most rel_coord shapes, see the next test.)"""
    _check_teeth(name, group)


@pytest.mark.parametrize("name", ["three_slices_uneven-rel-up2", "two_slices-rel-up4", "one_slice_tail-rel-up2"])
def test_a_wrong_feature_column_of_w0_hides_behind_the_coordinate_columns(name):
    _check_teeth(name, "w0_feat")


def _check_teeth(name, group):
    c = dc.case(name)
    want = dc.reference(name)[0]
    got = {k: v.clone() for k, v in dc.composition(c).items()}
    idx = dc.groups(c.rel)[group]
    scales = want["grad_params"][0][:, idx].abs().max(1).values
    inst = int(scales.argmin())
    col = idx[len(idx) // 2 + 3]                                # w0_feat: output channel 4, feature column 3
    got["grad_params"][0, inst, col] += 1e-3 * float(scales[inst])
    assert _old_measure_accepts(got["grad_params"], want["grad_params"])
    errs, bound = dc.group_errors(got, want, c.num_insts, c.rel), dc.bounds(name)
    entry = "params.%s[%d]" % (group, inst)
    assert errs[entry] > bound[entry] and errs[entry] > 0.9e-3
    bad = [e for e in errs if errs[e] > bound[e]]
    assert bad == [entry]                                       # and nothing else is accused
