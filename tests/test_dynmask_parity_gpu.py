"""GPU: the HIP dynamic mask head (include/dynmask_hip.h: forward, backward, aligned_bilinear and its backward) against the
float64 restatement of tests/dynmask_cases.py, per gradient GROUP, on the smallest shapes that reach the kernels' own edges.

Every entry (the forward output per instance, seven parameter groups per instance, grad_xy per instance, grad_feats per image) is
measured relative to its OWN largest reference value and held to a bound computed at run time:
max(8 x the float32 PyTorch composition's error of the same entry on the same case, 16 x 2^-24 x s), s the float64 restatement's
ratio of summed absolute summands to the entry's maximum.  The inputs satisfy the kink condition (asserted first), so nothing is
left out of a comparison.  The tables are printed; with DYNMASK_PARITY_TABLE set they are appended to that file."""
import ctypes

import pytest
import torch

import dynmask_cases as dc
from uninext_amd import _lib, ext, mask_head

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = dc.case_names()
LARGEST = ("three_slices_uneven-rel-up2", "three_slices_uneven-norel-up2")     # 529 pixels x 5 instances, a leading empty image


def _graph(fn, seen=None):
    """Names of the autograd nodes behind a tensor."""
    seen = set() if seen is None else seen
    if fn is not None and fn not in seen:
        seen.add(fn)
        for nxt, _ in fn.next_functions:
            _graph(nxt, seen)
    return {type(f).__name__ for f in seen}


def _autograd_route(c, grad_out=None, loss=None):
    """mask_head.dynamic_mask_with_coords under autograd.  A factor of 3 is no ratio of two strides at stride 8, so those cases call
    the two public steps dynamic_mask_with_coords itself consists of."""
    f, r, p = (t.to(DEV).requires_grad_(True) for t in (c.feats, c.ref, c.params))
    if dc.STRIDE % c.factor == 0:
        out = mask_head.dynamic_mask_with_coords(f, r, p, c.num_insts, dc.STRIDE, rel_coord=c.rel, mask_out_stride=dc.STRIDE // c.factor)
    else:
        logits = mask_head.aligned_bilinear(mask_head.dynamic_mask_logits(f, r, p, c.num_insts, dc.STRIDE, c.rel), c.factor)
        out = logits.reshape(1, -1, logits.shape[-2], logits.shape[-1])
    kernel = _lib.load().dynmask_hip_last_kernel().decode()
    nodes = _graph(out.grad_fn)
    if loss is not None:
        gf, gr, gp = torch.autograd.grad(loss(out), (f, r, p), allow_unused=True)
    elif grad_out is not None:
        gf, gr, gp = torch.autograd.grad(out, (f, r, p), grad_outputs=grad_out, allow_unused=True)
    else:
        gf, gr, gp = torch.autograd.grad((out * c.upstream.to(DEV)).sum(), (f, r, p), allow_unused=True)
    got = dict(out=out.detach(), grad_feats=gf, grad_xy=gr if gr is not None else torch.zeros_like(r), grad_params=gp)
    return got, kernel, nodes


def _direct_route(c, need_feats=True, need_params=True, need_xy=True, backward=True):
    """ext.dynmask_forward, ext.aligned_bilinear_forward and the two backward entry points called directly: a missing kernel raises."""
    n_all = sum(c.num_insts)
    f, xy, p = c.feats.to(DEV), c.ref.reshape(-1, 2).to(DEV), c.params.reshape(n_all, -1).to(DEV)
    logits = ext.dynmask_forward(f, xy, p, c.num_insts, dc.STRIDE, c.rel)
    kernel = _lib.load().dynmask_hip_last_kernel().decode()
    out = ext.aligned_bilinear_forward(logits, c.factor) if c.factor > 1 else logits
    got = dict(out=out.reshape(1, n_all, c.factor * c.H, c.factor * c.W))
    if backward:
        up = c.upstream.to(DEV).reshape(n_all, c.factor * c.H, c.factor * c.W)
        g_logits = ext.aligned_bilinear_backward(up, c.factor) if c.factor > 1 else up
        assert g_logits.shape == (n_all, c.H, c.W)
        gf, gp, gxy = ext.dynmask_backward(f, xy, p, c.num_insts, dc.STRIDE, c.rel, g_logits, need_xy=need_xy, need_feats=need_feats,
                                           need_params=need_params)
        got.update(grad_feats=gf, grad_params=None if gp is None else gp.reshape(1, n_all, -1),
                   grad_xy=None if gxy is None else gxy.reshape(1, n_all, 2))
    return got, kernel


def _report(name, route, errs, bound):
    rows = dc.worst_by_group(name, errs, bound)
    lines = ["%-32s %-8s %-15s %-22s %10.2e %10.2e %10.2e %7.3f" % ((name, route) + r) for r in rows]
    print("%-32s %-8s %-15s %-22s %10s %10s %10s %7s" % ("case", "route", "group", "entry", "kernel err", "comp err", "bound", "ratio"))
    print("\n".join(lines))
    if dc.table_path():
        with open(dc.table_path(), "a") as f:
            f.write("\n".join(lines) + "\n")


def _assert_within_bounds(name, route, got, report=True):
    c = dc.case(name)
    want, _, margin = dc.reference(name)
    assert margin >= dc.KINK                                       # the kink condition, before any comparison
    for key in want:
        assert got[key].shape == want[key].shape and got[key].dtype == torch.float32, key
    errs, bound = dc.group_errors(got, want, c.num_insts, c.rel), dc.bounds(name)
    if report:
        _report(name, route, errs, bound)
    bad = {e: (errs[e], bound[e]) for e in errs if not errs[e] <= bound[e]}
    assert not bad, bad


@pytest.mark.parametrize("name", CASES)
def test_hip_route_against_float64_per_group(name):
    c = dc.case(name)
    got, kernel, nodes = _autograd_route(c)
    # kernel identity: the HIP Functions recorded the graph and the HIP forward kernel ran -- not the PyTorch composition
    assert kernel.startswith("dynmask_fwd_"), kernel
    assert "DynMaskFunctionBackward" in nodes and ("AlignedBilinearFunctionBackward" in nodes) == (c.factor > 1), nodes
    assert not {"BmmBackward0", "CatBackward0", "UpsampleBilinear2DBackward0"} & nodes, nodes
    _assert_within_bounds(name, "autograd", got)
    direct, kernel = _direct_route(c)
    assert kernel.startswith("dynmask_fwd_"), kernel
    _assert_within_bounds(name, "direct", direct, report=False)    # (bitwise the autograd route's, next lines: one table row serves both)
    for key in got:                                                # one set of kernels behind both routes
        assert torch.equal(got[key], direct[key]), key


@pytest.mark.parametrize("name", LARGEST)
def test_need_subsets_equal_the_full_backward_bitwise(name):
    c = dc.case(name)
    full, _ = _direct_route(c)
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (True, False, True)):
        got, _ = _direct_route(c, need_feats=need[0], need_params=need[1], need_xy=need[2])
        for key, wanted in zip(("grad_feats", "grad_params", "grad_xy"), need):
            assert (got[key] is not None) == wanted, (need, key)
            if wanted:
                assert torch.equal(got[key], full[key]), (need, key)


@pytest.mark.parametrize("name", LARGEST)
def test_c_abi_writes_every_output_element(name):
    """dynmask_hip_backward_f32 through ctypes with outputs and a workspace of exactly dynmask_hip_backward_workspace_bytes, all
    pre-filled with NaN: every output element is written (the image without instances by the memset path), nothing of the
    workspace's padding reaches a result, and the results are those of the ext route."""
    c = dc.case(name)
    lib = _lib.load()
    n_all, N, nan = sum(c.num_insts), len(c.num_insts), float("nan")
    f, xy, p = c.feats.to(DEV), c.ref.reshape(-1, 2).to(DEV), c.params.reshape(n_all, -1).to(DEV)
    up = c.upstream.to(DEV).reshape(n_all, c.factor * c.H, c.factor * c.W)
    g_logits = torch.full((n_all, c.H, c.W), nan, device=DEV)
    p_ = lambda t: t.data_ptr()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.aligned_bilinear_hip_backward_f32(p_(up), n_all, c.H, c.W, c.factor, p_(g_logits), stream) == 0
    parts = lib.dynmask_hip_backward_parts(n_all, c.H, c.W)
    ws_bytes = int(lib.dynmask_hip_backward_workspace_bytes(n_all, c.H, c.W))
    assert parts == 3 and ws_bytes == n_all * parts * 176 * 4
    ws = torch.full((ws_bytes // 4,), nan, device=DEV)
    gf, gp, gxy = torch.full_like(f, nan), torch.full_like(p, nan), torch.full_like(xy, nan)
    counts = (ctypes.c_int * N)(*c.num_insts)
    rc = lib.dynmask_hip_backward_f32(p_(f), p_(xy), p_(p), counts, N, 8, c.H, c.W, dc.STRIDE, int(c.rel), p_(g_logits), p_(gf), p_(gp),
                                      p_(gxy), p_(ws), ws_bytes, stream)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    for t in (g_logits, gf, gp, gxy):
        assert bool(torch.isfinite(t).all())
    direct, _ = _direct_route(c)
    assert torch.equal(gf, direct["grad_feats"]) and torch.equal(gp, direct["grad_params"][0]) and torch.equal(gxy, direct["grad_xy"][0])
    # a workspace one byte short is refused before anything is enqueued
    assert lib.dynmask_hip_backward_f32(p_(f), p_(xy), p_(p), counts, N, 8, c.H, c.W, dc.STRIDE, int(c.rel), p_(g_logits), p_(gf), p_(gp),
                                        p_(gxy), p_(ws), ws_bytes - 1, stream) == -2


@pytest.mark.parametrize("name", LARGEST)
def test_repeatable_and_independent_of_the_upstream_layout(name):
    c = dc.case(name)
    a, _, _ = _autograd_route(c)
    b, _, _ = _autograd_route(c)
    for key in a:
        assert torch.equal(a[key], b[key]), key
    # a transposed view of the same upstream values
    up = c.upstream.to(DEV)
    up_t = up.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not up_t.is_contiguous() and torch.equal(up_t, up)
    plain, _, _ = _autograd_route(c, grad_out=up)
    viewed, _, _ = _autograd_route(c, grad_out=up_t)
    # the expanded gradient of .sum() against a contiguous tensor of ones
    summed, _, _ = _autograd_route(c, loss=lambda out: out.sum())
    ones, _, _ = _autograd_route(c, grad_out=torch.ones_like(up))
    for key in ("grad_feats", "grad_xy", "grad_params"):
        assert torch.equal(plain[key], a[key]) and torch.equal(viewed[key], plain[key]), key
        assert torch.equal(summed[key], ones[key]), key


@pytest.mark.parametrize("name", LARGEST)
def test_forward_variants_within_the_per_instance_bound(name):
    """The packed-FMA kernel and the two MFMA forms (dynmask_hip_set_variant 1, 2, 3): bitwise equal to each other and each within
    the forward's per-instance bound against float64."""
    c = dc.case(name)
    lib = _lib.load()
    want = dc.reference(name)[0]["out"]
    bound = dc.bounds(name)
    outs = []
    try:
        for variant, kernel_name in ((1, "dynmask_fwd_pkfma"), (2, "dynmask_fwd_mfma_q2"), (3, "dynmask_fwd_mfma_q4")):
            assert lib.dynmask_hip_set_variant(variant) == 0
            got, kernel = _direct_route(c, backward=False)
            assert kernel == kernel_name
            for i in range(sum(c.num_insts)):
                g, w = got["out"][0, i].cpu().double(), want[0, i]
                err = float((g - w).abs().max() / w.abs().max())
                print("%s variant %d out[%d]: err %.2e bound %.2e" % (name, variant, i, err, bound["out[%d]" % i]))
                assert err <= bound["out[%d]" % i], (variant, i)
            outs.append(got["out"])
    finally:
        lib.dynmask_hip_set_variant(0)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
