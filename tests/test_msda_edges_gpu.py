"""Every fp32 MSDeformAttn kernel on samples placed exactly on cell edges and cut-offs (tests/msda_edges.py), MI355X.

grad_sampling_loc jumps where floor() of the pixel coordinate changes, so there the kernels must take the reference's cell:
the one of the coordinate rounded ONCE (fma), as oracle/msda_oracle.c does.  Random locations almost never land there; these
inputs put about half of all samples there.  Bounds as in tests/test_msda_parity_gpu.py's header, but grad_sampling_loc is
compared ELEMENTWISE (max, no quantile) with the float32 oracle, within 1e-4 * max(H_l, W_l); grad_value and grad_attn_weight
(continuous in the location) against the float64 oracle on the same float32 inputs; the forward within 1e-4.  A sample cut off
exactly at -1 / H must get grad_sampling_loc and grad_attn_weight exactly 0.  The worst error is printed per category and
kernel, so a failure names the kind of edge."""
import numpy as np
import pytest
import torch

import msda_edges as E
from golden_util import carried

pytestmark = pytest.mark.gpu

POW2 = ((32, 64), (16, 32), (8, 16), (4, 8))
R50_QUARTER = ((25, 42), (13, 21), (7, 11), (4, 6))
THIN = ((3, 400), (2, 200), (1, 100), (1, 50))                     # test_msda_parity_gpu.ODD_PYRAMIDS' thin one
PYRAMIDS = {"pow2": POW2, "r50q": R50_QUARTER, "thin": THIN}

ENC_FWD = ("auto", "msda_fwd_win", "msda_fwd_lg3", "msda_fwd_lanegroup", "msda_fwd_generic")
ENC_BWD = ("auto", "msda_bwd_win", "msda_bwd_tiled", "msda_bwd_regions", "msda_bwd_lanegroup", "msda_bwd_generic")
DEC_FWD = ("auto", "msda_fwd_lg3", "msda_fwd_lanegroup", "msda_fwd_generic")
DEC_BWD = ("auto", "msda_bwd_dec", "msda_bwd_dst", "msda_bwd_lanegroup", "msda_bwd_generic")
AUTO_FWD = ("msda_fwd_win", "msda_fwd_lg3", "msda_fwd_lanegroup")
AUTO_BWD = ("msda_bwd_win", "msda_bwd_tiled", "msda_bwd_regions", "msda_bwd_dec")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def api():
    import MultiScaleDeformableAttention as MSDA
    from uninext_amd import _lib
    _lib.load()
    return MSDA, _lib


_cache = {}


def _case(kind, name, lq=None):
    """Edge inputs and the oracle's answers (float32: grad_loc; float64: forward, grad_value, grad_attn), computed once."""
    key = (kind, name, lq)
    if key not in _cache:
        from oracle import msda_oracle
        levels = PYRAMIDS[name] if name in PYRAMIDS else name
        x = E.make_edges(kind, levels, batch=2, num_query=lq, seed=11 + (lq or 0))
        f64 = lambda k: x[k].double()
        args = (x["shapes"], x["lsi"])
        ref = dict(out=msda_oracle.forward(f64("value"), *args, f64("loc"), f64("attn")))
        ref["gv32"], ref["gl32"], ref["ga32"] = msda_oracle.backward(x["grad_out"], x["value"], *args, x["loc"], x["attn"])
        ref["gv64"], _, ref["ga64"] = msda_oracle.backward(f64("grad_out"), f64("value"), *args, f64("loc"), f64("attn"))
        _cache[key] = (x, ref)
    return _cache[key]


def _on(x, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in x.items()}


def _run(lib, which, variant, fn):
    lib.set_variant(which, variant)
    try:
        out = fn()
    finally:
        lib.set_variant(which, "auto")
    ran = lib.last_kernel(which)
    assert ran in ((AUTO_FWD if which == "forward" else AUTO_BWD) + ("msda_fwd_generic", "msda_bwd_generic")
                   if variant == "auto" else (variant,)), (variant, ran)
    return out, ran


def _check_forward(x, ref, out, tag):
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref["out"]).max())
    print("%-40s forward max |err| %.2e" % (tag, err))
    assert err < 1e-4, (tag, err)


def _check_backward(x, ref, gv, gl, ga, tag):
    gv, gl, ga = (t.cpu().numpy().astype(np.float64) for t in (gv, gl, ga))
    levels = x["levels"]
    bound = np.array([1e-4 * max(h, w) for h, w in levels]).reshape(1, 1, 1, len(levels), 1)
    ratio = np.abs(gl - ref["gl32"]).max(-1) / bound                # [N, Lq, M, L, P]: < 1 passes
    worst = {c: (float(ratio[m].max()) if m.any() else None) for c, m in x["masks"].items()}
    worst["all"] = float(ratio.max())
    e_gv = float(np.abs(gv - ref["gv64"]).max())
    e_ga = float(np.abs(ga - ref["ga64"]).max())
    o_gv, o_ga = float(np.abs(ref["gv32"] - ref["gv64"]).max()), float(np.abs(ref["ga32"] - ref["ga64"]).max())
    out = x["masks"]["cut_out"]
    print("%-40s grad_loc / bound: %s  grad_value %.2e  grad_attn %.2e" % (
        tag, " ".join("%s %s" % (c, "-" if v is None else "%.3f" % v) for c, v in worst.items()), e_gv, e_ga))
    assert worst["all"] < 1.0, (tag, worst)
    assert not gl[out].any() and not ga[out].any(), (tag, "cut-off samples with non-zero gradients",
                                                      int((gl[out] != 0).any(-1).sum()), int((ga[out] != 0).sum()))
    assert e_gv < max(1e-4, 2.0 * o_gv), (tag, e_gv, o_gv)
    assert e_ga < max(1e-4, 2.0 * o_ga), (tag, e_ga, o_ga)


def _bwd(MSDA, lib, xd, variant):
    return _run(lib, "backward", variant, lambda: MSDA.ms_deform_attn_backward(
        xd["value"], xd["shapes"], xd["lsi"], xd["loc"], xd["attn"], xd["grad_out"], 64))


def _fwd(MSDA, lib, xd, variant):
    return _run(lib, "forward", variant, lambda: MSDA.ms_deform_attn_forward(
        xd["value"], xd["shapes"], xd["lsi"], xd["loc"], xd["attn"], 64))


@pytest.mark.parametrize("name", sorted(PYRAMIDS))
def test_encoder_forward_on_edges(name, dev, api):
    MSDA, lib = api
    x, ref = _case("encoder", name)
    xd = _on(x, dev)
    for variant in carried("forward", *ENC_FWD):
        out, ran = _fwd(MSDA, lib, xd, variant)
        _check_forward(x, ref, out, "encoder %s %s (%s)" % (name, variant, ran))


@pytest.mark.parametrize("variant", ENC_BWD)
@pytest.mark.parametrize("name", sorted(PYRAMIDS))
def test_encoder_backward_on_edges(name, variant, dev, api):
    MSDA, lib = api
    assert variant in carried("backward", variant)
    x, ref = _case("encoder", name)
    (gv, gl, ga), ran = _bwd(MSDA, lib, _on(x, dev), variant)
    _check_backward(x, ref, gv, gl, ga, "encoder %s %s (%s)" % (name, variant, ran))


@pytest.mark.parametrize("lq", [300, 1100])
@pytest.mark.parametrize("name", sorted(PYRAMIDS))
def test_decoder_on_edges(name, lq, dev, api):
    MSDA, lib = api
    x, ref = _case("decoder", name, lq)
    xd = _on(x, dev)
    for variant in carried("forward", *DEC_FWD):
        if variant == "msda_fwd_lg3" and lq < 1024:
            continue                                                 # (msda_fwd_lg3 takes 1024 queries and more)
        out, ran = _fwd(MSDA, lib, xd, variant)
        _check_forward(x, ref, out, "decoder %s Lq %d %s (%s)" % (name, lq, variant, ran))
    for variant in carried("backward", *DEC_BWD):
        (gv, gl, ga), ran = _bwd(MSDA, lib, xd, variant)
        _check_backward(x, ref, gv, gl, ga, "decoder %s Lq %d %s (%s)" % (name, lq, variant, ran))


def test_full_size_r50_window_kernels_on_edges(dev, api):
    """One encoder call at the R50 inference shapes through the two kernels the default training path takes there."""
    from uninext_amd import workloads
    MSDA, lib = api
    x, ref = _case("encoder", workloads.R50_LEVELS_INFER)
    _cache.pop(("encoder", workloads.R50_LEVELS_INFER, None))       # (large: not kept)
    xd = _on(x, dev)
    out, _ = _fwd(MSDA, lib, xd, "msda_fwd_win")
    _check_forward(x, ref, out, "encoder r50 msda_fwd_win")
    (gv, gl, ga), _ = _bwd(MSDA, lib, xd, "msda_bwd_win")
    _check_backward(x, ref, gv, gl, ga, "encoder r50 msda_bwd_win")


@pytest.mark.parametrize("name", ["pow2", "r50q"])
def test_float64_generic_kernels_on_edges(name, dev, api):
    """The float64 kernels on the same points against the float64 oracle, exact as in test_msda_gpu's border test."""
    from oracle import msda_oracle
    MSDA, lib = api
    x = E.make_edges("decoder", PYRAMIDS[name], batch=2, num_query=300, seed=23)
    d = {k: (v.to(dev, torch.float64) if torch.is_tensor(v) and v.is_floating_point() else v.to(dev) if torch.is_tensor(v) else v)
         for k, v in x.items()}
    out = MSDA.ms_deform_attn_forward(d["value"], d["shapes"], d["lsi"], d["loc"], d["attn"], 64)
    assert lib.last_kernel("forward") == "msda_fwd_generic"
    gv, gl, ga = MSDA.ms_deform_attn_backward(d["value"], d["shapes"], d["lsi"], d["loc"], d["attn"], d["grad_out"], 64)
    assert lib.last_kernel("backward") == "msda_bwd_generic"
    f64 = lambda k: x[k].double()
    ro = msda_oracle.forward(f64("value"), x["shapes"], x["lsi"], f64("loc"), f64("attn"))
    rgv, rgl, rga = msda_oracle.backward(f64("grad_out"), f64("value"), x["shapes"], x["lsi"], f64("loc"), f64("attn"))
    n = lambda t: t.cpu().numpy()
    errs = [float(np.abs(n(a) - b).max()) for a, b in ((out, ro), (gv, rgv), (gl, rgl), (ga, rga))]
    print("float64 %s: forward %.1e grad_value %.1e grad_loc %.1e grad_attn %.1e" % ((name,) + tuple(errs)))
    assert errs[0] < 1e-12 and errs[1] < 1e-12 and errs[2] < 1e-11 and errs[3] < 1e-12, errs


def _fused_lattice_inputs(levels, seed):
    """Reference points on pixel centres, integer offsets: on a power-of-two pyramid ref + off / W is exact, so every sample
    sits on the lattice (or exactly on a cut-off) whatever the order of the prologue's operations."""
    from uninext_amd import workloads
    g = torch.Generator().manual_seed(seed)
    S = sum(h * w for h, w in levels)
    N, M, L, P, D = 2, 8, len(levels), 4, 32
    ref = workloads.encoder_reference_points(levels, "cpu")           # [S, 2] pixel centres of the queries' own level
    ref = ref.view(1, S, 1, 2).expand(N, S, L, 2).contiguous()
    off = torch.randint(-3, 4, (N, S, M, L, P, 2), generator=g).float()
    # a quarter of the samples half a pixel off along x: exact as well, between two lattice columns
    off[..., 0] += 0.5 * (torch.rand(N, S, M, L, P, generator=g) < 0.25).float()
    logits = torch.randn(N, S, M * L * P, generator=g)
    value = torch.randn(N, S, M, D, generator=g)
    shapes, lsi = workloads.level_tensors(levels, "cpu")
    wh = torch.tensor([[w, h] for h, w in levels], dtype=torch.float32).view(1, 1, 1, L, 1, 2)
    loc = ref.view(N, S, 1, L, 1, 2) + off / wh
    assert torch.equal((loc.double() * wh.double() - 0.5), (loc * wh - 0.5).double())   # exact: the lattice for every rounding
    return dict(value=value, shapes=shapes, lsi=lsi, ref=ref, off=off.view(N, S, M * L * P * 2), logits=logits, loc=loc)


def test_fused_forward_and_function_on_the_lattice(dev, api):
    from oracle import msda_oracle
    from golden_util import grad_loc_err
    from uninext_amd import ext
    from uninext_amd.functions import MSDeformAttnFusedFunction
    MSDA, lib = api
    levels = POW2
    x = _fused_lattice_inputs(levels, 29)
    N, S, M, D = x["value"].shape
    L, P = len(levels), 4
    attn64 = torch.softmax(x["logits"].double().view(N, S, M, L * P), -1).view(N, S, M, L, P)
    loc = x["loc"]
    want = msda_oracle.forward(x["value"].double(), x["shapes"], x["lsi"], loc.double(), attn64)
    d = {k: v.to(dev) for k, v in x.items()}
    kernels = {"auto": ("msda_fwd_win_fused", "msda_fwd_lg3_fused"), "msda_fwd_win": ("msda_fwd_win_fused",),
               "msda_fwd_lg3": ("msda_fwd_lg3_fused",), "small": ("msda_fwd_fused",)}
    for head_major in (False, True):
        v = d["value"].permute(0, 2, 1, 3).contiguous() if head_major else d["value"]
        for variant in ("auto", "msda_fwd_win", "msda_fwd_lg3") + (() if head_major else ("small",)):
            q = 512 if variant == "small" else S                       # fewer than 1024 queries: the small-call fused kernel
            lib.set_variant("forward", "auto" if variant == "small" else variant)
            try:
                out = ext.ms_deform_attn_forward_fused(v, d["shapes"], d["lsi"], d["ref"][:, :q].contiguous(), d["off"][:, :q].contiguous(),
                                                       d["logits"][:, :q].contiguous(), P, value_head_major=head_major)
            finally:
                lib.set_variant("forward", "auto")
            ran = lib.last_kernel("forward")
            err = float(np.abs(out.cpu().numpy().astype(np.float64) - want[:, :q]).max())
            print("fused forward head_major=%d %s (%s): %.2e" % (head_major, variant, ran, err))
            assert ran in kernels[variant], (variant, ran)
            assert err < 1e-4, (head_major, variant, err)

    # the differentiable function: its backward recomputes the locations and runs the operator's backward kernels
    go = torch.randn(N, S, M * D, generator=torch.Generator().manual_seed(30))
    value = d["value"].clone().requires_grad_(True)
    off = d["off"].clone().requires_grad_(True)
    logits = d["logits"].clone().requires_grad_(True)
    out = MSDeformAttnFusedFunction.apply(value, d["shapes"], d["lsi"], d["ref"], off, logits, P)
    out.backward(go.to(dev))
    gv32, gl32, ga32 = msda_oracle.backward(go, x["value"], x["shapes"], x["lsi"], loc, attn64.float())
    gv64, _, ga64 = msda_oracle.backward(go.double(), x["value"].double(), x["shapes"], x["lsi"], loc.double(), attn64)
    wh = np.array([[w, h] for h, w in levels], dtype=np.float64).reshape(1, 1, 1, L, 1, 2)
    gl = off.grad.cpu().numpy().astype(np.float64).reshape(N, S, M, L, P, 2) * wh     # d/d(loc) = d/d(off) * (W, H): exact
    e_gl = grad_loc_err(gl, gl32, np.array(levels))
    a64 = attn64.numpy().reshape(N, S, M, L * P)

    def softmax_bwd(ga):
        ga = np.asarray(ga, dtype=np.float64).reshape(N, S, M, L * P)
        return (a64 * (ga - (a64 * ga).sum(-1, keepdims=True))).reshape(N, S, M * L * P)
    t_lg, o_lg = softmax_bwd(ga64), softmax_bwd(ga32)
    e_lg = float(np.abs(logits.grad.cpu().numpy() - t_lg).max())
    e_gv = float(np.abs(value.grad.cpu().numpy() - gv64).max())
    o_gv = float(np.abs(gv32 - gv64).max())
    print("fused function (%s): grad_loc / bound %.3f  grad_value %.2e  grad_logits %.2e" % (
        lib.last_kernel("backward"), e_gl, e_gv, e_lg))
    assert e_gl < 1.0, e_gl
    assert e_gv < max(1e-4, 2.0 * o_gv), (e_gv, o_gv)
    assert e_lg < max(1e-4, 2.0 * float(np.abs(o_lg - t_lg).max())), e_lg
