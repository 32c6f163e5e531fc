"""GPU: qsel_scores_hip_f32 and qsel_boxes_hip_f32 (include/dynmask_hip.h) through the C ABI against the float64 restatement of
tests/query_selection_ref.py, on seeded dyadic inputs at the shapes where the 32-row tile, the validity rule and the LayerNorm
statistics can go wrong.

Every output is handed over filled with NaN and followed by 64 sentinel floats: afterwards no NaN is left in it and the tail is
untouched.  Every entry (one logit per row, one output_memory row against its own largest value, one coordinate and one point per
row and component) is held to max(8 x the fp32 PyTorch composition's error of the same entry on the same case,
16 x 2^-24 x s), s the restatement's ratio of summed absolute summands to the entry's magnitude, computed at run time; the
project's bound (TOL of the tensor's largest value) is asserted on top.  The composition is the module's
gen_encoder_output_proposals with plain torch ops behind it, or _select_composition itself on the validity grid; it never runs
the kernels.  The tables are printed; with QSEL_PARITY_TABLE set they are appended to that file.

Largest kernel error / bound seen on an MI355X, per output over every case of this file (the entry's kernel error, the
composition's error and the bound are relative to the entry's own magnitude):
    logits             0.126   pyramid5/mean64            2.02e-05   2.00e-05   1.60e-04
    output_memory      0.078   pyramid5/down12            2.22e-07   1.33e-07   2.84e-06
    coords_unact       0.056   pyramid5/mean64 every row  3.63e-05   1.12e-05   6.53e-04
    reference_points   0.054   pyramid5/mean64 every row  6.18e-06   1.86e-06   1.15e-04
A one-pass fp32 variance on the mean64 rows is 2.8 (one tile) and 5.7 (pyramid) times over the output_memory bound.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_measure as PM         # noqa: E402
import query_selection_cases as C   # noqa: E402
import query_selection_ref as R     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = C.D_MODEL
EPS = 1e-5
TAIL = 64
SCALE = float(np.float32(np.exp(0.5)))          # a fp32 number: the kernel divides by exactly what the restatement divides by
SIX_LEVELS = [(3, 50), (2, 25), (2, 13), (1, 7), (1, 4), (1, 2)]


def _pyramid5():
    return C.padding_mask(C.PYRAMID, True)[[0, 1, 0, 1, 1]]


def _image1_padded():
    mask = C.padding_mask(C.PYRAMID, False)
    mask[1] = True
    return mask


def _every_other(B):
    return (torch.arange(B) % 2 == 1).view(B, 1)


# name -> (B, levels, mask or None, seed)
SWEEP = {
    "one_row": (1, [(1, 1)], None, 301),
    "tile_less_1": (1, [(1, 31)], None, 302),
    "one_tile": (1, [(4, 8)], None, 303),
    "tile_plus_1": (3, [(1, 11)], None, 304),
    "32_images_a_tile": (40, [(1, 1)], lambda: _every_other(40), 305),
    "pyramid5": (5, C.PYRAMID, _pyramid5, 306),
    "six_levels": (2, SIX_LEVELS, None, 307),
    "125_workgroups": (2, [(40, 50)], None, 308),
    "image1_padded": (2, C.PYRAMID, _image1_padded, 309),
}
GRID = "validity_grid"
STRESS = ("mean64", "constant", "up12", "down12")
PARAMS = ("enc_w", "enc_b", "ln_w", "ln_b", "vec", "bias", "w1", "b1", "w2", "b2", "w3", "b3")


@functools.lru_cache(maxsize=None)
def inputs(name, stress=None):
    """Float64 dyadic inputs of a case from its seed; left unchanged."""
    if name == GRID:
        mask, levels = R.validity_grid()
        B, mask, seed = mask.shape[0], torch.from_numpy(mask), 310
    else:
        B, levels, make_mask, seed = SWEEP[name]
        mask = make_mask() if make_mask else torch.zeros(B, sum(h * w for h, w in levels), dtype=torch.bool)
    S = sum(h * w for h, w in levels)
    assert tuple(mask.shape) == (B, S)
    g = torch.Generator().manual_seed(seed)
    rn = lambda *shape: torch.randn(*shape, generator=g)
    x = dict(levels=[tuple(l) for l in levels], mask=mask, B=B, S=S)
    x["enc_w"], x["enc_b"] = C.dyadic(rn(D, D), D ** -0.5), C.dyadic(rn(D), 0.1)
    x["ln_w"], x["ln_b"] = C.dyadic(1.0 + 0.1 * rn(D)), C.dyadic(rn(D), 0.1)
    x["vec"], x["bias"] = C.dyadic(rn(B, D), 0.25), C.dyadic(rn(B))
    x["w1"], x["b1"] = C.dyadic(rn(D, D), D ** -0.5), C.dyadic(rn(D), 0.1)
    x["w2"], x["b2"] = C.dyadic(rn(D, D), D ** -0.5), C.dyadic(rn(D), 0.1)
    x["w3"], x["b3"] = C.dyadic(rn(4, D), D ** -0.5), C.dyadic(rn(4), 0.1)
    x["memory"] = C.dyadic(rn(B, S, D))
    if stress == "mean64":
        # Row mean about 64, row spread about 1: enc_weight's products are 1/64 of the bias.  (Dividing the drawn weight by 64
        # as well would leave a spread of 1/16, a thousandth of the mean; rounding enc_output's result to fp32 once, half an ulp
        # of 64, then costs 1e-4 of the largest logit by itself, in any fp32 evaluation, and nothing could meet the project's
        # bound.)
        x["enc_b"] = 64.0 + C.dyadic(rn(D), 1.0 / 16)
    elif stress == "constant":      # every row constant: variance 0
        x["enc_b"] = torch.full((D,), 0.375, dtype=torch.float64)
        x["enc_w"] = torch.zeros(D, D, dtype=torch.float64)
    elif stress == "up12":
        x["memory"] = x["memory"] * 2.0 ** 12
    elif stress == "down12":
        x["memory"] = x["memory"] * 2.0 ** -12
    else:
        assert stress is None
    for k in PARAMS + ("memory",):
        x[k] = x[k] + 0.0                                           # rounding to the dyadic grid leaves -0.0 behind: +0.0
        assert torch.equal(x[k].float().double(), x[k]), k          # fp32 holds what float64 sees
    return x


@functools.lru_cache(maxsize=None)
def reference(name, stress=None):
    """The restatement of a case over every row: computed once, shared, left unchanged."""
    x = inputs(name, stress)
    n = lambda k: x[k].numpy()
    cx, cy, wh, live, valid_wh = R.proposals(n("mask"), x["levels"])
    mem, mag_mem = R.out_mem(n("memory"), live, n("enc_w"), n("enc_b"), n("ln_w"), n("ln_b"), EPS)
    coords, points, mag_coords = R.boxes(mem, mag_mem, cx, cy, wh, live, *(n(k) for k in PARAMS[6:]))
    with np.errstate(invalid="ignore"):
        mag_points = np.where(np.isinf(coords), 0.0, points * ((1.0 - points) * mag_coords + 4.0))
    return dict(live=live, valid_wh=valid_wh, mem=mem, mag_mem=mag_mem, coords=coords, points=points, mag_coords=mag_coords,
                mag_points=mag_points)


def ref_logits(name, stress, shared, scale, clamp=0.0):
    x, r = inputs(name, stress), reference(name, stress)
    vec, bias = (x["vec"][:1], x["bias"][:1]) if shared else (x["vec"], x["bias"])
    return R.logits(r["mem"], r["mag_mem"], vec.numpy(), bias.numpy(), scale, clamp)


@functools.lru_cache(maxsize=None)
def device(name, stress=None):
    x = inputs(name, stress)
    t = {k: x[k].float().to(DEV).contiguous() for k in PARAMS + ("memory",)}
    t["mask"] = x["mask"].to(DEV).contiguous()
    t["shapes"] = torch.as_tensor(x["levels"], dtype=torch.long, device=DEV)
    t["valid_wh"] = torch.from_numpy(reference(name, stress)["valid_wh"]).to(DEV).contiguous()
    t["scale"] = torch.tensor([SCALE], dtype=torch.float32, device=DEV)
    assert float(t["scale"][0]) == SCALE
    return t


@functools.lru_cache(maxsize=None)
def composition(name, stress=None):
    """The fp32 PyTorch composition on the device, as float64 numpy: output_memory, coords of every row, their sigmoid."""
    from uninext_amd.modules.query_selection import gen_encoder_output_proposals
    x, t = inputs(name, stress), device(name, stress)
    with torch.no_grad():
        mem, prop = gen_encoder_output_proposals(t["memory"], t["mask"], x["levels"], lambda v: F.linear(v, t["enc_w"], t["enc_b"]),
                                                 lambda v: F.layer_norm(v, (D,), t["ln_w"], t["ln_b"], EPS))
        h = F.relu(F.linear(F.relu(F.linear(mem, t["w1"], t["b1"])), t["w2"], t["b2"]))
        coords = F.linear(h, t["w3"], t["b3"]) + prop
        points = coords.sigmoid()
    assert mem.dtype == torch.float32 and coords.dtype == torch.float32
    return dict(mem_dev=mem, mem=mem.cpu().double().numpy(), coords=coords.cpu().double().numpy(), points=points.cpu().double().numpy())


def comp_logits(name, stress, shared, scale, clamp=0.0):
    t, mem = device(name, stress), composition(name, stress)["mem_dev"]
    vec, bias = (t["vec"][:1], t["bias"][:1]) if shared else (t["vec"], t["bias"])
    with torch.no_grad():
        lg = torch.matmul(mem, vec.unsqueeze(-1).expand(mem.shape[0], D, 1))[..., 0]
        lg = (lg / t["scale"] if scale is not None else lg) + bias.view(-1, 1)
        if clamp > 0:
            lg = lg.clamp(min=-clamp, max=clamp)
    return lg.cpu().double().numpy()


# ---------------------------------------------------------------------------------------------------------------- the C ABI

def _sentinel():
    return (torch.arange(TAIL, dtype=torch.float32, device=DEV) * -3.0 - 0.625)


def guarded(n):
    buf = torch.full((n + TAIL,), float("nan"), dtype=torch.float32, device=DEV)
    buf[n:] = _sentinel()
    return buf


def written(buf, shape, what):
    """The output of a guarded buffer: every entry written (no NaN left), nothing written behind it."""
    n = int(np.prod(shape))
    assert buf.numel() == n + TAIL
    assert not bool(torch.isnan(buf[:n]).any()), what + ": entries left unwritten"
    assert torch.equal(buf[n:].view(torch.int32), _sentinel().view(torch.int32)), what + ": written past the end"
    return buf[:n].view(*shape).clone()


def _geometry(t, x):
    p = lambda k: t[k].data_ptr()
    return (p("memory"), p("mask"), p("shapes"), len(x["levels"]), p("valid_wh"), p("enc_w"), p("enc_b"), p("ln_w"), p("ln_b"), EPS)


def run_scores(name, stress=None, shared=False, scale=None, clamp=0.0, want_memory=False):
    from uninext_amd import _lib
    x, t = inputs(name, stress), device(name, stress)
    B, S = x["B"], x["S"]
    logits, mem = guarded(B * S), guarded(B * S * D) if want_memory else None
    rc = _lib.load().qsel_scores_hip_f32(*_geometry(t, x), t["vec"].data_ptr(), 0 if shared else D, t["bias"].data_ptr(),
                                         0 if shared else 1, t["scale"].data_ptr() if scale is not None else None, float(clamp),
                                         B, S, D, logits.data_ptr(), mem.data_ptr() if want_memory else None, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert _lib.last_kernel("qsel") == ("qsel_scores<memory>" if want_memory else "qsel_scores")
    return written(logits, (B, S), "logits"), (written(mem, (B, S, D), "output_memory") if want_memory else None)


def run_boxes(name, idx, stress=None):
    from uninext_amd import _lib
    x, t = inputs(name, stress), device(name, stress)
    B, S = x["B"], x["S"]
    idx = torch.from_numpy(np.array(idx, dtype=np.int64)).to(DEV).contiguous()
    K = idx.shape[1]
    assert tuple(idx.shape) == (B, K)
    coords, points = guarded(B * K * 4), guarded(B * K * 4)
    rc = _lib.load().qsel_boxes_hip_f32(*_geometry(t, x), idx.data_ptr(), K, *(t[k].data_ptr() for k in PARAMS[6:]), B, S, D,
                                        coords.data_ptr(), points.data_ptr(), None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert _lib.last_kernel("qsel") == "qsel_boxes"
    return written(coords, (B, K, 4), "coords_unact"), written(points, (B, K, 4), "reference_points")


# -------------------------------------------------------------------------------------------------------- the error measure

HEAD = "%-30s %-16s %10s %10s %10s %7s" % ("case", "output", "kernel err", "comp err", "bound", "ratio")
_T = PM.Table(HEAD, env="QSEL_PARITY_TABLE")
TABLE, report = _T.lines, _T.report


def measure(case, what, got, want, mag, comp, per_row=False):
    """Every entry of `got` within entry_bound(the composition's error at the entry, s) of `want`, and the project's bound on top.
    Non-finite: no NaN in `got`; infinities identical to `want`'s and in the same places, the composition's in the same places.
    per_row: one entry per row of the last axis, reduced before the bound and measured against the row's own largest value.
    WORST: none is kept.  Line: case, output, the worst entry's errors relative to its own magnitude; a dash line where no
    finite entry is left.  Tolerance: TOL * max|want|."""
    got = got.detach().cpu().double().numpy()
    assert got.shape == want.shape == comp.shape == mag.shape, (case, what, got.shape, want.shape)
    assert not np.isnan(got).any(), (case, what)
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), (case, what, "infinities")
    assert np.array_equal(np.isinf(comp), inf), (case, what, "the composition's infinities")
    fin = lambda a: np.where(inf, 0.0, a)
    e = PM.errors(fin(got), fin(want), fin(mag), fin(comp))
    if per_row:
        e = PM.Errors(e.err.max(-1), e.cerr.max(-1), e.size.max(-1), fin(mag).max(-1))
    if e.err.size == 0 or inf.all():
        _T.add("%-30s %-16s %10s %10s %10s %7s" % (case, what, "-", "-", "-", "-"))
        return 0.0
    _T.add("%-30s %-16s %10.2e %10.2e %10.2e %7.3f" % ((case, what) + e.row()))
    e.check(case, what)
    assert float(e.err.max()) <= C.TOL * float(e.size.max()), (case, what, "the project's bound", float(e.err.max()), float(e.size.max()))
    return e.worst


def clamps_for(free):
    """Clamps that bite on some rows of the float64 logits and not on others: one between the two middle magnitudes, or, where
    every row has the same magnitude, one below it and one above it."""
    u = np.unique(np.abs(free))
    if len(u) >= 2:
        out = [float(np.float32((u[len(u) // 2 - 1] + u[len(u) // 2]) / 2))]
    else:
        out = [float(np.float32(u[0] / 2)), float(np.float32(u[0] * 2))]
    assert all(c > 0 for c in out)
    assert any((np.abs(free) > c).any() for c in out) and any((np.abs(free) < c).any() for c in out)
    return out


def dead_rows_agree(live, logits, mem):
    """All dead rows of one image carry bitwise the same logit and the same output_memory row."""
    for b in range(live.shape[0]):
        dead = torch.from_numpy(~live[b]).to(DEV)
        if bool(dead.any()):
            lg = logits[b][dead].view(torch.int32)
            assert bool((lg == lg[0]).all()), b
            if mem is not None:
                rows = mem[b][dead].view(torch.int32)
                assert bool((rows == rows[0]).all()), b


# ------------------------------------------------------------------------------------------------------------------ the sweep

@pytest.mark.parametrize("name", list(SWEEP))
def test_scores_sweep(name):
    from uninext_amd import ext
    x, r, t = inputs(name), reference(name), device(name)
    since = len(TABLE)
    assert x["B"] * x["S"] == {"one_row": 1, "tile_less_1": 31, "one_tile": 32, "tile_plus_1": 33, "32_images_a_tile": 40,
                               "pyramid5": 1165, "six_levels": 478, "125_workgroups": 4000, "image1_padded": 466}[name]
    live = r["live"]
    if name == "six_levels":
        starts = R.level_starts(x["levels"])
        assert live[:, starts[4]:starts[5]].any() and not live[:, starts[5]:].any()      # level 4 lives, level 5 is all dead
    if name == "image1_padded":
        assert (r["valid_wh"][1] == 0).all() and not live[1].any() and live[0].any()
    if name == "32_images_a_tile":
        assert np.array_equal(live[:, 0], np.arange(40) % 2 == 0)
    comp = composition(name)
    # with output_memory: per image class terms, a scale, no clamp
    logits, mem = run_scores(name, scale=SCALE, want_memory=True)
    want, mag, _ = ref_logits(name, None, False, SCALE)
    measure(name, "logits", logits, want, mag, comp_logits(name, None, False, SCALE))
    measure(name, "output_memory", mem, r["mem"], r["mag_mem"], comp["mem"], per_row=True)
    dead_rows_agree(live, logits, mem)
    # without: bitwise the same logits; every combination of shared / per image terms, scale and clamp
    bites, spares = False, False
    for shared in (False, True):
        for scale in (None, SCALE):
            free = ref_logits(name, None, shared, scale)[2]
            for clamp in [0.0] + clamps_for(free):
                got, none = run_scores(name, shared=shared, scale=scale, clamp=clamp)
                assert none is None
                want, mag, _ = ref_logits(name, None, shared, scale, clamp)
                what = "logits %s%s%s" % ("1" if shared else "B", " /s" if scale else "", " clamp" if clamp else "")
                measure(name, what, got, want, mag, comp_logits(name, None, shared, scale, clamp))
                dead_rows_agree(live, got, None)
                if clamp:
                    assert float(got.abs().max()) <= clamp
                    bites, spares = bites or bool((np.abs(free) > clamp).any()), spares or bool((np.abs(free) < clamp).any())
                    hit = torch.from_numpy(np.abs(free) - clamp > 4 * R.SUM_DEPTH * R.U * mag).to(DEV)      # beyond any rounding
                    assert bool((got[hit].abs() == clamp).all())
                if not shared and scale and not clamp:
                    assert torch.equal(got, logits)
                if shared and x["B"] == 1:      # ext.qsel_scores' stride choice for one image: [1, d] and [d]
                    args = (t["memory"], t["mask"], t["shapes"], t["valid_wh"], t["enc_w"], t["enc_b"], t["ln_w"], t["ln_b"], EPS)
                    for v in (t["vec"][:1], t["vec"][0]):
                        via = ext.qsel_scores(*args, v, t["bias"][:1], t["scale"] if scale else None, clamp)
                        assert torch.equal(via, got)
    assert bites and spares
    report(since)


def index_lists(name):
    """[(label, idx [B, K])]: the float64 logits' own top-K for every K, and one list with duplicates, descending and shuffled,
    dead rows among the picks."""
    x, r = inputs(name), reference(name)
    B, S = x["B"], x["S"]
    order = np.argsort(-ref_logits(name, None, False, SCALE)[0], axis=1, kind="stable")
    lists = [("top-%d" % K, order[:, :K]) for K in sorted({K for K in (1, 31, 32, 33, min(S, 100)) if K <= S})]
    dead_first = np.argsort(r["live"], axis=1, kind="stable")
    base = np.concatenate((order[:, :min(S, 5)], dead_first[:, :min(S, 3)]), 1)
    rng = np.random.default_rng(SWEEP[name][3])
    twice = np.concatenate((base, base), 1)
    mixed = np.concatenate((base, base[:, ::-1], twice[:, rng.permutation(twice.shape[1])]), 1)
    picks_dead = ~np.take_along_axis(r["live"], mixed, 1)
    assert picks_dead.any() == (~r["live"]).any()
    lists.append(("mixed-%d" % mixed.shape[1], mixed))
    return lists


def check_boxes(name, label, idx, coords, points, stress=None):
    r, comp = reference(name, stress), composition(name, stress)
    pick = lambda a, fill: R.gather_rows(a, idx, fill)
    want = pick(r["coords"], np.inf)
    dead = np.isinf(want)
    assert np.array_equal(dead.any(-1), dead.all(-1))
    assert bool((points[torch.from_numpy(dead).to(DEV)] == 1.0).all())                       # exactly 1
    case = "%s %s" % (name if stress is None else name + "/" + stress, label)
    measure(case, "coords_unact", coords, want, pick(r["mag_coords"], 0.0), pick(comp["coords"], np.inf))
    measure(case, "reference_points", points, pick(r["points"], 1.0), pick(r["mag_points"], 0.0), pick(comp["points"], 1.0))


@pytest.mark.parametrize("name", list(SWEEP))
def test_boxes_sweep(name):
    x = inputs(name)
    since = len(TABLE)
    for label, idx in index_lists(name):
        coords, points = run_boxes(name, idx)
        check_boxes(name, label, idx, coords, points)
    report(since)


def test_boxes_index_outside_the_image_counts_as_padded():
    """include/dynmask_hip.h: "an index outside [0, S) counts as a padded row".  -1, S and 2^40 come back as +inf and 1.0 and the
    other entries bitwise as without them (proposal_of returns before any read for such an index)."""
    name = "pyramid5"
    x = inputs(name)
    label, idx = index_lists(name)[-1]
    outside = idx.copy()
    K = idx.shape[1]
    places = {1: -1, K // 2: x["S"], K - 2: 2 ** 40}
    for b in range(x["B"]):
        for at, value in places.items():
            outside[b, (at + b) % K] = value
    moved = outside != idx
    assert moved.sum() == 3 * x["B"]
    since = len(TABLE)
    coords, points = run_boxes(name, idx)
    coords_o, points_o = run_boxes(name, outside)
    m = torch.from_numpy(moved).to(DEV)
    assert bool((coords_o[m] == float("inf")).all()) and bool((points_o[m] == 1.0).all())
    assert torch.equal(coords_o[~m].view(torch.int32), coords[~m].view(torch.int32))
    assert torch.equal(points_o[~m].view(torch.int32), points[~m].view(torch.int32))
    check_boxes(name, "outside", outside, coords_o, points_o)
    report(since)


# -------------------------------------------------------------------------------------------------- validity, exhaustively

def test_validity_grid_every_x_and_valid_size_up_to_128():
    from uninext_amd import modules as M
    from uninext_amd.modules.query_selection import TwoStageQuerySelection
    x, r, t = inputs(GRID), reference(GRID), device(GRID)
    assert (x["B"], x["S"]) == (128, 256) and x["B"] * x["S"] == 32768
    q = R.grid_quotients()
    assert (q == R.LO).any() and (q == R.HI).any()              # a property of the grid: quotients that ARE the two limits
    assert np.array_equal(r["live"][:, :128], ~np.isnan(q) & (q > R.LO) & (q < R.HI))
    since = len(TABLE)
    every = np.broadcast_to(np.arange(x["S"]), (x["B"], x["S"]))
    coords, points = run_boxes(GRID, every)
    assert np.array_equal(torch.isinf(coords).any(-1).cpu().numpy(), ~r["live"])                  # row by row
    # the module's own composition on the device in fp32: the same validity bits
    enc, norm = torch.nn.Linear(D, D), torch.nn.LayerNorm(D, eps=EPS)
    head, mlp = M.Still_Classifier(D), M.MLP(D, D, 4, 3)
    with torch.no_grad():
        for p, k in ((enc.weight, "enc_w"), (enc.bias, "enc_b"), (norm.weight, "ln_w"), (norm.bias, "ln_b"),
                     (mlp.layers[0].weight, "w1"), (mlp.layers[0].bias, "b1"), (mlp.layers[1].weight, "w2"),
                     (mlp.layers[1].bias, "b2"), (mlp.layers[2].weight, "w3"), (mlp.layers[2].bias, "b3")):
            p.copy_(x[k].float())
        head.body.weight.copy_(x["vec"][:1].float())
        head.body.bias.copy_(x["bias"][:1].float())
        mods = [m.to(DEV).eval() for m in (enc, norm, head, mlp)]
        out = TwoStageQuerySelection._select_composition(t["memory"], t["mask"], t["shapes"], *mods, None, 1, True)
    module_coords = out[4]
    assert module_coords.dtype == torch.float32
    assert np.array_equal(torch.isinf(module_coords).any(-1).cpu().numpy(), ~r["live"])
    # live rows' cx / cy logits (and the rest of the box) under the per-entry measure, against the module's composition
    measure(GRID, "coords_unact", coords, r["coords"], r["mag_coords"], module_coords.cpu().double().numpy())
    measure(GRID, "reference_points", points, r["points"], r["mag_points"], out[4].sigmoid().cpu().double().numpy())
    report(since)


# ------------------------------------------------------------------------------------------------------- LayerNorm stress

def one_pass_fp32(name, stress):
    """output_memory with the variance as E[x^2] - E[x]^2 in numpy fp32, from the float64 rows rounded to fp32 once."""
    x, r = inputs(name, stress), reference(name, stress)
    n = lambda k: x[k].numpy()
    y = ((n("memory") * r["live"][..., None]) @ n("enc_w").T + n("enc_b")).astype(np.float32)
    d = np.float32(D)
    mean = y.sum(-1, keepdims=True, dtype=np.float32) / d
    var = (y * y).sum(-1, keepdims=True, dtype=np.float32) / d - mean * mean
    with np.errstate(invalid="ignore", divide="ignore"):
        out = (y - mean) / np.sqrt(var + np.float32(EPS)) * n("ln_w").astype(np.float32) + n("ln_b").astype(np.float32)
    assert out.dtype == np.float32
    return out.astype(np.float64)


@pytest.mark.parametrize("stress", STRESS)
@pytest.mark.parametrize("name", ["one_tile", "pyramid5"])
def test_layernorm_stress(name, stress):
    x, r, comp = inputs(name, stress), reference(name, stress), composition(name, stress)
    case = name + "/" + stress
    since = len(TABLE)
    if stress == "mean64":
        # the case has teeth: a one-pass fp32 variance misses the bound the kernel is held to, before the kernel runs
        y = r["mem"]
        wrong = one_pass_fp32(name, stress)
        err = np.where(np.isnan(wrong), np.inf, np.abs(wrong - y)).max(-1)
        bound = R.entry_bound(np.abs(comp["mem"] - y).max(-1), r["mag_mem"].max(-1))
        print("%s: one-pass fp32 variance, worst row error / bound %.3g" % (case, float((err / bound).max())))
        assert (err > bound).any()
    logits, mem = run_scores(name, stress, scale=SCALE, want_memory=True)
    want, mag, _ = ref_logits(name, stress, False, SCALE)
    measure(case, "logits", logits, want, mag, comp_logits(name, stress, False, SCALE))
    measure(case, "output_memory", mem, r["mem"], r["mag_mem"], comp["mem"], per_row=True)
    dead_rows_agree(r["live"], logits, mem)
    if stress == "constant":        # variance 0: the normalised row is ln_bias itself, and the logit the one number that follows
        t = device(name, stress)
        assert bool((mem.view(torch.int32) == t["ln_b"].view(torch.int32)).all())
        for b in range(x["B"]):
            assert bool((logits[b].view(torch.int32) == logits[b, 0].view(torch.int32)).all())
    every = np.broadcast_to(np.arange(x["S"]), (x["B"], x["S"]))
    coords, points = run_boxes(name, every, stress)
    check_boxes(name, "every row", every, coords, points, stress)
    report(since)
