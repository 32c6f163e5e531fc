"""The edge-location inputs (tests/msda_edges.py) hold what they claim, and they can catch a kernel that is wrong on them.

A numpy restatement of the per-sample grad_sampling_loc is checked against the float32 C oracle on every category, then
mutated the way a kernel could go wrong on a cell edge: (a) the coordinate rounded twice, (b) a corner whose bilinear
weight is 0 read as 0 (the derivative still takes it), (c) the corner in row H (column W) read from the memory behind the
level instead of as 0.  Each mutation must miss the bound of tests/test_msda_edges_gpu.py on many samples of its category
-- otherwise the GPU test would pass because its inputs check nothing."""
import numpy as np
import pytest

import msda_edges as E

POW2 = ((32, 64), (16, 32), (8, 16), (4, 8))
R50_QUARTER = ((25, 42), (13, 21), (7, 11), (4, 6))
THIN = ((3, 400), (2, 200), (1, 100), (1, 50))
PYRAMIDS = {"pow2": POW2, "r50q": R50_QUARTER, "thin": THIN}

_cache = {}


def _edges(name, kind="encoder"):
    key = (name, kind)
    if key not in _cache:
        _cache[key] = E.make_edges(kind, PYRAMIDS[name], num_query=None if kind == "encoder" else 300, seed=5)
    return _cache[key]


def _oracle(x, dtype=np.float32):
    from oracle import msda_oracle
    f = lambda k: x[k].numpy().astype(dtype)
    return msda_oracle.backward(f("grad_out"), f("value"), x["shapes"].numpy(), x["lsi"].numpy(), f("loc"), f("attn"))


def restate_grad_loc(x, mask, mutation=None):
    """grad_sampling_loc [n, 2] of the samples `mask` ([N, Lq, M, L, P]) in float64 from the float32 coordinate
    (ops/src/cuda/ms_deform_im2col_cuda.cuh:87-159).  mutation: None, "two_roundings", "zero_weight_corner", "next_memory"."""
    value = x["value"].numpy().astype(np.float64)                   # [N, S, M, D]
    S = value.shape[1]
    loc, attn = x["loc"].numpy(), x["attn"].numpy().astype(np.float64)
    go = x["grad_out"].numpy().astype(np.float64).reshape(value.shape[0], loc.shape[1], value.shape[2], value.shape[3])
    b, q, m, l, p = np.nonzero(mask)
    shapes, lsi = x["shapes"].numpy(), x["lsi"].numpy()
    H, W, st = shapes[l, 0], shapes[l, 1], lsi[l]
    coord = E.coord_two if mutation == "two_roundings" else E.coord_fma
    lx, ly = loc[b, q, m, l, p, 0], loc[b, q, m, l, p, 1]
    w_im, h_im = coord(lx, W).astype(np.float64), coord(ly, H).astype(np.float64)
    inr = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)
    h0, w0 = np.floor(h_im), np.floor(w_im)
    lh, lw = h_im - h0, w_im - w0
    hh, hw = 1 - lh, 1 - lw
    h0, w0 = h0.astype(np.int64), w0.astype(np.int64)

    def corner(dy, dx, weight):
        y, xx = h0 + dy, w0 + dx
        ok = inr & (y >= 0) & (y <= H - 1) & (xx >= 0) & (xx <= W - 1)
        if mutation == "next_memory":   # row H / column W read through the flat index: the next level's rows, the next row's pixel
            flat = st + y * W + xx
            ok = inr & (y >= 0) & (xx >= 0) & (flat < S)
        else:
            flat = st + y * W + xx
        flat = np.where(ok, flat, 0)
        v = value[b, flat, m] * ok[:, None]
        if mutation == "zero_weight_corner":
            v = v * (weight != 0)[:, None]
        return v
    v1, v2 = corner(0, 0, hh * hw), corner(0, 1, hh * lw)
    v3, v4 = corner(1, 0, lh * hw), corner(1, 1, lh * lw)
    tgv = go[b, q, m] * attn[b, q, m, l, p][:, None]
    gw = (tgv * (-hh[:, None] * v1 + hh[:, None] * v2 - lh[:, None] * v3 + lh[:, None] * v4)).sum(1) * W
    gh = (tgv * (-hw[:, None] * v1 - lw[:, None] * v2 + hw[:, None] * v3 + lw[:, None] * v4)).sum(1) * H
    return np.stack([gw, gh], -1) * inr[:, None]


def _misses(x, mask, got, want):
    """Samples of `mask` where |got - want| exceeds the GPU test's bound 1e-4 * max(H_l, W_l)."""
    l = np.nonzero(mask)[3]
    bound = 1e-4 * x["shapes"].numpy()[l].max(1)
    return (np.abs(got - want).max(1) >= bound)


@pytest.mark.parametrize("name", sorted(PYRAMIDS))
@pytest.mark.parametrize("kind", ["encoder", "decoder"])
def test_categories_hold_their_claims(name, kind):
    x = _edges(name, kind)
    loc, masks = x["loc"].numpy(), x["masks"]
    for l, (h, w) in enumerate(PYRAMIDS[name]):
        cx, cy = E.coord_fma(loc[:, :, :, l, :, 0], w), E.coord_fma(loc[:, :, :, l, :, 1], h)
        inside = (cx > -1) & (cx < w) & (cy > -1) & (cy < h)
        lat, co, ci = masks["lattice"][:, :, :, l], masks["cut_out"][:, :, :, l], masks["cut_in"][:, :, :, l]
        assert lat.sum() > 0.3 * lat.size and co.sum() > 0 and ci.sum() > 0, (l, lat.sum(), co.sum(), ci.sum())
        assert inside[lat].all() and ((cx == np.floor(cx)) | (cy == np.floor(cy)))[lat].all()
        assert not inside[co].any()
        assert (np.isin(cx, [-1, w]) | np.isin(cy, [-1, h]))[co].all()
        assert inside[ci].all() and (np.isin(cx, E.cutoff_values(w)) | np.isin(cy, E.cutoff_values(h)))[ci].all()
        for axis, size in ((0, w), (1, h)):
            rows = E.lattice_rows(x, l, axis)
            reachable = np.nonzero(~np.isnan(E.lattice_table(size)))[0]
            if kind == "encoder" or size <= 64:
                assert np.array_equal(rows, reachable), (l, axis, np.setdiff1d(reachable, rows))
            if E.is_pow2(size):
                assert rows.tolist() == list(range(size))   # every pixel row / column, 0 and size - 1 and the tile edges among them
                c = loc[:, :, :, l, :, axis][lat]
                assert np.array_equal(E.coord_fma(c, size), E.coord_two(c, size))   # exact under any rounding
        wit = masks["witness"][:, :, :, l]
        if E.is_pow2(h) and E.is_pow2(w):
            assert not wit.any() and not masks["witness_cut"][:, :, :, l].any()
        elif len(E.witness_table(h)[0]) + len(E.witness_table(w)[0]):
            assert wit.sum() > 0, l
            tx, ty = E.coord_two(loc[:, :, :, l, :, 0], w), E.coord_two(loc[:, :, :, l, :, 1], h)
            assert ((np.floor(cx) != np.floor(tx)) | (np.floor(cy) != np.floor(ty)))[wit].all()
    if name == "pow2":
        rows = E.lattice_rows(x, 0, 1)
        assert {15, 16, 31}.issubset(rows.tolist())        # msda_bwd_dst's tile rows 16 t - 1, 16 t, 16 t + 15
    else:
        assert masks["witness"].sum() > 100


def test_cutoff_decisions_have_no_witness_on_the_shipped_sizes():
    """The `> -1` / `< size` decisions come out the same under one rounding and two on every float32 location searched:
    only the cell decisions separate the conventions (witness_cut stays empty on these sizes)."""
    from uninext_amd import workloads
    sizes = {s for lv in list(PYRAMIDS.values()) + [workloads.R50_LEVELS_INFER, workloads.R50_LEVELS_TRAIN] for hw in lv for s in hw}
    assert all(E.witness_table(s)[1].size == 0 for s in sizes)
    assert sum(E.witness_table(s)[0].size for s in sizes) > 20


def test_f32_and_f64_oracles_decide_alike_on_exact_points():
    """On a power-of-two pyramid the lattice and cut-off coordinates are exact in both precisions: the float32 and float64
    oracles take the same cell and the same in-range decision, so their grad_loc agree to rounding.  (On other sizes the
    float64 coordinate of a float32 edge location is only near the edge.)"""
    x = _edges("pow2", "decoder")
    _, gl32, ga32 = _oracle(x, np.float32)
    _, gl64, ga64 = _oracle(x, np.float64)
    masks = x["masks"]
    exact = masks["lattice"] | masks["cut_in"] | masks["cut_out"]
    assert not _misses(x, exact, gl32[exact], gl64[exact]).any()
    out = masks["cut_out"]
    assert not gl32[out].any() and not ga32[out].any() and not gl64[out].any() and not ga64[out].any()


@pytest.mark.parametrize("name", ["r50q", "thin"])
def test_f32_oracle_follows_the_fma_on_witnesses(name):
    x = _edges(name, "decoder")
    _, gl32, _ = _oracle(x, np.float32)
    wit = x["masks"]["witness"]
    assert wit.sum() > 100
    fma, two = restate_grad_loc(x, wit), restate_grad_loc(x, wit, "two_roundings")
    assert not _misses(x, wit, gl32[wit], fma).any()
    assert _misses(x, wit, gl32[wit], two).mean() > 0.5


@pytest.mark.parametrize("name", sorted(PYRAMIDS))
def test_restatement_matches_the_oracle(name):
    x = _edges(name, "decoder")
    _, gl32, _ = _oracle(x)
    for cat in ("lattice", "cut_out", "cut_in", "witness"):
        m = x["masks"][cat]
        if m.any():
            assert not _misses(x, m, restate_grad_loc(x, m), gl32[m]).any(), cat


@pytest.mark.parametrize("mutation,category,name,least", [
    ("two_roundings", "witness", "r50q", 0.5),
    ("two_roundings", "witness", "thin", 0.5),
    ("zero_weight_corner", "lattice", "pow2", 0.5),
    ("zero_weight_corner", "lattice", "r50q", 0.5),
    ("next_memory", "lattice", "pow2", 0.02),
    ("next_memory", "lattice", "r50q", 0.02),
])
def test_the_inputs_catch_a_mutated_kernel(mutation, category, name, least):
    """Each mutation misses the GPU test's bound on many samples of its category (on the last row / column for next_memory)."""
    x = _edges(name, "decoder")
    _, gl32, _ = _oracle(x)
    m = x["masks"][category]
    bad = _misses(x, m, restate_grad_loc(x, m, mutation), gl32[m])
    print("%s on %s %s: %d of %d samples over the bound" % (mutation, name, category, int(bad.sum()), bad.size))
    assert bad.sum() >= 50 and bad.mean() >= least, (int(bad.sum()), bad.size)
