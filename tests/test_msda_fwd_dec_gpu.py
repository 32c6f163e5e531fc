"""msda_fwd_lanegroup<8, 16> (fp32, D = 32, L = P = 4: the decoder's forward calls; uninext_amd/csrc/msda_fwd.hip) at
its wave and workgroup edges, MI355X.

(The file keeps the name the work was planned under; a separately named `msda_fwd_dec` kernel was not built, because
tests/test_msda_gpu.py and tests/test_capi_cpu.py fix the reported kernel name and the variant table.)

The kernel takes 32 consecutive (query, head) pairs per workgroup, a wave = one query x 8 heads at M = 8: query counts
1, 3, 4, 5 are the edges of a workgroup's four waves, 31 / 32 / 33 those of the general body's 32-queries-per-head
workgroups and 257 takes more than one workgroup per image with a partly filled last one.  Every output element is
compared with the C oracle (oracle/msda_oracle.py) within the forward bound of tests/test_msda_parity_gpu.py (its
header: |a - b| < 1e-4 on every element; that file states the figure inline and exports no name to import, so FWD_TOL
repeats it), and with torch.equal against the general lane-group instance <8, 0> on the same inputs
(_lib.set_lanegroup_general): same arithmetic, same summation order -- samples in order, corners 1 -> 4."""
import numpy as np
import pytest
import torch

import msda_edges as E

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-4
M, D = 8, 32
QUERIES = (1, 3, 4, 5, 31, 32, 33, 257)
PYRAMIDS = {
    "odd": ((3, 5), (2, 3), (1, 2), (1, 1)),
    "ones": ((1, 1), (1, 1), (1, 1), (1, 1)),
    "exact": ((7, 9), (4, 5), (2, 3), (1, 2)),       # S = the pixel count: the last pixel row ends the buffer
}


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


def _cut_locations(size):
    """float32 locations whose pixel coordinate loc * size - 0.5 is exactly -1, -1 + ulp, size - 1, size, size - ulp."""
    t = E.cutoff_table(size)
    v = [t["lo_out"], t["lo_in"], float(E.lattice_table(size)[size - 1]), t["hi_out"], t["hi_in"]]
    return [x for x in v if not np.isnan(x)]


_cache = {}


def _case(name, N):
    """Inputs of max(QUERIES) queries (CPU) and the oracle's forward, computed once; the tests slice query prefixes.
    Query 0 of every image carries, per level, every (x, y) combination of the cut-off locations -- so every corner
    combination at the cut-offs -- and one NaN, +inf, -inf and -1e30 location in single samples; the rest is uniform in
    [-0.2, 1.2]."""
    key = (name, N)
    if key not in _cache:
        from oracle import msda_oracle
        from uninext_amd.workloads import level_tensors
        levels = PYRAMIDS[name]
        Lq, S = max(QUERIES), sum(h * w for h, w in levels)
        g = torch.Generator().manual_seed(270 + 7 * N + len(name))
        value = torch.randn(N, S, M, D, generator=g)
        loc = (torch.rand(N, Lq, M, 4, 4, 2, generator=g) * 1.4 - 0.2).numpy()
        attn = torch.softmax(torch.randn(N, Lq, M, 16, generator=g), -1).view(N, Lq, M, 4, 4)
        for l, (h, w) in enumerate(levels):
            k = 0
            for lx in _cut_locations(w):
                for ly in _cut_locations(h):
                    loc[:, 0, k // 4, l, k % 4] = (lx, ly)      # 25 of the 32 (head, point) slots of query 0
                    k += 1
            assert k <= 28
        for l, bad in enumerate((np.nan, np.inf, -np.inf, -1e30)):
            loc[:, 0, 7, l, l, l % 2] = bad                     # slots 28 .. 31
        sh, lsi = level_tensors(levels, "cpu")
        x = dict(value=value, shapes=sh, lsi=lsi, loc=torch.from_numpy(loc), attn=attn)
        ref = msda_oracle.forward(x["value"], x["shapes"], x["lsi"], x["loc"], x["attn"])
        _cache[key] = (x, np.asarray(ref, dtype=np.float64).reshape(N, Lq, M * D))
    return _cache[key]


def _forward(MSDA, lib, x, lq, dev, variant, general=False):
    a = [x["value"].to(dev), x["shapes"].to(dev), x["lsi"].to(dev), x["loc"][:, :lq].contiguous().to(dev),
         x["attn"][:, :lq].contiguous().to(dev)]
    lib.set_variant("forward", variant)
    lib.set_lanegroup_general(general)
    try:
        out = MSDA.ms_deform_attn_forward(*a, 64)
    finally:
        lib.set_variant("forward", "auto")
        lib.set_lanegroup_general(False)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("name", sorted(PYRAMIDS))
def test_every_element_against_the_oracle(name, N, dev, api):
    MSDA, lib = api
    x, ref = _case(name, N)
    for lq in QUERIES:
        partner = _forward(MSDA, lib, x, lq, dev, "msda_fwd_lanegroup", general=True)    # the general <8, 0> instance
        assert lib.last_kernel("forward") == "msda_fwd_lanegroup"
        for variant in ("msda_fwd_lanegroup", "auto"):           # below 1024 queries both are this kernel
            out = _forward(MSDA, lib, x, lq, dev, variant)
            assert lib.last_kernel("forward") == "msda_fwd_lanegroup"
            got = out.cpu().numpy().astype(np.float64).reshape(N, lq, M * D)
            assert np.isfinite(got).all(), (name, N, lq)
            err = float(np.abs(got - ref[:, :lq]).max())
            print("%-5s N=%d Lq=%3d %-18s max |err| %.2e" % (name, N, lq, variant, err))
            assert err < FWD_TOL, (name, N, lq, variant, err)
            assert torch.equal(out, partner), (name, N, lq, variant)


def test_auto_on_both_sides_of_the_query_threshold(dev, api):
    """The threshold is the standing one (lg3_ok: 1024 queries; not moved, profiles/r27_decoder_forward.txt): 1023 queries
    take the lane-group kernel, 1024 msda_fwd_lg3.  Both against the oracle, the lane-group side also bitwise against
    the general instance at a size with 256 workgroups."""
    from oracle import msda_oracle
    from uninext_amd import workloads
    MSDA, lib = api
    x = workloads.make_inputs("decoder", "model", batch=1, levels=((25, 42), (13, 21), (7, 11), (4, 6)), num_query=1024,
                              seed=27, device="cpu")
    ref = np.asarray(msda_oracle.forward(x["value"], x["shapes"], x["lsi"], x["loc"], x["attn"]), dtype=np.float64).reshape(1, 1024, M * D)
    for lq, kernel in ((1023, "msda_fwd_lanegroup"), (1024, "msda_fwd_lg3")):
        out = _forward(MSDA, lib, x, lq, dev, "auto")
        assert lib.last_kernel("forward") == kernel
        assert float(np.abs(out.cpu().numpy().astype(np.float64).reshape(1, lq, M * D) - ref[:, :lq]).max()) < FWD_TOL
    assert torch.equal(_forward(MSDA, lib, x, 1023, dev, "auto"), _forward(MSDA, lib, x, 1023, dev, "auto", general=True))


@pytest.mark.parametrize("name", sorted(PYRAMIDS))
def test_an_inf_in_value_stays_with_the_query_that_samples_it(name, dev, api):
    """One inf in `value`, at a level-0 pixel that only query 2 of image 0 samples (every other sample that would load
    one of its corners, weight zero included, is moved out of the level): all other outputs equal the run without it.
    Dead corners must be dropped loads, not reads of a line some other sample also reads."""
    MSDA, lib = api
    x, _ = _case(name, 1)
    h, w = PYRAMIDS[name][0]
    y0, x0, lq, qs = h // 2, w // 2, 33, 2
    loc = x["loc"][:, :lq].numpy().copy()
    cx = E.coord_fma(loc[0, :, :, 0, :, 0], w)
    cy = E.coord_fma(loc[0, :, :, 0, :, 1], h)
    with np.errstate(invalid="ignore"):
        touch = (cx > -1) & (cx < w) & (cy > -1) & (cy < h) & np.isin(np.floor(cx), (x0 - 1, x0)) & np.isin(np.floor(cy), (y0 - 1, y0))
    lv = loc[0, :, :, 0]
    lv[touch] = (3.0, 3.0)                                      # outside level 0 (3 * size - 0.5 >= size for every size)
    lv[qs, 3, 1] = ((x0 + 0.5) / w, (y0 + 0.5) / h)             # query 2, head 3, point 1: the pixel's centre
    y = dict(x, loc=torch.from_numpy(loc), attn=x["attn"][:, :lq])
    clean = _forward(MSDA, lib, y, lq, dev, "msda_fwd_lanegroup")
    v = x["value"].clone()
    v[0, y0 * w + x0, 3, 5] = float("inf")
    dirty = _forward(MSDA, lib, dict(y, value=v), lq, dev, "msda_fwd_lanegroup")
    assert lib.last_kernel("forward") == "msda_fwd_lanegroup"
    keep = torch.ones(lq, dtype=torch.bool)
    keep[qs] = False
    assert torch.isfinite(clean).all()
    assert torch.equal(clean[0, keep], dirty[0, keep])
    assert not torch.isfinite(dirty[0, qs, 3 * D + 5])
