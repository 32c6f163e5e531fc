"""No GPU: tests/gemm_parity.py has teeth and its references alone satisfy their conditions.  The numpy split is the documented
bit recipe; every exact-tier case meets its 2^24 q condition and its significant-bit budget; on every bounded case the fp32
composition sits at 1 / COMP_MARGIN of its own bound and the restated split within SPLIT_EPS s (+ the accumulation term) of
the true product; each mutant of the restatement fails the tier named for it; the case table reaches every edge of the launch
code."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_parity as P     # noqa: E402
import parity_measure as PM     # noqa: E402


def f32(v):
    return {k: np.asarray(a[0] if isinstance(a, tuple) else a).astype(np.float32) for k, a in v.items()}


# ------------------------------------------------------------------------------------------------------------------ the split

def test_split_reproduces_x_within_2_to_minus_16():
    rs = PM.rng("gemm/split")
    x = (rs.randn(100000) * 2.0 ** rs.randint(-20, 21, size=100000)).astype(np.float32)
    hi, lo = P.split(x)
    assert np.all((hi.view(np.uint32) & 0xffff) == 0) and np.all((lo.view(np.uint32) & 0xffff) == 0)          # bf16 values
    x64 = x.astype(np.float64)
    assert np.all(np.abs(hi.astype(np.float64) - x64) < 2.0 ** -7 * np.abs(x64))
    err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - x64)
    assert np.all(err <= 2.0 ** -16 * np.abs(x64))
    assert err.max() > 2.0 ** -18 * np.abs(x64).min()                                    # and lo really rounds
    _, lt = P.split(x, truncate_lo=True)
    assert np.abs(lt.astype(np.float64)).sum() < np.abs(lo.astype(np.float64)).sum()      # truncation only ever shrinks lo


def test_split_rounds_to_nearest_and_carries():
    bits = np.array([0x3f800000,       # 1.0: lo = 0
                     0x3f80ffff,       # remainder 0xffff ulps: 16 ones, rounds up into the next binade of lo
                     0x3f808000,       # remainder exactly one bit: lo holds it
                     0x3f800001,       # one ulp: a power of two, lo holds it exactly
                     0x3f8000ff,       # 8 ones: fits lo's 8 bits exactly
                     0x3f8001ff,       # 9 ones: rounds up to 0x200
                     0x3f800180,       # 1.5 x 2^8 ulps: exact
                     0xbf8001ff], dtype=np.uint32)
    x = bits.view(np.float32)
    hi, lo = P.split(x)
    ulp = 2.0 ** -23
    assert np.array_equal(hi.astype(np.float64), [1, 1, 1, 1, 1, 1, 1, -1])
    assert np.array_equal(lo.astype(np.float64) / ulp, [0, 0x10000, 0x8000, 1, 0xff, 0x200, 0x180, -0x200])
    _, lt = P.split(x, truncate_lo=True)
    assert np.array_equal(lt.astype(np.float64) / ulp, [0, 0xff00, 0x8000, 1, 0xff, 0x1fe, 0x180, -0x1fe])


def test_exact_tier_values_split_exactly():
    rs = PM.rng("gemm/tiers")
    e8 = (P._small(rs, (4096,), 255) * P.QX).astype(np.float32)
    hi, lo = P.split(e8)
    assert np.array_equal(hi, e8) and not lo.any() and P.sig_bits(e8).max() == 8
    wide = (P._wide(rs, (4096, 8), 2 ** 16 - 1, 8) * P.QX).astype(np.float32)
    hi, lo = P.split(wide)
    assert P.sig_bits(wide).max() == 16 and lo.any()
    assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), wide.astype(np.float64))
    x, w = wide[:64], e8[:64 * 8].reshape(64, 8)
    assert np.array_equal(P.split_product(x, w), P.mm(x.astype(np.float64), w.astype(np.float64)))
    assert np.array_equal(P.sig_bits(np.array([0.0, 1.0, 3.0, 0.75, 255.0, 257.0, 65535.0])), [0, 1, 2, 2, 8, 9, 16])


def test_packed_layout_restates_the_documented_order():
    w = np.arange(3 * 32, dtype=np.float32).reshape(3, 32) + 0.5
    p = P.packed_layout(w)
    assert p.shape == (2, 2, 128, 16) and not p[:, :, 3:].any()
    hi, lo = P.split(w)
    assert p[1, 0, 2, 5] == hi.view(np.uint32)[2, 21] >> 16 and p[1, 1, 2, 5] == lo.view(np.uint32)[2, 21] >> 16
    w9 = np.arange(2 * 32 * 9, dtype=np.float32).reshape(2, 32, 3, 3)
    p9 = P.packed_layout(w9.reshape(2, -1), taps=9)
    assert p9.shape == (18, 2, 128, 16)
    g, kl = 13, 6                                           # group 13 = tap 4 of channels 16 .. 31
    assert p9[g, 0, 1, kl] == P.split(w9)[0].view(np.uint32)[1, 16 + kl, 1, 1] >> 16
    pe = P.packed_exact_layout(w9)
    assert pe.shape == (2, 9, 128, 16) and pe[1, 5, 1, 8 * 1 + 3] == w9[1, 16 + 2 * 3 + 1, 1, 2]


# ------------------------------------------------------------------------------------------------- the references' conditions

def _unique_inputs(names):
    """conv3x3 and patch_embed run the same shapes on several paths: one case per (shape, tier) is enough for a property of the
    inputs' construction; the GPU test asserts the condition of every case it runs."""
    seen, out = set(), []
    for n in names:
        c = dict(P.CASES[n])
        c.pop("prec", None), c.pop("path", None)
        key = tuple(sorted(c.items()))
        if key not in seen:
            seen.add(key)
            out.append(n)
    return out


@pytest.mark.parametrize("kind", ["lin", "pe", "conv"])
def test_exact_cases_meet_their_condition(kind):
    cases = _unique_inputs([n for n, c in P.CASES.items() if c["kind"] == kind and c["tier"] in P.EXACT])
    assert len(cases) > 100
    tops = [P.exact_condition(n) for n in cases]
    assert max(tops) < P.BUDGET and max(tops) > P.BUDGET / 4                # the budget is used, not merely respected


@pytest.mark.parametrize("kind", ["lin", "ln", "ffn", "pe", "conv"])
def test_bounded_references_alone(kind):
    cases = [n for n, c in P.CASES.items() if c["kind"] == kind and c["tier"] in P.BOUNDED]
    if kind in ("lin", "pe"):
        cases = [n for n in cases if P.CASES[n]["rows" if kind == "lin" else "Hp"] < 2000][::3]
    assert len(cases) >= 20
    for n in cases:
        comp = P.composition(n)
        worst = P.hold(n, "composition", f32(comp), check=False)
        # the composition, rounded to fp32 as it is: 1 / COMP_MARGIN of its own bound by construction (a masked row is 0 / 0)
        assert all(v <= 1.0 / P.COMP_MARGIN + 1e-12 for k, v in worst.items() if k != "true+eps"), (n, worst)
        if not P.packed_path(n):
            continue
        assert worst["true+eps"] <= 1.0, (n, worst)
        spl, true = P.reference(n, "split"), P.reference(n, "true")
        for what, (want, mag) in true.items():
            err = np.abs(spl[what][0] - want)
            assert np.all(err <= (P.SPLIT_EPS + P.SUM_DEPTH * P.U) * mag), (n, what, float((err / np.maximum(mag, 1e-300)).max()))
        if P.CASES[n]["tier"] == "dy20" and kind in ("lin", "conv", "pe"):
            assert max(float(np.abs(spl[w][0] - true[w][0]).max()) for w in true) > 0.0        # the split is not the product


# ------------------------------------------------------------------------------------------------------------------ the teeth

REPRESENTATIVE = {"lin": "lin/%s/k128/r65/n129/b1m1a0r0", "pe": "pe/packed/%s/k4c6/e33/p1x3x43/nhwc",
                  "conv": "conv/p2/%s/b2/c16/17x18/o65/b1r0"}
# mutant -> (the tiers it must fail, the families it applies to)
TEETH = {"drop_lh": (("EX",), ("lin", "pe", "conv")),
         "drop_hl": (("EW",), ("lin", "pe", "conv")),
         "truncate_lo": (("dy20",), ("lin", "pe", "conv")),
         "skip_last_chunk": (("E8",), ("lin", "pe", "conv")),
         "tail_row": (("E8", "dy10"), ("lin", "pe", "conv")),
         "bias_shift": (("E8", "dy10"), ("lin", "pe", "conv")),
         "mask_left": (("E8", "dy10"), ("lin",)),
         "edge_tap": (("E8", "dy10"), ("conv",)),
         "swap_taps": (("E8", "dy10"), ("pe", "conv"))}


def _fails(name, mutant):
    tier = P.CASES[name]["tier"]
    if tier in P.EXACT:
        got = f32(P.restate(name, "split", mutant))
        return P.hold(name, "mutant", got, check=False)["bits"] > 0
    got = {k: v[0] for k, v in P.restate(name, "split", mutant).items()}      # float64: not even fp32 rounding is added
    return P.hold(name, "mutant", got, check=False)["split"] > 1.0


@pytest.mark.parametrize("mutant", sorted(TEETH))
def test_mutants_fail(mutant):
    assert set(TEETH) == set(P.MUTANTS)
    tiers, kinds = TEETH[mutant]
    for kind in kinds:
        for tier in tiers:
            assert _fails(REPRESENTATIVE[kind] % tier, mutant), (kind, tier, mutant)


@pytest.mark.parametrize("kind", sorted(REPRESENTATIVE))
def test_the_restatement_itself_passes_and_a_nan_fails(kind):
    for tier in P.TIERS:
        name = REPRESENTATIVE[kind] % tier
        if tier in P.EXACT:
            assert P.hold(name, "restatement", f32(P.restate(name, "split")), check=False) == {"bits": 0}
            assert P.hold(name, "restatement", f32(P.restate(name, "true")), check=False) == {"bits": 0}
        else:
            got = f32(P.restate(name, "split"))
            worst = P.hold(name, "restatement", got, check=False)
            assert max(worst.values()) <= 1.0, (name, worst)
            got["out"].reshape(-1)[3] = np.nan
            assert P.hold(name, "restatement", got, check=False)["split"] == float("inf")
            with pytest.raises(AssertionError):
                P.hold(name, "restatement", got)
    del P.TABLE[:]
    P.WORST.clear()


def test_signed_zeros_compare_equal_and_nothing_else_does():
    want = np.array([0.0, 1.0, -2.5])
    assert len(P.bit_mismatches(np.array([-0.0, 1.0, -2.5], dtype=np.float32), want)) == 0
    assert len(P.bit_mismatches(np.array([0.0, np.nextafter(np.float32(1), np.float32(2)), -2.5], dtype=np.float32), want)) == 1
    with pytest.raises(AssertionError):
        P.bit_mismatches(np.zeros(1, dtype=np.float32), np.array([1.0 + 2.0 ** -30]))


# ---------------------------------------------------------------------------------------------------------------- the coverage

def _of(kind, **want):
    return [c for c in P.CASES.values() if c["kind"] == kind and all(c[k] == v for k, v in want.items())]


def test_linear_cases_reach_every_edge():
    for tier in P.EXACT:
        lin = _of("lin", tier=tier)
        assert {c["rows"] for c in lin} >= set(P.LIN_ROWS) and {c["N"] for c in lin} >= set(P.LIN_NS)
        assert {c["K"] for c in lin} == set(P.LIN_KS) - ({1024} if tier != "E8" else set())
        for K in (64, 256):
            assert {(c["rows"], c["N"]) for c in lin if c["K"] == K} >= {(r, n) for r in P.LIN_ROWS for n in P.LIN_NS}
    assert {c["rows"] % 64 for c in _of("lin")} >= {0, 1, 63} and {c["N"] % 32 for c in _of("lin")} >= {0, 1, 31}
    assert {c["K"] // 64 for c in _of("lin")} >= {1, 2, 3, 4, 5, 16}            # steps: below, at and past the ring's depth of 3 + 1
    assert any(c["K"] == 1024 for c in _of("lin", tier="dy20"))
    # the three tilings, each at the smallest row count that selects it, and the other side of each threshold
    took = {}
    for n, rows, tiling, below in P.LIN_TILINGS:
        assert P.linear_tiling(rows, n) == tiling and P.linear_tiling(rows - 1, n) == below != tiling
        assert rows % 64 == 1                                               # the last tile is a tail of one row
        for c in _of("lin", N=n, K=64):
            took.setdefault(P.linear_tiling(c["rows"], n), set()).add(c["tier"])
    assert set(took) == {(4, 1), (2, 1), (1, 2)} and all("E8" in t for t in took.values())
    assert "dy20" in took[(4, 1)] and "dy20" in took[(2, 1)]
    assert all(P.linear_tiling(r, n) == (1, 2) for r in P.LIN_ROWS for n in P.LIN_NS)
    for tier in P.TIERS:
        opt = [c for c in _of("lin", tier=tier, K=128) if c["rows"] in (65, 129) and not c["hm"] and not c["split_col"]]
        assert {(c["bias"], c["mask"], c["x_add"], c["relu"]) for c in opt} == {(a, b, c, d) for a in (False, True) for b in (False, True)
                                                                                 for c in (False, True) for d in (False, True)}
        assert {c["hm"] for c in _of("lin", tier=tier)} == {0, 64, 65, 100}
        assert {c["split_col"] for c in _of("lin", tier=tier)} == {0, 128, 256}
    m = P.lin_mask(129)
    assert m[128] and m[64:128].all() and not m[:64].all() and m[:64].any()
    m = P.lin_mask(65)
    assert m[64] and not m[:64].all()
    assert {c["rows"] for c in _of("ln")} == {1, 63, 64, 65} and {c["tier"] for c in _of("ln")} == set(P.BOUNDED)
    assert {(c["residual"], c["affine"], c["bias"]) for c in _of("ln")} >= set(P.LN_CFGS.values())
    ffn = _of("ffn")
    assert {c["F"] for c in ffn} == {128, 256, 384, 1024} and {c["rows"] for c in ffn} == {1, 63, 64, 65}
    assert {(c["F"] % 256 == 0, c["F"] > 256) for c in ffn} == {(False, False), (True, False), (False, True), (True, True)}
    assert {c["layer_norm"] for c in ffn} == {False, True} and any(c["plain"] for c in ffn) and any(c["negative"] for c in ffn)


@pytest.mark.parametrize("tier", P.BOUNDED)
def test_special_rows_are_what_they_are_named(tier):
    i = P.inputs("ln/%s/k256/r65/all" % tier)
    v, _ = P.product(P.mm, i["x"], i["w"]) + i["bias"] + i["residual"], None
    assert np.all(v[0] == 3.0)                                              # the constant row: variance 0
    res = i["residual"].astype(np.float64).mean(-1)                         # the rows whose residual carries a mean of 100
    assert np.all(np.abs(res[1::3] - 100.0) < 2.0) and np.all(np.abs(res[2::3]) < 2.0)
    for f in P.FFN_DS:
        i = P.inputs("ffn/%s/f%d/r65/negative" % (tier, f))
        assert np.all(P.product(P.mm, i["x"], i["w1"]) + i["b1"] < 0.0)
        assert np.all(P.product(P.mm, i["x"], i["w1"], "split") + i["b1"] < 0.0)


def test_patch_embed_cases_reach_every_edge():
    for path in ("packed", "exact"):
        for tier in P.EXACT:
            pe = _of("pe", path=path, tier=tier)
            ks = {c["C"] * c["k"] ** 2 for c in pe}
            assert ks == ({48, 96, 192, 768} | ({32, 80} if path == "exact" else set()))
            assert {c["k"] for c in pe} == {2, 4, 8, 16} and {c["cl"] for c in pe} == {False, True}
            assert {c["E"] for c in pe} >= set(P.PE_ES)
            assert {c["B"] * c["Hp"] * c["Wp"] for c in pe} >= {1, 127, 128, 129}
            assert any(c["W"] % 2 == 1 for c in pe) and any(c["W"] % 4 == 0 and c["H"] == c["Hp"] * c["k"] for c in pe)
            assert any(c["H"] > c["Hp"] * c["k"] and c["W"] > c["Wp"] * c["k"] for c in pe)
        assert {c["tier"] for c in _of("pe", path=path)} == set(P.TIERS)
    small = [c for c in _of("pe") if c["Hp"] < 128]
    assert not any(P.patch_packed_wide(c["B"] * c["Hp"] * c["Wp"], c["E"]) for c in small)
    assert {P.patch_exact_cfg(c["B"] * c["Hp"] * c["Wp"], c["E"], c["C"] * c["k"] ** 2) for c in small if c["path"] == "exact"} == {1, 2}
    big = [c for c in _of("pe") if c["Hp"] == 128]
    assert big and all(P.patch_packed_wide(16384, c["E"]) and P.patch_exact_cfg(16384, c["E"], 96) == 0 for c in big)
    assert not P.patch_packed_wide(16384 - 64, 130) and P.patch_exact_cfg(16384 - 128, 130, 96) == 1        # the smallest that does
    x = P.inputs("pe/packed/E8/k4c3/e33/p1x3x43/nhwc")["x"]
    assert x.shape == (1, 3, 13, 173) and np.all(x[:, :, 12] == P.SENTINEL) and np.all(x[:, :, :, 172] == P.SENTINEL)
    assert np.abs(x[:, :, :12, :172]).max() < P.SENTINEL / 1024


def test_conv_cases_reach_every_edge():
    for prec in P.CONV_PRECISIONS:
        for tier in P.EXACT:
            cv = _of("conv", prec=prec, tier=tier)
            assert {(c["H"], c["W"]) for c in cv} >= set(P.CONV_HW)
            assert {c["W"] % 4 for c in cv} == {0, 1, 2, 3} and {16, 17, 18} <= {c["W"] for c in cv} and any(c["W"] < 4 for c in cv)
            assert {c["cin"] for c in cv} == {16, 32, 48} and {c["cout"] for c in cv} >= set(P.CONV_COUTS)
            assert {c["B"] for c in cv} == {1, 2} and {(c["bias"], c["relu"]) for c in cv} == {(a, b) for a in (False, True) for b in (False, True)}
        assert {c["tier"] for c in _of("conv", prec=prec)} == set(P.TIERS)
    B, H, W = P.CONV_BIG
    units = {P.conv_exact_unit(c["B"], c["H"], c["W"], c["cout"]) for c in _of("conv", prec=3)}
    assert units == {1, 2, 3}
    assert P.conv_exact_unit(B, H, W, 65) == 1 and P.conv_exact_unit(B, H, W, 8) == 2 and P.conv_tiles(B, H, W) == 2048
    assert P.conv_exact_unit(B, H - 1, W, 65) == 2 and P.conv_exact_unit(B, H, W - 1, 8) == 3       # the smallest that does
    assert {c["tier"] for c in _of("conv", H=H, W=W)} == {"E8"}
    assert {P.conv_packed_wide(c["B"], c["H"], c["W"], c["cout"]) for c in _of("conv", prec=2)} == {False, True}
    assert {P.conv_fp32_big(c["B"], c["H"], c["W"], c["cout"]) for c in _of("conv", prec=0)} == {False, True}
