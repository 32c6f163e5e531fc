"""No GPU: the error measure of tests/dec_bwd_parity.py has teeth.

A numpy fp32 emulation of the three kernels, written from the header comment of uninext_amd/csrc/dec_attn_bwd.hip: attn_lse is
the forward of tests/test_attn_parity_cpu.py (tiles of 32 keys, the two waves' ranges of per_wave = ceil(tiles / 2) tiles
combined by wave 0) with lse = max + log(sum) of the combined ranges in fp32, -inf for a dead query; delta = g . out of the
emulated fp32 `out`, as two half sums and one exchange; p = exp((s + m) - lse) with that fp32 lse, a dead query's lse and delta
read as 0; the second products' sums in register order, tile after tile, wave 0's tiles and wave 1's into accumulators of their
own that are added in that order; a streamed tile is skipped when no lane of the 64 has an open pair in it.  It is held to the
measure against the float64 restatement with the fp32 PyTorch composition on the CPU as `comp`: the correct emulation stays
within the bound on EVERY case of the sweep, and each wrong variant is over it on the case named in WRONG, where the correct
emulation passes.  The restatement agrees with float64 autograd on every case (dec_bwd_parity.agrees_with_autograd).

For each wrong variant the old one-number measure (decoder_train_cases.group_err <= TOL, dq over the live queries) is recorded
too.  OLD_MISSES names the variants that pass it on their case and fail the new one; the test asserts that list, which holds
the transposed mask on the near-symmetric case and the one-pair skip.

Worst error / bound of the correct emulation over the sweep: lse 0.125, dq 0.023, dk 0.027, dv 0.055 (the stress cases).
Of each wrong variant on its named case, the largest over the groups, and the old measure's largest group error (TOL = 1e-4):
    dead_g_kept          L97/bool_row45/1x1      6.8e+05 (dv; dk 3.0e+05)      old 1.8e+01
    dk_unscaled_q        L32/bool/1x1            7.5e+04 (dk)                  old 4.7
    dq_no_scale          L32/bool/1x1            7.7e+04 (dq)                  old 4.7
    ds_no_delta          L64/none/1x1            5.5e+03 (dq; dk 2.7e+03)      old 3.5e-01
    float_mask_dropped   L65/f32_asym/1x1        2.1e+04 (dv; dq, dk 1e+04)    old 1.0
    lse_wave0_only       L65/f32/1x1             6.1e+03 (lse; dv 846)         old 2.4e-02
    mask_transposed_kv   L65/f32_near_sym/1x1    7.6     (dv; dk 1.7)          old 6.0e-05   MISSED by the old measure
    skip_half0           L97/bool_one_pair/1x1   2.3e+04 (dv; dk 4.0e+03)      old 3.3e-06   MISSED by the old measure
    tail_keys_open       L33/none/1x1            8.3e+04 (lse; dv 1.5e+04)     old 3.8e-01
    wave1_dropped        L33/none/1x1            1.5e+04 (dv; dq, dk 8e+03)    old 5.9e-01
    wave1_twice          L33/none/1x1            1.5e+04 (dv; dq, dk 8e+03)    old 5.9e-01
`rows of the tail tile past L treated as open` is tail_keys_open, in attn_lse: in the two backward passes those rows' k, q and
g are zero rows and add nothing whatever their probability.  The transposed read on the fully asymmetric mask (L65/f32_asym)
is far over both measures.

Dropped: `q scaled in float64, not rounded in fp32`.  The two products differ by at most u |q_d scale| per channel, so a score
moves by at most u amp_ij, which is what A_i of every magnitude allows by derivation; test_f64_scaled_q_is_inside_the_bound
prints its largest ratio over the sweep (below 1 on every case) in place of an assertion that it fails.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dec_bwd_parity as P              # noqa: E402
import test_attn_parity_cpu as FE       # noqa: E402  (the forward's emulation: dot32, stream, pad_keys, ROWS, heads_of, merged)

F32, F64 = np.float32, np.float64
NEG = F32("-inf")
TILE = P.TILE

# variant -> the case of the sweep on which it must exceed the bound
WRONG = {
    "mask_transposed_kv": "L65/f32_near_sym/1x1",   # the key pass reads m[j, i]
    "float_mask_dropped": "L65/f32_asym/1x1",       # the backward adds 0 for a finite mask value, -inf for -inf
    "skip_half0": "L97/bool_one_pair/1x1",          # the skip test sees lane half 0's registers only
    "wave1_dropped": "L33/none/1x1",                # wave 1's accumulators never reach the sum
    "wave1_twice": "L33/none/1x1",                  # ... are added twice
    "tail_keys_open": "L33/none/1x1",               # the 31 keys of the tail tile that do not exist count as open in attn_lse
    "ds_no_delta": "L64/none/1x1",                  # ds = p dp
    "dq_no_scale": "L32/bool/1x1",                  # dq without the final q_scale
    "dk_unscaled_q": "L32/bool/1x1",                # dk from q, not from q_scale q
    "lse_wave0_only": "L65/f32/1x1",                # lse from wave 0's max and sum alone
    "dead_g_kept": "L97/bool_row45/1x1",            # a dead query's row enters the key pass as if it were open
}
OLD_MISSES = ("mask_transposed_kv", "skip_half0")   # pass group_err <= TOL on their case, fail the per-entry measure


def f32(t):
    return t.numpy().astype(F32)


def fma32(a, b, c):
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def tile_order(t, n):
    """the rows below n of tile t in the order the second product adds them: register v of lane half 0, then of half 1"""
    return [j for j in (TILE * t + FE.ROWS[half][v] for v in range(16) for half in (0, 1)) if j < n]


def emulate(name, sw=()):
    """{group: float64 numpy} of the emulated kernels, shaped as dec_bwd_parity.reference has them."""
    c, x = P.CASES[name], P.inputs(name)
    B, heads, L = c["B"], c["heads"], c["L"]
    N = B * heads
    tiles = -(-L // TILE)
    SP = tiles * TILE
    per = -(-tiles // 2)
    waves = (range(0, per), range(per, tiles))
    q, k, v, g = (FE.heads_of(f32(x[n]), heads) for n in ("q", "k", "v", "g"))
    scale = F32(x["scale"])
    qs = q * scale
    if "q_scaled_f64" in sw:            # the unrounded product, carried in float64 through the score's sum
        qs64 = q.astype(F64) * float(scale)
        X = np.einsum("nid,njd->nij", qs64, k.astype(F64)).astype(F32)
        qs = qs64
    else:
        X = FE.dot32(qs, k, ())
    mask = x["mask"]
    add = np.zeros((L, L), F32)
    if mask is not None:
        add = np.where(mask.numpy(), NEG, F32(0)) if mask.dtype == P.torch.bool else f32(mask)
    add = add.astype(F32)
    open_ = ~(add == NEG)

    # ---- attn_lse
    Xp, vp = FE.pad_keys(X + add[None], v, F32(0) if "tail_keys_open" in sw else NEG)
    (m0, l0, a0), (m1, l1, a1) = (FE.stream(Xp, vp, w, ()) for w in waves)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = np.maximum(m0, m1)
        m_use = np.where(m == NEG, F32(0), m)
        w0, w1 = np.exp(m0 - m_use), np.exp(m1 - m_use)
        l = l0 * w0 + l1 * w1
        out = (a0 * w0[..., None] + a1 * w1[..., None]) * (F32(1) / l)[..., None]
        lse = (m0 + np.log(l0)) if "lse_wave0_only" in sw else m + np.log(l)
    assert out.dtype == F32 and lse.dtype == F32

    # ---- what both passes share: delta, the recomputed scores, dp
    dead = lse == NEG
    lse_use = np.where(dead, F32(0), lse)
    halves = []
    with np.errstate(invalid="ignore"):
        for half in (0, 1):
            a = np.zeros((N, L), F32)
            for ss in range(P.D // 8):
                for u in range(4):
                    d = 8 * ss + 4 * half + u
                    a = fma32(g[..., d], out[..., d], a)
            halves.append(a)
        dl = np.where(dead, F32(0), halves[0] + halves[1])
    DP = FE.dot32(g, v, ())
    badd = np.where(open_, F32(0), NEG).astype(F32) if "float_mask_dropped" in sw else add

    def probs(a):                       # a [L, L]: what this pass adds to score [i, j]
        with np.errstate(under="ignore", over="ignore"):
            p = np.exp((X + a[None]) - lse_use[..., None])
        ds = p * ((DP - dl[..., None]) if "ds_no_delta" not in sw else DP)
        assert p.dtype == F32 and ds.dtype == F32
        return p, ds

    def live_tiles(op):
        """[owned groups, streamed tiles]: some lane of the wave has an open pair.  op [owned, streamed].  In the correct
        emulation the skip changes no number (a skipped tile's p is exactly 0); it matters for skip_half0 only."""
        o = np.zeros((SP, SP), bool)
        o[:L, :L] = op
        if "skip_half0" in sw:          # lane half 0 holds the streamed rows with row % 8 < 4
            o[:, (np.arange(SP) % 8) >= 4] = False
        return o.reshape(tiles, TILE, tiles, TILE).any((1, 3))

    def second_product(rows, weights, live):
        """sum over the streamed rows, per wave and tile in register order, skipped tiles left out.  rows [N, L, D] of the
        streamed side, weights [N, owned, streamed]; returns the two waves' accumulators [N, owned, D]."""
        accs = []
        grp = np.arange(L) // TILE
        for w in waves:
            acc = np.zeros((N, L, P.D), F32)
            for t in w:
                on = live[grp, t].astype(F32)[None, :, None]            # the owned token's workgroup takes this tile or not
                for r in tile_order(t, L):
                    acc = acc + on * (rows[:, None, r, :] * weights[:, :, r, None])
            accs.append(acc)
        return accs

    # ---- bwd_q: the lane's query i, the tile's keys
    p, ds = probs(badd)
    a0, a1 = second_product(k, ds, live_tiles(~(badd == NEG)))
    accq = a0 if "wave1_dropped" in sw else (a0 + a1) + a1 if "wave1_twice" in sw else a0 + a1
    dq = accq if "dq_no_scale" in sw else accq * scale
    dq = np.where(dead[..., None], F32("nan"), dq)

    # ---- bwd_kv: the lane's key j, the tile's queries; the same scores and dp, transposed
    kadd = badd.T.copy() if "mask_transposed_kv" in sw else badd.copy()
    if "dead_g_kept" in sw:
        kadd[np.all(kadd == NEG, axis=1)] = F32(0)
    pk, dsk = probs(kadd)
    tr = lambda a: a.transpose(0, 2, 1)
    live = live_tiles(~(kadd == NEG).T)
    v0, v1 = second_product(g, tr(pk), live)
    k0, k1 = second_product(q if "dk_unscaled_q" in sw else qs.astype(F32), tr(dsk), live)
    if "wave1_dropped" in sw:
        dk, dv = k0, v0
    elif "wave1_twice" in sw:
        dk, dv = (k0 + k1) + k1, (v0 + v1) + v1
    else:
        dk, dv = k0 + k1, v0 + v1
    for a in (dq, dk, dv):
        assert a.dtype == F32
    return {"lse": lse.astype(F64), "dq": FE.merged(dq, B).astype(F64), "dk": FE.merged(dk, B).astype(F64), "dv": FE.merged(dv, B).astype(F64)}


def ratios(name, sw=(), check=True):
    """({group: error / bound} of the emulation on a case, the old measure's {dq, dk, dv})"""
    ref, comp = P.reference(name), P.composition(name, "cpu")
    got = emulate(name, sw)
    assert sorted(got) == sorted(ref) == sorted(comp), name
    new = {what: P.measure(name, what, got[what], want, mag, comp[what], check=check) for what, (want, mag) in ref.items()}
    live = np.ones(P.CASES[name]["L"], bool)
    live[list(P.inputs(name)["dead"])] = False
    old = P.group_err(got, {k: ref[k][0] for k in ("dq", "dk", "dv")}, live)
    return new, old


PIECES = ("len", "pattern", "float", "dead", "stress", "bh")


@pytest.mark.parametrize("group", PIECES)
def test_correct_emulation_within_the_bound(group):
    since = len(P.TABLE)
    worst = {}
    for name in P.names(group=group):
        P.mask_property(name)
        P.residue_groups(name)
        if P.CASES[name]["stress"]:
            P.stress_property(name)
        for what, r in ratios(name)[0].items():
            worst[what] = max(worst.get(what, 0.0), r)
    P.report(since)
    print("worst error / bound of the correct emulation:", "   ".join("%s %.3f" % (k, worst[k]) for k in P.GROUPS))
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("group", PIECES)
def test_restatement_agrees_with_float64_autograd(group):
    for name in P.names(group=group):
        P.agrees_with_autograd(name)


@pytest.mark.parametrize("variant", sorted(WRONG))
def test_wrong_variant_exceeds_the_bound_on_its_named_case(variant):
    name = WRONG[variant]
    assert max(ratios(name)[0].values()) <= 1.0                     # the correct emulation passes the same case
    new, old = ratios(name, (variant,), check=False)
    caught = max(old.values()) > P.TOL
    print("%-20s %-24s error / bound %s   old measure %s: %s" % (
        variant, name, "   ".join("%s %.3g" % (k, new[k]) for k in P.GROUPS), "   ".join("%s %.1e" % kv for kv in old.items()),
        "catches it" if caught else "MISSES it"))
    assert max(new.values()) > 1.0, (variant, name, new)
    assert caught == (variant not in OLD_MISSES), (variant, name, old)


def test_transposed_mask_on_the_asymmetric_case_fails_both_measures():
    new, old = ratios("L65/f32_asym/1x1", ("mask_transposed_kv",), check=False)
    print("mask_transposed_kv on L65/f32_asym/1x1: error / bound %.3g, old measure %.1e" % (max(new.values()), max(old.values())))
    assert max(new.values()) > 1.0 and max(old.values()) > P.TOL


def test_f64_scaled_q_is_inside_the_bound():
    """The dropped variant (module docstring): on no case of the 1x1 sweep does it leave the bound."""
    worst = max(max(ratios(name, ("q_scaled_f64",), check=False)[0].values()) for name in P.names(B=1, heads=1, group="len"))
    print("q scaled in float64: worst error / bound %.3f" % worst)
    assert worst <= 1.0


def test_every_case_of_the_issue_is_in_the_sweep():
    assert P.AP.DEC_LENS == (1, 31, 32, 33, 64, 65, 97, 130)
    assert len(P.names(group="len")) == 3 * 2 * len(P.AP.DEC_LENS)
    for pat, Ls in P.PATTERNS:
        assert 65 in Ls and (97 in Ls or 130 in Ls)
        assert len(P.names(pattern=pat)) == 2 * 2 * len(Ls)
    assert [p for p, _ in P.PATTERNS] == ["dn", "last_open", "first_open", "one_pair", "closed_key", "closed_tile"]
    assert len(P.names(pattern="asym")) == 4 and len(P.names(pattern="near_sym")) == 2
    assert P.DEAD == (("row45", 97), ("last_row", 65), ("dead_tile", 97), ("row70", 97)) and len(P.names(group="dead")) == 16
    assert len(P.names(group="stress")) == 2 * 6 and all(P.CASES[n]["L"] == 130 and P.CASES[n]["mask"] == "none" for n in P.names(group="stress"))
    assert sorted({(P.CASES[n]["B"], P.CASES[n]["heads"]) for n in P.names(group="bh")}) == [(1, 7), (7, 1)]
    assert all(P.CASES[n]["group"] == "stress" for n in P.RESIDUE_GROUPS)
    for name in WRONG.values():
        assert name in P.CASES
    # the workspace: delta, B heads roundup(L, 32) floats, rounded up to 256 bytes
    assert P.delta_bytes(1, 1, 1) == 256 and P.delta_bytes(2, 3, 65) == 2304 and P.delta_bytes(2, 2, 40) == 1024
    n_pos, dist = P.large_positive_keys()
    assert 2 <= n_pos < 130 and dist < 1e-5
