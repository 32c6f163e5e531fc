"""Per-entry parity of the re-ID kernels (uninext_amd/csrc/reid.hip: select, scores, loss, the four backward kernels) at their
block, wave and rank edges: the cases, a float64 restatement written from include/ota_hip.h and the kernels' comments (numpy
only, nothing of uninext_amd/reid.py), the exact restatement of the selection (oracle/ota_oracle.py's dynamic_k behind a thin
wrapper), the fp32 PyTorch composition and the error measure.  No GPU is needed to import this.
tests/test_reid_parity_cpu.py checks the conditions the cases claim, pins the restatements and shows that the measure has
teeth; tests/test_reid_parity_gpu.py holds the kernels to it.

Inputs are dyadic, so float64 sees exactly what fp32 holds: embeddings, hand-built dot and cos are multiples of 2^-10; IoUs are
multiples of 2^-10 in [0, 1] (a candidate sum of up to 100 of them is exact in fp32 in any order, so a case can sit exactly on an
integer k); costs are multiples of 2^-6 below 64 (the + 10000 and the first + 100000 are exact).  The named exceptions: the
sub-eps rows (one entry of 2^-45, the rest 0: norm 2^-45 < kNormEps = 1e-12f), the merge pair of the selection (5 and 5 + 2^-10:
closer than the spacing 2^-7 at 1e5) with the +inf that keeps the other rows out of that column, and the planted NaNs.

The batch layout is include/ota_hip.h's: image b owns targets off[b] .. off[b + 1] - 1, its [Q, G_b] block starts at Q * off[b].

The magnitude s of every float output (units of u = 2^-24, to first order, nothing fitted; the bound is entry_bound(comp_err, s)
of tests/parity_measure.py = max(COMP_MARGIN x the fp32 composition's error at the entry, SUM_DEPTH u s), and on top the
project's 1e-4 max(1, max|ref|)).  C channels, n items, m the items of an image or of a key row, eps = 1e-12f:
  * dot: one chain of C terms, (C + 2) S with S = sum |r_c| |k_c| (test_scores_entry_by_entry_against_float64)      =: E_d
  * a norm: |x|^2 is a sum of C non-negative terms, (C + 2) of itself; the root halves that and rounds once: (C / 2 + 2) |x|
  * cos = dot / (max(|r|, eps) max(|k|, eps)): E_d / den + |cos| (C + 8)                                            =: E_c
    (a hand-built dot or cos is exact: E_d = E_c = 0)
  * the maxima mn = max over the negatives of d, mp = max over the positives of -d: exact maxima of inexact numbers,
    E_mn = max over the set of E_d
  * a shifted exponential t_j = exp(d_j - mn): the argument rounds once, expf is good to 2 u: g_j = |d_j - mn| + 2, and d_j
    moves by E_dj.  S_neg = sum of n_neg such terms carries n_neg of itself and is NOT shift invariant:
        s(S_neg) = sum_j t_j (g_j + E_dj) + S_neg E_mn + n_neg S_neg                 A_neg := sum_j t_j (g_j + E_dj) / S_neg
  * t = mn + mp + log S_neg + log S_pos IS shift invariant; formed in fp32 it rounds at every term:
        s(t) = A_neg + n_neg + A_pos + n_pos + |mn| + |mp| + |log S_neg| + |log S_pos| + |t|
    term = softplus(t): sigma s(t) + 2 term;  sigma = sigmoid(t): s(sigma) = sigma (1 - sigma) s(t) + 2 sigma
  * sigma / S: (s(sigma) + sigma s(S) / S + sigma) / S
  * the auxiliary term, the mean of n_aux squares (c - label)^2: each square carries 2 |c - label| E_c + 3 of itself, the sum
    n_aux of itself, the division one more
  * a loss: the mean of n terms: sum s(term_i) / n + (n + 1) |loss|
  * gd = (sigma p_q [negative] - sigma p'_q [positive]) (grad0 / n) with p_q = t_q / S_neg, a softmax entry (shift invariant):
        s(sigma p_q) = p_q s(sigma) + sigma p_q (E_dq + g_q + A_neg + n_neg + 3);      s(gd) = |grad0 / n| (sum + 3 |raw|)
  * gc = ec (2 / n_aux) (grad1 / n), ec = (c - 1) [positive] + c [sampled]: s(ec) = (roles) E_c + |ec|, s(gc) = |w1| s(ec) + 4 |gc|
  * coef0 = gd + gc / den, den = max(|r|, eps) max(|k|, eps) carrying (C + 5) den:  s = s(gd) + s(gc) / den + |gc / den| (C + 6) + |coef0|
    coef1 = gc c:  s = s(gc) |c| + |gc| E_c + |coef1|
  * grad_ref[b, q] = sum over the image's m items (ascending) of coef0 k_i  -  [|r| > eps] (sum coef1) / |r|^2 r:
        sum_i (s(coef0_i) |k_i| + (m + 1) |coef0_i k_i|)  +  (s(O) / |r|^2 + |f| (C + 6)) |r| + |f r| + |result|,
        O = sum_i coef1_i carrying sum_i s(coef1_i) + m sum_i |coef1_i|, f = -O / |r|^2
    key_item_grad[i] the same over the Q queries (any order: depth Q) with k and |k| in the second term
  * grad_key[b, k] = the m item rows on key row k in ascending item order: sum s(row) + m sum |row|
An entry whose reference is exactly 0 with s = 0 (an unreferenced key row, a reference row of an image without items, a role-less
coefficient) has bound 0: it must be exactly 0.  Where the fp32 composition is not finite at a finite reference entry, its term
is dropped for that entry and the derived term stands alone.  Entries the contract leaves unwritten are excluded BY NAME
(unwritten()): ref_norm of an image without a valid target, key_norm of an invalid target.

What the measure can and cannot see: E_d carries the worst-case depth C + 2 and everything downstream inherits it through the
exponentials, so at C = 512 a gradient's bound is several 1e-3 of the entry; the measure rejects STRUCTURAL mistakes per entry
(the mutants of tests/test_reid_parity_cpu.py), not 1e-4-relative ones.  It is per entry, which is what the aggregate
scaled_error of tests/test_reid_gpu.py is not: a row thousands of times smaller than the largest is held to its own size.
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import ota_oracle as O                                          # noqa: E402
import parity_measure as PM                                                 # noqa: E402
from parity_measure import COMP_MARGIN, SUM_DEPTH, U, entry_bound          # noqa: E402,F401

F32, F64 = np.float32, np.float64
TOL = 1e-4                                  # tests/reid_cases.py: TOLERANCE
STEP = 1024.0
EPS = float(F32(1e-12))                     # kNormEps, the fp32 number
TINY = 2.0 ** -45                           # the norm of a sub-eps row
STATS = ("term", "aux", "max_neg", "max_pos", "sig_over_sneg", "sig_over_spos")
META = 5


_rng, dy, is_dyadic = PM.rng, PM.dy, PM.is_dyadic        # seeded by name; float32 multiples of 2^-10 (never -0.0)


def offsets(sizes):
    return np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)


def block(flat, off, Q, b):
    """image b's [Q, G_b] view of a flat array in the batch layout"""
    return flat[Q * off[b]:Q * off[b + 1]].reshape(Q, off[b + 1] - off[b])


def pack(blocks, dtype):
    return np.concatenate([np.asarray(x, dtype=dtype).reshape(-1) for x in blocks] + [np.zeros(0, dtype)])


def key_row(key_index, target, Qk):
    k = int(key_index[target])
    if k < 0:
        k += Qk
    return min(max(k, 0), Qk - 1)


def num_sample_neg(n_pos, n_neg):
    """pos_neg_select.py:76-81, never more than there are"""
    return min(10 if n_pos == 0 else (n_neg if n_pos * 10 >= n_neg else n_pos * 10), n_neg)


# ============================================================================================================ selection, exactly

def select_exact(cost, iou, flags, valid, max_rounds=10000, carry=True):
    """One image, hand-built: cost, iou fp32 [Q, G], flags uint8 [Q, G], valid [G].  The background penalty once (a query that is
    foreground for no VALID target), the valid columns compacted, oracle.dynamic_k with 10 and then 100 candidates on the ONE
    matrix, the result scattered back.  -> None without a valid target, else dict(pos, neg uint8 [Q, G], n_pos, n_neg [G] (-1
    for invalid targets), status (bits 2 and 4), cost: the valid columns as the two runs leave them, repaired: the first run's
    repair loop ran).  carry=False runs the second assignment on a fresh matrix: NOT the contract, only to show dependence."""
    valid = np.asarray(valid).astype(bool)
    Q, G = cost.shape
    if not valid.any():
        return None
    c, i, f = cost[:, valid].astype(F32), iou[:, valid].astype(F32), flags[:, valid].astype(np.uint8)
    fg = (f & 1).any(1)
    with np.errstate(invalid="ignore"):
        c[~fg] = c[~fg] + O.BG_PENALTY
    start = c.copy()
    f = f | 1                                                     # (every row foreground: the oracle does not add it again)
    _, _, _, m_pos, st1 = O.dynamic_k(c, i, f, max_rounds=max_rounds, candidates=10)
    repaired = not np.array_equal(start, c, equal_nan=True)
    if not carry:
        c = start.copy()
    _, _, _, m_neg, st2 = O.dynamic_k(c, i, f, max_rounds=max_rounds, candidates=100)
    pos, neg = np.zeros((Q, G), np.uint8), np.zeros((Q, G), np.uint8)
    pos[:, valid], neg[:, valid] = m_pos, m_neg
    n_pos, n_neg = np.full(G, -1, np.int64), np.full(G, -1, np.int64)
    n_pos[valid], n_neg[valid] = m_pos.sum(0), Q - m_neg.sum(0)
    return dict(pos=pos, neg=neg, n_pos=n_pos, n_neg=n_neg, status=int(st1 | st2), first_status=int(st1), second_status=int(st2), cost=c,
                repaired=repaired)


def select_batch(x, carry=True):
    """The whole batch of a selection case: dict(pos, neg flat uint8, counts int32 [G_total, 2], status int32 [bs],
    cost: per image the valid columns after both runs or None)."""
    Q, Qk, off = x["Q"], x["Qk"], x["off"]
    pos, neg, cost = [], [], []
    counts = np.full((off[-1], 2), -1, np.int32)
    status = np.zeros(len(x["images"]), np.int32)
    for b, im in enumerate(x["images"]):
        G = off[b + 1] - off[b]
        r = select_exact(im["cost"], im["iou"], im["flags"], im["valid"], x["max_rounds"], carry) if G else None
        if r is None:
            pos.append(np.zeros((Q, G), np.uint8)); neg.append(np.zeros((Q, G), np.uint8)); cost.append(None)
            continue
        pos.append(r["pos"]); neg.append(r["neg"]); cost.append(r["cost"])
        counts[off[b]:off[b + 1], 0], counts[off[b]:off[b + 1], 1] = r["n_pos"], r["n_neg"]
        bad = any(not -Qk <= int(k) < Qk for k, v in zip(im["keys"], im["valid"]) if v)
        status[b] = r["status"] | (8 if bad else 0)
    return dict(pos=pack(pos, np.uint8), neg=pack(neg, np.uint8), counts=counts, status=status, cost=cost)


def base_image(g, Q, G, near=12, valid=None, keys=None):
    """IoUs below 0.05 and costs in [8, 64) everywhere; per target `near` queries with an IoU in [0.29, 0.9), a cost below 8
    and the foreground bit.  The targets' query sets overlap freely: conflicts and repairs come by themselves."""
    iou = g.randint(0, 52, (Q, G)) / STEP
    cost = g.randint(8 * 64, 64 * 64, (Q, G)) / 64.0
    flags = np.zeros((Q, G), np.uint8)
    for t in range(G):
        rows = g.choice(Q, min(near, Q), replace=False)
        iou[rows, t] = g.randint(300, 920, len(rows)) / STEP
        cost[rows, t] = g.randint(0, 8 * 64, len(rows)) / 64.0
        flags[rows, t] = 1
        top = int(np.argmax(iou[:, t])) if Q else 0
        while any(float(np.sort(iou[:, t])[::-1][:k].sum()).is_integer() for k in (10, 100)):
            iou[top, t] += 1 / STEP                 # (a sum on an integer only where a case plants one)
    return dict(cost=cost.astype(F32), iou=iou.astype(F32), flags=flags, valid=np.ones(G, np.uint8) if valid is None else np.asarray(valid, np.uint8),
                keys=np.asarray(g.randint(0, 8, G) if keys is None else keys, np.int64), plain=True)


def _pattern(kind, G):
    v = np.zeros(G, np.uint8)
    if kind == "first":
        v[0] = 1
    elif kind == "last":
        v[-1] = 1
    elif kind == "alt":
        v[::2] = 1
    elif kind == "all":
        v[:] = 1
    else:
        assert kind == "none"
    return v


INT_ROWS = (3, 17, 64, 65, 80, 99)              # the six IoUs of 0.5 of the integer-sum columns
TIE_ROWS = (7, 20, 33, 41)                      # four equal costs around a k of 3
MERGE_A, MERGE_B = 10, 20


def plant_intsum(g, Q):
    """column 0: six IoUs of 0.5, nothing else: the sum is exactly 3 with 10 and with 100 candidates; column 1: one of them
    2^-10 lower: 3 - 2^-10, k = 2; column 2 is plain"""
    im = base_image(g, Q, 3)
    im["iou"][:, :2] = 0
    im["iou"][list(INT_ROWS), 0] = 0.5
    im["iou"][list(INT_ROWS), 1] = 0.5
    im["iou"][INT_ROWS[2], 1] = 0.5 - 1 / STEP
    im["plain"] = False
    return im


def plant_tie_iou(g, Q):
    """column 0: fifteen IoUs of 0.25 and nothing else: the cut after 10 candidates runs through equal values (2.5, k = 2; with
    100 candidates 3.75, k = 3)"""
    im = base_image(g, Q, 2)
    im["iou"][:, 0] = 0
    im["iou"][5:95:6, 0] = 0.25
    im["plain"] = False
    return im


def plant_tie_cost(g, Q):
    """every query foreground.  column 0: k = 3 and four costs of 1.0 at TIE_ROWS: the three lowest rows win the top-k.
    columns 1 and 2: k = 1 and both cheapest at row 50 with cost 2.0: the row keeps column 1 (argmin); column 2 is repaired and
    finds 3.0 at rows 60 and 70: row 60."""
    im = base_image(g, Q, 3, near=0)
    im["flags"][:] = 1
    im["iou"][:] = 0
    im["iou"][list(INT_ROWS), 0] = 0.5
    im["cost"][list(TIE_ROWS), 0] = 1.0
    im["cost"][50, 1:] = 2.0
    im["cost"][[60, 70], 2] = 3.0
    im["plain"] = False
    return im


def plant_merge(g, Q):
    """every query foreground, every k = 1.  Column 0 takes row B, column 1 row A; column 2 holds 5 + 2^-10 at A, 5 at B and +inf
    elsewhere: it claims B, loses it to column 0, and is repaired after both rows took + 100000 -- where the two costs are one
    number, and the lower row A wins.  Without the merge it would be B."""
    im = base_image(g, Q, 3, near=0)
    im["flags"][:] = 1
    im["iou"][:] = 0
    im["cost"][MERGE_B, 0] = 1.0
    im["cost"][MERGE_A, 1] = 1.0
    im["cost"][:, 2] = np.inf
    im["cost"][MERGE_A, 2], im["cost"][MERGE_B, 2] = 5.0 + 1 / STEP, 5.0
    im["plain"] = False
    return im


def plant_dup(g, Q):
    """column 1 is column 0 again: after the conflict resolution one of them has no query, the repair loop runs in the first run"""
    im = base_image(g, Q, 4)
    for k in ("cost", "iou", "flags"):
        im[k][:, 1] = im[k][:, 0]
    return im


def plant_nan(g, Q):
    """a NaN IoU in column 0 (k = 1), a row of NaN costs, NaN costs in column 2"""
    im = base_image(g, Q, 4)
    im["iou"][5, 0] = np.nan
    im["cost"][7, :] = np.nan
    im["cost"][[9, 30], 2] = np.nan
    im["plain"] = False
    return im


SPLIT_ROWS = (30, 40, 50)


def plant_split(g, Q, second):
    """For max_rounds = 0: status bit 2 from ONE run alone.  Every query foreground; both columns' cheapest row is 40 and it is
    cheaper in column 0, so wherever both claim it column 1 loses it and would need a repair.
    second=True: column 0 has k = 1 over 10 candidates (1.25) and k = 2 over 100 (2.65625) and its cheapest row is 30, row 40 its
    second: the first run has no conflict (status 0), the second cuts column 1's repair off (status 2).
    second=False: column 0 has k = 1 throughout and takes row 40 in both runs; column 1 has k = 1 and then k = 2 with row 50 its
    second: the first run is cut off (2), in the second column 1 keeps row 50 and nothing needs a repair (0)."""
    im = base_image(g, Q, 2, near=0)
    im["flags"][:] = 1
    im["iou"][:] = 0
    wide = 0 if second else 1
    im["iou"][:, wide] = 1 / 64.0
    im["iou"][:10, wide] = 0.125
    r30, r40, r50 = SPLIT_ROWS
    im["cost"][r40, 0], im["cost"][r40, 1] = 1.5, 2.0
    if second:
        im["cost"][r30, 0] = 1.0
    else:
        im["cost"][r50, 1] = 3.0
    im["plain"] = False
    return im


def _keys_flags(g, Q, Qk):
    a = base_image(g, Q, 3, valid=[1, 0, 1], keys=[-1, 999, -Qk])       # negative indices; the invalid target's index is not looked at
    a["flags"][11, 1] |= 2                                              # a degenerate pair in an INVALID column: no bit 4
    b = base_image(g, Q, 2, keys=[Qk, 0])                               # one past the key rows: bit 8
    c = base_image(g, Q, 2, keys=[0, 1])
    c["flags"][13, 1] |= 2                                              # in a valid column: bit 4
    d = base_image(g, Q, 2, keys=[-Qk - 1, 0])                          # one before: bit 8
    return [a, b, c, d]


SELECT = {
    "q100_g1_16_17_33": dict(Q=100, build=lambda g, Q: [base_image(g, Q, G) for G in (1, 16, 17, 33)]),
    "q128_valid_patterns": dict(Q=128, build=lambda g, Q: [base_image(g, Q, 16, valid=_pattern("first", 16)), base_image(g, Q, 17, valid=_pattern("last", 17)),
                                                           base_image(g, Q, 33, valid=_pattern("alt", 33)), base_image(g, Q, 16, valid=_pattern("none", 16)),
                                                           base_image(g, Q, 1)]),
    "q1024_g17_33": dict(Q=1024, build=lambda g, Q: [base_image(g, Q, 17), base_image(g, Q, 33, near=40)]),
    "q1025_g16_1": dict(Q=1025, build=lambda g, Q: [base_image(g, Q, 16, near=40), base_image(g, Q, 1, near=120)]),
    "q100_batch64": dict(Q=100, build=lambda g, Q: [base_image(g, Q, (b * 7) % 4) for b in range(64)]),
    "q100_plants": dict(Q=100, build=lambda g, Q: [plant_intsum(g, Q), plant_tie_iou(g, Q), plant_tie_cost(g, Q), plant_merge(g, Q), plant_nan(g, Q)]),
    "q100_dup": dict(Q=100, build=lambda g, Q: [plant_dup(g, Q)]),
    "q100_dup_rounds0": dict(Q=100, seed="q100_dup", max_rounds=0, build=lambda g, Q: [plant_dup(g, Q)]),
    "q100_dup_rounds1": dict(Q=100, seed="q100_dup", max_rounds=1, build=lambda g, Q: [plant_dup(g, Q)]),
    "q100_split_rounds0": dict(Q=100, max_rounds=0, build=lambda g, Q: [plant_split(g, Q, True), plant_split(g, Q, False)]),
    "q100_keys_flags": dict(Q=100, build=lambda g, Q: _keys_flags(g, Q, 8)),
}
SELECT_QS, SELECT_GS = (100, 128, 1024, 1025), (1, 16, 17, 33)
MAX_ROUNDS = 50             # (both sides cut a repair loop off at the same round, so nothing hangs on a case that would spin)


@functools.lru_cache(maxsize=None)
def select_inputs(name):
    c = SELECT[name]
    images = c["build"](_rng("select/" + c.get("seed", name)), c["Q"])
    sizes = [im["cost"].shape[1] for im in images]
    return dict(Q=c["Q"], Qk=8, images=images, sizes=sizes, off=offsets(sizes), max_rounds=c.get("max_rounds", MAX_ROUNDS))


@functools.lru_cache(maxsize=None)
def select_expected(name):
    return select_batch(select_inputs(name))


# ======================================================================================================= the float problems

def _roles_and_ranks(g, Q, mpos, mneg):
    """ranks of the sampled negatives of one column, n_aux"""
    n_pos, n_neg = int((mpos & 1).sum()), int((mneg == 0).sum())
    k = num_sample_neg(n_pos, n_neg)
    return g.choice(n_neg, k, replace=False).astype(np.int32) if k else np.zeros(0, np.int32), n_pos + k


def _embed_problem(name, Q, C, Qk, images, grads, special):
    """ref [bs, Q, C], key [bs, Qk, C] dyadic; per image valid and keys; hand-built matching columns; one item per valid target.
    special: None, or the image whose key rows Qk - 1 (zeros) and 1 (norm 2^-45) are planted -- the image whose targets point at
    them; the last image's reference rows 0 (zeros) and 1 (2^-45)."""
    g = _rng("embed/" + name)
    bs = len(images)
    sizes = [len(im["valid"]) for im in images]
    off = offsets(sizes)
    ref, key = dy(0.5 * g.standard_normal((bs, Q, C))), dy(0.5 * g.standard_normal((bs, Qk, C)))
    zero_rows = dict(ref=[], key=[])
    if special is not None:
        key[special, Qk - 1] = 0
        key[special, 1] = 0
        key[special, 1, C // 2] = TINY
        zero_rows["key"] = [(special, Qk - 1), (special, 1)]
        if Q >= 4:
            ref[bs - 1, 0] = 0
            ref[bs - 1, 1] = 0
            ref[bs - 1, 1, 3] = TINY
            zero_rows["ref"] = [(bs - 1, 0), (bs - 1, 1)]
    valid = pack([im["valid"] for im in images], np.uint8)
    keys = pack([im["keys"] for im in images], np.int64)
    mpos, mneg, meta, ranks, counts = [], [], [], [], []
    for b, im in enumerate(images):
        G = sizes[b]
        p = (g.rand(Q, G) < 0.15).astype(np.uint8)
        n = (p | (g.rand(Q, G) < 0.3)).astype(np.uint8)
        p, n = p * np.asarray(im["valid"], np.uint8)[None, :], n * np.asarray(im["valid"], np.uint8)[None, :]
        count = 0
        for t in range(G):
            if not im["valid"][t]:
                continue
            if special is not None and b == bs - 1 and Q >= 4:                          # the zero row a positive, the sub-eps row a negative
                p[0, t], n[0, t], p[1, t], n[1, t] = 1, 1, 0, 0
            if not (p[:, t] & 1).any() and n[:, t].all():                   # (no role at all: the mean of nothing)
                n[0, t] = 0
            drawn, n_aux = _roles_and_ranks(g, Q, p[:, t], n[:, t])
            if special is not None and b == bs - 1 and Q >= 4 and int((n[:1, t] == 0).sum()) not in drawn.tolist():
                drawn[0] = int((n[:1, t] == 0).sum())                       # the sub-eps row's rank: it is sampled
            meta.append((b, off[b] + t, len(ranks), len(drawn), n_aux))
            ranks.extend(drawn.tolist())
            count += 1
        mpos.append(p); mneg.append(n); counts.append(count)
    return dict(name=name, Q=Q, Qk=Qk, C=C, sizes=sizes, off=off, ref=ref, key=key, valid=valid, keys=keys, mpos=pack(mpos, np.uint8),
                mneg=pack(mneg, np.uint8), meta=np.asarray(meta, np.int32).reshape(-1, META), ranks=np.asarray(ranks or [0], np.int32),
                item_counts=counts, grads=np.asarray(grads, F32), zero_rows=zero_rows, hand_scores=False)


def _img(valid, keys):
    return dict(valid=list(valid), keys=list(keys))


QK = 6
# three images with an item-less one in the middle; an invalid target first (first_valid = 1); items 0 and 1 share key row 3,
# item 2 has the zero key row through index -1, item 3 the sub-eps one; the last image's three items share key row 2 (once as -4)
_BWD_IMAGES = [_img([0, 1, 1, 1, 1], [0, 3, 3, -1, 1]), _img([0], [0]), _img([1, 1, 1], [2, 2 - QK, 2])]
BACKWARD = {"q%d_c%d_g%g_%g" % (Q, C, g0, g1): dict(Q=Q, C=C, grads=(g0, g1))
            for Q, C, g0, g1 in ((1, 64, 1, 2), (4, 192, 0, 1), (5, 512, 1, 0), (257, 64, 0, 1), (257, 192, 1, 0), (257, 512, 1, 2))}
BACKWARD_QS, BACKWARD_CS, BACKWARD_GRADS = (1, 4, 5, 257), (64, 192, 512), ((1, 2), (0, 1), (1, 0))


def _score_images(g, sizes):
    out = []
    for G in sizes:
        valid = [1] * G
        keys = g.randint(-QK, QK, G).tolist()
        if G >= 16:
            valid[0], valid[5] = 0, 0                                       # an invalid target first: first_valid is not 0
            keys[2], keys[3], keys[4], keys[6] = QK - 1, 1, 4, 4 - QK       # the zero key row, the sub-eps one, two targets on row 4
        out.append(_img(valid, keys))
    return out


SCORES = {"q1_c64_g1": (1, 64, (1,)), "q15_c192_g16": (15, 192, (16,)), "q16_c512_g17": (16, 512, (17,)), "q17_c64_g17_1": (17, 64, (17, 1)),
          "q33_c192_g16_17": (33, 192, (16, 17)), "q33_c512_g1_16": (33, 512, (1, 16))}
SCORE_QS, SCORE_CS, SCORE_GS = (1, 15, 16, 17, 33), (64, 192, 512), (1, 16, 17)


@functools.lru_cache(maxsize=None)
def problem(kind, name):
    """The inputs of one float case: kind "scores", "backward" or "loss".  Left unchanged by its callers."""
    if kind == "backward":
        c = BACKWARD[name]
        return _embed_problem("backward/" + name, c["Q"], c["C"], QK, _BWD_IMAGES, c["grads"], 0)
    if kind == "scores":
        Q, C, sizes = SCORES[name]
        return _embed_problem("scores/" + name, Q, C, QK, _score_images(_rng("scoreimg/" + name), sizes), (1, 1),
                              int(np.argmax(np.asarray(sizes) >= 16)) if max(sizes) >= 16 else None)
    assert kind == "loss"
    return _loss_problem(name)


# ---- loss forward: hand-built dot, cos, matchings, items, ranks ------------------------------------------------------------------
POSITIVES = (1, 5, 61, 130, 253, 300)           # item A's positives: they make a negative's rank differ from its query index
EDGE_QUERIES = (0, 63, 64, 255, 256)            # lane 0, lane 63, the first lane of wave 1, the last query of a pass, the first of the next
LOSS = {"q63": dict(Q=63), "q64_nan": dict(Q=64, nan_item=True), "q255_malformed": dict(Q=255, malformed=True), "q256": dict(Q=256),
        "q257_extreme": dict(Q=257, extreme=True), "q513": dict(Q=513), "q513_extreme_malformed": dict(Q=513, extreme=True, malformed=True)}
LOSS_QS = (63, 64, 255, 256, 257, 513)
LOSS_SIZES = (3, 0, 17)
INTERIOR = 8                                    # item D's column of the G = 17 image


def _loss_problem(name):
    c, g = LOSS[name], _rng("loss/" + name)
    Q, sizes = c["Q"], list(LOSS_SIZES)
    off = offsets(sizes)
    span = 80.0 if c.get("extreme") else 8.0
    dot = [dy(g.uniform(-span, span, (Q, G))) for G in sizes]
    cos = [dy(g.uniform(-1, 1, (Q, G))) for G in sizes]
    mpos = [(g.rand(Q, G) < 0.1).astype(np.uint8) for G in sizes]
    mneg = [(p | (g.rand(Q, G) < 0.2)).astype(np.uint8) for p, G in zip(mpos, sizes)]
    meta, ranks, planted = [], [], {}

    def item(b, t, drawn):
        n_pos = int(mpos[b][:, t].sum())
        meta.append((b, off[b] + t, len(ranks), len(drawn), n_pos + len(drawn)))
        ranks.extend(int(r) for r in drawn)

    # A: positives at POSITIVES, everything else a negative but two overlapping queries; the sampled negatives are the edge queries
    pos = [q for q in POSITIVES if q < Q]
    mpos[0][:, 0], mneg[0][:, 0] = 0, 0
    mpos[0][pos, 0], mneg[0][pos, 0] = 1, 1
    mneg[0][[q for q in (2, 66) if q < Q], 0] = 1
    isneg = mneg[0][:, 0] == 0
    edge = sorted({q for q in EDGE_QUERIES if q < Q} | {Q - 1})
    assert all(isneg[q] for q in edge)
    rank_of = np.cumsum(isneg) - 1
    drawn = [int(rank_of[q]) for q in edge]
    assert drawn[-1] == int(isneg.sum()) - 1
    if c.get("extreme"):
        dot[0][0, 0], dot[0][1, 0] = 80.0, -80.0          # a negative of +80 and a positive of -80: e^80 e^80 is no fp32 number
    planted["edge_queries"] = edge
    item(0, 0, g.permutation(drawn))
    # B: no positive
    mpos[0][:, 1] = 0
    item(0, 1, g.choice(int((mneg[0][:, 1] == 0).sum()), 10, replace=False))
    # C: no negative, nothing sampled
    mneg[0][:, 2] = 1
    item(0, 2, [])
    if c.get("malformed"):                                # image 0 with a target of image 2: zero roles and stats
        meta.append((0, off[2] + 5, 0, 3, 5))
    # D: an interior column of the G = 17 image, every negative sampled
    item(2, INTERIOR, g.permutation(int((mneg[2][:, INTERIOR] == 0).sum())))
    # E: nothing sampled; with nan_item no positive either: n_aux = 0, the mean of nothing
    if c.get("nan_item"):
        mpos[2][:, 3] = 0
    else:
        mpos[2][7, 3] = 1
    item(2, 3, [])
    return dict(name=name, Q=Q, sizes=sizes, off=off, dot=pack(dot, F32), cos=pack(cos, F32), mpos=pack(mpos, np.uint8), mneg=pack(mneg, np.uint8),
                meta=np.asarray(meta, np.int32).reshape(-1, META), ranks=np.asarray(ranks or [0], np.int32), planted=planted, hand_scores=True,
                malformed=[i for i, m in enumerate(meta) if not off[m[0]] <= m[1] < off[m[0] + 1]])


# ========================================================================================================== the restatement

def scores64(p, mutant=None):
    """dot, cos [Q * G_total], ref_norm [bs, Q], key_norm [G_total] in float64 and their magnitudes (mag_*).  Unwritten norms
    are NaN.  mutant "first_valid_0": the reference norms are written by target 0's threads only."""
    ref, key = p["ref"].astype(F64), p["key"].astype(F64)
    bs, Q, C = ref.shape
    off, Qk = p["off"], p["Qk"]
    out = {k: np.zeros(Q * off[-1]) for k in ("dot", "cos", "mag_dot", "mag_cos")}
    out.update(ref_norm=np.full((bs, Q), np.nan), key_norm=np.full(off[-1], np.nan), mag_ref_norm=np.zeros((bs, Q)), mag_key_norm=np.zeros(off[-1]))
    for b in range(bs):
        v = p["valid"][off[b]:off[b + 1]]
        if not v.any():
            continue
        nr = np.sqrt((ref[b] * ref[b]).sum(1))
        if not (mutant == "first_valid_0" and not v[0]):
            out["ref_norm"][b], out["mag_ref_norm"][b] = nr, (C / 2 + 2) * nr
        for t in np.flatnonzero(v):
            k = key[b, key_row(p["keys"], off[b] + t, Qk)]
            nk = np.sqrt((k * k).sum())
            d, S = ref[b] @ k, np.abs(ref[b]) @ np.abs(k)
            den = np.maximum(nr, EPS) * max(nk, EPS)
            c = d / den
            block(out["dot"], off, Q, b)[:, t], block(out["mag_dot"], off, Q, b)[:, t] = d, (C + 2) * S
            block(out["cos"], off, Q, b)[:, t], block(out["mag_cos"], off, Q, b)[:, t] = c, (C + 2) * S / den + np.abs(c) * (C + 8)
            out["key_norm"][off[b] + t], out["mag_key_norm"][off[b] + t] = nk, (C / 2 + 2) * nk
    return out


def unwritten(p):
    """BY NAME what ota_reid_scores_hip_f32 leaves unwritten: ref_norm of an image without a valid target, key_norm of an
    invalid target.  -> (ref_norm mask [bs, Q], key_norm mask [G_total])"""
    off = p["off"]
    rows = np.asarray([not p["valid"][off[b]:off[b + 1]].any() for b in range(len(p["sizes"]))])
    return np.repeat(rows[:, None], p["Q"], 1), p["valid"] == 0


def loss64(p, sc=None, mutant=None):
    """roles uint8 [n, Q], stats [n, 6], losses [2] with mag_stats and mag_losses, and per item what the backward needs.  sc:
    scores64's result, or None for the hand-built dot and cos of a loss case.  mutants: "rank_pass" (the rank of a negative
    behind the first 256 queries is one too large), "max_all" (the negatives' maximum taken over every query)."""
    Q, off = p["Q"], p["off"]
    if sc is None:
        dot, cos = p["dot"].astype(F64), p["cos"].astype(F64)
        Ed, Ec = np.zeros_like(dot), np.zeros_like(cos)
    else:
        dot, cos, Ed, Ec = sc["dot"], sc["cos"], sc["mag_dot"], sc["mag_cos"]
    n = len(p["meta"])
    roles, stats, mag, items = np.zeros((n, Q), np.uint8), np.zeros((n, 6)), np.zeros((n, 6)), []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i, (b, tgt, roff, rcnt, n_aux) in enumerate(p["meta"].tolist()):
            b = min(max(b, 0), len(p["sizes"]) - 1)
            t = tgt - off[b]
            if not 0 <= t < off[b + 1] - off[b]:
                items.append(None)
                continue
            d, c, ed, ec = (block(a, off, Q, b)[:, t] for a in (dot, cos, Ed, Ec))
            isneg, ispos = block(p["mneg"], off, Q, b)[:, t] == 0, (block(p["mpos"], off, Q, b)[:, t] & 1) != 0
            rank = np.cumsum(isneg) - isneg
            if mutant == "rank_pass":
                rank[256:] += 1
            flag = np.zeros(Q + 2, bool)
            for r in p["ranks"][roff:roff + rcnt]:
                if 0 <= r < Q:
                    flag[r] = True
            sampled = isneg & flag[np.minimum(rank, Q + 1)]
            roles[i] = ispos * 1 + isneg * 2 + sampled * 4
            n_neg, n_pos = int(isneg.sum()), int(ispos.sum())
            mn = d[isneg].max() if n_neg else -np.inf
            mp = (-d[ispos]).max() if n_pos else -np.inf
            if mutant == "max_all":
                mn = d.max()
            e_mn, e_mp = (ed[isneg].max() if n_neg else 0.0), (ed[ispos].max() if n_pos else 0.0)
            tn, tp = np.where(isneg, np.exp(d - mn), 0.0), np.where(ispos, np.exp(-d - mp), 0.0)
            gn, gp = np.abs(d - mn) + 2.0, np.abs(-d - mp) + 2.0
            sn, sp = tn.sum(), tp.sum()
            An = (tn * np.where(isneg, gn + ed, 0.0)).sum() / sn if sn > 0 else 0.0
            Ap = (tp * np.where(ispos, gp + ed, 0.0)).sum() / sp if sp > 0 else 0.0
            s_sn, s_sp = sn * (An + e_mn + n_neg), sp * (Ap + e_mp + n_pos)
            term = sig = s_t = 0.0
            if sn > 0 and sp > 0:
                tt = mn + mp + np.log(sn) + np.log(sp)
                term = max(tt, 0.0) + np.log1p(np.exp(-abs(tt)))
                sig = 1.0 / (1.0 + np.exp(-tt))
                s_t = An + n_neg + Ap + n_pos + abs(mn) + abs(mp) + abs(np.log(sn)) + abs(np.log(sp)) + abs(tt)
            s_sig = sig * (1 - sig) * s_t + 2 * sig
            sq = np.where(ispos, (c - 1) ** 2, 0.0) + np.where(sampled, c * c, 0.0)
            s_sq = np.where(ispos, 2 * np.abs(c - 1) * ec + 3 * (c - 1) ** 2, 0.0) + np.where(sampled, 2 * np.abs(c) * ec + 3 * c * c, 0.0)
            aux = F64(sq.sum()) / F64(n_aux)
            stats[i] = (term, aux, mn, mp, sig / sn if sn > 0 else 0.0, sig / sp if sp > 0 else 0.0)
            mag[i] = (sig * s_t + 2 * term, F64(s_sq.sum()) / F64(n_aux) + (n_aux + 1) * abs(aux), e_mn, e_mp,
                      (s_sig + sig * s_sn / sn + sig) / sn if sn > 0 else 0.0, (s_sig + sig * s_sp / sp + sig) / sp if sp > 0 else 0.0)
            items.append(dict(b=b, t=t, target=tgt, n_aux=n_aux, isneg=isneg, ispos=ispos, sampled=sampled, sig=sig, s_sig=s_sig,
                              pn=tn / sn if sn > 0 else tn, pp=tp / sp if sp > 0 else tp, gn=gn, gp=gp, An=An, Ap=Ap, n_neg=n_neg, n_pos=n_pos))
        losses = stats[:, :2].sum(0) / n
        mag_losses = mag[:, :2].sum(0) / n + (n + 1) * np.abs(losses)
    return dict(roles=roles, stats=stats, mag_stats=mag, losses=losses, mag_losses=mag_losses, items=items)


def backward64(p, sc, ls, grads=None, mutant=None):
    """coef [2, n, Q], key_item_grad [n, C], grad_ref [bs, Q, C], grad_key [bs, Qk, C] in float64 with their magnitudes.
    mutants: "drop_own" (the own-norm term of both gradients dropped), "key_wrong_row" (an item's key gradient added to the
    key row of the item before it)."""
    ref, key = p["ref"].astype(F64), p["key"].astype(F64)
    bs, Q, C = ref.shape
    off, Qk, n = p["off"], p["Qk"], len(p["meta"])
    g0, g1 = (float(v) for v in (p["grads"] if grads is None else grads))
    coef, s_coef = np.zeros((2, n, Q)), np.zeros((2, n, Q))
    kig, s_kig = np.zeros((n, C)), np.zeros((n, C))
    gref, s_gref = np.zeros((bs, Q, C)), np.zeros((bs, Q, C))
    gkey, s_gkey = np.zeros((bs, Qk, C)), np.zeros((bs, Qk, C))
    nr_all = np.sqrt((ref * ref).sum(2))
    rows = []
    for i, it in enumerate(ls["items"]):
        if it is None:
            rows.append(None)
            continue
        b, t = it["b"], it["t"]
        row = key_row(p["keys"], it["target"], Qk)
        rows.append((b, row))
        k = key[b, row]
        nk = np.sqrt((k * k).sum())
        d, c, ed, ec = (block(a, off, Q, b)[:, t] for a in (sc["dot"], sc["cos"], sc["mag_dot"], sc["mag_cos"]))
        sig, s_sig = it["sig"], it["s_sig"]
        neg, pos = sig * it["pn"], sig * it["pp"]
        with np.errstate(invalid="ignore"):             # (0 x inf in the unselected branch of a set that is empty)
            s_neg = np.where(it["isneg"], it["pn"] * s_sig + neg * (ed + it["gn"] + it["An"] + it["n_neg"] + 3), 0.0)
            s_pos = np.where(it["ispos"], it["pp"] * s_sig + pos * (ed + it["gp"] + it["Ap"] + it["n_pos"] + 3), 0.0)
        raw = neg - pos
        w0 = g0 / n
        gd, s_gd = raw * w0, abs(w0) * (s_neg + s_pos + 3 * np.abs(raw))
        ecv = np.where(it["ispos"], c - 1, 0.0) + np.where(it["sampled"], c, 0.0)
        n_roles = it["ispos"].astype(F64) + it["sampled"]
        w1 = (2.0 / it["n_aux"]) * (g1 / n) if it["n_aux"] else 0.0
        gc, s_gc = ecv * w1, abs(w1) * (n_roles * ec + np.abs(ecv)) + 4 * np.abs(ecv * w1)
        den = np.maximum(nr_all[b], EPS) * max(nk, EPS)
        a = gd + gc / den
        own = gc * c
        coef[0, i], coef[1, i] = a, own
        s_coef[0, i] = s_gd + s_gc / den + np.abs(gc / den) * (C + 6) + np.abs(a)
        s_coef[1, i] = s_gc * np.abs(c) + np.abs(gc) * ec + np.abs(own)
        if mutant == "drop_own":
            own = np.zeros(Q)
        total, s_total = a @ ref[b], s_coef[0, i] @ np.abs(ref[b]) + (Q + 1) * (np.abs(a) @ np.abs(ref[b]))
        Osum, s_O = own.sum(), s_coef[1, i].sum() + Q * np.abs(own).sum()
        f, s_f = (-Osum / nk ** 2, s_O / nk ** 2) if nk > EPS else (0.0, 0.0)
        kig[i] = total + f * k
        s_kig[i] = s_total + (s_f + abs(f) * (C + 6)) * np.abs(k) + np.abs(f * k) + np.abs(kig[i])
    for b in range(bs):
        mine = [i for i, r in enumerate(rows) if r is not None and r[0] == b]
        m = len(mine)
        if not m:
            continue
        acc, s_acc, Osum, s_O, absO = np.zeros((Q, C)), np.zeros((Q, C)), np.zeros(Q), np.zeros(Q), np.zeros(Q)
        for i in mine:
            k = key[b, rows[i][1]]
            acc += coef[0, i][:, None] * k[None, :]
            s_acc += s_coef[0, i][:, None] * np.abs(k)[None, :] + (m + 1) * np.abs(coef[0, i])[:, None] * np.abs(k)[None, :]
            if mutant != "drop_own":
                Osum += coef[1, i]
            s_O += s_coef[1, i]
            absO += np.abs(coef[1, i])
        nr = nr_all[b]
        live = nr > EPS
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(live, -Osum / nr ** 2, 0.0)
            s_f = np.where(live, (s_O + m * absO) / nr ** 2, 0.0)
        gref[b] = acc + f[:, None] * ref[b]
        s_gref[b] = s_acc + (s_f + np.abs(f) * (C + 6))[:, None] * np.abs(ref[b]) + np.abs(f[:, None] * ref[b]) + np.abs(gref[b])
        for j, i in enumerate(mine):
            row = rows[mine[j - 1]][1] if mutant == "key_wrong_row" and j else rows[i][1]
            gkey[b, row] += kig[i]
        for row in {rows[i][1] for i in mine}:
            on = [i for i in mine if rows[i][1] == row]
            s_gkey[b, row] = s_kig[on].sum(0) + len(on) * np.abs(kig[on]).sum(0)
    return dict(coef=coef, mag_coef=s_coef, key_item_grad=kig, mag_key_item_grad=s_kig, grad_ref=gref, mag_grad_ref=s_gref, grad_key=gkey,
                mag_grad_key=s_gkey, rows=rows)


@functools.lru_cache(maxsize=None)
def reference(kind, name):
    """dict(sc, ls, bw) of a case: what its kind has"""
    p = problem(kind, name)
    if kind == "loss":
        return dict(sc=None, ls=loss64(p), bw=None)
    sc = scores64(p)
    ls = loss64(p, sc)
    return dict(sc=sc, ls=ls, bw=backward64(p, sc, ls) if kind == "backward" else None)


def key_sum32(key_item_grad, p, rows):
    """grad_key from the KERNEL's key_item_grad by float32 adds in ascending item order: the one sum whose order is contract"""
    out = np.zeros((len(p["sizes"]), p["Qk"], p["C"]), F32)
    for i, r in enumerate(rows):
        if r is not None:
            out[r[0], r[1]] = out[r[0], r[1]] + key_item_grad[i].astype(F32)
    return out


# ================================================================================================== the fp32 PyTorch composition

def composition(p, roles, device="cpu", grads=None):
    """The same formulas in fp32 PyTorch on `device`, as float64 numpy: dot, cos, ref_norm, key_norm (not for a hand-built loss
    case), stats, losses, and with an embedding problem coef, key_item_grad and by autograd grad_ref and grad_key.  `roles`: the
    restatement's (integers, the composition does not re-derive them).  It never runs the kernels."""
    import torch
    Q, off, n = p["Q"], p["off"], len(p["meta"])
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(device)
    out = {}
    hand = p["hand_scores"]
    if hand:
        dot, cos = t32(p["dot"]), t32(p["cos"])
    else:
        ref, key = t32(p["ref"]).requires_grad_(True), t32(p["key"]).requires_grad_(True)
        bs, Qk, C = ref.shape[0], p["Qk"], p["C"]
        nr = ref.norm(dim=2)
        dot_b, cos_b, krows = {}, {}, {}
        out.update(dot=np.zeros(Q * off[-1]), cos=np.zeros(Q * off[-1]), ref_norm=nr.detach().cpu().double().numpy(), key_norm=np.zeros(off[-1]))
        for b in range(bs):
            for t in np.flatnonzero(p["valid"][off[b]:off[b + 1]]):
                kr = key[b, key_row(p["keys"], off[b] + t, Qk)] + 0
                kr.retain_grad()
                nk = kr.norm()
                d = ref[b] @ kr
                c = d / (nr[b].clamp_min(EPS) * nk.clamp_min(EPS))
                dot_b[off[b] + t], cos_b[off[b] + t], krows[off[b] + t] = d, c, (kr, nk)
                block(out["dot"], off, Q, b)[:, t] = d.detach().cpu().double().numpy()
                block(out["cos"], off, Q, b)[:, t] = c.detach().cpu().double().numpy()
                out["key_norm"][off[b] + t] = float(nk.detach())
    stats = np.zeros((n, 6))
    terms, auxs, keep = [], [], []
    zero = torch.zeros((), device=device)
    for i, (b, tgt, roff, rcnt, n_aux) in enumerate(p["meta"].tolist()):
        t = tgt - off[b]
        if not 0 <= t < off[b + 1] - off[b]:
            terms.append(zero); auxs.append(zero); keep.append(None)
            continue
        if hand:
            at = torch.from_numpy(Q * off[b] + np.arange(Q) * (off[b + 1] - off[b]) + t).to(device)
            d, c = dot[at], cos[at]
        else:
            d, c = dot_b[tgt], cos_b[tgt]
        ix = lambda bit: torch.from_numpy(np.flatnonzero(roles[i] & bit)).to(device)
        neg, pos, smp = ix(2), ix(1), ix(4)
        dn, dp = d[neg], -d[pos]
        mn = dn.max() if len(neg) else zero - float("inf")
        mp = dp.max() if len(pos) else zero - float("inf")
        sn = (dn - mn.detach()).exp().sum() if len(neg) else zero
        sp = (dp - mp.detach()).exp().sum() if len(pos) else zero
        if len(neg) and len(pos):
            tt = mn.detach() + mp.detach() + sn.log() + sp.log()
            term, sig = torch.nn.functional.softplus(tt), torch.sigmoid(tt)
        else:
            term, sig = zero, zero
        aux = (((c[pos] - 1) ** 2).sum() + (c[smp] ** 2).sum()) / torch.tensor(float(n_aux), device=device)
        terms.append(term); auxs.append(aux)
        s4, s5 = (sig / sn if len(neg) else zero), (sig / sp if len(pos) else zero)
        stats[i] = [float(v.detach()) for v in (term, aux, mn, mp, s4, s5)]
        keep.append((d, c, neg, pos, smp, mn, mp, s4, s5, n_aux, b, tgt))
    loss0, loss1 = torch.stack(terms).sum() / n, torch.stack(auxs).sum() / n
    out.update(stats=stats, losses=np.asarray([float(loss0.detach()), float(loss1.detach())]))
    if hand or grads is False:
        return out
    g0, g1 = (float(v) for v in (p["grads"] if grads is None else grads))
    (g0 * loss0 + g1 * loss1).backward()
    out["grad_ref"], out["grad_key"] = ref.grad.cpu().double().numpy(), key.grad.cpu().double().numpy()
    coef, kig = np.zeros((2, n, Q)), np.zeros((n, C))
    with torch.no_grad():
        inv_n = 1.0 / torch.tensor(float(n), device=device)
        for i, k in enumerate(keep):
            if k is None:
                continue
            d, c, neg, pos, smp, mn, mp, s4, s5, n_aux, b, tgt = k
            gd, ec = torch.zeros(Q, device=device), torch.zeros(Q, device=device)
            gd[neg] += s4 * (d[neg] - mn).exp()
            gd[pos] -= s5 * (-d[pos] - mp).exp()
            gd = gd * (g0 * inv_n)
            ec[pos] += c[pos] - 1
            ec[smp] += c[smp]
            gc = ec * (2.0 / float(n_aux)) * (g1 * inv_n) if n_aux else ec * 0
            kr, nk = krows[tgt]
            coef[0, i] = (gd + gc / (nr[b].clamp_min(EPS) * nk.clamp_min(EPS))).cpu().double().numpy()
            coef[1, i] = (gc * c).cpu().double().numpy()
            kig[i] = kr.grad.cpu().double().numpy() if kr.grad is not None else 0.0
    out.update(coef=coef, key_item_grad=kig)
    return out


# ========================================================================================================== the error measure

HEAD = "%-19s %-28s %10s %10s %10s %8s" % ("output", "case", "kernel err", "comp err", "bound", "ratio")
_T = PM.Table(HEAD)                                         # printed only: no file is written
TABLE, WORST, report = _T.lines, _T.worst, _T.report        # WORST: output -> (ratio, table line)


def measure(case, what, got, want, mag, comp, exclude=None, check=True):
    """Every entry of `got` within entry_bound(the composition's error at the entry, s) of `want`, and the project's bound on top.
    Returns the largest error / bound; check=False only returns it (inf where check=True refuses) and adds no line.
    Non-finite: the entries of `exclude` (what the contract leaves unwritten) are not compared; a NaN or an infinity of `want` has
    to be met as such (the mean of nothing; the maximum of no negative); no other non-finite entry in `got`; `comp` may be.
    WORST: output.  Line: output, case, the worst entry's errors relative to its own magnitude.
    Tolerance: TOL * max(1, max|want|)."""
    got, want, mag, comp = (np.asarray(a, dtype=F64) for a in (got, want, mag, comp))
    assert got.shape == want.shape == comp.shape == mag.shape, (case, what, got.shape, want.shape, comp.shape, mag.shape)
    live = np.ones(want.shape, bool) if exclude is None else ~np.asarray(exclude, bool)
    got, want, mag, comp = got[live], want[live], mag[live], comp[live]
    if not got.size:
        return 0.0
    odd = ~np.isfinite(want)
    same_odd = np.where(np.isnan(want), np.isnan(got), got == want)
    if not same_odd[odd].all():
        assert not check, (case, what, "a NaN or infinity of the reference is not met", int((~same_odd[odd]).sum()))
        return float("inf")
    got, want, mag, comp = got[~odd], want[~odd], mag[~odd], comp[~odd]
    if not got.size:
        return 0.0
    assert np.isfinite(mag).all(), (case, what, "magnitude")
    if not np.isfinite(got).all():
        assert not check, (case, what, "non-finite entries", int((~np.isfinite(got)).sum()))
        return float("inf")
    e = PM.errors(got, want, mag, comp)
    if not check:
        return e.worst
    _T.add("%-19s %-28s %10.2e %10.2e %10.2e %8.3f" % ((what, case) + e.row()), what, e.worst)
    e.check(case, what)
    tol = TOL * max(1.0, float(e.size.max()))
    assert float(e.err.max()) <= tol, (case, what, "the project's bound", float(e.err.max()), tol)
    return e.worst


SCORE_OUTPUTS = ("dot", "cos", "ref_norm", "key_norm")
BACKWARD_OUTPUTS = ("coef", "key_item_grad", "grad_ref", "grad_key")


def measure_scores(case, p, got, ref, comp, check=True):
    ex_r, ex_k = unwritten(p)
    ex = dict(ref_norm=ex_r, key_norm=ex_k)
    return max(measure(case, k, got[k], np.where(ex[k], 0.0, ref[k]) if k in ex else ref[k], ref["mag_" + k], comp[k], ex.get(k), check)
               for k in SCORE_OUTPUTS)


def measure_loss(case, got, ref, comp, check=True):
    """got: dict(stats [n, 6], losses [2]); every stats column under its own name"""
    worst = [measure(case, "stats." + name, got["stats"][:, j], ref["stats"][:, j], ref["mag_stats"][:, j], comp["stats"][:, j], None, check)
             for j, name in enumerate(STATS)]
    worst.append(measure(case, "losses", got["losses"], ref["losses"], ref["mag_losses"], comp["losses"], None, check))
    return max(worst)


def measure_backward(case, got, ref, comp, check=True):
    return max(measure(case, k, got[k], ref[k], ref["mag_" + k], comp[k], None, check) for k in BACKWARD_OUTPUTS)


def worst_table():
    return "\n".join(WORST[k][1] for k in sorted(WORST))
