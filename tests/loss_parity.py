"""Per-entry parity of the loss kernels (uninext_amd/csrc/criterion.hip: token focal, mask focal and dice; uninext_amd/csrc/boxinst.hip:
projection and pairwise losses, colour similarity, box bitmasks) at their slice, band and halo edges: the cases, float64
restatements written from include/dynmask_hip.h and the two kernels' header comments (numpy only, nothing of uninext_amd), the
fp32 PyTorch compositions of tests/test_criterion_gpu.py and tests/test_boxinst_gpu.py evaluated per gradient group, and the
error measure.  No GPU is needed to import this.  tests/test_loss_parity_cpu.py checks the conditions the cases claim, pins the
restatements and shows that the measure has teeth; tests/test_loss_parity_gpu.py holds the kernels to it.

Inputs are numbers float64 sees exactly as fp32 holds them: logits and fractional targets are multiples of 2^-10, the saturated
logits are +-10, +-17, +-30, +-88 (where expf leaves the normal range) and +-100; `sim` is multiples of 2^-10 plus plants at
exactly float32(thresh) and one fp32 step below it (the compare is done on the fp32 numbers); alpha = 0.25, so alpha_t is exact;
fp32 images are multiples of 1/4 below 256, so a pooled sum of up to 16 of them and its division by 1, 4 or 16 are exact in any
order; the device scalars (warmup, the upstream gradients) are the fp32 numbers.

The magnitude s of every float output, in units of u = 2^-24, to first order, nothing fitted; the bound of an entry is
entry_bound(comp_err, s) of tests/parity_measure.py = max(COMP_MARGIN x the fp32 composition's error at the entry,
SUM_DEPTH u s), and on top the project's 1e-4 of max|ref| over the tensor (criterion_cases.scaled_error).  s is carried
along with the value by the class V through the operations of the formula, one rule an operation:
  * a rounding of a result v costs rnd(v) = max(|v|, 2^-126): u |v| for a normal number, half the subnormal spacing below
    (exp(-88) and beyond).  A product with 0 or +-1, a sum with 0 and a multiplication by 2 are exact and cost nothing.
  * a b: s_a |b| + |a| s_b + rnd;  a + b: s_a + s_b + rnd;  a / b: s_a / |b| + |a / b| s_b / |b| + rnd
  * expf, log1pf, expm1f are good to 2 u: exp(a): |v| s_a + 2 rnd(v);  log1p(a): s_a / (1 + a) + 2 rnd(v);  exp(0) = 1 is exact
  * sqrt(a): min(s_a / (2 v), sqrt(s_a / u)) + rnd(v)   (the second form where v is 0 or tiny: |sqrt(a + e) - sqrt(a)| <= sqrt|e|)
  * sigmoid: e = exp(-|x|), r = 1 / (1 + e); the larger of p, q is r, the smaller e r; the softplus term is log1p(e)
  * a sum that the kernel keeps in float64 (a workgroup's partial sums, `sums`, `totals`, the BoxInst dice sums) carries the s of
    the fp32 terms added and nothing for the additions; stored as fp32 it takes one rnd more.  A count (sum t, sum w) is exact.
  * arithmetic the kernel does in float64 (the projection term, Lab) costs 2^-29 rnd a rounding (2^-53 / u).
The formulas the rules run through are the well-conditioned ones, so a cancellation in a kernel is not in the budget:
  token / mask focal    ce = max(x, 0) - x t + sp,  m = p (1 - t) + q t,  term = a_t (ce m^2),
                        grad = a_t ((p (1 - t) - q t) m^2 + 2 ce m (1 - 2 t) p q)                 (p - t without the subtraction at t = 0, 1)
  dice gradient         cf = g_mask / (P nb), gd = g_dice / nb, den = (S + T) + 1, ca = gd (2 I + 1) / den^2, cb = 2 gd / den from the
                        fp32 `sums` (their s goes in), grad = cf focal' + (ca - cb t) p q
  pairwise              lf = min(x, 0) - sp, lb = min(-x, 0) - sp;  a = lf_c + lf_j, b = lb_c + lb_j (the centre's alone at a neighbour
                        outside), l = -(max(a, b) + log1p(exp(-|a - b|)));  its gradient at c, with z = a - b (= x_c + x_j) and
                        x_j = lf_j - lb_j:  -p_c (1 - sigmoid(z)) expm1(x_j) for x_j < 0 and q_c sigmoid(z) expm1(-x_j) otherwise
                        (= sigmoid(x_c) - sigmoid(x_c + x_j), which cancels); a pixel adds its terms as a centre and as a neighbour
                        (those carry the CENTRE's weight), then the fp32 scale g_pair warmup / max(sum w, 1)
  projection            float64: p = sigmoid(x at the maximum), I = sum p t, U = sum (p^2 + t^2) + 1e-5, the gradient
                        (g_prj / n) (4 I p - 2 t U) / U^2 p q per row maximum and per column maximum, rounded to fp32 once
  colour similarity     bytes exactly; Lab in float64 rounded to fp32 once; exp(-0.5 sqrt(sum of 3 squared fp32 differences))
An entry whose reference is exactly 0 with s = 0 (a masked token, a row no instance reads, a pixel without a weighted term that is no
maximum, a neighbour outside the image) has bound 0: it must be exactly 0.  Where the fp32 composition is not finite at a finite
reference entry its term is dropped for that entry.  Entries the contract leaves unwritten would be excluded BY NAME in
UNWRITTEN; these kernels write every element of every output, so it is empty and the excluded share of every output is 0.
pos, tmax, sum w, sum t and the bitmasks are integers and must be equal exactly.

What the measure can and cannot see: the composition forms p - t and sigmoid(x_c) - sigmoid(x_c + x_j) by subtraction too, so at an
entry where it is as far off as a cancelling kernel its term excuses the kernel; the report prints both errors against the derived
term alone so that this is visible.
"""
import functools
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from criterion_cases import MARGIN as TOL, scaled_error                      # noqa: E402,F401
import parity_measure as PM                                                 # noqa: E402
from parity_measure import COMP_MARGIN, SUM_DEPTH, U, entry_bound          # noqa: E402,F401

F32, F64 = np.float32, np.float64
MINN = 2.0 ** -126                          # the smallest normal fp32 number
D64 = 2.0 ** -29                            # a float64 rounding in units of u
SATURATED = (10.0, -10.0, 17.0, -17.0, 30.0, -30.0, 88.0, -88.0, 100.0, -100.0)
ALPHA, NUM_BOXES = 0.25, 3.0
WARMUP = float(F32(0.4))
THRESH = F32(0.3)
BAND, LDS_BYTES, MAX_DILATION, TILE = 8, 63 * 1024, 8, 16
UNWRITTEN = {}                              # output -> mask builder; empty: every output is written in full


_rng, dy, is_dyadic = PM.rng, PM.dy, PM.is_dyadic        # seeded by name; float32 multiples of 2^-10 (never -0.0)


# ============================================================================================ values that carry their magnitude

def rnd(v):
    v = np.abs(v)
    return np.where(v != 0, np.maximum(v, MINN), 0.0)


class V:
    """a float64 value and the magnitude s of its fp32 evaluation's error (units of u)"""
    __slots__ = ("v", "s")

    def __init__(self, v, s=None):
        self.v = np.asarray(v, dtype=F64)
        self.s = np.zeros_like(self.v) if s is None else np.asarray(s, dtype=F64) + np.zeros_like(self.v)

    def exact(self, *values):
        hit = np.zeros(self.v.shape, bool)
        for c in values:
            hit |= np.abs(self.v) == c
        return hit & (self.s == 0)

    def __neg__(self):
        return V(-self.v, self.s)

    def __getitem__(self, ix):
        return V(self.v[ix], self.s[ix])


def mul(a, b, exact=False, unit=1.0):
    v = a.v * b.v
    free = a.exact(0.0, 1.0) | b.exact(0.0, 1.0) | bool(exact)
    with np.errstate(invalid="ignore", over="ignore"):
        return V(v, a.s * np.abs(b.v) + np.abs(a.v) * b.s + np.where(free, 0.0, unit * rnd(v)))


def add(a, b, unit=1.0):
    v = a.v + b.v
    free = a.exact(0.0) | b.exact(0.0)
    return V(v, a.s + b.s + np.where(free, 0.0, unit * rnd(v)))


def sub(a, b, unit=1.0):
    return add(a, -b, unit)


def div(a, b, unit=1.0):
    v = a.v / b.v
    return V(v, a.s / np.abs(b.v) + np.abs(v) * b.s / np.abs(b.v) + unit * rnd(v))


def exp_(a):
    v = np.exp(a.v)
    return V(v, v * a.s + np.where(a.exact(0.0), 0.0, 2 * rnd(v)))


def expm1_(a):
    v = np.expm1(a.v)
    return V(v, np.exp(a.v) * a.s + 2 * rnd(v))


def log1p_(a):
    v = np.log1p(a.v)
    return V(v, a.s / (1 + a.v) + 2 * rnd(v))


def sqrt_(a):
    v = np.sqrt(a.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        prop = np.minimum(np.where(v > 0, a.s / (2 * v), np.inf), np.sqrt(a.s / U))
    return V(v, prop + rnd(v))


def where_(c, a, b):
    return V(np.where(c, a.v, b.v), np.where(c, a.s, b.s))


def stored(a):
    """a float64 quantity stored as fp32"""
    return V(a.v, a.s + rnd(a.v))


def total(a, axis=None):
    """a sum the kernel keeps in float64: the terms' s, nothing for the additions"""
    return V(a.v.sum(axis), a.s.sum(axis))


ONE, TWO = V(1.0), V(2.0)


def sig_(x):
    """(p, q, sp) = sigmoid(x), sigmoid(-x), log(1 + exp(-|x|)) of a V"""
    e = exp_(V(-np.abs(x.v), x.s))
    r = div(ONE, add(ONE, e))
    small = mul(e, r)
    pos = x.v >= 0
    return where_(pos, r, small), where_(pos, small, r), log1p_(e)


def focal_chain(x, t, alpha=ALPHA, swap=False):
    """(term, d term / dx, p, q) of the focal loss at gamma 2 as V; x, t float64 arrays of fp32 numbers.  swap: the mutant with alpha
    and 1 - alpha exchanged."""
    X, T_, T1 = V(x), V(t), V(1.0 - t)
    p, q, sp = sig_(X)
    ce = add(sub(V(np.maximum(x, 0.0)), mul(X, T_)), sp)
    m = add(mul(p, T1), mul(q, T_))
    a, b = (1.0 - alpha, alpha) if swap else (alpha, 1.0 - alpha)
    A = V(a * t + b * (1.0 - t))                                        # exact at alpha = 0.25 and t a multiple of 2^-10
    mm = mul(m, m)
    term = mul(A, mul(ce, mm))
    pt = sub(mul(p, T1), mul(q, T_))                                    # p - t
    dm = mul(V(1.0 - 2.0 * t), mul(p, q))
    grad = mul(A, add(mul(pt, mm), mul(TWO, mul(ce, mul(m, dm)), exact=True)))
    return term, grad, p, q


# ===================================================================================================================== token focal

def _tok(B, Q, T, mask, misaligned=False):
    return dict(B=B, Q=Q, T=T, mask=mask, misaligned=misaligned)


TOKEN = {
    "b1_q1_t1_none": _tok(1, 1, 1, "none"), "b1_q3_t3_int64": _tok(1, 3, 3, "int64"), "b1_q4_t4_bool": _tok(1, 4, 4, "bool"),
    "b1_q5_t63_none": _tok(1, 5, 63, "none"), "b1_q5_t64_int64": _tok(1, 5, 64, "int64"), "b5_q1_t65_bool": _tok(5, 1, 65, "bool"),
    "b2_q2_t252_int64": _tok(2, 2, 252, "int64"), "b1_q3_t255_bool": _tok(1, 3, 255, "bool"), "b1_q4_t256_none": _tok(1, 4, 256, "none"),
    "b3_q3_t64_int64": _tok(3, 3, 64, "int64"), "b3_q3_t65_bool": _tok(3, 3, 65, "bool"),
    "b1_q5_t256_int64_misaligned": _tok(1, 5, 256, "int64", True), "b3_q3_t4_bool_misaligned": _tok(3, 3, 4, "bool", True),
}
TOKEN_TS, TOKEN_ROWS, TOKEN_G = (1, 3, 4, 63, 64, 65, 252, 255, 256), (1, 3, 4, 5), 3
# positive-map rows: 0 binary, 1 fractional, 2 all ones; then "unmatched" as -1 and as G, one past the end
ROW_TARGETS = (0, 1, 2, -1, TOKEN_G)


@functools.lru_cache(maxsize=None)
def token_inputs(name):
    c, g = TOKEN[name], _rng("token/" + name)
    B, Q, T = c["B"], c["Q"], c["T"]
    logits = dy(np.clip(3.0 * g.standard_normal((B, Q, T)), -9.0, 9.0))
    flat = logits.reshape(-1)
    at = g.permutation(flat.size)[:min(flat.size // 2 + 1, 4 * len(SATURATED))]
    flat[at] = np.resize(np.asarray(SATURATED, F32), len(at))
    pm = np.zeros((TOKEN_G, T), F32)
    pm[0] = g.rand(T) < 0.3
    pm[1] = dy(g.rand(T))
    pm[2] = 1.0
    row_target = np.resize(np.roll(np.asarray(ROW_TARGETS, np.int32), zlib.crc32(name.encode()) % 5), B * Q).reshape(B, Q).astype(np.int32)
    mask = None
    if c["mask"] != "none":
        mask = np.zeros((B, T), np.int64)
        for b in range(B):
            mask[b, :max(1, T - (T // 4) * (b % 3))] = 2 - b % 2            # any value > 0 counts; int64 also holds a negative one
        if T >= 3:
            mask[0, 1] = -3 if c["mask"] == "int64" else 0
        if c["mask"] == "bool":
            mask = (mask > 0).astype(np.uint8)
    return dict(name=name, logits=logits, mask=mask, mask_kind=c["mask"], row_target=row_target, pm=pm, alpha=ALPHA, scale=1.0,
                misaligned=c["misaligned"])


def token_targets(p, row=None):
    """(t [B, Q, T] float64, counted [B, Q, T] bool): the positive-map row of every query, zeros for a row outside [0, G)"""
    B, Q, T = p["logits"].shape
    rt = p["row_target"] if row is None else row
    ok = (rt >= 0) & (rt < p["pm"].shape[0])
    t = np.where(ok[:, :, None], p["pm"].astype(F64)[np.clip(rt, 0, p["pm"].shape[0] - 1)], 0.0)
    counted = np.ones((B, Q, T), bool) if p["mask"] is None else np.broadcast_to((p["mask"] > 0)[:, None, :], (B, Q, T))
    return t, counted


def token64(p, mutant=None):
    """loss, grad [B, Q, T] (scale x d loss / d logits) with mag_*.  mutant: "alpha_swap"."""
    t, counted = token_targets(p)
    term, grad, _, _ = focal_chain(p["logits"].astype(F64), t, p["alpha"], swap=mutant == "alpha_swap")
    z = V(np.zeros(t.shape))
    loss = stored(total(where_(counted, term, z)))
    grad = mul(V(p["scale"]), where_(counted, grad, z))
    return dict(loss=loss.v, mag_loss=loss.s, grad=grad.v, mag_grad=grad.s, t=t, counted=counted)


def token_slices(p, ref):
    """the report's slices of the gradient: (t = 0, t = 1, fractional t) x (moderate, saturated logits), counted tokens only"""
    sat = np.abs(p["logits"]) >= 10
    out = {}
    for tn, tm in (("t0", ref["t"] == 0), ("t1", ref["t"] == 1), ("tfrac", (ref["t"] > 0) & (ref["t"] < 1))):
        for sn, sm in (("moderate", ~sat), ("saturated", sat)):
            out[tn + "." + sn] = tm & sm & ref["counted"]
    return out


def token_composition(p, device="cpu"):
    """tests/test_criterion_gpu.py: token_composition, in fp32 on `device`: dict(loss, grad) as float64 numpy"""
    import torch
    from uninext_amd.criterion import token_sigmoid_binary_focal_loss
    x = torch.from_numpy(p["logits"]).to(device).requires_grad_(True)
    t, _ = token_targets(p)
    onehot = torch.from_numpy(t.astype(F32)).to(device)
    mask = None if p["mask"] is None else torch.from_numpy(p["mask"].astype(np.int64)).to(device)
    loss = token_sigmoid_binary_focal_loss(x, onehot, alpha=p["alpha"], text_mask=mask)
    loss.backward()
    return dict(loss=np.asarray(float(loss.detach())), grad=x.grad.cpu().double().numpy() * p["scale"])


# ===================================================================================================================== mask losses

def _mk(F, h, w, stride, n=4):
    return dict(F=F, h=h, w=w, stride=stride, n=n)


# P = F h w.  An odd P has neither F = 2 nor w % 4 == 0: those take F = 3 or 5 (a frame boundary inside a slice all the same)
MASK = {
    "p1023_f3_11x31_s3": _mk(3, 11, 31, 3), "p1024_f2_16x32_s4": _mk(2, 16, 32, 4), "p1024_f2_256x2_s1": _mk(2, 256, 2, 1),
    "p1025_f5_5x41_s2": _mk(5, 5, 41, 2), "p2048_f2_32x32_s1": _mk(2, 32, 32, 1), "p2048_f2_512x2_s3": _mk(2, 512, 2, 3),
    "p2049_f3_1x683_s4": _mk(3, 1, 683, 4), "p2048_f2_8x128_s2": _mk(2, 8, 128, 2),
    "empty_slice_scalar": _mk(1, 3, 174763, 1), "empty_slice_vec4": _mk(1, 3, 174764, 1),
}
MASK_PS = (1023, 1024, 1025, 2048, 2049)
TARGET_BLOCKS, MIN_SLICE, THREADS = 2048, 1024, 256


def mask_slices(n, P):
    """(slices, chunk) restated from criterion.hip: mask_slices and the launcher's chunk"""
    slices = min(-(-TARGET_BLOCKS // n), -(-P // MIN_SLICE))
    chunk = -(-(-(-P // slices)) // 4) * 4
    return slices, chunk


def empty_slices(n, P):
    slices, chunk = mask_slices(n, P)
    return [s for s in range(slices) if s * chunk >= P]


@functools.lru_cache(maxsize=None)
def mask_inputs(name):
    c, g = MASK[name], _rng("mask/" + name)
    n, F, h, w, stride = c["n"], c["F"], c["h"], c["w"], c["stride"]
    start = stride // 2
    H_im, W_im = start + stride * (h - 1) + 1, start + stride * (w - 1) + 1        # the smallest that fit
    R = 2 * F
    gt = (g.rand(R, H_im, W_im) < 0.35).astype(np.uint8)
    gt[F:] = 1                                                      # rows R - F .. R - 1: an all-one target
    gt[:F][gt[:F] != 0] = g.randint(1, 256, int((gt[:F] != 0).sum()))              # any non-zero byte counts
    gt_row = np.asarray([0, R - F, -1, R - F + 1], np.int32)[:n]
    src = dy(np.clip(3.0 * g.standard_normal((n, F, h, w)), -9.0, 9.0))
    flat = src.reshape(n, -1)
    k = min(len(SATURATED), flat.shape[1])
    flat[:, g.permutation(flat.shape[1])[:k]] = np.asarray(SATURATED[:k], F32)
    return dict(name=name, src=src, gt=gt, gt_row=gt_row, stride=stride, num_boxes=NUM_BOXES)


def strided_targets(gt, rows, F, h, w, stride, start=None):
    """[n, F, h, w] float64: gt[row + f, start + stride y, start + stride x] != 0; a row outside [0, R - F] reads as zeros.  `start`
    other than stride // 2 is a mutant's; a pixel past the mask then reads 0."""
    R = gt.shape[0]
    start = stride // 2 if start is None else start
    pad = np.zeros((R, start + stride * h + 1, start + stride * w + 1), np.uint8)
    pad[:, :gt.shape[1], :gt.shape[2]] = gt
    picked = pad[:, start::stride, start::stride][:, :h, :w] != 0
    out = np.zeros((len(rows), F, h, w))
    for i, r in enumerate(np.asarray(rows).tolist()):
        if 0 <= r <= R - F:
            out[i] = picked[r:r + F]
    return out


def mask64(p, grads=(1.0, 0.0), mutant=None):
    """sums [n, 4], losses [2], grad [n, F, h, w] for the upstream gradients `grads` = (grad_mask, grad_dice), with mag_*.
    mutants: "skip_last_slice", "den_no_plus1", "alpha_swap", "start_up"."""
    src = p["src"].astype(F64)
    n, F, h, w = src.shape
    P, nb, stride = F * h * w, p["num_boxes"], p["stride"]
    t = strided_targets(p["gt"], p["gt_row"], F, h, w, stride, (stride + 1) // 2 if mutant == "start_up" else None)
    term, fgrad, pr, q = focal_chain(src, t, ALPHA, swap=mutant == "alpha_swap")
    live = np.ones(P, bool)
    if mutant == "skip_last_slice":
        slices, chunk = mask_slices(n, P)
        last = max(s for s in range(slices) if s * chunk < P)
        live[last * chunk:] = False
    live = live.reshape(1, F, h, w)
    z = V(np.zeros(src.shape))
    pt = mul(pr, V(t))
    raw = [total(where_(live, a, z), (1, 2, 3)) for a in (term, pt, pr, V(t))]           # float64 sums of fp32 terms
    sums = [stored(a) for a in raw[:3]] + [raw[3]]
    loss0 = stored(V(raw[0].v.sum() / P / nb, raw[0].s.sum() / P / nb))
    den64 = raw[2].v + raw[3].v + 1.0
    dice = 1.0 - (2.0 * raw[1].v + 1.0) / den64
    loss1 = stored(V(dice.sum() / nb, (2.0 * raw[1].s / den64 + (2.0 * raw[1].v + 1.0) / den64 ** 2 * raw[2].s).sum() / nb))
    # the backward, from the fp32 sums
    col = lambda a: V(a.v.reshape(n, 1, 1, 1), a.s.reshape(n, 1, 1, 1))
    I, S, T_ = col(sums[1]), col(sums[2]), col(sums[3])
    den = add(S, T_) if mutant == "den_no_plus1" else add(add(S, T_), ONE)
    gd = div(V(float(grads[1])), V(nb))
    cf = div(V(float(grads[0])), mul(V(float(P)), V(nb)))
    ca = div(mul(gd, add(mul(TWO, I, exact=True), ONE)), mul(den, den))
    cb = div(mul(gd, TWO, exact=True), den)
    grad = add(mul(cf, fgrad), mul(sub(ca, mul(cb, V(t))), mul(pr, q)))
    return dict(sums=np.stack([a.v for a in sums], 1), mag_sums=np.stack([a.s for a in sums], 1), losses=np.asarray([loss0.v, loss1.v]),
                mag_losses=np.asarray([loss0.s, loss1.s]), grad=grad.v, mag_grad=grad.s, t=t)


def mask_composition(p, t, device="cpu"):
    """tests/test_criterion_gpu.py: mask_composition, in fp32 on `device`, the two gradients apart: dict(losses, grad_focal,
    grad_dice, sums) as float64 numpy.  t: the restatement's targets (integers)."""
    import torch
    from uninext_amd.criterion import dice_loss, sigmoid_focal_loss
    x = torch.from_numpy(p["src"]).to(device).requires_grad_(True)
    tt = torch.from_numpy(t.astype(F32)).to(device).flatten(1)
    lm, ld = sigmoid_focal_loss(x.flatten(1), tt, p["num_boxes"]), dice_loss(x.flatten(1), tt, p["num_boxes"])
    gm, = torch.autograd.grad(lm, x, retain_graph=True)
    gd, = torch.autograd.grad(ld, x)
    with torch.no_grad():
        from uninext_amd.criterion import _focal_terms
        pr = x.sigmoid().flatten(1)
        sums = torch.stack([_focal_terms(x.flatten(1), tt, ALPHA, 2).sum(1), (pr * tt).sum(1), pr.sum(1), tt.sum(1)], 1)
    return dict(losses=np.asarray([float(lm.detach()), float(ld.detach())]), grad_focal=gm.cpu().double().numpy(), grad_dice=gd.cpu().double().numpy(),
                sums=sums.cpu().double().numpy())


# ========================================================================================================================= BoxInst

def tile_bytes(w, d):
    """boxinst.hip: tile_bytes: (8 + 2 d) rows of two fp32 planes and a byte plane"""
    return (BAND + 2 * d) * w * 9


def widest(d):
    return max(w for w in range(1, 2000) if tile_bytes(w, d) <= LDS_BYTES)


def offsets(d, transposed=False):
    """neighbour k of 8: unfold's order, row-major over the 3 x 3 window without the centre"""
    out = [((c // 3 - 1) * d, (c % 3 - 1) * d) for c in range(9) if c != 4]
    return [(b, a) for a, b in out] if transposed else out


def _bx(h, w, d, stride, plant=None, n=2, N=3):
    return dict(h=h, w=w, d=d, stride=stride, plant=plant, n=n, N=N)


BOX = {}
for _i, (_d, _h) in enumerate((d, h) for d in (1, 2, 3, 7, 8) for h in (7, 8, 9, 16, 17, 25)):
    BOX["d%d_h%d" % (_d, _h)] = _bx(_h, (6, 8, 5, 12)[_i % 4], _d, 1 + (_i + _i // 4) % 4)
BOX.update({
    "h2_w3_d7": _bx(2, 3, 7, 2), "h1_w1_d8": _bx(1, 1, 8, 1), "h5_w2_d3": _bx(5, 2, 3, 3), "h2_w9_d3": _bx(2, 9, 3, 4),
    "lds_d1_w716": _bx(2, 716, 1, 1, n=1, N=1), "lds_d8_w298": _bx(2, 298, 8, 2, n=1, N=1),
    "ties_h17_w200": _bx(17, 200, 2, 1, plant="ties"), "all_equal": _bx(9, 12, 2, 2, plant="all_equal"),
    "w_band_first_row": _bx(17, 8, 2, 3, plant="band_first"), "w_band_last_row": _bx(17, 8, 3, 1, plant="band_last"),
    "w_border_only": _bx(10, 9, 1, 2, plant="border"), "no_weight": _bx(9, 8, 2, 4, plant="no_weight"),
    "img_out_of_range": _bx(9, 7, 2, 1, plant="bad_img"), "rows_out_of_range": _bx(9, 8, 2, 2, plant="bad_rows", n=3, N=3),
})
BOX_DS, BOX_HS = (1, 2, 3, 7, 8), (7, 8, 9, 16, 17, 25)
TIE_ROWS = {0: (5, 9), 1: (7, 71), 2: (67, 130)}        # row -> columns of its repeated maximum: across lanes of one 64-column step; one
#                                                         lane, two steps; two lanes, two steps (the lower column in the higher lane)
TIE_COLS = {0: (4, 6), 1: (3, 12), 2: (9, 16)}          # column -> rows: within band 0; bands 0 and 1; bands 1 and 2


@functools.lru_cache(maxsize=None)
def box_inputs(name):
    c, g = BOX[name], _rng("box/" + name)
    h, w, d, stride, n, N, plant = c["h"], c["w"], c["d"], c["stride"], c["n"], c["N"], c["plant"]
    start = stride // 2
    H_im, W_im = start + stride * (h - 1) + 1, start + stride * (w - 1) + 1
    B, R = 2, 4
    src = dy(np.clip(3.0 * g.standard_normal((N, 1, h, w)), -9.0, 9.0))
    for i in range(N):                                          # saturated logits, also next to each other (pairs d apart exist by chance and by plant)
        at = g.permutation(h * w)[:min(len(SATURATED), h * w // 3)]
        src[i, 0].reshape(-1)[at] = np.asarray(SATURATED[:len(at)], F32)
        if h > d and w > d:
            src[i, 0, 0, 0], src[i, 0, d, d], src[i, 0, h - 1, w - 1], src[i, 0, h - 1 - d, w - 1] = 10.0, 10.0, -17.0, -17.0
    inst = g.permutation(N)[:n].astype(np.int32)
    gt = np.zeros((R, H_im, W_im), np.uint8)
    for r in range(R):                                          # box masks in mask pixels, any non-zero byte
        y1, x1 = g.randint(0, max(1, h // 2)), g.randint(0, max(1, w // 2))
        y2, x2 = g.randint(y1, h), g.randint(x1, w)
        gt[r, start + stride * y1:start + stride * y2 + 1, start + stride * x1:start + stride * x2 + 1] = 1 + 63 * r
    gt[0, :, :] = 200                                           # row 0: a full target
    gt_row = g.randint(0, R, n).astype(np.int32)
    gt_row[0] = 0
    img = g.randint(0, B, n).astype(np.int32)
    sim = dy(g.rand(B, 8, h, w))
    below = np.nextafter(THRESH, F32(0))
    for b in range(B):                                          # plants: exactly the threshold (counts) and one fp32 step below (does not)
        flat = sim[b].reshape(-1)
        at = g.permutation(flat.size)[:max(2, flat.size // 8)]
        flat[at[0::2]], flat[at[1::2]] = THRESH, below
    thresh = THRESH
    if plant == "ties":
        src[:] = dy(g.uniform(-3.0, 3.0, src.shape))
        for i in range(N):
            for r, cols in TIE_ROWS.items():
                src[i, 0, r, list(cols)] = 5.0
            for col, rows in TIE_COLS.items():
                src[i, 0, list(rows), col] = 6.0
    elif plant == "all_equal":
        src[:] = 0.5
    elif plant in ("band_first", "band_last"):
        gt[:] = 0
        y = 8 if plant == "band_first" else 15
        gt[:, start + stride * y, :] = 1
    elif plant == "border":
        gt[:] = 1
        gt[:, start + stride:start + stride * (h - 1), start + stride:start + stride * (w - 1)] = 0
    elif plant == "no_weight":
        thresh = F32(2.0)
    elif plant == "bad_img":
        img[:] = (B, -1)[:n]
    elif plant == "bad_rows":
        inst[1], gt_row[2] = N, R                               # one past the end: logits 0; an all-zero target
        inst[0], inst[2] = 0, 2
    return dict(name=name, src=src, inst=inst, gt=gt, gt_row=gt_row, sim=sim, img=img, thresh=thresh, d=d, stride=stride, warmup=WARMUP,
                plant=plant)


def _shift(a, dy_, dx_):
    """(a[y + dy, x + dx] with zeros outside, the inside mask) of a [h, w] array"""
    h, w = a.shape[-2:]
    ys, xs = np.arange(h)[:, None] + dy_, np.arange(w)[None, :] + dx_
    inside = (ys >= 0) & (ys < h) & (xs >= 0) & (xs < w)
    return np.where(inside, a[..., np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)], 0), inside


def _vshift(a, dy_, dx_):
    v, inside = _shift(a.v, dy_, dx_)
    return V(v, _shift(a.s, dy_, dx_)[0]), inside


def _argmax(a, axis, highest=False):
    if highest:
        return a.shape[axis] - 1 - np.argmax(np.flip(a, axis), axis)
    return np.argmax(a, axis)


def box64(p, mutant=None):
    """pos int [n, h + w], tmax [n, h + w], sums [n, 4], totals [2], losses [2], grad_prj and grad_pair [N, 1, h, w] (each for its
    upstream gradient 1, the other 0) with mag_*; t [n, h, w], weights [n, 8, h, w], row_max / col_max bool [N, h, w].
    mutants: "nbr_order", "centre_weight", "drop_halo", "tie_high", "start_up"."""
    src = p["src"].astype(F64)
    N, _, h, w = src.shape
    n, d, stride = len(p["inst"]), p["d"], p["stride"]
    R, Bn = p["gt"].shape[0], p["sim"].shape[0]
    rows = np.where((p["gt_row"] >= 0) & (p["gt_row"] < R), p["gt_row"], -1)
    t = strided_targets(p["gt"], rows, 1, h, w, stride, (stride + 1) // 2 if mutant == "start_up" else None)[:, 0]
    th = F32(p["thresh"])
    offs = offsets(d, transposed=mutant == "nbr_order")
    yy = np.arange(h)[:, None] + np.zeros((1, w), int)
    pos, tmax = np.zeros((n, h + w), np.int64), np.zeros((n, h + w), np.int64)
    sums, mag_sums = np.zeros((n, 4)), np.zeros((n, 4))
    weights = np.zeros((n, 8, h, w))
    inst_tot = []
    gprj, sprj = np.zeros((N, h, w)), np.zeros((N, h, w))
    row_max, col_max = np.zeros((N, h, w), bool), np.zeros((N, h, w), bool)
    pair_terms = {}
    for i in range(n):
        r = int(p["inst"][i])
        x = src[r, 0] if 0 <= r < N else np.zeros((h, w))
        # ---- the maxima of the logits, the lowest index among equals, and the dice sums in float64
        pr_, pc_ = _argmax(x, 1, mutant == "tie_high"), _argmax(x, 0, mutant == "tie_high")
        pos[i, :h], pos[i, h:] = pr_, pc_
        tmax[i, :h], tmax[i, h:] = t[i].max(1), t[i].max(0)
        sg = lambda v: np.where(v >= 0, 1 / (1 + np.exp(-np.abs(v))), np.exp(-np.abs(v)) / (1 + np.exp(-np.abs(v))))
        for o, (xm, tm, depth) in enumerate(((x[np.arange(h), pr_], tmax[i, :h], h), (x[pc_, np.arange(w)], tmax[i, h:], w))):
            pm_ = sg(xm)
            I, Uu = (pm_ * tm).sum(), (pm_ * pm_ + tm * tm).sum() + 1e-5
            sums[i, 2 * o:2 * o + 2] = I, Uu
            mag_sums[i, 2 * o:2 * o + 2] = D64 * (depth + 4) * I, D64 * (depth + 4) * Uu
        if 0 <= r < N and not any(int(p["inst"][k]) == r for k in range(i)):
            pm_, qm_ = sg(x), sg(-x)
            rm, cm = np.arange(w)[None, :] == pr_[:, None], np.arange(h)[:, None] == pc_[None, :]
            row_max[r], col_max[r] = rm, cm
            for hit, (I, Uu), tm, depth in ((rm, sums[i, :2], tmax[i, :h][:, None], h), (cm, sums[i, 2:], tmax[i, h:][None, :], w)):
                gprj[r] += np.where(hit, (4 * I * pm_ - 2 * tm * Uu) / (Uu * Uu) * pm_ * qm_ / n, 0.0)
                sprj[r] += np.where(hit, D64 * (depth + 8) * (4 * I * pm_ + 2 * tm * Uu) / (Uu * Uu) * pm_ * qm_ / n, 0.0)
        # ---- the pairwise term
        b = int(p["img"][i])
        if not 0 <= b < Bn:
            inst_tot.append((V(0.0), 0.0))
            continue
        X = V(x)
        pV, qV, sp = sig_(X)
        lf, lb = sub(V(np.minimum(x, 0.0)), sp), sub(V(np.minimum(-x, 0.0)), sp)
        tot, cnt = V(0.0), 0.0
        terms = []
        for k, (oy, ox) in enumerate(offs):
            wk = (t[i] != 0) & (p["sim"][b, k] >= th)
            weights[i, k] = wk
            lfj, inside = _vshift(lf, oy, ox)
            lbj, _ = _vshift(lb, oy, ox)
            if mutant == "drop_halo" and oy > 0:                # the last staged row below a band is missing
                inside = inside & ~(yy + oy == (yy // BAND) * BAND + BAND + d - 1)
                lfj, lbj = where_(inside, lfj, V(np.zeros((h, w)))), where_(inside, lbj, V(np.zeros((h, w))))
            a, bb = add(lf, lfj), add(lb, lbj)
            z = sub(a, bb)
            lse = add(where_(a.v >= bb.v, a, bb), log1p_(exp_(V(-np.abs(z.v), z.s))))
            tot = V(tot.v - (lse.v * wk).sum(), tot.s + (lse.s * wk).sum())
            cnt += float(wk.sum())
            terms.append((k, oy, ox, wk, inside))
        inst_tot.append((tot, cnt))
        if 0 <= r < N and r not in pair_terms:
            pair_terms[r] = (lf, lb, pV, qV, terms)
    tot0 = V(sum(a.v for a, _ in inst_tot), sum(a.s for a, _ in inst_tot))
    tot1 = float(sum(c for _, c in inst_tot))
    loss_prj = ((1 - 2 * sums[:, 0] / sums[:, 1]) + (1 - 2 * sums[:, 2] / sums[:, 3])).sum() / n
    mag_prj = rnd(loss_prj) + D64 * 2 * (max(h, w) + 8) * (2 * sums[:, 0] / sums[:, 1] + 2 * sums[:, 2] / sums[:, 3] + 2).sum() / n
    wm = p["warmup"]
    loss_pair = stored(V(wm * tot0.v / max(tot1, 1.0), wm * tot0.s / max(tot1, 1.0)))
    # ---- the pairwise gradient for an upstream gradient of 1
    scale = stored(V(wm / max(tot1, 1.0)))
    gpair, spair = np.zeros((N, h, w)), np.zeros((N, h, w))
    for r, (lf, lb, pV, qV, terms) in pair_terms.items():
        res = V(np.zeros((h, w)))
        for k, oy, ox, wk, inside in terms:
            for sign, use in ((1, wk & inside), (-1, None)):
                lfj, _ = _vshift(lf, sign * oy, sign * ox)
                lbj, _ = _vshift(lb, sign * oy, sign * ox)
                if use is None:                                 # as a neighbour: the centre at c - off carries the weight
                    use = _shift((wk & inside).astype(F64), -oy, -ox)[0] != 0
                    if mutant == "centre_weight":               # ... the mutant takes the pixel's own
                        use = wk & _shift(np.ones((h, w)), -oy, -ox)[1]
                z = sub(add(lf, lfj), add(lb, lbj))
                xj = sub(lfj, lbj)
                pz, qz, _ = sig_(z)
                neg = xj.v < 0
                e = expm1_(V(-np.abs(xj.v), xj.s))              # expm1(x_j) for x_j < 0, expm1(-x_j) otherwise
                term = where_(neg, -mul(mul(pV, qz), e), mul(mul(qV, pz), e))
                res = add(res, where_(use, term, V(np.zeros((h, w)))))
        res = mul(res, scale)
        gpair[r], spair[r] = res.v, res.s
    return dict(pos=pos, tmax=tmax, sums=sums, mag_sums=mag_sums, totals=np.asarray([tot0.v, tot1]), mag_totals=np.asarray([tot0.s, 0.0]),
                losses=np.asarray([loss_prj, loss_pair.v]), mag_losses=np.asarray([mag_prj, loss_pair.s]),
                grad_prj=gprj[:, None], mag_grad_prj=(sprj + rnd(gprj))[:, None], grad_pair=gpair[:, None], mag_grad_pair=spair[:, None],
                t=t, weights=weights, row_max=row_max, col_max=col_max)


def box_slices(ref):
    """the projection gradient's slices: row maxima only, column maxima only, both"""
    r, c = ref["row_max"][:, None], ref["col_max"][:, None]
    return {"row_max": r & ~c, "col_max": c & ~r, "both": r & c, "neither": ~r & ~c}


def box_composition(p, ref, device="cpu"):
    """tests/test_boxinst_gpu.py: composition, in fp32 on `device`, the two gradients apart: dict(losses, grad_prj, grad_pair) as
    float64 numpy.  The integer decisions are the restatement's (targets, weights, where the maxima sit): torch takes the maxima of
    the fp32 sigmoids, which collide at saturation."""
    import torch
    from uninext_amd.boxinst import compute_pairwise_term
    from uninext_amd.criterion import dice_coefficient
    N, _, h, w = p["src"].shape
    n = len(p["inst"])
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(device)
    x_all = t32(p["src"]).requires_grad_(True)
    x = torch.stack([x_all[int(r)] if 0 <= int(r) < N else torch.zeros(1, h, w, device=device) for r in p["inst"]])
    pos = torch.from_numpy(ref["pos"]).to(device)
    tmax = t32(ref["tmax"])
    pr = x.sigmoid()[:, 0]
    rowmax, colmax = pr.gather(2, pos[:, :h, None]), pr.gather(1, pos[:, None, h:])
    prj = (dice_coefficient(rowmax, tmax[:, :h]) + dice_coefficient(colmax, tmax[:, h:])).mean()
    wts = t32(ref["weights"])
    pair = (compute_pairwise_term(x, 3, p["d"]) * wts).sum() / wts.sum().clamp(min=1.0) * p["warmup"]
    zero = lambda g: torch.zeros_like(x_all) if g is None else g
    g_prj = zero(torch.autograd.grad(prj, x_all, retain_graph=True, allow_unused=True)[0])
    g_pair = zero(torch.autograd.grad(pair, x_all, allow_unused=True)[0])
    return dict(losses=np.asarray([float(prj.detach()), float(pair.detach())]), grad_prj=g_prj.cpu().double().numpy(),
                grad_pair=g_pair.cpu().double().numpy())


# =============================================================================================================== colour similarity

def srgb_table():
    """the host's table: the sRGB linearisation of byte / 255 in float64"""
    c = np.arange(256, dtype=F64) / 255
    return np.where(c > 0.04045, ((c + 0.055) / 1.055) ** 2.4, c / 12.92)


COLOR_HS, COLOR_WS, COLOR_DS, COLOR_STRIDES = (15, 16, 17, 31, 32, 33), (1, 16, 17), (1, 2, 8), (1, 2, 4)
COLOR = {"h%d_w%d" % (h, w): dict(h=h, w=w, d=COLOR_DS[(i % 3 + 2 * (i // 3)) % 3], stride=COLOR_STRIDES[(i % 3 + i // 3) % 3])
         for i, (h, w) in enumerate((h, w) for h in COLOR_HS for w in COLOR_WS)}
GREY_BELOW, GREY_ABOVE = 23, 24           # grey bytes either side of the 0.008856 branch of Lab


@functools.lru_cache(maxsize=None)
def color_inputs(name, kind):
    """images [2, 3, H, W] (uint8, or fp32 multiples of 1/4), keep [2, H, W] uint8, stride, d, and `honest`: keep without its
    holes at pixels no neighbour read touches"""
    c, g = COLOR[name], _rng("color/" + name)
    h, w, d, s = c["h"], c["w"], c["d"], c["stride"]
    H, W = h * s, w * s
    base = g.randint(0, 256, (2, 3, h, w))
    base[1] = (base[1] // 8) * 8                                # image 1: coarser colours, other content
    img = np.repeat(np.repeat(base, s, 2), s, 3).astype(F64)
    img += g.randint(-6, 7, img.shape)
    img = np.clip(img, 0, 255)
    blocks = [(0, 0), (h - 1, w - 1), (h // 2, 0), (h - 1, 0), (0, w - 1), (h // 3, w // 2)]
    vals = [0.0, 255.0, float(GREY_BELOW), float(GREY_ABOVE), 77.0, 77.0]
    for (y, x), v in zip(blocks, vals):
        img[:, :, y * s:(y + 1) * s, x * s:(x + 1) * s] = v
    if kind == "f32":
        img = np.clip(img + g.randint(-3, 4, img.shape) / 4.0, 0, 255)
        for (y, x), v in zip(blocks, vals):
            img[:, :, y * s:(y + 1) * s, x * s:(x + 1) * s] = v
        y, x = blocks[-1]                                       # a pooled mean exactly 1/4 below the integer 77
        if s == 1:
            img[:, :, y, x] = 76.75
        else:
            img[:, :, y * s:y * s + (1 if s == 2 else 2), x * s:x * s + (1 if s == 2 else 2)] = 76.0
    keep = np.ones((2, H, W), np.uint8)
    honest = keep.copy()
    st = s // 2
    holes = g.rand(2, h, w) < 0.15
    for b, y, x in np.argwhere(holes):
        keep[b, st + s * y, st + s * x] = honest[b, st + s * y, st + s * x] = 0
    if s > 1:                                                   # holes next to strided pixels: they must not matter
        for b, y, x in np.argwhere(g.rand(2, h, w) < 0.3):
            keep[b, s * y + (st + 1) % s, s * x + (st + 1) % s] = 0
            keep[b, s * y + st, s * x + (st + 1) % s] = 0
    images = img.astype(np.uint8) if kind == "u8" else img.astype(F32)
    return dict(name=name, kind=kind, images=images, keep=keep, honest=honest, stride=s, d=d, blocks=blocks)


def pooled_bytes(images, stride):
    bs, _, H, W = images.shape
    mean = images.astype(F64).reshape(bs, 3, H // stride, stride, W // stride, stride).sum((3, 5)) / (stride * stride)
    return np.trunc(np.clip(mean, 0, 255)).astype(np.int64), mean


def lab64(byte):
    """[bs, 3, h, w] BGR bytes -> Lab as V (float64 arithmetic, rounded to fp32 once), with the constants of lab_of"""
    lin = srgb_table()[byte]
    r, gch, b = lin[:, 2], lin[:, 1], lin[:, 0]
    xyz = np.stack([0.412453 * r + 0.357580 * gch + 0.180423 * b, 0.212671 * r + 0.715160 * gch + 0.072169 * b,
                    0.019334 * r + 0.119193 * gch + 0.950227 * b], 1) / np.asarray([0.95047, 1.0, 1.08883])[None, :, None, None]
    f = np.where(xyz > 0.008856, np.cbrt(xyz), 7.787 * xyz + 16.0 / 116.0)
    lab = np.stack([116.0 * f[:, 1] - 16.0, 500.0 * (f[:, 0] - f[:, 1]), 200.0 * (f[:, 1] - f[:, 2])], 1)
    size = np.stack([116.0 * f[:, 1] + 16.0, 500.0 * (f[:, 0] + f[:, 1]), 200.0 * (f[:, 1] + f[:, 2])], 1)
    return V(lab, rnd(lab) + D64 * 8 * size), xyz


def color64(p, keep=None, mutant=None):
    """lab [bs, 3, h, w], sim [bs, 8, h, w] with mag_*.  mutants: "unstrided_mask", "nbr_order", "start_up"."""
    s, d = p["stride"], p["d"]
    keep = p["keep"] if keep is None else keep
    byte, _ = pooled_bytes(p["images"], s)
    lab, _ = lab64(byte)
    bs, _, h, w = byte.shape
    st = (s + 1) // 2 if mutant == "start_up" else s // 2
    padded = np.zeros((bs, st + s * h + 1, st + s * w + 1), np.uint8)
    padded[:, :keep.shape[1], :keep.shape[2]] = keep
    kept = (keep[:, :h, :w] if mutant == "unstrided_mask" else padded[:, st::s, st::s][:, :h, :w]) != 0
    out, mag = np.zeros((bs, 8, h, w)), np.zeros((bs, 8, h, w))
    for k, (oy, ox) in enumerate(offsets(d, transposed=mutant == "nbr_order")):
        nb, inside = _vshift(lab, oy, ox)
        a = sub(lab, nb)
        sq = mul(a, a)
        ss = V(sq.v[:, 0], sq.s[:, 0])
        for ch in (1, 2):
            ss = add(ss, V(sq.v[:, ch], sq.s[:, ch]))
        v = exp_(mul(sqrt_(ss), V(-0.5), exact=True))
        on = inside[None] & (_shift(kept.astype(F64), oy, ox)[0] != 0)
        out[:, k], mag[:, k] = np.where(on, v.v, 0.0), np.where(on, v.s, 0.0)
    return dict(lab=lab.v, mag_lab=lab.s, sim=out, mag_sim=mag, byte=byte)


def color_composition(p, device="cpu"):
    """The project's composition (uninext_amd/boxinst.py: boxinst_targets with fused=False) piece by piece in fp32 on `device`:
    dict(lab, sim) as float64 numpy"""
    import torch
    import torch.nn.functional as Fn
    from uninext_amd.boxinst import get_images_color_similarity, rgb2lab
    s, st = p["stride"], p["stride"] // 2
    batch = torch.from_numpy(p["images"]).to(device)
    down = Fn.avg_pool2d(batch.float(), kernel_size=s, stride=s)[:, [2, 1, 0]]
    sampled = torch.from_numpy(p["keep"]).to(device)[:, st::s, st::s].float()
    labs, sims = [], []
    for b in range(batch.shape[0]):
        lab = torch.as_tensor(rgb2lab(down[b].byte().permute(1, 2, 0).cpu().numpy()), device=device, dtype=torch.float32).permute(2, 0, 1)[None]
        labs.append(lab[0])
        sims.append(get_images_color_similarity(lab, sampled[b], 3, p["d"])[0])
    return dict(lab=torch.stack(labs).cpu().double().numpy(), sim=torch.stack(sims).cpu().double().numpy())


# ===================================================================================================================== box bitmasks

BITMASK_WS, BITMASK_H = (15, 16, 17, 32), 6


def bitmask_boxes(W, H=BITMASK_H):
    nan, inf = float("nan"), float("inf")
    return np.asarray([
        [0.0, 0.0, W - 1.0, H - 1.0], [2.0, 1.0, float(W), float(H)], [1.5, 0.25, W - 1.5, 3.75],     # ending exactly at W - 1 and at W
        [nan, 1.0, 5.0, 3.0], [1.0, nan, 5.0, 3.0], [1.0, 1.0, nan, 3.0], [1.0, 1.0, 5.0, nan],
        [-inf, 0.0, inf, 2.0], [inf, 0.0, inf, 2.0], [2.0, -inf, 4.0, -inf], [0.0, 0.0, -inf, 5.0],
        [-0.5, -0.5, 3.0, 2.0], [-1.0, -1.0, 3.0, 2.0], [-1.5, -1.5, 3.0, 2.0], [2.0, 1.0, -0.5, -0.5], [2.0, 1.0, -1.0, -1.0],
        [2.0, 1.0, -1.5, -1.5], [6.0, 4.0, 3.0, 1.0], [3.0, 2.0, 3.0, 2.0], [3.25, 2.0, 3.75, 2.5], [W + 4.0, 1.0, W + 9.0, 2.0],
        [5.0, 3.0, 3.5, 3.0],                                                                          # inverted by less than a pixel
    ], dtype=F32)


def _trunc_clamped(v, most):
    """boxinst.hip: trunc_clamped, as documented: at least `most` -> most; above -1 -> truncation toward zero; NaN -> most; else 0"""
    v = F32(v)
    if v >= F32(most):
        return most
    if v > F32(-1.0):
        return int(v)
    return most if v != v else 0


def bitmasks_exact(boxes, H, W):
    out = np.zeros((len(boxes), H, W), np.uint8)
    with np.errstate(invalid="ignore"):
        for slot, box in zip(out, np.asarray(boxes, F32)):
            x_lo, x_hi = _trunc_clamped(box[0], W), _trunc_clamped(F32(box[2] + F32(1.0)), W)
            y_lo, y_hi = _trunc_clamped(box[1], H), _trunc_clamped(F32(box[3] + F32(1.0)), H)
            if y_hi > y_lo and x_hi > x_lo:
                slot[y_lo:y_hi, x_lo:x_hi] = 1
    return out


# ========================================================================================================== the error measure

HEAD = "%-15s %-13s %-30s %9s %9s | %9s %9s %9s %9s" % ("kernel", "group", "case", "ratio", "rel err", "comp/s", "comp rel", "comp err", "bound")
_T = PM.Table(HEAD)                                         # printed only: no file is written
TABLE, WORST, report = _T.lines, _T.worst, _T.report        # WORST: (kernel, group) -> dict(ratio, rel, comp_ratio, comp_rel, line)


def measure(kernel, group, case, got, want, mag, comp=None, where=None, check=True, aggregate=True):
    """Every entry of `got` within entry_bound(the composition's error at the entry, s) of `want`, and the project's bound on top.
    Returns the largest error / bound; check=False only returns it (inf for a non-finite entry of `got`) and adds no line.
    where: a report slice (the entries outside it belong to another slice, nothing is left out overall).
    Non-finite: none in `want`, `mag` or `got`; `comp` may be; comp=None: the derived term alone (float64 sums).
    WORST: (kernel, group), the maxima of four columns and the line of the largest ratio.  Line: the largest ratio, relative
    error, composition error / derived term and relative composition error of the slice, then the worst entry's composition error
    and bound (absolute).
    Tolerance: TOL * (max|want| or 1), the maximum taken before slicing; aggregate=False leaves it out (it is the kernels'
    contract, not the composition's)."""
    got, want, mag = (np.atleast_1d(np.asarray(a, dtype=F64)) for a in (got, want, mag))
    comp = want if comp is None else np.atleast_1d(np.asarray(comp, dtype=F64))
    assert got.shape == want.shape == comp.shape == mag.shape, (kernel, group, case, got.shape, want.shape, comp.shape, mag.shape)
    scale = float(np.abs(want).max()) if want.size else 0.0
    where = np.ones(want.shape, bool) if where is None else np.broadcast_to(where, want.shape)
    got, want, mag, comp = got[where], want[where], mag[where], comp[where]
    if not got.size:
        return 0.0
    assert np.isfinite(want).all() and np.isfinite(mag).all(), (kernel, group, case, "reference")
    if not np.isfinite(got).all():
        assert not check, (kernel, group, case, "non-finite entries", int((~np.isfinite(got)).sum()))
        return float("inf")
    e = PM.errors(got, want, mag, comp)
    worst = e.worst
    if not check:
        return worst
    cratio = PM.quotient(e.cerr, SUM_DEPTH * U * mag)               # the composition's error over the derived term
    with np.errstate(divide="ignore", invalid="ignore"):
        rel, crel = np.where(e.size > 0, e.err / e.size, 0.0), np.where(e.size > 0, e.cerr / e.size, 0.0)
    line = "%-15s %-13s %-30s %9.3f %9.2e | %9.2e %9.2e %9.2e %9.2e" % (kernel, group, case, worst, rel.max(), cratio.max(), crel.max(), e.cerr[e.at], e.bound[e.at])
    _T.add(line)
    w = WORST.setdefault((kernel, group), dict(ratio=0.0, rel=0.0, comp_ratio=0.0, comp_rel=0.0, line=line))
    if worst >= w["ratio"]:
        w["line"] = line
    w.update(ratio=max(w["ratio"], worst), rel=max(w["rel"], float(rel.max())), comp_ratio=max(w["comp_ratio"], float(cratio.max())),
             comp_rel=max(w["comp_rel"], float(crel.max())))
    e.check(kernel, group, case)
    assert not aggregate or float(e.err.max()) <= TOL * (scale if scale > 0 else 1.0), (kernel, group, case, "the project's bound", float(e.err.max()), scale)
    return worst


def worst_table():
    head = "%-15s %-13s %9s %9s %9s %9s" % ("kernel", "group", "ratio", "rel err", "comp/s", "comp rel")
    return head + "\n" + "\n".join("%-15s %-13s %9.3f %9.2e %9.2e %9.2e" % (k + (w["ratio"], w["rel"], w["comp_ratio"], w["comp_rel"]))
                                  for k, w in sorted(WORST.items()))
