"""Per-entry parity of the GEMM family (uninext_amd/csrc/gemm_core.hpp and its users linear.hip, patch_embed.hip, conv3x3.hip):
the cases, the inputs, float64 restatements that return every output entry's VALUE and its MAGNITUDE, a numpy restatement of
the bf16 split on the fp32 bit patterns, the fp32 CPU compositions and the measure.  No GPU is needed to import this.
tests/test_gemm_parity_cpu.py checks that the measure has teeth, tests/test_gemm_parity_gpu.py holds the kernels to it.

The split (gemm_core.hpp's header comment is the specification): hi = the upper 16 bits of x, lo = bf16 of the fp32 remainder
x - hi by (bits + 0x8000) >> 16 (nearest, ties away, a carry runs into the exponent as it should), and
a b ~ hi_a lo_b + lo_a hi_b + hi_a hi_b, small terms first, lo_a lo_b dropped.

Three kinds of rule:
  bits     The exact tiers.  E8: both operands have at most 8 significant bits (lo == 0, only hi hi contributes); EX: x has
           up to 16 and w at most 8 (x == hi + lo, the result is hi_x w + lo_x w: lo_a hi_w stands alone); EW: its mirror.
           All values are integers times one power of two per operand, q is the product of the two steps, and
           sum_k |x| |w| + |bias| < 2^24 q at every entry (exact_condition asserts it on the CPU): every partial sum in every
           order is an fp32 number, so the output equals the float64 sum bit for bit -- on the split paths and the exact-fp32
           paths alike.  -0.0 and +0.0 compare equal (a sum that cancels is +0.0, a ReLU may keep either zero); every other
           value is compared through its uint32 view.
  split    The packed paths on dy10 / dy20 inputs against the restated split in float64: entry_bound(comp_err, s) of
           tests/parity_measure.py unchanged, comp_err the error of an fp32 CPU composition of the same three split products
           summed small-first.  Only fp32 accumulation separates the kernel from this reference.
  true     The packed paths against the true float64 product: that bound + SPLIT_EPS s, SPLIT_EPS = 2^-14 + 2^-15.  With
           x = h + l + r (h the truncated hi: |l + r| < 2^-7 |x|; r the rounding of lo: |r| <= 2^-16 |x|) the three products give
           P = ha hb + ha lb + la hb and a b - P = la lb + ra b + (ha + la) rb, at most (2^-14 + 2^-16 + 2^-16) |a| |b|.
           The exact-fp32 paths (conv3x3 precision 0 and the packed exact kernel, patch_embed_forward): entry_bound against
           float64 alone, the composition being torch's fp32 CPU convolution.
A NaN fails every rule.

The magnitude s of an entry is the sum of the absolute summands behind it: sum_k |x| |w| + |bias| (x is x + x_add where there
is one, added in fp32 as the kernel adds it; a masked row has s = 0 and must be an exact zero).
  LayerNorm epilogue (linear_packed_ln, ffn_packed): as tests/convnext_parity.py.  v the value that is normalised, A its own
  magnitude as above (+ |residual|), u = mean v, var = mean (v - u)^2, r = 1 / sqrt(var + eps), o^ = (v - u) r, o = g o^ + b:
  the inner error (a multiple of u32 A) reaches o times r |g|; u moves by at most u32 mean A; v - u rounds by u32 (|v| + |u|);
  r moves by at most r^2 u32 rms A relative to 1 (Cauchy-Schwarz), o by |g| |o^| r times that; the last roundings are relative
  to |o| + |b|:   s = r |g| (A + mean A + |v| + |u| + |o^| rms A) + |o| + |b|.  A row of variance 0 must give b bit for bit.
  Fused FFN: the kernel keeps the hidden layer h = relu(x W1^T + b1) as fp32 numbers, so the split restatement rounds its own
  h to fp32 before the second product.  The kernel's h differs from that by the first product's accumulation error, a
  multiple of u32 A1 (A1 = sum |x| |W1| + |b1|; relu is 1-Lipschitz), which the second product passes on times |W2|:
  A = sum_j (|h_j| + A1_j) |W2_nj| + |b2| + |residual|.  Against the true composition the split term counts twice, once per
  product, and both are inside SPLIT_EPS A.
Nothing in these forms is fitted.

Worst kernel error / bound on an MI355X per entry point and reference (test_gemm_parity_gpu.py's table, committed as
profiles/r35_gemm_parity.txt).  These are measurements; the bounds above are derived and were not tightened to them:
    conv3x3_forward<0>             bits    0 differing entries
    conv3x3_forward<0>             true    0.328   conv/p0/dy20/b2/c16/17x18/o65/b1r0/stress
    conv3x3_forward<1>             bits    0 differing entries
    conv3x3_forward<1>             split   0.383   conv/p1/dy20/b2/c16/17x18/o65/b1r0/stress
    conv3x3_forward<1>             true+   0.161   conv/p1/dy20/b2/c16/17x18/o65/b1r0/stress
    conv3x3_packed_forward         bits    0 differing entries
    conv3x3_packed_forward         split   0.273   conv/p2/dy20/b2/c16/17x18/o65/b1r0/stress
    conv3x3_packed_forward         true+   0.169   conv/p2/dy20/b2/c16/17x18/o65/b1r0/stress
    conv3x3_packed_forward<exact>  bits    0 differing entries
    conv3x3_packed_forward<exact>  true    0.312   conv/p3/dy10/b1/c48/33x47/o130/b1r0
    ffn_packed<4 waves>            split   0.192   ffn/dy10/f128/r65/ln0
    ffn_packed<4 waves>            true+   0.007   ffn/dy10/f128/r64/ln0
    ffn_packed<8 waves>            split   0.097   ffn/dy10/f256/r65/plain
    ffn_packed<8 waves>            true+   0.005   ffn/dy10/f256/r65/plain
    linear_packed_forward          bits    0 differing entries
    linear_packed_forward          split   0.417   lin/dy20/k256/r129/n129/stress
    linear_packed_forward          true+   0.136   lin/dy20/k256/r129/n129/stress
    linear_packed_forward<ex>      bits    0 differing entries
    linear_packed_forward<ex>      split   0.166   lin/dy20/k128/r65/n384/b0m1a1r1
    linear_packed_forward<ex>      true+   0.076   lin/dy20/k128/r129/n129/b0m1a1r0
    linear_packed_forward<hm>      bits    0 differing entries
    linear_packed_forward<hm>      split   0.179   lin/dy10/k128/r195/n64/hm65/b0m0
    linear_packed_forward<hm>      true+   0.082   lin/dy20/k128/r300/n64/hm100/b0m0
    linear_packed_ln               split   0.079   ln/dy20/k256/r65/stress
    linear_packed_ln               true+   0.039   ln/dy20/k256/r65/stress
    linear_packed_split_forward    bits    0 differing entries
    linear_packed_split_forward    split   0.170   lin/dy10/k128/r129/n384/sc128/a1
    linear_packed_split_forward    true+   0.074   lin/dy10/k128/r65/n384/sc256/a0
    patch_embed_forward            bits    0 differing entries
    patch_embed_forward            true    0.335   pe/exact/dy20/k8c3/e130/p1x3x43/nhwc/stress
    patch_embed_packed_forward     bits    0 differing entries
    patch_embed_packed_forward     split   0.196   pe/packed/dy20/k8c3/e130/p1x3x43/nhwc/stress
    patch_embed_packed_forward     true+   0.116   pe/packed/dy10/k4c3/e130/p1x3x43/nhwc
No entry was over its bound and no exact-tier entry off by a bit: the sweep found no kernel bug.
"""
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_measure as PM                                                 # noqa: E402
from parity_measure import COMP_MARGIN, SUM_DEPTH, U, entry_bound          # noqa: E402,F401

SPLIT_EPS = 2.0 ** -14 + 2.0 ** -15
EXACT, BOUNDED = ("E8", "EX", "EW"), ("dy10", "dy20")
TIERS = EXACT + BOUNDED
QX, QW = 2.0 ** -3, 2.0 ** -6          # the steps of x and w in the exact tiers; bias and products step by Q
Q = QX * QW
BUDGET = 2 ** 24
BIAS_TOP = 4095
SENTINEL = 2.0 ** 20                    # what fills the pixel rows and columns a patch embedding must not read
LN_EPS = float(np.float32(1e-5))

# ------------------------------------------------------------------------------------------------------------------ the split

def split(x, truncate_lo=False):
    """fp32 array -> (hi, lo) fp32 arrays holding bf16 values, on the bit patterns as gemm_core::split_pairs has them.
    truncate_lo is the mutant that drops lo's low bits instead of rounding."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    rem = np.ascontiguousarray(x - hi)                       # an fp32 subtraction, exact: the remainder has at most 16 bits
    bits = rem.view(np.uint32)
    if not truncate_lo:
        bits = bits + np.uint32(0x8000)                      # a carry out of the mantissa raises the exponent: still nearest
    return hi, (bits & np.uint32(0xffff0000)).view(np.float32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def mm(a, b):
    """a [M, K] x b [N, K] -> [M, N] in the operands' precision"""
    return (_t(a) @ _t(b).T).numpy()


def conv(stride, pad):
    return lambda a, b: F.conv2d(_t(a), _t(b), stride=stride, padding=pad).numpy()


def product(op, x, w, how="true", drop=None, truncate_lo=False):
    """float64 op(x, w): the true product, or the restated split hi lo + lo hi + hi hi (`drop` one of "hl", "lh", "hh")."""
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    if how == "true":
        return op(f64(x), f64(w))
    assert how == "split"
    (xh, xl), (wh, wl) = split(x, truncate_lo), split(w, truncate_lo)
    terms = (("hl", xh, wl), ("lh", xl, wh), ("hh", xh, wh))
    return sum(op(f64(a), f64(b)) for k, a, b in terms if k != drop)


def split_product(x, w):
    """[M, K] x [N, K]: the float64 value of hi lo + lo hi + hi hi"""
    return product(mm, x, w, "split")


def comp3(op, x, w):
    """fp32: the three split products, each accumulated in fp32 on the CPU, summed small-first"""
    (xh, xl), (wh, wl) = split(x), split(w)
    return (op(xh, wl) + op(xl, wh)) + op(xh, wh)


def sig_bits(a):
    """The number of significant bits of every entry (0 for 0)."""
    m, _ = np.frexp(np.asarray(a, dtype=np.float64))
    k = np.round(np.abs(m) * 2.0 ** 53).astype(np.int64)
    low = k & -k
    return np.where(k == 0, 0, 54 - np.log2(np.maximum(low, 1)).astype(np.int64) - 1).astype(np.int64)


def packed_layout(w2d, taps=1):
    """weight [N, K] -> uint16 [K / 16 groups][hi, lo][N padded to 128][16] as pack_weight_kernel writes it.  taps = 9: k is
    (channel, tap) and group g is tap g % 9 of channels 16 (g / 9) onward.  Rows past N are zero."""
    N, K = w2d.shape
    n_pad = (N + 127) // 128 * 128
    g, kl = np.arange(K // 16)[:, None], np.arange(16)[None, :]
    k = ((g // taps) * 16 + kl) * taps + g % taps                       # [groups, 16]
    hi, lo = split(w2d)
    out = np.zeros((K // 16, 2, n_pad, 16), dtype=np.uint16)
    out[:, 0, :N] = (hi.view(np.uint32) >> 16).astype(np.uint16)[:, k].transpose(1, 0, 2)
    out[:, 1, :N] = (lo.view(np.uint32) >> 16).astype(np.uint16)[:, k].transpose(1, 0, 2)
    return out


def packed_exact_layout(w):
    """conv weight [cout, cin, 3, 3] -> fp32 [cin / 16][9 taps][cout padded to 128][16], position 8 h + s = channel 2 s + h"""
    cout, cin = w.shape[:2]
    n_pad = (cout + 127) // 128 * 128
    pos = np.arange(16)
    cl = 2 * (pos & 7) + (pos >> 3)
    out = np.zeros((cin // 16, 9, n_pad, 16), dtype=np.float32)
    wr = w.reshape(cout, cin // 16, 16, 9)[:, :, cl, :]                  # [cout, chunk, pos, tap]
    out[:, :, :cout] = wr.transpose(1, 3, 0, 2)
    return out


# ---------------------------------------------------------------------------------------- shapes as the kernels' hosts have them

def linear_tiling(rows, N):
    """(TJ, WM) of linear_impl: 64 TJ columns per workgroup, WM waves along the rows (the split column is 0 or a multiple
    of 256 here)."""
    mt = -(-rows // 64)
    if N == 256 and mt * (N // 256) >= 512:
        return 4, 1
    if N > 64 and mt * -(-N // 128) >= 512:
        return 2, 1
    return 1, 2


def conv_tiles(B, H, W):
    return B * -(-W // 16) * -(-H // 8)                                   # kTW = 16, kTH = 8


def conv_exact_unit(B, H, W, cout):
    """conv3x3_hip_packed_exact_f32: 1 = 8 x 16 pixels x 128 channels, 2 = 8 x 16 x 64, 3 = 4 x 16 x 64"""
    t = conv_tiles(B, H, W)
    if cout > 64 and t * -(-cout // 128) >= 2048:
        return 1
    return 2 if t * -(-cout // 64) >= 2048 else 3


def conv_packed_wide(B, H, W, cout):
    return cout > 64 and conv_tiles(B, H, W) * -(-cout // 128) >= 512


def conv_fp32_big(B, H, W, cout):
    return cout > 64 and -(-(B * H * W) // 128) * -(-cout // 128) >= 256


def patch_exact_cfg(M, E, K):
    """patch_embed_hip_f32's tile: 0 = 128 x 128, 1 = 64 x 128, 2 = 64 x 64"""
    if K <= 64:
        return 2
    return 0 if -(-M // 128) * -(-E // 128) >= 256 else 1


def patch_packed_wide(M, E):
    return E > 64 and -(-M // 64) * -(-E // 128) >= 512


# ------------------------------------------------------------------------------------------------------------------- the cases

CASES, GROUPS = {}, {}


def _add(group, name, **spec):
    assert name not in CASES, name
    CASES[name] = spec
    GROUPS.setdefault(group, []).append(name)


LIN_ROWS = (1,      # one row: a tail in the first 32-row MFMA half
            63,     # a tail of one row short of the 64-row tile
            64,     # exactly one tile
            65,     # a second workgroup that owns one row
            127,    # the second tile one short
            129)    # a third workgroup
LIN_NS = (1, 31, 33,            # inside and across the 32-column fragment
          64, 65,               # the 64 TJ columns of the TJ = 1 workgroup and one more
          127, 128, 129,        # the 128-wide weight padding
          256, 384)             # two and three paddings; 384 takes the two-output split
LIN_KS = (64,       # one step of 64 k
          128,      # two: fewer than the ring's three-ahead prefetch can fill
          192,      # exactly the ring depth
          256,      # one more than it (the size the layers use)
          320,      # an odd number of steps
          1024)     # many


def _lin(group, tier, rows, N, K, tag="", **opt):
    spec = dict(kind="lin", tier=tier, rows=rows, N=N, K=K, bias=True, mask=False, x_add=False, relu=False, hm=0, split_col=0,
                stress=False)
    spec.update(opt)
    _add(group, "lin/%s/k%d/r%d/n%d%s" % (tier, K, rows, N, tag), **spec)


for _tier in EXACT:
    for _K in LIN_KS:
        if _K == 1024 and _tier != "E8":
            continue
        _full = _K in (64, 256)
        for _r in (LIN_ROWS if _full else (1, 65, 129)):
            for _n in (LIN_NS if _full else (33, 128, 129, 384)):
                _lin("lin/%s/k%d" % (_tier, _K), _tier, _r, _n, _K)
for _tier in BOUNDED:
    for _K in (128, 320):
        for _r in (65, 129):
            for _n in (33, 129, 384):
                _lin("lin/%s" % _tier, _tier, _r, _n, _K)
_lin("lin/dy20", "dy20", 65, 129, 1024)
_lin("lin/dy20", "dy20", 129, 129, 256, "/stress", stress=True)
# The three tilings at K = 64 by row count alone (linear_tiling above restates linear_impl; _lib.last_kernel has no entry for this
# family).  TJ = 2: mt ceil(N / 128) >= 512, so N = 384 needs mt = 171 = rows 10881 (a tail of one row) and N = 129 (a 128-column
# workgroup that owns one column) mt = 256 = rows 16321; TJ = 4: N == 256 and mt = 512 = rows 32705.  rows - 1 is a full last
# tile on the other side of the threshold (TJ = 1; TJ = 2 at N = 256, whose 511 x 2 workgroups are past that rule's 512), rows +
# 62 a tail of 63 rows.  (N, rows, the tiling, the tiling of rows - 1)
LIN_TILINGS = ((384, 10881, (2, 1), (1, 2)), (129, 16321, (2, 1), (1, 2)), (256, 32705, (4, 1), (2, 1)))
for _n, _r, _tj, _below in LIN_TILINGS:
    for _rr in (_r - 1, _r, _r + 62):
        _lin("lin/tiling/n%d" % _n, "E8", _rr, _n, 64, "/tiling")
    _lin("lin/tiling/n%d" % _n, "dy20", _r, _n, 64, "/tiling")
# options, crossed at the tail shapes
for _tier in TIERS:
    for _r in (65, 129):
        for _n in (129, 384):
            for _o in range(16):
                _b, _m, _a, _re = bool(_o & 1), bool(_o & 2), bool(_o & 4), bool(_o & 8)
                _lin("lin/opt/%s" % _tier, _tier, _r, _n, 128, "/b%dm%da%dr%d" % (_b, _m, _a, _re), bias=_b, mask=_m, x_add=_a,
                     relu=_re)
    for _rpi in (64, 65, 100):          # three images: a 64-row tile straddles an image boundary unless rows_per_image is 64
        for _n in (64, 128):
            for _b, _m in ((True, True), (False, False)):
                _lin("lin/hm/%s" % _tier, _tier, 3 * _rpi, _n, 128, "/hm%d/b%dm%d" % (_rpi, _b, _m), hm=_rpi, bias=_b, mask=_m)
    for _r in (65, 129):
        for _sc in (128, 256):
            for _a in (False, True):
                _lin("lin/split/%s" % _tier, _tier, _r, 384, 128, "/sc%d/a%d" % (_sc, _a), split_col=_sc, x_add=_a)

LN_CFGS = {"all": (True, True, True), "none": (False, False, False), "res": (True, False, False),
           "affine": (False, True, False), "bias": (False, False, True)}          # residual, gamma / beta, bias
for _tier in BOUNDED:
    for _r in (1, 63, 64, 65):
        for _K in (64, 256):
            for _cfg, (_res, _aff, _b) in LN_CFGS.items():
                _add("ln/%s" % _tier, "ln/%s/k%d/r%d/%s" % (_tier, _K, _r, _cfg), kind="ln", tier=_tier, rows=_r, K=_K, N=256,
                     residual=_res, affine=_aff, bias=_b, stress=False)
_add("ln/dy20", "ln/dy20/k256/r65/stress", kind="ln", tier="dy20", rows=65, K=256, N=256, residual=True, affine=True, bias=True,
     stress=True)

FFN_DS = (128,      # the 4-wave kernel, one hidden tile
          256,      # the 8-wave kernel, one hidden tile
          384,      # 4 waves, three tiles
          1024)     # 8 waves, four tiles
for _tier in BOUNDED:
    for _f in FFN_DS:
        for _r in (1, 63, 64, 65):
            for _ln in (False, True):
                _add("ffn/%s" % _tier, "ffn/%s/f%d/r%d/ln%d" % (_tier, _f, _r, _ln), kind="ffn", tier=_tier, rows=_r, F=_f,
                     layer_norm=_ln, plain=False, negative=False, stress=False)
        _add("ffn/%s" % _tier, "ffn/%s/f%d/r65/plain" % (_tier, _f), kind="ffn", tier=_tier, rows=65, F=_f, layer_norm=False,
             plain=True, negative=False, stress=False)
        _add("ffn/%s" % _tier, "ffn/%s/f%d/r65/negative" % (_tier, _f), kind="ffn", tier=_tier, rows=65, F=_f, layer_norm=False,
             plain=False, negative=True, stress=False)
_add("ffn/dy20", "ffn/dy20/f384/r65/stress", kind="ffn", tier="dy20", rows=65, F=384, layer_norm=True, plain=False,
     negative=False, stress=True)

# patch embedding: (patch, channels) -> C k k
PE_PACKED = ((4, 3), (2, 12),       # 48: one step of the packed kernel
             (4, 6), (2, 24),       # 96
             (8, 3), (4, 12),       # 192
             (16, 3))               # 768
PE_EXACT_ONLY = ((4, 2), (2, 8),    # 32
                 (4, 5))            # 80: no packed path (not a multiple of 48)
PE_ES = (1, 31, 33, 127, 128, 129, 130)
PE_GRIDS = {1: (1, 1, 1), 127: (1, 127, 1), 128: (2, 8, 8), 129: (1, 3, 43)}       # patches -> (B, Hp, Wp)


def _pe(group, tier, path, k, C, E, grid, cl, extra=(1, 1), tag="", stress=False):
    B, Hp, Wp = grid
    # extra pixel rows / columns (< patch) that belong to no patch; an odd width leaves rows only 4-byte aligned
    _add(group, "pe/%s/%s/k%dc%d/e%d/p%dx%dx%d/%s%s" % (path, tier, k, C, E, B, Hp, Wp, "nhwc" if cl else "nchw", tag), kind="pe",
         tier=tier, path=path, k=k, C=C, E=E, B=B, Hp=Hp, Wp=Wp, H=Hp * k + extra[0], W=Wp * k + extra[1], cl=cl, stress=stress)


for _path in ("packed", "exact"):
    for _tier in TIERS:
        _exact = _tier in EXACT
        for _k, _C in PE_PACKED + (PE_EXACT_ONLY if _path == "exact" else ()):
            for _p, _grid in PE_GRIDS.items():
                if not _exact and _p not in (1, 129):
                    continue
                for _E in (PE_ES if _p in (1, 129) and _exact else (33, 130)):
                    for _cl in (True, False):
                        _pe("pe/%s/%s/k%dc%d" % (_path, _tier, _k, _C), _tier, _path, _k, _C, _E, _grid, _cl)
        # an image that is a whole number of patches, 16-byte aligned rows
        _pe("pe/%s/%s/k4c3" % (_path, _tier), _tier, _path, 4, 3, 130, PE_GRIDS[129], True, extra=(0, 0), tag="/whole")
    # 16384 patches x 130 columns: the packed kernel's 128-column workgroups (256 row tiles x 2 >= 512) and the exact kernel's
    # 128 x 128 tiles (128 x 2 >= 256) -- the smallest patch count that reaches either with two column tiles
    for _cl in (True, False):
        _pe("pe/%s/big" % _path, "E8", _path, 2, 24, 130, (1, 128, 128), _cl, tag="/big")
    _pe("pe/%s/dy20/k8c3" % _path, "dy20", _path, 8, 3, 130, PE_GRIDS[129], True, tag="/stress", stress=True)

# conv3x3: H x W of test_conv3x3_gpu.py's test_vs_oracle (every residue of W mod 4, W < 4, 1 x 1) and the widths 16, 17 and 18
# around the 16-pixel tile and its halo
CONV_HW = ((5, 7), (33, 47), (6, 5), (3, 2), (17, 18), (1, 1), (4, 21), (9, 16), (8, 17), (100, 167), (9, 300))
CONV_COUTS = (1, 8, 63, 64, 65, 128, 130)
CONV_PRECISIONS = (0, 1, 2, 3)          # 0 exact fp32; 1 split; 2 split from packed weights; 3 exact fp32 from packed weights
# The larger units of the exact kernel at cin = 16: tiles ceil(cout / 64 or 128) >= 2048 with cout <= 128 needs 2048 tiles of
# 8 x 16 pixels: B = 2 images of 32 x 32 tiles, the smallest being H = 8 * 31 + 1, W = 16 * 31 + 1.  cout = 65 selects unit 1
# (and the packed kernel's 128-channel workgroups and precision 0's 128 x 128 tiles), cout = 8 unit 2.
CONV_BIG = (2, 249, 497)


def _cv(group, tier, prec, B, cin, H, W, cout, bias=True, relu=False, tag="", stress=False):
    _add(group, "conv/p%d/%s/b%d/c%d/%dx%d/o%d/b%dr%d%s" % (prec, tier, B, cin, H, W, cout, bias, relu, tag), kind="conv",
         tier=tier, prec=prec, B=B, cin=cin, H=H, W=W, cout=cout, bias=bias, relu=relu, stress=stress)


for _prec in CONV_PRECISIONS:
    for _tier in TIERS:
        _g = "conv/p%d/%s" % (_prec, _tier)
        if _tier in EXACT:
            for _H, _W in CONV_HW:
                _big = _H * _W > 2000
                for _o in ((8,) if _big else (8, 65)):
                    _cv(_g, _tier, _prec, 1 if _big else 2, 16, _H, _W, _o)
            for _o in CONV_COUTS:
                for _H, _W in ((17, 18), (6, 5)):
                    if _o not in (8, 65):
                        _cv(_g, _tier, _prec, 1, 16, _H, _W, _o)
        for _H, _W in ((17, 18), (6, 5), (33, 47)):
            if _tier in BOUNDED:
                _cv(_g, _tier, _prec, 2, 16, _H, _W, 65)
            for _cin, _o in ((32, 65), (48, 130)):
                _cv(_g, _tier, _prec, 1, _cin, _H, _W, _o)
        for _b, _re in ((False, False), (True, True), (False, True)):
            _cv(_g, _tier, _prec, 2, 16, 17, 18, 65, bias=_b, relu=_re)
    for _o in (65, 8):
        _cv("conv/p%d/big" % _prec, "E8", _prec, CONV_BIG[0], 16, CONV_BIG[1], CONV_BIG[2], _o, tag="/big")
    _cv("conv/p%d/dy20" % _prec, "dy20", _prec, 2, 16, 17, 18, 65, tag="/stress", stress=True)


def names(group):
    return list(GROUPS[group])


def groups(prefix):
    return [g for g in GROUPS if g.startswith(prefix)]


# ------------------------------------------------------------------------------------------------------------------ the inputs

def _small(rs, shape, top):
    return rs.randint(-top, top + 1, size=shape).astype(np.float64)


def _wide(rs, shape, top16, K):
    """16-significant-bit integers in about 16 places of every K (an eighth at most), 8-bit ones elsewhere: the budget 2^24 q
    leaves the other operand a few bits more than it would with 16 bits everywhere"""
    frac = min(0.125, 16.0 / K)
    big = rs.randint(2 ** 15, top16 + 1, size=shape) * rs.choice((-1.0, 1.0), size=shape)
    return np.where(rs.rand(*shape) < frac, big, _small(rs, shape, 255))


def _bounded(tier, rs, shape):
    if tier == "dy10":
        return PM.dy(rs.randn(*shape))
    v = np.round(rs.uniform(-8.0, 8.0, size=shape) * 2.0 ** 20)         # multiples of 2^-20 below 8: up to 23 significant bits
    return (np.clip(v, -(2.0 ** 23 - 1), 2.0 ** 23 - 1) / 2.0 ** 20 + 0.0).astype(np.float32)


def _feature_scales(rs, n):
    """powers of two over 10^-4 .. 10^4"""
    return 2.0 ** rs.randint(-13, 14, size=n)


def _operands(name, tier, xshape, wshape, nbias, op, with_add=False, sparse=False, stress_axis=None):
    """x, x_add (or None), w, bias as fp32 arrays.  op(|x|, ones) gives the sum of |x| behind every entry of one output
    column: the exact tiers size the other operand by it."""
    rs = PM.rng(name)
    if tier in BOUNDED:
        x, w = _bounded(tier, rs, xshape), _bounded(tier, rs, wshape)
        xa = _bounded(tier, rs, xshape) if with_add else None
        if stress_axis is not None:
            sc = _feature_scales(rs, xshape[stress_axis]).reshape([-1 if a == stress_axis else 1 for a in range(len(xshape))])
            x = (x * sc).astype(np.float32)
            xa = None if xa is None else (xa * sc).astype(np.float32)
        return x, xa, w, _bounded(tier, rs, (nbias,))
    room, K = BUDGET - 1 - BIAS_TOP, int(np.prod(wshape[1:]))
    ones = np.ones((1,) + tuple(wshape[1:]))
    keep = (rs.rand(*xshape) < 0.25) if sparse else 1.0
    if tier in ("E8", "EX"):
        if tier == "E8":
            xi = _small(rs, xshape, 127 if with_add else 255) * keep
        else:
            xi = _wide(rs, xshape, 2 ** 16 - 1 - (127 if with_add else 0), K) * keep
        xa = _small(rs, xshape, 127) * keep if with_add else None
        behind = float(op(np.abs(xi + (0.0 if xa is None else xa)), ones).max())
        cap = int(min(255, room // max(behind, 1.0)))
        assert cap >= 2, (name, "no room for w", behind)
        wi = _small(rs, wshape, cap)
    else:
        wi = _wide(rs, wshape, 2 ** 16 - 1, K)
        cap = int(min(255, room // np.abs(wi).reshape(wshape[0], -1).sum(1).max()))
        if with_add:
            cap //= 2
        assert cap >= 2, (name, "no room for x")
        xi = _small(rs, xshape, cap) * keep
        xa = _small(rs, xshape, cap) * keep if with_add else None
    f32 = lambda a, q: None if a is None else (a * q + 0.0).astype(np.float32)
    return f32(xi, QX), f32(xa, QX), f32(wi, QW), f32(_small(rs, (nbias,), BIAS_TOP), Q)


def lin_mask(rows):
    """Masked rows: the last (tail) row, every row of the second tile where there is a third, and every seventh."""
    m = np.arange(rows) % 7 == 3
    m[rows - 1] = True
    if rows > 128:
        m[64:128] = True
    return m


@functools.lru_cache(maxsize=4)
def inputs(name):
    """The fp32 numpy inputs of a case (None where an option is off): computed once, shared, left unchanged."""
    c = CASES[name]
    tier, kind = c["tier"], c["kind"]
    if kind == "lin":
        x, xa, w, b = _operands(name, tier, (c["rows"], c["K"]), (c["N"], c["K"]), c["N"], mm, c["x_add"], c["K"] == 1024,
                                1 if c["stress"] else None)
        return dict(x=x, x_add=xa, w=w, bias=b if c["bias"] else None, mask=lin_mask(c["rows"]) if c["mask"] else None)
    if kind == "ln":
        rows = c["rows"]
        x, _, w, b = _operands(name, tier, (rows, c["K"]), (256, c["K"]), 256, mm, False, False, 1 if c["stress"] else None)
        rs = PM.rng(name + "/ln")
        res = _bounded(tier, rs, (rows, 256)) if c["residual"] else None
        if rows > 1:                                     # row 0 is constant: variance 0, the output is beta
            x[0] = 0.0
            if res is not None:
                res[0] = 3.0 - (b if c["bias"] else 0.0)
        if res is not None:
            res[1::3] += 100.0                            # rows of mean 100
        return dict(x=x, w=w, bias=b if c["bias"] else None, residual=res,
                    gamma=_bounded(tier, rs, (256,)) if c["affine"] else None, beta=_bounded(tier, rs, (256,)) if c["affine"] else None)
    if kind == "ffn":
        rows, Fd = c["rows"], c["F"]
        x, _, w1, b1 = _operands(name, tier, (rows, 256), (Fd, 256), Fd, mm, False, False, 1 if c["stress"] else None)
        rs = PM.rng(name + "/ffn")
        w2, b2 = _bounded(tier, rs, (256, Fd)), _bounded(tier, rs, (256,))
        if c["negative"]:
            b1 = np.full(Fd, -2.0 ** 15, dtype=np.float32)          # |x W1| <= 256 * 8 * 8 < 2^15: every pre-activation is negative
        res = _bounded(tier, rs, (rows, 256))
        if c["plain"]:
            b1 = b2 = res = None
        ln = c["layer_norm"]
        return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, residual=res, gamma=_bounded(tier, rs, (256,)) if ln else None,
                    beta=_bounded(tier, rs, (256,)) if ln else None)
    if kind == "pe":
        k, hh, ww = c["k"], c["Hp"] * c["k"], c["Wp"] * c["k"]
        x, _, w, b = _operands(name, tier, (c["B"], c["C"], hh, ww), (c["E"], c["C"], k, k), c["E"], conv(k, 0), False, False,
                               1 if c["stress"] else None)
        full = np.full((c["B"], c["C"], c["H"], c["W"]), SENTINEL, dtype=np.float32)
        full[:, :, :hh, :ww] = x
        return dict(x=full, w=w, bias=b)
    assert kind == "conv"
    x, _, w, b = _operands(name, tier, (c["B"], c["cin"], c["H"], c["W"]), (c["cout"], c["cin"], 3, 3), c["cout"], conv(1, 1),
                           False, False, 1 if c["stress"] else None)
    return dict(x=x, w=w, bias=b if c["bias"] else None)


def _op(c):
    return {"lin": mm, "pe": conv(c.get("k"), 0), "conv": conv(1, 1)}[c["kind"]]


def _x_used(c, i):
    """The activation operand as the kernel multiplies it: x + x_add in fp32; the pixels that belong to a patch."""
    x = i["x"]
    if c["kind"] == "lin" and i["x_add"] is not None:
        x = x + i["x_add"]
    if c["kind"] == "pe":
        x = x[:, :, :c["Hp"] * c["k"], :c["Wp"] * c["k"]]
    return np.ascontiguousarray(x)


def exact_condition(name):
    """Asserts what makes an exact-tier case exact: the steps, the significant-bit budget (of x + x_add where there is one) and
    sum |x| |w| + |bias| < 2^24 q at every entry.  Returns the largest sum in units of q."""
    c, i = CASES[name], inputs(name)
    tier = c["tier"]
    assert tier in EXACT and c["kind"] in ("lin", "pe", "conv"), name
    x, w = _x_used(c, i), i["w"]
    if c["kind"] == "lin" and i["x_add"] is not None:
        assert np.array_equal(x.astype(np.float64), i["x"].astype(np.float64) + i["x_add"].astype(np.float64)), (name, "x + x_add is exact")
    step = lambda a, q: np.array_equal(np.round(a.astype(np.float64) / q) * q, a.astype(np.float64))
    assert step(x, QX) and step(w, QW) and (i["bias"] is None or step(i["bias"], Q)), (name, "steps")
    bx, bw = int(sig_bits(x).max()), int(sig_bits(w).max())
    assert bx <= (16 if tier == "EX" else 8) and bw <= (16 if tier == "EW" else 8), (name, bx, bw)
    if tier != "E8" and min(x.size, w.size) >= 64:
        assert (bx if tier == "EX" else bw) > 8, (name, "the wide operand uses its low half")
    total = _op(c)(np.abs(x).astype(np.float64), np.abs(w).astype(np.float64))
    if i["bias"] is not None:
        total = total + _chan(c, np.abs(i["bias"]).astype(np.float64))
    top = float(total.max()) / Q
    assert top < BUDGET, (name, top)
    return top


# ------------------------------------------------------------------------------------------------------------ the restatements

def _chan(c, v):
    """a per-output-feature vector, shaped to broadcast over the product's layout"""
    return v[None, :] if c["kind"] == "lin" else v[None, :, None, None]


def _flat_neighbour_pad(x):
    """The mutant's padding: a tap left or right of the image reads the neighbouring pixel of the flat row-major plane (the
    previous row's last, the next row's first) instead of zero."""
    B, C, H, W = x.shape
    flat = np.concatenate((np.zeros((B, C, 1), x.dtype), x.reshape(B, C, -1), np.zeros((B, C, 1), x.dtype)), -1)
    out = np.zeros((B, C, H + 2, W + 2), x.dtype)
    out[:, :, 1:-1, 1:-1] = x
    idx = np.arange(H) * W
    out[:, :, 1:-1, 0] = flat[:, :, idx]                 # flat index y W - 1, shifted by the leading zero
    out[:, :, 1:-1, -1] = flat[:, :, idx + W + 1]
    return out


def _layout(c, v):
    """The product's layout ([rows, N] or NCHW) -> {output: array} as the entry point returns it"""
    if c["kind"] == "lin":
        if c["hm"]:
            return {"out": v.reshape(-1, c["hm"], c["N"] // 32, 32).transpose(0, 2, 1, 3)}
        if c["split_col"]:
            return {"out_a": v[:, :c["split_col"]], "out_b": v[:, c["split_col"]:]}
    if c["kind"] == "pe" and c["cl"]:
        return {"out": v.transpose(0, 2, 3, 1)}
    return {"out": v}


MUTANTS = ("drop_lh", "drop_hl", "truncate_lo", "skip_last_chunk", "tail_row", "bias_shift", "mask_left", "edge_tap", "swap_taps")


def _layer_norm(v, A, gamma, beta, eps=LN_EPS):
    g = np.ones(v.shape[-1]) if gamma is None else gamma.astype(np.float64)
    b = np.zeros(v.shape[-1]) if beta is None else beta.astype(np.float64)
    u = v.mean(-1, keepdims=True)
    r = 1.0 / np.sqrt(((v - u) ** 2).mean(-1, keepdims=True) + eps)
    oh = (v - u) * r
    o = g * oh + b
    rms = np.sqrt((A ** 2).mean(-1, keepdims=True))
    s = r * np.abs(g) * (A + A.mean(-1, keepdims=True) + np.abs(v) + np.abs(u) + np.abs(oh) * rms) + np.abs(o) + np.abs(b)
    return o, s


def _f64(a):
    return None if a is None else a.astype(np.float64)


def restate(name, how="true", mutant=None):
    """{output: (value, magnitude)} in float64.  how: "true" or "split".  mutant: one of MUTANTS (the CPU test's teeth)."""
    assert mutant is None or mutant in MUTANTS
    c, i = CASES[name], inputs(name)
    kind = c["kind"]
    if kind == "ln":
        v = product(mm, i["x"], i["w"], how)
        A = mm(np.abs(_f64(i["x"])), np.abs(_f64(i["w"])))
        for t in (i["bias"], i["residual"]):
            if t is not None:
                v, A = v + _f64(t), A + np.abs(_f64(t))
        return {"out": _layer_norm(v, A, i["gamma"], i["beta"])}
    if kind == "ffn":
        x, w1, w2 = i["x"], i["w1"], i["w2"]
        pre = product(mm, x, w1, how)
        A1 = mm(np.abs(_f64(x)), np.abs(_f64(w1)))
        if i["b1"] is not None:
            pre, A1 = pre + _f64(i["b1"]), A1 + np.abs(_f64(i["b1"]))
        h = np.maximum(pre, 0.0)
        if how == "split":
            h = h.astype(np.float32)                     # the kernel keeps the hidden layer as fp32 numbers
        v = product(mm, h, w2, how)
        A = mm(np.abs(_f64(h)) + A1, np.abs(_f64(w2)))
        for t in (i["b2"], i["residual"]):
            if t is not None:
                v, A = v + _f64(t)[None] if t.ndim == 1 else v + _f64(t), A + np.abs(_f64(t))
        if c["layer_norm"]:
            return {"out": _layer_norm(v, A, i["gamma"], i["beta"])}
        return {"out": (v, A)}
    x, w, bias = _x_used(c, i), i["w"], i["bias"]
    op = _op(c)
    if mutant == "skip_last_chunk":                      # the last group of 16 k of the packed order
        w = w.copy()
        if kind == "conv":
            w[:, -16:, 2, 2] = 0.0
        else:
            w.reshape(w.shape[0], -1)[:, -16:] = 0.0
    if mutant == "swap_taps":
        w = np.ascontiguousarray(w.transpose(0, 1, 3, 2))
    if mutant == "edge_tap":
        x, op = _flat_neighbour_pad(x), conv(1, 0)
        x = np.pad(x[:, :, 1:-1], ((0, 0), (0, 0), (1, 1), (0, 0)))     # rows above and below stay zero
    drop = {"drop_lh": "lh", "drop_hl": "hl"}.get(mutant)
    v = product(op, x, w, how, drop, mutant == "truncate_lo")
    s = op(np.abs(_f64(x)), np.abs(_f64(w)))
    if bias is not None:
        b = np.roll(bias, 1) if mutant == "bias_shift" else bias
        v, s = v + _chan(c, _f64(b)), s + _chan(c, np.abs(_f64(bias)))
    if c.get("relu"):
        v = np.maximum(v, 0.0)
    if kind == "lin" and i["mask"] is not None:
        m = i["mask"].copy()
        if mutant == "mask_left":
            m[np.flatnonzero(m)[-1]] = False
        v, s = np.where(m[:, None], 0.0, v), np.where(i["mask"][:, None], 0.0, s)
    if mutant == "tail_row":                             # the last row / pixel takes its neighbour's accumulator
        v = v.copy()
        if kind == "lin":
            v[-1] = v[-2]
        else:
            vf = v.reshape(v.shape[0], v.shape[1], -1)
            vf[:, :, -1] = vf[:, :, -2]
    lv, ls = _layout(c, v), _layout(c, s)
    return {k: (np.ascontiguousarray(lv[k]), np.ascontiguousarray(ls[k])) for k in lv}


@functools.lru_cache(maxsize=4)
def reference(name, how="true"):
    return restate(name, how)


def packed_path(name):
    """True where the entry point multiplies split-bf16 products (held to the restated split and, with SPLIT_EPS, to the true
    product); False on the exact-fp32 paths."""
    c = CASES[name]
    if c["kind"] == "pe":
        return c["path"] == "packed"
    return c["kind"] != "conv" or c["prec"] in (1, 2)


def composition(name):
    """{output: float64 numpy} of the fp32 CPU composition: the three split products summed small-first on the packed paths,
    torch's fp32 convolution on the exact ones; the epilogue in fp32.  It never runs the kernels."""
    c, i = CASES[name], inputs(name)
    kind = c["kind"]
    f = lambda a: None if a is None else _t(a)
    with torch.no_grad():
        if kind in ("ln", "ffn"):
            if kind == "ln":
                v = _t(comp3(mm, i["x"], i["w"]))
                extra, ln = (i["bias"], i["residual"]), True
            else:
                h = _t(comp3(mm, i["x"], i["w1"]))
                h = torch.relu(h if i["b1"] is None else h + f(i["b1"]))
                v = _t(comp3(mm, h.numpy(), i["w2"]))
                extra, ln = (i["b2"], i["residual"]), c["layer_norm"]
            for t in extra:
                if t is not None:
                    v = v + f(t)
            if ln:
                v = F.layer_norm(v, (256,), f(i["gamma"]), f(i["beta"]), LN_EPS)
            assert v.dtype == torch.float32
            return {"out": v.double().numpy()}
        x, op = _x_used(c, i), _op(c)
        v = comp3(op, x, i["w"]) if packed_path(name) else op(x, i["w"])
        assert v.dtype == np.float32
        if i["bias"] is not None:
            v = v + _chan(c, i["bias"])
        if c.get("relu"):
            v = np.maximum(v, np.float32(0.0))
        if kind == "lin" and i["mask"] is not None:
            v = np.where(i["mask"][:, None], np.float32(0.0), v)
        assert v.dtype == np.float32
        return {k: np.ascontiguousarray(a).astype(np.float64) for k, a in _layout(c, v).items()}


# ---------------------------------------------------------------------------------------------------------- the error measure

HEAD = "%-52s %-28s %-5s %10s %10s %10s %8s" % ("case", "entry point", "ref", "kernel err", "comp err", "bound", "ratio")
_T = PM.Table(HEAD, env="GEMM_PARITY_TABLE")
TABLE, WORST, report = _T.lines, _T.worst, _T.report        # WORST: (entry point, ref) -> (ratio, table line)


def _np64(got):
    return got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)


def bit_mismatches(got, want):
    """The entries of fp32 `got` whose bits differ from float64 `want` (which must be an fp32 number); -0.0 equals +0.0."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    w32 = want.astype(np.float32)
    assert np.array_equal(w32.astype(np.float64), want), "the reference is not an fp32 number: the case is not exact"
    return np.argwhere((got + np.float32(0.0)).view(np.uint32) != (w32 + np.float32(0.0)).view(np.uint32))


def measure_bits(case, entry, what, got, want, check=True):
    """An exact-tier output: every entry equal in bits.  Returns the number of entries that differ."""
    bad = bit_mismatches(got, want)
    if check:
        _T.add("%-52s %-28s %-5s %10d %10s %10s %8s" % (case, entry, "bits", len(bad), "-", "-", "-"), (entry, "bits"), float(len(bad)))
        assert len(bad) == 0, (case, entry, what, "entries differ in bits", len(bad), bad[:8].tolist())
    return len(bad)


def measure(case, entry, what, got, want, mag, comp, ref, check=True):
    """Every entry of `got` within entry_bound(the composition's error at the entry, s) of `want`; ref = "true" on a packed path
    adds SPLIT_EPS s (`comp` then is still compared with the SPLIT reference by the caller: pass its error through `comp` =
    want + that error).  Returns the largest error / bound; check=False only returns it and adds no line.  A NaN fails."""
    got = _np64(got)
    assert got.shape == want.shape == comp.shape == mag.shape, (case, what, got.shape, want.shape, comp.shape, mag.shape)
    assert np.isfinite(want).all() and np.isfinite(comp).all() and np.isfinite(mag).all(), (case, what, "a finite reference")
    finite = bool(np.isfinite(got).all())
    if not finite and not check:
        return float("inf")
    assert finite, (case, entry, what, "NaN or infinity", np.argwhere(~np.isfinite(got))[:8].tolist())
    e = PM.errors(got, want, mag, comp)
    if ref == "true+eps":
        e.bound = e.bound + SPLIT_EPS * mag
        e.ratio = PM.quotient(e.err, e.bound)
    if not check:
        return e.worst
    _T.add("%-52s %-28s %-5s %10.2e %10.2e %10.2e %8.3f" % ((case, entry, ref[:5]) + e.row()), (entry, ref), e.worst)
    e.check(case, entry, what, ref)
    return e.worst


def hold(name, entry, got, check=True):
    """`got` {output: fp32 array or tensor} of a case under its tier's rule.  Returns {rule: worst}."""
    c = CASES[name]
    worst = {}
    if c["tier"] in EXACT:
        true = reference(name, "true")
        worst["bits"] = sum(measure_bits(name, entry, what, got[what], want, check) for what, (want, _) in true.items())
        return worst
    comp = composition(name)
    true = reference(name, "true")
    if not packed_path(name):
        worst["true"] = max(measure(name, entry, what, got[what], want, mag, comp[what], "true", check) for what, (want, mag) in true.items())
        return worst
    spl = reference(name, "split")
    worst["split"] = max(measure(name, entry, what, got[what], want, mag, comp[what], "split", check) for what, (want, mag) in spl.items())
    # the composition's error is its distance from the SPLIT reference; hand the true reference a composition that far from it
    worst["true+eps"] = max(measure(name, entry, what, got[what], want, mag, want + (comp[what] - spl[what][0]), "true+eps", check)
                            for what, (want, mag) in true.items())
    return worst
