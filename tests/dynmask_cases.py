"""Shared by tests/test_dynmask_parity_cpu.py and tests/test_dynmask_parity_gpu.py: the dynamic mask head restated in plain
PyTorch with a `dtype` argument (the float64 reference the kernels of include/dynmask_hip.h are held against), the sweep of
shapes that reach the kernels' own edges, the error measure per gradient GROUP, and the bound of every entry.

The restatement follows oracle/dynmask_torch.py step by step (relative coordinates through `.float()` as ddetrs_dn.py:783 has
them, cat([rel, feats]), the reference's parameter order w0 w1 w2 b0 b1 b2, aligned_bilinear) but keeps the dtype it is given
and is differentiable; tests/test_dynmask_parity_cpu.py pins it to the reference-minted dynmask_bwd_* fixtures in float64.

Inputs are seeded float32 values cast exactly to float64, so both sides see the same numbers.  Every seed is chosen (by
`python tests/dynmask_cases.py`, a search on the CPU) so that NO ReLU pre-activation of the float64 restatement is within
float32 rounding of zero -- the kink condition below -- hence no unit may legitimately switch in the kernel and nothing has to
be left out of a comparison."""
import functools
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.dynmask_torch import upsample_aligned  # noqa: E402
# U: float32 unit round-off.  COMP_MARGIN: the kernel and the composition add the same terms in different orders.
# u * SUM_DEPTH * sum |summand|: per-thread chain (1), butterfly (6), waves (3), slices (<= 2), summand
from parity_measure import COMP_MARGIN, SUM_DEPTH, U  # noqa: E402

KINK = 64 * U                   # |a| >= KINK * (|b| + sum |w_i x_i|): the fp32 chain's forward error is <= 11 u sum|terms|
STRIDE = 8
DYN = 8                         # dynamic channels

# name -> H, W, instances per image, up-sampling factors, rel_coord settings: the smallest shapes that reach each edge
SHAPES = {
    "one_pixel": (1, 1, [1], (1, 2), (True, False)),                  # HW = 1; aligned_bilinear_bwd with h = w = 1
    "row": (1, 37, [2], (2, 3), (True, False)),                       # one-row image in the up-sampling gather
    "column": (37, 1, [2], (2, 3), (True, False)),                    # one-column image
    "one_slice_tail": (9, 14, [2, 0, 3], (2,), (True, False)),        # 126 < 256 threads; feats chunk with 2 idle threads; empty image in the middle
    "feats_chunk_128": (8, 16, [1], (1,), (True, False)),             # exactly one feats chunk; one instance: no second staging buffer
    "feats_chunk_129": (3, 43, [1], (1,), (True, False)),             # one pixel into a second chunk
    "two_slices": (17, 16, [3], (4,), (True, False)),                 # parts = 2, 136 pixels each
    "three_slices_uneven": (23, 23, [0, 4, 1], (2,), (True, False)),  # parts = 3, per = 177, last slice 175; leading empty image
    "many_instances": (2, 3, [1025], (1,), (True, False)),            # 1024 / n_all = 0, clamped to one slice
    "trailing_empty": (5, 7, [2, 0], (3,), (True, False)),            # last image empty: its grad_feats exactly zero
    "far_reference": (9, 14, [3], (2,), (True,)),                     # reference points at the image corners: |rel| largest
}
# (shape name, rel_coord) -> seed with the kink condition, found by `python tests/dynmask_cases.py`
SEEDS = {
    ("one_pixel", True): 1, ("one_pixel", False): 1, ("row", True): 1, ("row", False): 1, ("column", True): 1, ("column", False): 1,
    ("one_slice_tail", True): 1, ("one_slice_tail", False): 2, ("feats_chunk_128", True): 2, ("feats_chunk_128", False): 1,
    ("feats_chunk_129", True): 1, ("feats_chunk_129", False): 1, ("two_slices", True): 1, ("two_slices", False): 1,
    ("three_slices_uneven", True): 1, ("three_slices_uneven", False): 1, ("many_instances", True): 1, ("many_instances", False): 1,
    ("trailing_empty", True): 1, ("trailing_empty", False): 1, ("far_reference", True): 1,
}


def case_names():
    return ["%s-%s-up%d" % (n, "rel" if rel else "norel", f) for n, (_, _, _, fs, rels) in SHAPES.items() for rel in rels for f in fs]


def num_params(rel):
    return ((DYN + 2) if rel else DYN) * DYN + DYN * DYN + DYN + DYN + DYN + 1


def groups(rel):
    """The seven named groups of a parameter row as index lists: 169 values with rel_coord, 153 without (w0_rel is then empty)."""
    cin = DYN + 2 if rel else DYN
    lead = 2 if rel else 0
    w1 = cin * DYN
    w2 = w1 + DYN * DYN
    b0 = w2 + DYN
    return {
        "w0_rel": [o * cin + d for o in range(DYN) for d in range(lead)],
        "w0_feat": [o * cin + lead + c for o in range(DYN) for c in range(DYN)],
        "w1": list(range(w1, w2)),
        "w2": list(range(w2, b0)),
        "b0": list(range(b0, b0 + DYN)),
        "b1": list(range(b0 + DYN, b0 + 2 * DYN)),
        "b2": [b0 + 2 * DYN],
    }


def _inputs(shape, rel, seed):
    H, W, num_insts, _, _ = SHAPES[shape]
    g = torch.Generator().manual_seed(seed)
    n_all = sum(num_insts)
    feats = torch.randn(len(num_insts), 8, H, W, generator=g)
    ref = torch.rand(1, n_all, 2, generator=g) * torch.tensor([W * float(STRIDE), H * float(STRIDE)])
    if shape == "far_reference":
        ref = torch.tensor([[[0.0, 0.0], [W * float(STRIDE), 0.0], [W * float(STRIDE), H * float(STRIDE)]]])
    params = torch.randn(1, n_all, num_params(rel), generator=g) * 0.3
    return feats, ref, params


@functools.lru_cache(maxsize=None)
def case(name):
    """Seeded float32 inputs of a sweep case and an upstream gradient of the output's shape (read-only: shared by the tests)."""
    shape, rel, up = name.rsplit("-", 2)
    rel, factor = rel == "rel", int(up[2:])
    H, W, num_insts, _, _ = SHAPES[shape]
    seed = SEEDS[(shape, rel)]
    feats, ref, params = _inputs(shape, rel, seed)
    g = torch.Generator().manual_seed(seed * 1000 + factor)
    upstream = torch.randn(1, sum(num_insts), H * factor, W * factor, generator=g)
    return SimpleNamespace(name=name, shape=shape, rel=rel, factor=factor, H=H, W=W, num_insts=list(num_insts), seed=seed,
                           feats=feats, ref=ref, params=params, upstream=upstream)


def head(mask_feats, reference_points, mask_head_params, num_insts, stride, rel_coord, factor, dtype=torch.float64):
    """The head in `dtype`: (out [1, n_all, f H, f W], acts).  acts holds the layer input x [n_all, cin, HW], the pre-activations
    a0, a1 [n_all, 8, HW] and s0, s1 = |b| + sum |w_i x_i| of each of them."""
    feats, ref, params = (t.to(dtype) for t in (mask_feats, reference_points, mask_head_params))
    n, c, h, w = feats.shape
    counts = [int(k) for k in num_insts]
    n_all = sum(counts)
    xs = torch.arange(0, w * stride, step=stride, dtype=torch.float32)
    ys = torch.arange(0, h * stride, step=stride, dtype=torch.float32)
    yy, xx = torch.meshgrid(ys, xs, indexing="ij")
    loc = (torch.stack((xx.reshape(-1), yy.reshape(-1)), dim=1) + stride // 2).to(dtype)               # [HW, 2]
    img = torch.repeat_interleave(torch.arange(n), torch.as_tensor(counts))
    x = feats.reshape(n, c, h * w)[img]                                                                # [n_all, c, HW]
    if rel_coord:
        rel = ref.reshape(n_all, 1, 2) - loc.reshape(1, h * w, 2)
        rel = rel.float().to(dtype).permute(0, 2, 1)                                                   # `.float()`: ddetrs_dn.py:783
        x = torch.cat([rel, x], dim=1)
    cin = x.shape[1]
    w0, w1, w2, b0, b1, b2 = torch.split_with_sizes(params.reshape(n_all, -1), [cin * DYN, DYN * DYN, DYN, DYN, DYN, 1], dim=1)
    w0, w1 = w0.reshape(n_all, DYN, cin), w1.reshape(n_all, DYN, DYN)
    a0 = torch.bmm(w0, x) + b0[:, :, None]
    s0 = torch.bmm(w0.abs(), x.abs()) + b0.abs()[:, :, None]
    h0 = torch.relu(a0)
    a1 = torch.bmm(w1, h0) + b1[:, :, None]
    s1 = torch.bmm(w1.abs(), h0.abs()) + b1.abs()[:, :, None]
    y = torch.bmm(w2.reshape(n_all, 1, DYN), torch.relu(a1)) + b2[:, :, None]
    out = upsample_aligned(y.reshape(n_all, 1, h, w), int(factor))
    acts = dict(x=x, a0=a0, s0=s0, a1=a1, s1=s1, w0=w0, w1=w1, w2=w2, b1=b1, b2=b2, img=img)
    return out.reshape(1, n_all, out.shape[-2], out.shape[-1]), acts


def kink_margin(acts):
    """min over every pre-activation of |a| / (|b| + sum |w_i x_i|); the kink condition is kink_margin >= KINK."""
    worst = float("inf")
    for a, s in ((acts["a0"], acts["s0"]), (acts["a1"], acts["s1"])):
        if a.numel():
            worst = min(worst, float((a.detach().abs() / s.detach()).min()))
    return worst


def _magnitudes(c, acts):
    """Sum of the ABSOLUTE summands behind every value of `reference(c)`, from the float64 restatement: the same backward with
    every factor replaced by its magnitude (and an activation by the s = |b| + sum |w_i x_i| its rounding error scales with), so
    that n u magnitude bounds the rounding error of a float32 evaluation with sums of depth n, in any order."""
    n_all, hw = acts["a0"].shape[0], acts["a0"].shape[2]
    h, w = c.H, c.W
    z = torch.zeros(n_all, 1, h, w, dtype=torch.float64, requires_grad=True)
    (ag,) = torch.autograd.grad((upsample_aligned(z, c.factor) * c.upstream.double().abs().reshape(n_all, 1, c.factor * h, c.factor * w)).sum(), (z,))
    ag = ag.reshape(n_all, 1, hw)                                           # the interpolation weights are not negative
    m0, m1 = (acts["a0"] > 0).double(), (acts["a1"] > 0).double()
    w0, w1, w2 = acts["w0"].detach().abs(), acts["w1"].detach().abs(), acts["w2"].detach().abs()
    x = acts["x"].detach().abs()
    s0h = acts["s0"].detach() * m0
    s1h = (torch.bmm(w1, s0h) + acts["b1"].detach().abs()[:, :, None]) * m1
    s2 = torch.bmm(w2.reshape(n_all, 1, DYN), s1h) + acts["b2"].detach().abs()[:, :, None]
    gh1 = ag * w2[:, :, None] * m1
    gh0 = torch.bmm(w1.transpose(1, 2), gh1) * m0
    g_b0 = gh0.sum(-1)
    params = torch.cat([torch.bmm(gh0, x.transpose(1, 2)).flatten(1), torch.bmm(gh1, s0h.transpose(1, 2)).flatten(1),
                        (ag * s1h).sum(-1), g_b0, gh1.sum(-1), ag.sum(-1)], dim=1)
    lead = 2 if c.rel else 0
    xy = torch.einsum("nod,no->nd", w0[:, :, :lead], g_b0) if c.rel else torch.zeros(n_all, 2, dtype=torch.float64)
    per_inst = torch.bmm(w0[:, :, lead:].transpose(1, 2), gh0)               # [n_all, 8, HW]
    feats = torch.zeros(len(c.num_insts), 8, hw, dtype=torch.float64).index_add_(0, acts["img"], per_inst)
    out = upsample_aligned(s2.reshape(n_all, 1, h, w), c.factor)
    return dict(out=out.reshape(1, n_all, out.shape[-2], out.shape[-1]), grad_feats=feats.reshape(-1, 8, h, w),
                grad_xy=xy.reshape(1, n_all, 2), grad_params=params.reshape(1, n_all, -1))


def _run(fn, c, dtype):
    """out and the three gradients of sum(out * upstream) of `fn(feats, ref, params)` as a dict of detached tensors."""
    f, r, p = (t.to(dtype).requires_grad_(True) for t in (c.feats, c.ref, c.params))
    res = fn(f, r, p)
    out = res[0] if isinstance(res, tuple) else res
    gf, gr, gp = torch.autograd.grad((out * c.upstream.to(dtype)).sum(), (f, r, p), allow_unused=True)
    got = dict(out=out.detach(), grad_feats=gf, grad_xy=gr if gr is not None else torch.zeros_like(r), grad_params=gp)
    return got, (res[1] if isinstance(res, tuple) else None)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(want, magnitudes, kink margin) of a sweep case from the float64 restatement; computed once, shared, left unchanged."""
    c = case(name)
    want, acts = _run(lambda f, r, p: head(f, r, p, c.num_insts, STRIDE, c.rel, c.factor), c, torch.float64)
    return want, _magnitudes(c, acts), kink_margin(acts)


def composition(c, device="cpu"):
    """The project's float32 PyTorch composition (the fallback route) of a sweep case under autograd."""
    from uninext_amd import mask_head

    def fn(f, r, p):
        logits = mask_head._dynamic_convs_torch(f, r.reshape(-1, 2), p.flatten(0, 1), c.num_insts, STRIDE, c.rel)
        return mask_head._aligned_bilinear_torch(logits.reshape(-1, 1, c.H, c.W), c.factor).reshape(1, -1, c.factor * c.H, c.factor * c.W)
    c = SimpleNamespace(**{k: (v.to(device) if torch.is_tensor(v) else v) for k, v in vars(c).items()})
    return _run(fn, c, torch.float32)[0]


@functools.lru_cache(maxsize=None)
def composition_errors(name):
    """group_errors of the float32 composition on the CPU against float64: the yardstick of every entry's bound."""
    c = case(name)
    return group_errors(composition(c), reference(name)[0], c.num_insts, c.rel)


def entries(num_insts, rel):
    """(entry name, tensor key, index) of every compared entry: one per instance for the forward output, one per parameter group
    per instance, one per instance for grad_xy, one per image for grad_feats."""
    n_all = sum(num_insts)
    for i in range(n_all):
        yield "out[%d]" % i, "out", (0, i)
    for i in range(n_all):
        for g, idx in groups(rel).items():
            if idx:
                yield "params.%s[%d]" % (g, i), "grad_params", (0, i, idx)
    for i in range(n_all):
        yield "xy[%d]" % i, "grad_xy", (0, i)
    for b in range(len(num_insts)):
        yield "feats[%d]" % b, "grad_feats", (b,)


def group_of(entry):
    return entry.split("[")[0]


def group_errors(got, want, num_insts, rel):
    """entry -> max |got - want| / max |want| over the entry's own values, no floor.  An entry whose reference is identically
    zero (an image without instances, grad_xy without rel_coord) must be identically zero in `got`: 0.0, else inf."""
    errs = {}
    got = {k: v.detach().cpu().double() for k, v in got.items()}
    for name, key, idx in entries(num_insts, rel):
        g, w = got[key][idx], want[key][idx]
        assert g.shape == w.shape, (name, g.shape, w.shape)
        scale = float(w.abs().max())
        if scale == 0.0:
            errs[name] = 0.0 if float(g.abs().max()) == 0.0 else float("inf")
        else:
            errs[name] = float((g - w).abs().max()) / scale if bool(torch.isfinite(g).all()) else float("inf")
    return errs


def summand_ratios(name):
    """entry -> s: the largest sum of absolute summands over the entry's values divided by the entry's largest reference value
    (>= 1; 0.0 for a structurally zero entry)."""
    c = case(name)
    want, mags, _ = reference(name)
    s = {}
    for entry, key, idx in entries(c.num_insts, c.rel):
        scale = float(want[key][idx].abs().max())
        s[entry] = float(mags[key][idx].max()) / scale if scale > 0.0 else 0.0
    return s


def bounds(name, comp_errs=None):
    """entry -> max(COMP_MARGIN x the composition's error of the same entry, SUM_DEPTH u s): computed, never written down."""
    comp = composition_errors(name) if comp_errs is None else comp_errs
    return {e: max(COMP_MARGIN * comp[e], SUM_DEPTH * U * s) for e, s in summand_ratios(name).items()}


def worst_by_group(name, errs, bound):
    """Per group of a case: the entry with the largest error / bound -> (group, entry, error, composition error, bound)."""
    comp = composition_errors(name)
    rows = {}
    for e, err in errs.items():
        ratio = err / bound[e] if bound[e] > 0.0 else (0.0 if err == 0.0 else float("inf"))
        if group_of(e) not in rows or ratio > rows[group_of(e)][0]:
            rows[group_of(e)] = (ratio, e, err, comp[e], bound[e])
    return [(g,) + r[1:] + (r[0],) for g, r in rows.items()]


def table_path():
    """Where the tests write their tables: the file DYNMASK_PARITY_TABLE names (profiles/r16_dynmask_parity.txt was made so);
    unset, the tables are only printed."""
    return os.environ.get("DYNMASK_PARITY_TABLE") or None


def structurally_zero(entry, num_insts, rel):
    """Entries whose gradient is zero whatever the inputs: grad_xy without rel_coord, grad_feats of an image without instances."""
    if entry.startswith("xy["):
        return not rel
    return entry.startswith("feats[") and num_insts[int(entry[6:-1])] == 0


def unexercised(name):
    """Entries whose reference scale max |want| is zero although they are not structurally zero (none, for a recorded seed)."""
    c = case(name)
    want = reference(name)[0]
    return [e for e, key, idx in entries(c.num_insts, c.rel)
            if float(want[key][idx].abs().max()) == 0.0 and not structurally_zero(e, c.num_insts, c.rel)]


def find_seed(shape, rel, first=1, tries=20000):
    """The first seed whose inputs satisfy the kink condition and leave no group of any instance without a gradient."""
    _, _, num_insts, fs, _ = SHAPES[shape]
    for seed in range(first, first + tries):
        feats, ref, params = _inputs(shape, rel, seed)
        with torch.no_grad():
            _, acts = head(feats, ref, params, num_insts, STRIDE, rel, 1)
        if kink_margin(acts) < KINK:
            continue
        SEEDS[(shape, rel)] = seed
        case.cache_clear()
        reference.cache_clear()
        if not any(unexercised("%s-%s-up%d" % (shape, "rel" if rel else "norel", f)) for f in fs):
            return seed
    raise RuntimeError("no seed for %s rel=%s" % (shape, rel))


if __name__ == "__main__":
    for shape, (_, _, _, _, rels) in SHAPES.items():
        for rel in rels:
            print("    (%r, %r): %d," % (shape, rel, find_seed(shape, rel)))
