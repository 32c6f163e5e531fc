"""A float64 restatement of two-stage query selection, written from the formulas of include/dynmask_hip.h (the qsel_* block)
alone: numpy, nothing of the package.  tests/test_query_selection_cpu.py pins it to the committed fixtures and to the module's
fp32 validity; tests/test_query_selection_parity_gpu.py holds the two HIP kernels to it.

Every token s of image b proposes a box from its level l and its (y, x) in the level: cx = (x + 0.5) / valid_W and
cy = (y + 0.5) / valid_H as IEEE fp32 divisions, w = h = 0.05f * 2^l.  It is live iff it is not padded and all four numbers lie
strictly inside (fp32(0.01), fp32(0.99)).  The proposals are fp32 by definition; everything after them is float64.

Besides its value every output carries `mag`, the size its fp32 rounding error scales with: the sum of the ABSOLUTE summands of
the value's own sum (a Linear's |b| + sum |w| |x|: n * 2^-24 * that bounds the rounding of a sum of depth n in any order), plus
what its inputs hand on to first order.  The roundings of the 256 inputs of a Linear are independent, so their `mag`s pass through
it in quadrature, sqrt(sum w^2 mag(x)^2): passing them on as sum |w| mag(x) would grow s by sqrt(256) a layer and leave the
box head, three layers on, with a bound a thousand times its values' rounding.  A LayerNorm passes its centring and its variance
on through their derivatives; ReLU passes a magnitude on unchanged (|relu(a) - relu(a')| <= |a - a'|, so no kink condition is
needed).  `mag / |value|` is the ratio s of the error measure.
"""
import numpy as np

from parity_measure import COMP_MARGIN, SUM_DEPTH, U, entry_bound    # noqa: F401  (the bound every sweep shares; exported as before)

LO, HI = np.float32(0.01), np.float32(0.99)


def level_starts(levels):
    return np.concatenate(([0], np.cumsum([h * w for h, w in levels]))).astype(np.int64)


def proposals(mask, levels):
    """mask [B, S] (nonzero = padded), levels [(H, W), ...] -> (cx, cy, wh) fp32 [B, S], live bool [B, S], valid_wh fp32
    [B, n_levels, 2] = (valid_W, valid_H) counted along the first row and the first column of each level."""
    mask = np.asarray(mask).astype(bool)
    B, S = mask.shape
    starts = level_starts(levels)
    assert starts[-1] == S
    cx, cy, wh = (np.zeros((B, S), np.float32) for _ in range(3))
    valid_wh = np.zeros((B, len(levels), 2), np.float32)
    half = np.float32(0.5)
    with np.errstate(divide="ignore", invalid="ignore"):
        for l, (H, W) in enumerate(levels):
            m = mask[:, starts[l]:starts[l + 1]].reshape(B, H, W)
            vw = (~m[:, 0, :]).sum(1).astype(np.float32)
            vh = (~m[:, :, 0]).sum(1).astype(np.float32)
            valid_wh[:, l, 0], valid_wh[:, l, 1] = vw, vh
            xs = (np.arange(W, dtype=np.float32) + half)[None, None, :] / vw[:, None, None]
            ys = (np.arange(H, dtype=np.float32) + half)[None, :, None] / vh[:, None, None]
            assert xs.dtype == np.float32 and ys.dtype == np.float32
            cx[:, starts[l]:starts[l + 1]] = np.broadcast_to(xs, (B, H, W)).reshape(B, -1)
            cy[:, starts[l]:starts[l + 1]] = np.broadcast_to(ys, (B, H, W)).reshape(B, -1)
            wh[:, starts[l]:starts[l + 1]] = np.float32(0.05) * np.float32(2.0 ** l)
        inside = lambda v: (v > LO) & (v < HI)
        live = inside(cx) & inside(cy) & inside(wh) & ~mask
    return cx, cy, wh, live, valid_wh


def _f64(*arrays):
    return [np.asarray(a, dtype=np.float64) for a in arrays]


def linear(x, mag_x, w, b):
    """(x w^T + b, its mag: |b| + |x| |w|^T of its own sum, the inputs' mag_x in quadrature)."""
    return x @ w.T + b, np.abs(b) + np.abs(x) @ np.abs(w).T + np.sqrt((mag_x * mag_x) @ (w * w).T)


def out_mem(memory, live, enc_w, enc_b, ln_w, ln_b, eps):
    """LayerNorm(row @ enc_w^T + enc_b) * ln_w + ln_b in float64, a dead row counting as zeros; biased variance, eps inside the
    root.  memory [..., d], live [...].  Returns (value, mag)."""
    memory, enc_w, enc_b, ln_w, ln_b = _f64(memory, enc_w, enc_b, ln_w, ln_b)
    x = memory * np.asarray(live, dtype=np.float64)[..., None]
    y, mag_y = linear(x, np.zeros_like(x), enc_w, enc_b)               # the memory itself is exact
    mean = y.mean(-1, keepdims=True)
    c = y - mean
    var = (c * c).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    mag_c = mag_y + mag_y.mean(-1, keepdims=True)
    mag_var = (2.0 * np.abs(c) * mag_c).mean(-1, keepdims=True) + eps        # d var = mean(2 c dc)
    mag_n = mag_c * rstd + np.abs(c) * rstd * 0.5 * mag_var / (var + eps)    # d rstd / rstd = -d var / (2 (var + eps))
    return c * rstd * ln_w + ln_b, mag_n * np.abs(ln_w) + np.abs(ln_b)


def logits(mem, mag_mem, class_vec, class_bias, scale=None, clamp=0.0):
    """dot(mem[b, s], class_vec[b]) / scale + class_bias[b], clamped to +-clamp when clamp > 0.  mem [B, S, d], class_vec [B, d]
    or [1, d], class_bias [B] or [1].  Returns (value [B, S], mag, the value before the clamp)."""
    class_vec, class_bias = _f64(class_vec, class_bias)
    sc = 1.0 if scale is None else float(scale)
    free = (mem * class_vec[:, None, :]).sum(-1) / sc + class_bias[:, None]
    mag = ((np.abs(mem) * np.abs(class_vec)[:, None, :]).sum(-1) + np.sqrt((mag_mem ** 2 * (class_vec ** 2)[:, None, :]).sum(-1))) / abs(sc) \
        + np.abs(class_bias)[:, None]
    return (np.clip(free, -clamp, clamp) if clamp > 0 else free), mag, free


def proposal_logit(p):
    """(log(p / (1 - p)), |log p| + |log(1 - p)|) of fp32 proposals taken to float64."""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(p / (1.0 - p)), np.abs(np.log(p)) + np.abs(np.log1p(-p))


def proposal_logit_fp32(p):
    """The logit as the fixtures' generator took it: torch's fp32 division and fp32 log, taken to float64 afterwards (numpy's
    fp32 log differs from it in the last bit on some entries)."""
    import torch
    p = torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32))
    return torch.log(p / (1 - p)).double().numpy()


def boxes(mem, mag_mem, cx, cy, wh, live, w1, b1, w2, b2, w3, b3, fp32_logit=False):
    """coords_unact = w3 relu(w2 relu(w1 mem + b1) + b2) + b3 + the proposal's logit, +inf on dead rows, and its sigmoid, exactly
    1 there.  mem [..., d] and cx, cy, wh, live [...] are those of the same rows.  fp32_logit: the proposal's logit rounded to
    fp32 as the fixtures hold it, not the float64 one.  Returns (coords [..., 4], points, mag)."""
    w1, b1, w2, b2, w3, b3 = _f64(w1, b1, w2, b2, w3, b3)
    h, mag = linear(mem, mag_mem, w1, b1)
    h, mag = linear(np.maximum(h, 0.0), mag, w2, b2)
    h, mag = linear(np.maximum(h, 0.0), mag, w3, b3)
    live = np.asarray(live, dtype=bool)
    prop, mag_prop = proposal_logit(np.stack((cx, cy, wh, wh), -1))
    if fp32_logit:
        prop = proposal_logit_fp32(np.stack((cx, cy, wh, wh), -1))
    dead = np.broadcast_to(~live[..., None], h.shape)
    coords = np.where(dead, np.inf, h + np.where(dead, 0.0, prop))
    mag = np.where(dead, 0.0, mag + np.where(dead, 0.0, mag_prop))
    with np.errstate(over="ignore"):
        points = np.where(dead, 1.0, 1.0 / (1.0 + np.exp(-np.where(dead, 0.0, coords))))
    return coords, points, mag


def gather_rows(a, idx, fill):
    """a [B, S, ...] at idx [B, K]; an index outside [0, S) gives `fill`."""
    a, idx = np.asarray(a), np.asarray(idx)
    S = a.shape[1]
    ok = (idx >= 0) & (idx < S)
    out = np.take_along_axis(a, np.where(ok, idx, 0).reshape(idx.shape + (1,) * (a.ndim - 2)), 1)
    return np.where(ok.reshape(ok.shape + (1,) * (a.ndim - 2)), out, fill)


def vl_align_terms(state, pool):
    """(class_vec [B, d], class_bias [B], scale, clamp) of the alignment head for one pooled text token per image:
    e = pool / max(|pool|, 1e-12); vec = W (e / 2) + b; bias = e . bias_lang + bias0; scale = exp(log_scale); clamp 50000."""
    pool = np.asarray(pool, dtype=np.float64)
    w, b, lang, bias0, log_scale = _f64(state["dot_product_projection_text.weight"], state["dot_product_projection_text.bias"],
                                        state["bias_lang"], state["bias0"], state["log_scale"])
    e = pool / np.maximum(np.sqrt((pool * pool).sum(-1, keepdims=True)), 1e-12)
    return (e / 2.0) @ w.T + b, e @ lang + bias0[0], float(np.exp(log_scale[0])), 50000.0


def still_terms(state):
    w, b = _f64(state["body.weight"], state["body.bias"])
    return w.reshape(1, -1), b.reshape(1), None, 0.0


def select(memory, mask, levels, enc, norm, eps, class_terms, mlp, topk, fp32_logit=False):
    """The whole selection in float64: a dict of logits [B, S], output_memory, output_proposals (+inf on dead rows),
    coords_unact of every row, its sigmoid, and the top-k rows by logit (descending).  fp32_logit: see boxes()."""
    cx, cy, wh, live, valid_wh = proposals(mask, levels)
    mem, mag_mem = out_mem(memory, live, enc[0], enc[1], norm[0], norm[1], eps)
    vec, bias, scale, clamp = class_terms
    lg, mag_lg, _ = logits(mem, mag_mem, vec, bias, scale, clamp)
    coords, points, mag_coords = boxes(mem, mag_mem, cx, cy, wh, live, *mlp, fp32_logit=fp32_logit)
    p4 = np.stack((cx, cy, wh, wh), -1)
    prop = np.where(live[..., None], proposal_logit_fp32(p4) if fp32_logit else proposal_logit(p4)[0], np.inf)
    order = np.argsort(-lg, axis=1, kind="stable")[:, :topk]
    return dict(logits=lg, mag_logits=mag_lg, output_memory=mem, mag_memory=mag_mem, output_proposals=prop, coords=coords,
                points=points, mag_coords=mag_coords, topk=order, live=live, valid_wh=valid_wh)


def validity_grid(n=128):
    """(mask [n, 2 n] bool, levels): image b is padded to valid_W = b + 1 on level 0 (1 x n) and to valid_H = b + 1 on level 1
    (n x 1), so the unpadded tokens are every pair (x, valid) with x < valid <= n, once as a column and once as a row."""
    mask = np.zeros((n, 2 * n), dtype=bool)
    pad = np.arange(n)[None, :] > np.arange(n)[:, None]
    mask[:, :n], mask[:, n:] = pad, pad
    return mask, [(1, n), (n, 1)]


def grid_quotients(n=128):
    """fp32 (x + 0.5) / valid for every x < valid <= n: [valid - 1, x], NaN where x >= valid."""
    x, valid = np.arange(n, dtype=np.float32)[None, :], np.arange(1, n + 1, dtype=np.float32)[:, None]
    return np.where(x < valid, (x + np.float32(0.5)) / valid, np.float32("nan"))
