"""The training route of the bi-directional attention core (include/biattn_hip.h: biattn_hip_train_f32 and
biattn_hip_backward_f32) for tests/test_vlfuse_train_cpu.py and tests/test_vlfuse_train_gpu.py: seeded dyadic inputs, the float64
restatement of the header's formulas, the fp32 composition as the comparison term, and per-entry magnitudes for
parity_measure.errors.  Plain numpy, next to attn_parity.py.

The restatement reproduces the fp32 facts the header names: qs = fp32(q * q_scale), and a masked score is SET to -9e15 (what
the fp32 add leaves), so an all-masked row is uniform over T.  ds_l is the header's formula: autograd's argmax routing through
torch.max is not imitated (it is analytically zero).

Magnitudes (the `s` of parity_measure.entry_bound: the absolute summands behind an entry).  A score's own summands are
amp = |qs| . |k| (+ |m|), 0 where the clamp or the mask fixes it; exp turns an absolute score error into a relative one of the
probability, once for the entry and once for the row's sum, hence the factor (1 + 2 A) with A the row's largest amp, as in
attn_parity.softmax_pv.  With it
    mds_v = (1 + 2 A_v[i]) p_v (|g_v| . |vl| + |g_v| . (p_v |vl|))       mds_l likewise with A_l[j], p_l, g_l, vv
    mag dq = q_scale (gate (mds_v + mds_l)) |k|      mag dk = (gate (mds_v + mds_l))^T |qs|
    mag dvl = ((1 + 2 A_v) p_v)^T |g_v|              mag dvv = ((1 + 2 A_l) p_l^T)^T |g_l|
    mag max = A + |max|                              mag log sum = 1 + 2 A + |log sum|     (the kept row statistics)
"""
import numpy as np

import parity_measure as PM

D = 256
CLAMP = 50000.0
MASKED = -9e15
SS = (1, 31, 32, 33, 127, 128, 129, 257)
TS = (1, 31, 32, 33, 65, 129, 256)
BHS = ((1, 1), (2, 3))
MASKS = ("none", "i64", "allmasked", "f32")
S_UNEVEN = 64 * 32 * 2 + 1                  # more tiles than ranges and an uneven split, at B x heads = 1 x 1
SPECIALS = ("beyond", "equal", "inner")


def mask_of(kind, B, T):
    """[B, T] int64 / float32 (0 = masked, else the value that is added) or None.  allmasked: the last batch has no token."""
    if kind == "none":
        return None
    keep = np.arange(T)[None, :] < np.array([max(1, (2 * T + 2) // 3), max(1, T // 2)])[:B, None]
    if kind == "allmasked":
        keep = keep.copy()
        keep[B - 1] = False
    if kind in ("i64", "allmasked"):
        return keep.astype(np.int64)
    vals = np.array([1.0, 0.5, 2.0, 1.0, -0.25], dtype=np.float32)[np.arange(T) % 5]
    return (keep * vals[None, :]).astype(np.float32)


def make(B, H, S, T, mask="none", special=None):
    """The inputs of a case: float32 dyadic q, vv, g_v [B, S, E], k, vl, g_l [B, T, E], the mask and the scale.
    special: "beyond"  scores beyond +-50000 (entry [0, 0] above, [S - 1, T - 1] below: dr there is exactly 0)
             "equal"   r[0, 0] = 50000 exactly, from a sum that is exact in any order (the gradient passes)
             "inner"   a text column whose scores span more than 50000 (s - M < -50000 at image token 0)"""
    name = "vlfuse_train/%dx%d/S%d_T%d/%s/%s" % (B, H, S, T, mask, special)
    g = PM.rng(name)
    E = H * D
    x = dict(B=B, H=H, S=S, T=T, scale=float(np.float32(D ** -0.5)), mask=mask_of(mask, B, T), name=name)
    for key, n in (("q", S), ("vv", S), ("gv", S), ("k", T), ("vl", T), ("gl", T)):
        x[key] = PM.dy(g.randn(B, n, E), 0.5, 64.0)
    x["q"] = PM.dy(g.randn(B, S, E), 2.0, 64.0)          # scores of a few units: a softmax that is neither flat nor one-hot
    if special == "beyond":
        x["q"][0, :, :2] = 0.0                                                    # the other tokens of either side meet the two large
        x["k"][0, :, :2] = 0.0                                                    # channels with 0: no score of some hundreds, whose
                                                                                  # probability fp32 cannot hold (exp underflows)
        x["q"][0, 0, :D] = 0.0
        x["k"][0, :2, :D] = 0.0                                                   # two clamped entries in one row: p_v = 1/2 each,
        x["q"][0, 0, 0], x["k"][0, :2, 0] = 16.0 * 4096.0, 16.0 * 64.0            # so a gate that is dropped shows; r = 262144
        x["q"][0, S - 1, :D] = 0.0
        x["k"][0, T - 1, :D] = 0.0
        x["q"][0, S - 1, 1], x["k"][0, T - 1, 1] = -16.0 * 4096.0, 16.0 * 64.0
    elif special == "equal":
        x["q"][0, :, 0] = 0.0                                                     # the other tokens of either side meet the large channel
        x["k"][0, :, 0] = 0.0                                                     # with 0 (no probability below what fp32 holds)
        x["q"][0, 0, :D] = 0.0
        x["k"][0, :2, :D] = 0.0                                                   # two such entries in the row: p_v = 1/2 each
        x["q"][0, 0, 0], x["k"][0, :2, 0] = 16.0 * 3125.0, 16.0                  # (50000 / 16) * 16: one exact product
    elif special == "inner":
        x["q"][0, :, :D] = 0.0
        x["q"][0, 0, 0] = -16.0 * 3050.0                                          # s[0, j] = -3050 k[0, j, 0] in [-48848, -48800]
        x["q"][0, 1, 0] = 16.0 * 100.0                                            # M[j] = 100 k[0, j, 0] >= 1600: s - M < -50000
        x["k"][0, :, 0] = 16.0 + (np.arange(T) % 2) / 64.0                        # row 0 spreads by 48: no probability fp32 cannot hold
    for key in ("q", "vv", "gv", "k", "vl", "gl"):
        assert x[key].dtype == np.float32
    return x


def _split(t, H):
    B, N, E = t.shape
    return t.reshape(B, N, H, E // H).transpose(0, 2, 1, 3)


def _merge(t):
    B, H, N, Dh = t.shape
    return np.ascontiguousarray(t.transpose(0, 2, 1, 3)).reshape(B, N, H * Dh)


def _softmax(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def core(x, dt=np.float64, variant=None):
    """The header's formulas in `dt` (float64: the restatement; float32: the composition).  Returns a dict of out_v, out_l, dq,
    dk, dvv, dvl (token-major), the statistics, and -- in float64 -- the magnitudes under "mag_*".
    variant: one of the wrong variants the CPU test must see leave the bound."""
    H = x["H"]
    scale = np.float32(x["scale"])
    qs = _split((x["q"] * scale).astype(np.float32).astype(dt), H)                # fp32(q * q_scale)
    k, vv, vl = (_split(x[n].astype(dt), H) for n in ("k", "vv", "vl"))
    gv, gl = _split(x["gv"].astype(dt), H), _split(x["gl"].astype(dt), H)
    r = qs @ k.transpose(0, 1, 3, 2)                                             # [B, H, S, T]
    s = np.clip(r, -CLAMP, CLAMP)
    gate = (r >= -CLAMP) & (r <= CLAMP)
    if variant == "gate_dropped":
        gate = np.ones_like(gate)
    elif variant == "gate_exclusive":
        gate = (r > -CLAMP) & (r < CLAMP)
    amp = np.where(np.abs(r) >= CLAMP, 0.0, np.abs(qs) @ np.abs(k).transpose(0, 1, 3, 2))
    a, amp_a = s, amp
    if x["mask"] is not None:
        m = x["mask"].astype(dt)[:, None, None, :]
        a = np.where(m == 0, dt(MASKED), (s + m).astype(dt))                      # SET, as the fp32 add has it
        amp_a = np.where(m == 0, 0.0, amp + np.abs(m))
    p_v = _softmax(a)
    st = s.transpose(0, 1, 3, 2)                                                  # [B, H, T, S]
    M = st.max(-1, keepdims=True)
    e = np.maximum(st - M, -CLAMP)
    if variant == "mask_on_text" and x["mask"] is not None:
        e = np.where(x["mask"][:, None, :, None] == 0, dt(MASKED), e)              # a masked text token's row becomes uniform
    p_l = _softmax(e)                                                             # [B, H, T, S]
    out_v, out_l = p_v @ vl, p_l @ vv
    delta_v = (gv * out_v).sum(-1, keepdims=True)                                 # [B, H, S, 1]
    delta_l = (gl * out_l).sum(-1, keepdims=True)                                 # [B, H, T, 1]
    if variant == "delta_swapped":
        delta_v, delta_l = np.broadcast_to(delta_l.mean(2, keepdims=True), delta_v.shape), np.broadcast_to(
            delta_v.mean(2, keepdims=True), delta_l.shape)
    dp_v = gv @ vl.transpose(0, 1, 3, 2)                                          # [B, H, S, T]
    dp_l = gl @ vv.transpose(0, 1, 3, 2)                                          # [B, H, T, S]
    ds_v = p_v * (dp_v - delta_v)
    ds_l = (p_l * (dp_l - delta_l)).transpose(0, 1, 3, 2)                         # [B, H, S, T]
    dr = np.where(gate, ds_v + ds_l, 0.0)
    dr_k = np.where(gate, ds_v, 0.0) if variant == "dk_without_ds_l" else dr
    out = dict(out_v=_merge(out_v), out_l=_merge(out_l),
               dq=_merge((dr @ k) * (dt(1.0) if variant == "dq_unscaled" else dt(scale))),
               dk=_merge(dr_k.transpose(0, 1, 3, 2) @ qs),
               dvl=_merge(p_v.transpose(0, 1, 3, 2) @ gv), dvv=_merge(p_l.transpose(0, 1, 3, 2) @ gl),
               max_v=a.max(-1), logsum_v=np.log(np.exp(a - a.max(-1, keepdims=True)).sum(-1)),
               M=M[..., 0], logL=np.log(np.maximum(np.exp(e).sum(-1), np.finfo(dt).tiny)), dr=dr, r=r, e=e)
    if dt is np.float64 and variant is None:
        A_v = (1.0 + 2.0 * amp_a.max(-1, keepdims=True))                          # [B, H, S, 1]
        A_l = (1.0 + 2.0 * amp.max(-2, keepdims=True))                            # [B, H, 1, T]
        av, al = np.abs(vl), np.abs(vv)
        mds_v = A_v * p_v * (np.abs(gv) @ av.transpose(0, 1, 3, 2) + (np.abs(gv) * (p_v @ av)).sum(-1, keepdims=True))
        mds_l = A_l * p_l.transpose(0, 1, 3, 2) * (
            (np.abs(gl) @ al.transpose(0, 1, 3, 2)) + (np.abs(gl) * (p_l @ al)).sum(-1, keepdims=True)).transpose(0, 1, 3, 2)
        mdr = np.where(gate, mds_v + mds_l, 0.0)
        # the kept statistics: a maximum carries its score's summands; the log of a sum moves by the largest score error of the row
        # (d log sum = sum p d a) and by the relative error of the sum and of log's own rounding
        Av, Al = amp_a.max(-1), amp.max(-2)
        out.update(mag_max_v=Av + np.abs(out["max_v"]), mag_M=Al + np.abs(out["M"]),
                   mag_logsum_v=1.0 + 2.0 * Av + np.abs(out["logsum_v"]), mag_logL=1.0 + 2.0 * Al + np.abs(out["logL"]))
        out.update(mag_out_v=_merge(A_v * (p_v @ av)), mag_out_l=_merge(A_l.transpose(0, 1, 3, 2) * (p_l @ al)),
                   mag_dq=_merge(mdr @ np.abs(k)) * float(scale), mag_dk=_merge(mdr.transpose(0, 1, 3, 2) @ np.abs(qs)),
                   mag_dvl=_merge((A_v * p_v).transpose(0, 1, 3, 2) @ np.abs(gv)),
                   mag_dvv=_merge((A_l * p_l.transpose(0, 1, 3, 2)) @ np.abs(gl)))
    return out


GRADS = ("dq", "dk", "dvv", "dvl")


def check(got, x, who, outputs=GRADS + ("out_v", "out_l"), worst=None):
    """Every entry of got[name] within parity_measure.entry_bound of the float64 restatement, with the fp32 composition as the
    comparison term; records the worst ratio per output in `worst`."""
    want, comp = core(x, np.float64), core(x, np.float32)
    for name in outputs:
        err = PM.errors(np.asarray(got[name], dtype=np.float64), want[name], want["mag_" + name], comp[name].astype(np.float64))
        if worst is not None and err.worst >= worst.get(name, (-1.0,))[0]:
            worst[name] = (err.worst, "%-48s %-6s %10.3e %10.3e %10.3e %8.3f" % ((who, name) + tuple(err.row())))
        err.check(who, name)
