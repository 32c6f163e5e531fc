"""The attention dropout inside the bi-directional attention core (include/biattn_hip.h: biattn_hip_train_dropout_f32,
biattn_hip_backward_dropout_f32, biattn_hip_dropout_keep_u8) for tests/test_vlfuse_dropout_cpu.py and
tests/test_vlfuse_dropout_gpu.py: a numpy Philox4x32-10, the keep masks with exactly the header's counter layout, the float64
restatement of the header's formulas with the masks applied, its fp32 composition, and per-entry magnitudes for
parity_measure.errors.  Plain numpy.  The inputs are tests/vlfuse_train_cases.py's (make, mask_of).

The restatement is vlfuse_train_cases.core with c m carried through, in the same order of operations, so that at p = 0 (c = 1,
m = 1) it is that function bit for bit.  Magnitudes: those of vlfuse_train_cases.core with the factor c m multiplying
|g| . |v| inside mds_v / mds_l and multiplying p in mag_out_*, mag_dvl and mag_dvv; the delta term is |g| . (c m p |v|).
"""
import zlib

import numpy as np

import vlfuse_train_cases as VC

M0, M1 = 0xD2511F53, 0xCD9E8D57            # the round's multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85            # the key's increments
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays of one shape (or ints), key: two ints -> four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK32) for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)                      # 32 x 32 -> 64 bits, exact in uint64
        h0, l0 = p0 >> np.uint64(32), p0 & np.uint64(MASK32)
        h1, l1 = p1 >> np.uint64(32), p1 & np.uint64(MASK32)
        c = [h1 ^ c[1] ^ np.uint64(k0), l1, h0 ^ c[3] ^ np.uint64(k1), l0]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [x.astype(np.uint32) for x in c]


def threshold_of(p):
    """(uint32) llrint(p 2^32): keep <=> word >= threshold"""
    return int(np.rint(np.float64(np.float32(p)) * 4294967296.0))


def scale_of(p):
    """c = 1.0f / (1.0f - p) in fp32"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def seed_of(name):
    """A fixed (seed, offset) per name as two int64: all four 32-bit halves in use."""
    a, b = zlib.crc32(name.encode()), zlib.crc32((name + "/offset").encode())
    return np.array([(a << 32) | (b ^ 0x5bd1e995), (b << 32) | (a ^ 0x2545f491)], dtype=np.uint64).view(np.int64)


def keep_masks(seed, p, BH, S, T):
    """keep_v [BH, S, T] and keep_l [BH, T, S] as bool, by the header's layout: key = the seed's two halves, counter = (offset
    low, offset high, i, side << 31 | bh << 8 | j / 4), word j % 4, keep <=> word >= threshold."""
    sd, off = (int(x) for x in np.asarray(seed).view(np.uint64))
    thr = threshold_of(p)
    G = (T + 3) // 4
    bh, i, g = np.meshgrid(np.arange(BH, dtype=np.uint64), np.arange(S, dtype=np.uint64), np.arange(G, dtype=np.uint64), indexing="ij")
    out = []
    for side in (0, 1):
        c3 = np.uint64(side << 31) | (bh << np.uint64(8)) | g
        w = philox4x32_10((off & MASK32, off >> 32, i, c3), (sd & MASK32, sd >> 32))
        words = np.stack(w, axis=-1).reshape(BH, S, 4 * G)[:, :, :T]              # [BH, S, T]: entry (i, j)
        out.append(words.astype(np.uint64) >= thr)
    return out[0], np.ascontiguousarray(out[1].transpose(0, 2, 1))


def case_masks(x, p, seed):
    return keep_masks(seed, p, x["B"] * x["H"], x["S"], x["T"])


VARIANTS = ("delta_undropped", "dvl_without_c", "one_mask", "mask_l_transposed")


def core(x, keep_v, keep_l, p, dt=np.float64, variant=None):
    """The header's formulas with dropout in `dt` (float64: the restatement; float32: the composition).  keep_v [B * H, S, T],
    keep_l [B * H, T, S] bool.  Returns out_v, out_l, dq, dk, dvv, dvl (token-major) and -- in float64 -- "mag_*"."""
    B, H, S, T = x["B"], x["H"], x["S"], x["T"]
    if variant == "one_mask":
        keep_l = keep_v.transpose(0, 2, 1)
    elif variant == "mask_l_transposed":
        keep_l = np.ascontiguousarray(keep_l).reshape(B * H, S, T).transpose(0, 2, 1)   # its memory read as [B * H, S, T]
    c = dt(scale_of(p))
    cm_v = c * keep_v.reshape(B, H, S, T).astype(dt)
    cm_l = c * keep_l.reshape(B, H, T, S).astype(dt)
    scale = np.float32(x["scale"])
    qs = VC._split((x["q"] * scale).astype(np.float32).astype(dt), H)
    k, vv, vl = (VC._split(x[n].astype(dt), H) for n in ("k", "vv", "vl"))
    gv, gl = VC._split(x["gv"].astype(dt), H), VC._split(x["gl"].astype(dt), H)
    r = qs @ k.transpose(0, 1, 3, 2)
    s = np.clip(r, -VC.CLAMP, VC.CLAMP)
    gate = (r >= -VC.CLAMP) & (r <= VC.CLAMP)
    amp = np.where(np.abs(r) >= VC.CLAMP, 0.0, np.abs(qs) @ np.abs(k).transpose(0, 1, 3, 2))
    a, amp_a = s, amp
    if x["mask"] is not None:
        m = x["mask"].astype(dt)[:, None, None, :]
        a = np.where(m == 0, dt(VC.MASKED), (s + m).astype(dt))
        amp_a = np.where(m == 0, 0.0, amp + np.abs(m))
    p_v = VC._softmax(a)
    st = s.transpose(0, 1, 3, 2)
    M = st.max(-1, keepdims=True)
    e = np.maximum(st - M, -VC.CLAMP)
    p_l = VC._softmax(e)
    pd_v, pd_l = cm_v * p_v, cm_l * p_l                                           # the dropped probabilities
    out_v, out_l = pd_v @ vl, pd_l @ vv
    delta_v = (gv * out_v).sum(-1, keepdims=True)
    delta_l = (gl * out_l).sum(-1, keepdims=True)
    if variant == "delta_undropped":
        delta_v = (gv * (p_v @ vl)).sum(-1, keepdims=True)
        delta_l = (gl * (p_l @ vv)).sum(-1, keepdims=True)
    dp_v = gv @ vl.transpose(0, 1, 3, 2)
    dp_l = gl @ vv.transpose(0, 1, 3, 2)
    ds_v = p_v * (cm_v * dp_v - delta_v)
    ds_l = (p_l * (cm_l * dp_l - delta_l)).transpose(0, 1, 3, 2)
    dr = np.where(gate, ds_v + ds_l, 0.0)
    pd_vl = keep_v.reshape(B, H, S, T).astype(dt) * p_v if variant == "dvl_without_c" else pd_v
    out = dict(out_v=VC._merge(out_v), out_l=VC._merge(out_l), dq=VC._merge((dr @ k) * dt(scale)),
               dk=VC._merge(dr.transpose(0, 1, 3, 2) @ qs), dvl=VC._merge(pd_vl.transpose(0, 1, 3, 2) @ gv),
               dvv=VC._merge(pd_l.transpose(0, 1, 3, 2) @ gl), dr=dr, r=r, e=e)
    if dt is np.float64 and variant is None:
        A_v = (1.0 + 2.0 * amp_a.max(-1, keepdims=True))
        A_l = (1.0 + 2.0 * amp.max(-2, keepdims=True))
        av, al = np.abs(vl), np.abs(vv)
        mds_v = A_v * p_v * (cm_v * (np.abs(gv) @ av.transpose(0, 1, 3, 2)) + (np.abs(gv) * (pd_v @ av)).sum(-1, keepdims=True))
        mds_l = A_l * p_l.transpose(0, 1, 3, 2) * (
            cm_l * (np.abs(gl) @ al.transpose(0, 1, 3, 2)) + (np.abs(gl) * (pd_l @ al)).sum(-1, keepdims=True)).transpose(0, 1, 3, 2)
        mdr = np.where(gate, mds_v + mds_l, 0.0)
        out.update(mag_out_v=VC._merge(A_v * (pd_v @ av)), mag_out_l=VC._merge(A_l.transpose(0, 1, 3, 2) * (pd_l @ al)),
                   mag_dq=VC._merge(mdr @ np.abs(k)) * float(scale), mag_dk=VC._merge(mdr.transpose(0, 1, 3, 2) @ np.abs(qs)),
                   mag_dvl=VC._merge((A_v * pd_v).transpose(0, 1, 3, 2) @ np.abs(gv)),
                   mag_dvv=VC._merge((A_l * pd_l.transpose(0, 1, 3, 2)) @ np.abs(gl)))
    return out


OUTPUTS = VC.GRADS + ("out_v", "out_l")


def check(got, x, keep_v, keep_l, p, who, worst=None):
    """Every entry of the six outputs within parity_measure.entry_bound of the float64 restatement, with the fp32 composition
    under the same masks as the comparison term; records the worst ratio per output in `worst`."""
    want, comp = core(x, keep_v, keep_l, p, np.float64), core(x, keep_v, keep_l, p, np.float32)
    for name in OUTPUTS:
        err = VC.PM.errors(np.asarray(got[name], dtype=np.float64), want[name], want["mag_" + name], comp[name].astype(np.float64))
        if worst is not None and err.worst >= worst.get(name, (-1.0,))[0]:
            worst[name] = (err.worst, "%-52s %-6s %10.3e %10.3e %10.3e %8.3f" % ((who, name) + tuple(err.row())))
        err.check(who, name)
