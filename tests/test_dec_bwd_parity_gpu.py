"""GPU: the decoder self-attention core's training route through the C ABI (biattn_hip_self_train_f32,
biattn_hip_self_backward_f32) against the float64 restatement of tests/dec_bwd_parity.py, entry by entry, on seeded dyadic
inputs at the lengths, mask patterns, dead queries and stress inputs where the 32-token tile, the two-wave split of the streamed
tiles, the skip test and the [L, L] mask's two reading directions can go wrong.

Every buffer the entries write is NaN-filled, exactly sized and followed by 64 sentinel floats.  Per case: `out` is bitwise
biattn_hip_self_forward_f32's; every one of the B heads x SP lse entries is written, the rows past L are exactly 0, a dead
query's is exactly -inf, every other is finite; the workspace is exactly biattn_hip_self_backward_workspace_bytes, which is
dec_bwd_parity.delta_bytes; after the backward no NaN is left outside dead dq rows, every sentinel is bitwise intact, every
input (q, k, v, mask, out, lse, grad_out) is bitwise unchanged and the route name tells the mask kind.  Every entry of lse, dq,
dk, dv is held to max(8 x the fp32 PyTorch composition's error of the same entry, computed on the device, 16 x 2^-24 x the
entry's magnitude) with the project's bound on top (dec_bwd_parity's docstring).  The tables are printed; with
DEC_BWD_PARITY_TABLE set they are appended to that file.

Beyond the sweep: six independent row strides with sentinels in the gaps (bitwise the contiguous run's results), a bool mask at
an odd byte address, bool against its -inf float form on every mask-pattern case, rejected calls that leave NaN-filled outputs
untouched (the return codes themselves are tests/test_decoder_train_cpu.py::test_error_codes_without_a_device's, which pins
every one of them without a device; here the same calls are made on real buffers for what that test cannot see), and a dead
query with a non-finite grad_out row (include/biattn_hip.h: dk and dv of that (batch, head) are then not finite; nothing else
is touched).

Largest kernel error / bound seen on an MI355X, per group over every case of this file (the entry's kernel error, the
composition's error and the bound are relative to the entry's magnitude; profiles/r34_dec_bwd_parity.txt has every line):
    lse   0.141   L130/sharp/2x3           1.34e-07   1.03e-07   9.54e-07
    dq    0.021   L130/f32_last_open/2x3   2.00e-08   0.00e+00   9.54e-07
    dk    0.022   L130/sharp/2x3           2.07e-08   1.84e-08   9.54e-07
    dv    0.055   L130/sharp/2x3           5.26e-08   5.13e-08   9.54e-07
Every entry of every case met its bound with the magnitudes as derived in dec_bwd_parity's docstring: no term had to be added
after the run, and the sweep found no kernel bug.  With a NaN or +inf grad_out row of a dead query all 1280 entries of dk and of
dv of its (batch, head) came out NaN (L = 40), the rest bitwise unchanged.  The file takes 4.3 s (28 tests).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dec_bwd_parity as P     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAIL = 64
D = P.D
ROUTE = {"none": "dec_bwd_q<none>+dec_bwd_kv<none>", "bool": "dec_bwd_q<bool>+dec_bwd_kv<bool>", "f32": "dec_bwd_q<f32>+dec_bwd_kv<f32>"}


def _sentinel(n=TAIL):
    return (torch.arange(n, dtype=torch.float32, device=DEV) % 4096) * -3.0 - 0.625


def guarded(n):
    buf = torch.full((n + TAIL,), float("nan"), dtype=torch.float32, device=DEV)
    buf[n:] = _sentinel()
    return buf


def intact(buf, n, what):
    assert buf.numel() == n + TAIL
    assert torch.equal(buf[n:].view(torch.int32), _sentinel().view(torch.int32)), what + ": written past the end"


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Rows:
    """[B, L, E] rows `stride` floats apart in a buffer of exactly B L stride floats (+ the tail), the gaps between the rows
    and the tail holding sentinels; the payload is `fill` (a tensor, or NaN)."""

    def __init__(self, B, L, E, stride, fill=None, offset=0, base=None):
        self.n = B * L * stride
        self.buf = base if base is not None else torch.cat([_sentinel(self.n), _sentinel()])
        self.view = self.buf[:self.n].view(B, L, stride)[..., offset:offset + E]
        self.view[...] = float("nan") if fill is None else fill
        self.stride = stride
        self.rest = torch.ones(self.n + TAIL, dtype=torch.bool, device=DEV)       # everything but the payload
        self.rest[:self.n].view(B, L, stride)[..., offset:offset + E] = False

    def ptr(self):
        return self.view.data_ptr()

    def freeze(self):
        self.before = self.buf.clone()

    def gaps_intact(self, what):
        """everything but the payload is bitwise what it was at freeze()"""
        now, was = self.buf.view(torch.int32)[self.rest], self.before.view(torch.int32)[self.rest]
        assert now.numel() == self.n + TAIL - self.view.numel() and torch.equal(now, was), what + ": a gap between rows or the tail was written"


def device_mask(mask, odd=False):
    """(tensor that owns the memory, pointer, kind code, kind) of a case's mask on the device; odd: a bool mask at an address
    with data_ptr() % 4 == 1"""
    from uninext_amd import _lib
    if mask is None:
        return None, None, _lib.BIATTN_MASK_NONE, "none"
    if mask.dtype == torch.bool:
        if odd:
            raw = torch.zeros(mask.numel() + 8, dtype=torch.uint8, device=DEV)
            start = (1 - raw.data_ptr()) % 4
            m = raw[start:start + mask.numel()]
            m.copy_(mask.reshape(-1).to(torch.uint8))
            assert m.data_ptr() % 4 == 1
            return m, m.data_ptr(), _lib.BIATTN_MASK_BOOL, "bool"
        m = mask.to(DEV).contiguous()
        return m, m.data_ptr(), _lib.BIATTN_MASK_BOOL, "bool"
    m = mask.float().to(DEV).contiguous()
    return m, m.data_ptr(), _lib.BIATTN_MASK_F32, "f32"


def run(name, strided=False, odd_mask=False, mask=None):
    """{lse, dq, dk, dv, out} of the two entries on a case, every contract of the C ABI asserted on the way.  strided: six
    independent row strides, q and k the halves of one buffer.  mask: another mask than the case's (its -inf float form)."""
    from uninext_amd import _lib
    c, x = P.CASES[name], P.inputs(name)
    B, heads, L, scale = c["B"], c["heads"], c["L"], x["scale"]
    E, BH = heads * D, B * heads
    SP = -(-L // P.TILE) * P.TILE
    lib = _lib.load()
    f = lambda t: t.float().to(DEV)
    if strided:
        sq = sk = 2 * E + 8
        q = Rows(B, L, E, sq, f(x["q"]))
        k = Rows(B, L, E, sk, f(x["k"]), offset=E, base=q.buf)
        v = Rows(B, L, E, E + 4, f(x["v"]))
        dq, dk, dv = Rows(B, L, E, 2 * E + 8), Rows(B, L, E, E + 12), Rows(B, L, E, E + 4)
    else:
        q, k, v = (Rows(B, L, E, E, f(x[n])) for n in ("q", "k", "v"))
        dq, dk, dv = (Rows(B, L, E, E) for _ in range(3))
    g = f(x["g"]).contiguous()
    m_own, m_ptr, kind, kind_name = device_mask(x["mask"] if mask is None else mask, odd_mask)
    dead = list(x["dead"])

    # ---- the train entry
    out, lse = guarded(B * L * E), guarded(BH * SP)
    rc = lib.biattn_hip_self_train_f32(q.ptr(), k.ptr(), v.ptr(), q.stride, k.stride, v.stride, m_ptr, kind, B, heads, L, D, scale,
                                       out.data_ptr(), lse.data_ptr(), None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    intact(out, B * L * E, name + " out")
    intact(lse, BH * SP, name + " lse")
    out_t, lse_t = out[:B * L * E].view(B, L, E), lse[:BH * SP].view(BH, SP)
    assert not bool(torch.isnan(lse_t).any()), name + ": lse entries left unwritten"
    assert bool((lse_t[:, L:] == 0).all()), name + ": lse rows past L"
    live = [i for i in range(L) if i not in dead]
    assert bool((lse_t[:, dead] == float("-inf")).all()) and bool(torch.isfinite(lse_t[:, live]).all()), name + ": lse of dead / live queries"
    assert bool(torch.isnan(out_t[:, dead]).all()) and bool(torch.isfinite(out_t[:, live]).all()), name + ": out of dead / live queries"
    out2 = guarded(B * L * E)
    rc = lib.biattn_hip_self_forward_f32(q.ptr(), k.ptr(), v.ptr(), q.stride, k.stride, v.stride, m_ptr, kind, B, heads, L, D, scale,
                                         out2.data_ptr(), None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    intact(out2, B * L * E, name + " inference out")
    assert same_bits(out, out2), name + ": out is not the inference entry's"

    # ---- the backward entry
    nb = lib.biattn_hip_self_backward_workspace_bytes(B, heads, L, D)
    assert nb == P.delta_bytes(B, heads, L) and nb % 256 == 0, (name, nb)
    ws = guarded(nb // 4)
    held = [t for t in (q.buf, None if k.buf is q.buf else k.buf, v.buf, m_own, out, lse, g) if t is not None]
    assert len(held) == 7 - (k.buf is q.buf) - (m_own is None)      # q, k, v, mask, out, lse, grad_out: every input
    before = [t.clone() for t in held]
    for r in (dq, dk, dv):
        r.freeze()
    rc = lib.biattn_hip_self_backward_f32(q.ptr(), k.ptr(), v.ptr(), q.stride, k.stride, v.stride, m_ptr, kind, out.data_ptr(),
                                          lse.data_ptr(), g.data_ptr(), B, heads, L, D, scale, dq.ptr(), dk.ptr(), dv.ptr(), dq.stride,
                                          dk.stride, dv.stride, ws.data_ptr(), nb, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert _lib.last_kernel("dec_attn_bwd") == ROUTE[kind_name], name
    intact(ws, nb // 4, name + " workspace")
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.uint8)
    for was, now in zip(before, held):
        assert torch.equal(bits(was), bits(now)), name + ": an input was written"
    for r, what in ((dq, "dq"), (dk, "dk"), (dv, "dv")):
        r.gaps_intact(name + " " + what)
    got = {"lse": lse_t[:, :L].clone(), "dq": dq.view.clone(), "dk": dk.view.clone(), "dv": dv.view.clone(), "out": out_t.clone()}
    assert bool(torch.isnan(got["dq"][:, dead]).all()) and not bool(torch.isnan(got["dq"][:, live]).any()), name + ": NaN in dq"
    assert not bool(torch.isnan(got["dk"]).any()) and not bool(torch.isnan(got["dv"]).any()), name + ": entries left unwritten"
    return got


def check(name):
    P.mask_property(name)
    if P.CASES[name]["stress"]:
        P.stress_property(name)
    got = run(name)
    ref, comp = P.reference(name), P.composition(name, DEV)
    assert sorted(ref) == sorted(comp) == sorted(P.GROUPS), name
    for what, (want, mag) in ref.items():
        P.measure(name, what, got[what], want, mag, comp[what])
    return got


def sweep(cases, count):
    since = len(P.TABLE)
    assert len(cases) == count, (len(cases), count)
    got = {name: check(name) for name in cases}
    P.report(since)
    return got


@pytest.mark.parametrize("L", P.AP.DEC_LENS)
def test_lengths(L):
    sweep(P.names(group="len", L=L), 6)                             # none, bool, f32 at both batch x heads


@pytest.mark.parametrize("pattern", [p for p, _ in P.PATTERNS])
def test_mask_patterns_bool_and_inf_give_the_same_bits(pattern):
    got = sweep(P.names(group="pattern", pattern=pattern), 8)
    for name, b in got.items():
        if "/bool_" in name:            # the same tensors (a case's are seeded by its name) under the mask's -inf float form
            f = run(name, mask=P._as_f32_mask(P.inputs(name)["mask"]))
            for key in ("out", "lse", "dq", "dk", "dv"):
                assert same_bits(b[key], f[key]), (name, key, "bool and its -inf float form")
    if pattern in ("last_open", "closed_tile", "closed_key"):      # the keys nobody attends to: exact zeros, stored
        for name, t in got.items():
            closed = P.inputs(name)["mask"]
            closed = (closed if closed.dtype == torch.bool else closed == P.NEG).all(0).to(DEV)
            assert bool(closed.any()) and bool((t["dk"][:, closed] == 0).all()) and bool((t["dv"][:, closed] == 0).all()), name


def test_finite_float_masks():
    sweep(P.names(group="float"), 6)


@pytest.mark.parametrize("pattern", [p for p, _ in P.DEAD])
def test_dead_queries(pattern):
    sweep(P.names(group="dead", pattern=pattern), 4)


def test_stress():
    sweep(P.names(group="stress"), 12)


def test_batch_and_head_counts():
    sweep(P.names(group="bh"), 6)


def test_six_row_strides_give_the_contiguous_bits_and_leave_the_gaps():
    name = "L65/bool/2x3"
    a, b = run(name), run(name, strided=True)
    for key in ("out", "lse", "dq", "dk", "dv"):
        assert same_bits(a[key], b[key]), key


def test_bool_mask_at_an_odd_byte_address():
    for name in ("L65/bool/2x3", "L97/bool_row45/1x1"):
        a, b = run(name), run(name, odd_mask=True)
        for key in ("out", "lse", "dq", "dk", "dv"):
            assert same_bits(a[key], b[key]), (name, key)


def test_rejected_calls_leave_the_outputs_untouched():
    """The codes are pinned without a device by tests/test_decoder_train_cpu.py::test_error_codes_without_a_device (every one
    below but head_dim 16); here each rejected call gets real, NaN-filled outputs, and they are all NaN afterwards."""
    from uninext_amd import _lib
    lib = _lib.load()
    B, heads, L = 2, 2, 40
    E = heads * D
    t = lambda *s: torch.randn(*s, device=DEV)
    q, k, v, g, out = t(B, L, E + 4)[..., :E], t(B, L, E), t(B, L, E), t(B, L, E), t(B, L, E)
    lse = t(B * heads, 64)
    fmask, bmask = torch.zeros(L * L + 4, device=DEV), torch.zeros(L, L, dtype=torch.bool, device=DEV)
    nb = lib.biattn_hip_self_backward_workspace_bytes(B, heads, L, D)
    ws = torch.zeros(nb // 4, device=DEV)
    outs = [guarded(B * L * E) for _ in range(3)]
    tout, tlse = guarded(B * L * E), guarded(B * heads * 64)
    base = dict(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), qs=E + 4, ks=E, vs=E, mask=None, kind=_lib.BIATTN_MASK_NONE,
                out=out.data_ptr(), lse=lse.data_ptr(), g=g.data_ptr(), B=B, heads=heads, L=L, D=D, dq=outs[0].data_ptr(),
                dk=outs[1].data_ptr(), dv=outs[2].data_ptr(), dqs=E, dks=E, dvs=E, ws=ws.data_ptr(), nb=nb)

    def back(**kw):
        a = dict(base, **kw)
        return lib.biattn_hip_self_backward_f32(a["q"], a["k"], a["v"], a["qs"], a["ks"], a["vs"], a["mask"], a["kind"], a["out"], a["lse"],
                                                a["g"], a["B"], a["heads"], a["L"], a["D"], 0.25, a["dq"], a["dk"], a["dv"], a["dqs"],
                                                a["dks"], a["dvs"], a["ws"], a["nb"], None)

    def train(**kw):
        a = dict(base, out=tout.data_ptr(), lse=tlse.data_ptr())
        a.update(kw)
        return lib.biattn_hip_self_train_f32(a["q"], a["k"], a["v"], a["qs"], a["ks"], a["vs"], a["mask"], a["kind"], a["B"], a["heads"],
                                             a["L"], a["D"], 0.25, a["out"], a["lse"], None)

    NULL, DIMS, UNSUP, WS = -1, -2, -5, -6
    both = [(dict(D=16), UNSUP), (dict(D=64), UNSUP), (dict(L=0), DIMS), (dict(L=65536), DIMS), (dict(qs=E - 4), DIMS),
            (dict(ks=E + 2), UNSUP), (dict(q=None), NULL), (dict(k=None), NULL), (dict(v=None), NULL), (dict(out=None), NULL),
            (dict(lse=None), NULL), (dict(kind=_lib.BIATTN_MASK_BOOL), NULL), (dict(kind=_lib.BIATTN_MASK_F32), NULL),
            (dict(q=q.data_ptr() + 4), UNSUP), (dict(mask=fmask.data_ptr() + 2, kind=_lib.BIATTN_MASK_F32), UNSUP),
            (dict(mask=bmask.data_ptr(), kind=_lib.BIATTN_MASK_INT64), UNSUP), (dict(mask=bmask.data_ptr(), kind=7), UNSUP)]
    only_back = [(dict(dvs=E - 4), DIMS), (dict(dqs=E + 2), UNSUP), (dict(g=None), NULL), (dict(dq=None), NULL), (dict(dk=None), NULL),
                 (dict(dv=None), NULL), (dict(ws=None), NULL), (dict(nb=nb - 1), WS), (dict(dk=outs[1].data_ptr() + 4), UNSUP)]
    for kw, code in both:
        assert train(**kw) == code, ("train", kw, _lib.last_error())
    for kw, code in both + only_back:
        assert back(**kw) == code, ("backward", kw, _lib.last_error())
    none = dict(q=None, k=None, v=None, out=None, lse=None, g=None, dq=None, dk=None, dv=None, ws=None, nb=0, B=0)
    assert back(**none) == 0 and train(**none) == 0                 # batch == 0 with every pointer null
    torch.cuda.synchronize()
    for buf, n in [(o, B * L * E) for o in outs] + [(tout, B * L * E), (tlse, B * heads * 64)]:
        intact(buf, n, "a rejected call")
        assert bool(torch.isnan(buf[:n]).all()), "a rejected call wrote an output"


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("kind", ["bool", "float"])
def test_a_dead_query_with_a_non_finite_grad_out_row(kind, bad):
    """include/biattn_hip.h: a dead query adds exactly nothing to dk and dv FOR A FINITE grad_out ROW.  With a non-finite row the
    key pass's 0 * g products are NaN wherever the query's tile is streamed: what is pinned is that they stay inside that
    query's (batch, head), every other (batch, head) of dk and dv and ALL of dq (the query pass reads no other query's g; the
    dead row is the same NaN) keeping the bits of the run with a finite row, and that a finite row gives the bits of the run
    with that row zeroed.  Through the C ABI.  Printed: how many entries of dk and dv of the (batch, head) are not finite."""
    import decoder_cases as C
    import decoder_train_cases as T
    from uninext_amd import _lib
    lib = _lib.load()
    L, dead, B, heads = 40, 17, 2, 2
    E, SP = heads * D, 64
    qk, v = C.kernel_case(62, B, L, heads)
    G = T.upstream(62, B, L, E)
    mask = T.mask_of(kind, 62, L)
    mask[dead] = True if kind == "bool" else float("-inf")
    q, k, v_d = qk[..., :E].contiguous().to(DEV), qk[..., E:].contiguous().to(DEV), v.to(DEV)
    m_own, m_ptr, code, kind_name = device_mask(mask.double() if kind == "float" else mask)
    scale = P.AP.fp32_scale(D)
    out, lse = guarded(B * L * E), guarded(B * heads * SP)
    rc = lib.biattn_hip_self_train_f32(q.data_ptr(), k.data_ptr(), v_d.data_ptr(), E, E, E, m_ptr, code, B, heads, L, D, scale,
                                       out.data_ptr(), lse.data_ptr(), None)
    assert rc == 0, _lib.last_error()
    nb = lib.biattn_hip_self_backward_workspace_bytes(B, heads, L, D)

    def back(g):
        g = g.to(DEV).contiguous()
        ws, bufs = guarded(nb // 4), [guarded(B * L * E) for _ in range(3)]
        rc = lib.biattn_hip_self_backward_f32(q.data_ptr(), k.data_ptr(), v_d.data_ptr(), E, E, E, m_ptr, code, out.data_ptr(),
                                              lse.data_ptr(), g.data_ptr(), B, heads, L, D, scale, *(t.data_ptr() for t in bufs), E, E, E,
                                              ws.data_ptr(), nb, None)
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        assert _lib.last_kernel("dec_attn_bwd") == ROUTE[kind_name]
        intact(ws, nb // 4, "workspace")
        for t in bufs:
            intact(t, B * L * E, "a gradient")
        return {key: t[:B * L * E].view(B, L, E).clone() for key, t in zip(("dq", "dk", "dv"), bufs)}

    zeroed = G.clone()
    zeroed[:, dead] = 0.0
    fin, zer = back(G), back(zeroed)
    for key in ("dk", "dv"):
        assert torch.isfinite(fin[key]).all() and same_bits(fin[key], zer[key]), (key, "a finite row adds exactly nothing")
    b, h = 1, 0
    poisoned = G.clone()
    poisoned[b, dead, h * D:(h + 1) * D] = bad
    got = back(poisoned)
    inside = torch.zeros(B, L, E, dtype=torch.bool, device=DEV)
    inside[b, :, h * D:(h + 1) * D] = True
    zero = torch.zeros((), device=DEV)
    for key in ("dk", "dv"):
        print("%s %s grad_out row %s: %d of %d entries of that (batch, head) not finite" % (
            kind, key, bad, int((~torch.isfinite(got[key][inside])).sum()), int(inside.sum())))
        assert same_bits(torch.where(inside, zero, got[key]), torch.where(inside, zero, fin[key])), key
    assert bool(torch.isnan(got["dq"][:, dead]).all()) and same_bits(got["dq"], fin["dq"]), "dq: the poisoned row is the dead query's own"
