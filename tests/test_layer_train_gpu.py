"""MI355X tests of the encoder layer's training kernels (include/dynmask_hip.h, uninext_amd/csrc/layer_train.hip): the exported keep
decisions against the numpy masks byte for byte, every output entry of the C ABI against the float64 restatements of
tests/layer_train_cases.py (parity_measure.entry_bound), the bitwise facts the header states, its refusals, and the functions and the
encoder layer under torch.autograd."""
import ctypes

import numpy as np
import pytest
import torch
from torch.utils.checkpoint import checkpoint

import layer_train_cases as LC
from golden_util import enclayer_names, load_golden

pytestmark = pytest.mark.gpu
TOL = 1e-4            # the project's bound, of max(1, the tensor's largest value)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from uninext_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def worst_table():
    yield
    print("\nWORST per output, error / bound\n" + LC.HEAD + "\n" + LC.worst_table())


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _nan(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _np(t):
    return t.detach().cpu().numpy()


class Ln:
    """One LN_CASE on the device, driven through the C ABI with exactly sized, NaN-filled outputs and an 0xFF-filled workspace."""

    def __init__(self, case, dev, lib):
        self.case, self.dev, self.lib = case, dev, lib
        self.rows, self.f, self.p = case[:3]
        self.x = LC.ln_inputs(case)
        self.t = {k: _dev(self.x[k], dev) for k in ("x", "res", "gamma", "beta", "go")}
        self.seed = _dev(self.x["seed"], dev)
        self.keep = LC.keep_mask(self.x["seed"], self.p, self.rows, self.f)

    def forward(self, p=None):
        t, shape = self.t, (self.rows, self.f)
        z, out = _nan(shape, self.dev), _nan(shape, self.dev)
        rc = self.lib.dropout_add_layernorm_hip_train_f32(_p(t["x"]), _p(t["res"]), _p(t["gamma"]), _p(t["beta"]), self.x["eps"], self.rows,
                                                          self.f, self.p if p is None else p, _p(self.seed), _p(z), _p(out), _stream())
        assert rc == 0, rc
        return z, out

    def backward(self, z, need=(True, True, True, True), p=None):
        shape = (self.rows, self.f)
        outs = [_nan(shape, self.dev) if need[0] else None, _nan(shape, self.dev) if need[1] else None,
                _nan((self.f,), self.dev) if need[2] else None, _nan((self.f,), self.dev) if need[3] else None]
        nbytes = int(self.lib.dropout_add_layernorm_hip_backward_workspace_bytes(self.rows, self.f)) if need[2] or need[3] else 0
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=self.dev) if nbytes else None
        rc = self.lib.dropout_add_layernorm_hip_backward_f32(_p(self.t["go"]), _p(z), _p(self.t["gamma"]), self.x["eps"], self.rows, self.f,
                                                             self.p if p is None else p, _p(self.seed), *[_p(o) for o in outs], _p(ws),
                                                             nbytes, _stream())
        assert rc == 0, rc
        return outs

    def unchanged(self):
        for k, t in self.t.items():
            assert t is None or np.array_equal(_np(t), self.x[k]), k
        assert np.array_equal(_np(self.seed), self.x["seed"])


# ---------------------------------------------------------------------------------------------------------------------- export

@pytest.mark.parametrize("features", LC.EXPORT_FEATURES)
def test_export_is_the_numpy_mask(features, dev, lib):
    from uninext_amd import ext
    for rows in LC.EXPORT_ROWS:
        seed = LC.seed_of("export/%d/%d" % (rows, features))
        for p in LC.EXPORT_PS:
            got = ext.row_dropout_keep(_dev(seed, dev), p, rows, features)
            assert got.dtype == torch.uint8 and got.shape == (rows, features)
            assert np.array_equal(_np(got), LC.keep_mask(seed, p, rows, features).astype(np.uint8)), (rows, features, p)
        assert bool((ext.row_dropout_keep(_dev(seed, dev), 0.0, rows, features) == 1).all())


# ------------------------------------------------------------------------------------------------------------- C ABI parity

@pytest.mark.parametrize("case", LC.LN_CASES, ids=LC.ln_name)
def test_dropout_add_layernorm_parity(case, dev, lib):
    c = Ln(case, dev, lib)
    x, who = c.x, LC.ln_name(case)
    z, out = c.forward()
    args = (x["x"], x["res"], x["gamma"], x["beta"], x["eps"], c.keep, c.p)
    LC.check(dict(z=_np(z), out=_np(out)), LC.ln_forward(*args), LC.ln_forward(*args, dt=np.float32), LC.LN_OUTPUTS, who)
    zn = _np(z)
    got = c.backward(z)
    torch.cuda.synchronize()
    c.unchanged()
    assert np.array_equal(_np(z), zn)
    bargs = (x["go"], zn, x["gamma"], x["eps"], c.keep, c.p)
    LC.check(dict(zip(LC.LN_GRADS, (_np(t) for t in got))), LC.ln_backward(*bargs), LC.ln_backward(*bargs, dt=np.float32), LC.LN_GRADS, who)


@pytest.mark.parametrize("case", LC.RELU_CASES, ids=LC.relu_name)
def test_relu_dropout_parity(case, dev, lib):
    rows, f, p = case
    x, who = LC.relu_inputs(case), LC.relu_name(case)
    h, go, seed = _dev(x["h"], dev), _dev(x["go"], dev), _dev(x["seed"], dev)
    keep = LC.keep_mask(x["seed"], p, rows, f)
    out, gh = _nan((rows, f), dev), _nan((rows, f), dev)
    assert lib.relu_dropout_hip_f32(_p(h), rows, f, p, _p(seed), _p(out), _stream()) == 0
    assert lib.relu_dropout_hip_backward_f32(_p(go), _p(out), rows, f, p, _p(gh), _stream()) == 0
    on = _np(out)
    LC.check(dict(out=on), LC.relu_forward(x["h"], keep, p), LC.relu_forward(x["h"], keep, p, np.float32), ("out",), who)
    assert np.array_equal(on > 0, keep & (x["h"] > 0))                     # positive exactly where h was positive and kept
    LC.check(dict(gh=_np(gh)), LC.relu_backward(x["go"], on, p), LC.relu_backward(x["go"], on, p, np.float32), ("gh",), who)
    assert np.array_equal(_np(h), x["h"]) and np.array_equal(_np(go), x["go"]) and np.array_equal(_np(seed), x["seed"])


# --------------------------------------------------------------------------------------------------------------- bitwise facts

BITWISE = [(5, 256, 0.1, True, True), (257, 260, 0.5, False, True), (1031, 768, 0.1, True, True), (4, 2048, 0.1, False, True),
           (5, 4096, 0.5, True, False)]       # one per chunk count: 1, 2, 4, 8, 16


@pytest.mark.parametrize("case", BITWISE, ids=LC.ln_name)
def test_bitwise_facts(case, dev, lib):
    c = Ln(case, dev, lib)
    t = c.t
    z0, out0 = c.forward(p=0.0)                                            # p = 0: add_layernorm's bits, grad_x = grad_residual
    plain = _nan((c.rows, c.f), dev)
    assert lib.add_layernorm_hip_f32(_p(t["x"]), _p(t["res"]), _p(t["gamma"]), _p(t["beta"]), c.x["eps"], c.rows, c.f, _p(plain), _stream()) == 0
    assert torch.equal(out0, plain)
    gx0, gres0, _, _ = c.backward(z0, p=0.0)
    assert torch.equal(gx0, gres0)
    z, out = c.forward()
    first = c.backward(z)
    z2, out2 = c.forward()                                                 # two runs
    second = c.backward(z2)
    assert torch.equal(z, z2) and torch.equal(out, out2)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    side = torch.cuda.Stream()                                             # a side stream
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        z3, out3 = c.forward()
        third = c.backward(z3)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(z, z3) and torch.equal(out, out3) and all(torch.equal(a, b) for a, b in zip(first, third))
    for need in ((True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True),
                 (True, True, False, False), (False, False, True, True)):
        for got, want, needed in zip(c.backward(z, need), first, need):    # NULL pointers leave the other outputs' bits alone
            assert (got is None) != needed and (got is None or torch.equal(got, want)), need


def test_relu_dropout_bitwise(dev):
    from uninext_amd import ext
    x = LC.relu_inputs((1031, 2048, 0.1))
    h, go, seed = _dev(x["h"], dev), _dev(x["go"], dev), _dev(x["seed"], dev)
    out = ext.relu_dropout(h, 0.1, seed)
    assert torch.equal(out, ext.relu_dropout(h, 0.1, seed))
    assert torch.equal(ext.relu_dropout(h, 0.0, None), torch.relu(h))
    gh = ext.relu_dropout_backward(go, out, 0.1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out2 = ext.relu_dropout(h, 0.1, seed)
        gh2 = ext.relu_dropout_backward(go, out2, 0.1)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(out, out2) and torch.equal(gh, gh2)


# -------------------------------------------------------------------------------------------------------------------- refusals

def test_refusals_write_nothing(dev, lib):
    from uninext_amd import _lib
    NULLP, DIMS, UNSUP, WS = (_lib.LAYERNORM_ERR_NULL_POINTER, _lib.LAYERNORM_ERR_BAD_DIMS, _lib.LAYERNORM_ERR_UNSUPPORTED,
                              _lib.LAYERNORM_ERR_WORKSPACE)
    rows, f = 40, 256
    x, go = torch.randn(rows, f, device=dev), torch.randn(rows, f, device=dev)
    seed = _dev(LC.seed_of("refusals"), dev)
    a, b, ga, gb = (_nan((rows, f), dev) for _ in range(4))
    va, vb = _nan((f,), dev), _nan((f,), dev)
    big = torch.randn(2, 65540, device=dev)
    bout = _nan((2, 65540), dev)
    need = int(lib.dropout_add_layernorm_hip_backward_workspace_bytes(rows, f))
    assert need == 2 * 2 * f * 8
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    keep = torch.full((rows, f), 7, dtype=torch.uint8, device=dev)
    train, bwd = lib.dropout_add_layernorm_hip_train_f32, lib.dropout_add_layernorm_hip_backward_f32
    s = _stream()
    calls = [
        (UNSUP, train, (_p(x), None, None, None, 1e-5, rows * f // 6, 6, 0.0, None, _p(a), _p(b), s)),
        (UNSUP, train, (_p(big), None, None, None, 1e-5, 2, 65540, 0.0, None, _p(bout), _p(bout), s)),
        (DIMS, train, (_p(x), None, None, None, 1e-5, rows, f, 1.0, _p(seed), _p(a), _p(b), s)),
        (DIMS, train, (_p(x), None, None, None, 1e-5, rows, f, -0.5, _p(seed), _p(a), _p(b), s)),
        (DIMS, train, (_p(x), None, None, None, 1e-5, rows, f, float("nan"), _p(seed), _p(a), _p(b), s)),
        (NULLP, train, (_p(x), None, None, None, 1e-5, rows, f, 0.1, None, _p(a), _p(b), s)),
        (NULLP, train, (None, None, None, None, 1e-5, rows, f, 0.0, None, _p(a), _p(b), s)),
        (NULLP, train, (_p(x), None, None, None, 1e-5, rows, f, 0.0, None, None, _p(b), s)),
        (NULLP, train, (_p(x), None, None, None, 1e-5, rows, f, 0.0, None, _p(a), None, s)),
        (UNSUP, bwd, (_p(go), _p(x), None, 1e-5, rows * f // 6, 6, 0.0, None, _p(ga), _p(gb), _p(va), _p(vb), _p(ws), need, s)),
        (DIMS, bwd, (_p(go), _p(x), None, 1e-5, rows, f, 1.5, _p(seed), _p(ga), _p(gb), _p(va), _p(vb), _p(ws), need, s)),
        (NULLP, bwd, (_p(go), _p(x), None, 1e-5, rows, f, 0.1, None, _p(ga), _p(gb), _p(va), _p(vb), _p(ws), need, s)),
        (NULLP, bwd, (None, _p(x), None, 1e-5, rows, f, 0.0, None, _p(ga), _p(gb), _p(va), _p(vb), _p(ws), need, s)),
        (NULLP, bwd, (_p(go), None, None, 1e-5, rows, f, 0.0, None, _p(ga), _p(gb), _p(va), _p(vb), _p(ws), need, s)),
        (NULLP, bwd, (_p(go), _p(x), None, 1e-5, rows, f, 0.0, None, _p(ga), _p(gb), _p(va), _p(vb), None, need, s)),
        (WS, bwd, (_p(go), _p(x), None, 1e-5, rows, f, 0.0, None, _p(ga), _p(gb), _p(va), _p(vb), _p(ws), need - 1, s)),
        (UNSUP, lib.relu_dropout_hip_f32, (_p(big), 2, 65540, 0.0, None, _p(bout), s)),
        (UNSUP, lib.relu_dropout_hip_f32, (_p(x), rows * f // 6, 6, 0.0, None, _p(a), s)),
        (DIMS, lib.relu_dropout_hip_f32, (_p(x), rows, f, 1.0, _p(seed), _p(a), s)),
        (NULLP, lib.relu_dropout_hip_f32, (_p(x), rows, f, 0.1, None, _p(a), s)),
        (NULLP, lib.relu_dropout_hip_f32, (None, rows, f, 0.0, None, _p(a), s)),
        (UNSUP, lib.relu_dropout_hip_backward_f32, (_p(go), _p(x), rows * f // 6, 6, 0.0, _p(ga), s)),
        (DIMS, lib.relu_dropout_hip_backward_f32, (_p(go), _p(x), rows, f, 1.0, _p(ga), s)),
        (NULLP, lib.relu_dropout_hip_backward_f32, (_p(go), None, rows, f, 0.1, _p(ga), s)),
        (UNSUP, lib.row_dropout_hip_keep_u8, (_p(seed), 0.1, rows * f // 6, 6, _p(keep), s)),
        (DIMS, lib.row_dropout_hip_keep_u8, (_p(seed), 1.0, rows, f, _p(keep), s)),
        (NULLP, lib.row_dropout_hip_keep_u8, (None, 0.1, rows, f, _p(keep), s)),
    ]
    for k, (code, fn, args) in enumerate(calls):
        assert fn(*args) == code, (k, fn.__name__)
        assert _lib.last_error(), k
    for fn, args in ((train, (None, None, None, None, 1e-5, 0, f, 0.0, None, None, None, s)),            # rows == 0: nothing to do
                     (bwd, (None, None, None, 1e-5, 0, f, 0.0, None, None, None, None, None, None, 0, s)),
                     (lib.relu_dropout_hip_f32, (None, 0, f, 0.0, None, None, s)),
                     (lib.relu_dropout_hip_backward_f32, (None, None, 0, f, 0.0, None, s)),
                     (lib.row_dropout_hip_keep_u8, (_p(seed), 0.1, 0, f, None, s))):
        assert fn(*args) == 0, fn.__name__
    torch.cuda.synchronize()
    for t in (a, b, ga, gb, va, vb, bout):
        assert bool(torch.isnan(t).all())
    assert bool((ws == 0xFF).all()) and bool((keep == 7).all())


# ---------------------------------------------------------------------------------------------------------------------- module

def test_functions_against_the_c_abi(dev, lib):
    from uninext_amd.functions import DropoutAddLayerNormFunction, ReluDropoutFunction
    case = (257, 260, 0.5, True, True)
    c = Ln(case, dev, lib)
    z, out = c.forward()
    want = c.backward(z)
    leaves = [c.t[k].clone().requires_grad_(True) for k in ("x", "res", "gamma", "beta")]
    got = DropoutAddLayerNormFunction.apply(*leaves, c.x["eps"], c.p, c.seed)
    assert torch.equal(got, out)
    got.backward(c.t["go"])
    assert all(torch.equal(leaf.grad, w) for leaf, w in zip(leaves, want))
    x_only = c.t["x"].clone().requires_grad_(True)                         # needs_input_grad: a single gradient, the same bits
    DropoutAddLayerNormFunction.apply(x_only, c.t["res"], c.t["gamma"], c.t["beta"], c.x["eps"], c.p, c.seed).backward(c.t["go"])
    assert torch.equal(x_only.grad, want[0])
    x = LC.relu_inputs((5, 252, 0.5))
    h, go, seed = _dev(x["h"], dev).requires_grad_(True), _dev(x["go"], dev), _dev(x["seed"], dev)
    keep = LC.keep_mask(x["seed"], 0.5, 5, 252)
    out = ReluDropoutFunction.apply(h, 0.5, seed)
    out.backward(go)
    assert np.array_equal(_np(out), LC.relu_forward(x["h"], keep, 0.5, np.float32)["out"])          # p = 0.5: c = 2, exact
    assert np.array_equal(_np(h.grad), LC.relu_backward(x["go"], _np(out), 0.5, np.float32)["gh"])


def _golden_layer(name, dev, dropout, dtype=torch.float32):
    from uninext_amd.modules import DeformableTransformerEncoderLayer
    g = load_golden(name)
    params = {k[2:]: torch.from_numpy(v).to(dtype) for k, v in g.items() if k.startswith("p:")}
    d_model, d_ffn = params["linear1.weight"].shape[1], params["linear1.weight"].shape[0]
    layer = DeformableTransformerEncoderLayer(d_model=d_model, d_ffn=d_ffn, dropout=dropout, n_heads=d_model // 32)
    layer.load_state_dict(params)
    f = lambda k: torch.from_numpy(g[k]).to(dev)
    inputs = dict(src=f("src").to(dtype), pos=f("pos").to(dtype), ref=f("ref").to(dtype), shapes=f("shapes"), lsi=f("lsi"),
                  mask=f("mask") if "mask" in g else None)
    return g, layer.to(dev).to(dtype), inputs


def _run(layer, x, go, wrap=None):
    """(out, grad_src, grad_pos, parameter gradients by name) of one forward + backward."""
    layer.zero_grad(set_to_none=True)
    src, pos = x["src"].clone().requires_grad_(True), x["pos"].clone().requires_grad_(True)
    fn = layer if wrap is None else (lambda *a: wrap(layer, *a))
    out = fn(src, pos, x["ref"], x["shapes"], x["lsi"], x["mask"])
    out.backward(go)
    return out.detach(), src.grad, pos.grad, {n: p.grad.clone() for n, p in layer.named_parameters()}


def _close(a, b, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert float((a - b).abs().max()) < TOL * max(1.0, float(b.abs().max())), (what, float((a - b).abs().max()))


def _differing(a, b):
    """the names of what is not bitwise the same in two results of _run"""
    names = [what for what, u, v in zip(("out", "grad_src", "grad_pos"), a[:3], b[:3]) if not torch.equal(u, v)]
    return names + [n for n in a[3] if not torch.equal(a[3][n], b[3][n])]


# What MSDeformAttn's grad_value feeds.  On these fixtures' shapes the operator's backward adds grad_value with float atomics
# ("not deterministic, exactly as in the reference": include/msda_hip.h), so these three differ in the last bits between ANY two
# backward passes, checkpointed or not, with the flags on or off; nothing this route computes lies behind them.
THROUGH_GRAD_VALUE = ("grad_src", "self_attn.value_proj.weight", "self_attn.value_proj.bias")


def _bitwise_under_checkpoint(plain, ckpt):
    """Every output and gradient bitwise the same, but for THROUGH_GRAD_VALUE, which are held to the project's bound."""
    assert [n for n in _differing(plain, ckpt) if n not in THROUGH_GRAD_VALUE] == []
    _close(ckpt[1], plain[1], "grad_src")
    for n in THROUGH_GRAD_VALUE[1:]:
        _close(ckpt[3][n], plain[3][n], n)


def _plain_and_checkpointed(layer, x, go, before=lambda: None):
    """_run without and under checkpoint(use_reentrant=False).  The MSDeformAttn operator chooses its kernels by what its call site
    has seen (a checkpointed step calls the forward twice) unless determinism is asked for, and its kernels differ in their fp32
    summation order: determinism is asked for around both runs, as tests/test_encoder_layer_gpu.py does to compare bit for bit."""
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        before()
        plain = _run(layer, x, go)
        before()
        return plain, _run(layer, x, go, wrap=lambda m, *a: checkpoint(m, *a, use_reentrant=False))
    finally:
        torch.use_deterministic_algorithms(False)


def _counting(monkeypatch):
    from uninext_amd.functions import layer_train
    calls = []
    for cls in (layer_train.DropoutAddLayerNormFunction, layer_train.ReluDropoutFunction):
        real = cls.apply
        monkeypatch.setattr(cls, "apply", staticmethod(lambda *a, _real=real, _n=cls.__name__: (calls.append(_n), _real(*a))[1]))
    return calls


@pytest.mark.parametrize("name", enclayer_names())
def test_layer_without_dropout_against_the_composition(name, dev, monkeypatch):
    g, layer, x = _golden_layer(name, dev, 0.0)
    layer.train()
    go = torch.from_numpy(LC.PM.dy(LC.PM.rng("layer/" + name).standard_normal(tuple(x["src"].shape)))).to(dev)
    want = _run(layer, x, go)
    calls = _counting(monkeypatch)
    layer.own_training = True
    got = _run(layer, x, go)
    assert calls == ["DropoutAddLayerNormFunction", "ReluDropoutFunction", "DropoutAddLayerNormFunction"]
    _close(got[0], torch.from_numpy(g["out"]), "out vs the fixture")
    for k, what in enumerate(("out", "grad_src", "grad_pos")):
        _close(got[k], want[k], what)
    assert sorted(got[3]) == sorted(want[3])
    for n in want[3]:
        _close(got[3][n], want[3][n], n)
    _bitwise_under_checkpoint(*_plain_and_checkpointed(layer, x, go))


def test_layer_with_dropout_against_float64_masks(dev, monkeypatch):
    """dropout 0.1, train(), set_own_training(True, dropout=True), fixed seeds: against a float64 CPU copy of the layer whose three
    dropouts multiply by the exported masks x 1 / (1 - p)."""
    from oracle.msda_gridsample import msda_gridsample
    from uninext_amd import ext
    from uninext_amd.modules import DeformableTransformerEncoderVL
    from uninext_amd.modules import ms_deform_attn as mod
    name, p = enclayer_names()[0], 0.1
    g, layer, x = _golden_layer(name, dev, p)
    enc = DeformableTransformerEncoderVL(torch.nn.Identity(), layer, torch.nn.Identity(), 1, num_vl_layers=0).to(dev).train()
    own = enc.layers[0]
    go = torch.from_numpy(LC.PM.dy(LC.PM.rng("layer/drop/" + name).standard_normal(tuple(x["src"].shape)))).to(dev)
    seeds = [_dev(LC.seed_of("layer/site%d" % k), dev) for k in range(3)]

    def fixed_seeds():
        """site k of every forward draws seeds[k]: a checkpoint's recompute, which restores the generator, draws the same again"""
        drawn = []
        return lambda device: (drawn.append(0), seeds[(len(drawn) - 1) % 3])[1]

    calls = _counting(monkeypatch)
    enc.set_own_training(True)                                             # dropout active, own_dropout off: the composition
    monkeypatch.setattr(ext, "bi_attention_seed", fixed_seeds())
    _run(own, x, go)
    assert calls == []
    enc.set_own_training(True, dropout=True)
    monkeypatch.setattr(ext, "bi_attention_seed", fixed_seeds())
    got = _run(own, x, go)
    assert calls == ["DropoutAddLayerNormFunction", "ReluDropoutFunction", "DropoutAddLayerNormFunction"]
    plain, ckpt = _plain_and_checkpointed(own, x, go, before=lambda: monkeypatch.setattr(ext, "bi_attention_seed", fixed_seeds()))
    _bitwise_under_checkpoint(plain, ckpt)

    rows, d_model, d_ffn = x["src"].shape[0] * x["src"].shape[1], x["src"].shape[2], own.linear1.out_features
    widths = (d_model, d_ffn, d_model)
    masks = [ext.row_dropout_keep(seeds[k], p, rows, widths[k]).cpu().double() * float(LC.scale_of(p)) for k in range(3)]
    _, ref, x64 = _golden_layer(name, torch.device("cpu"), p, torch.float64)
    levels = [tuple(int(v) for v in hw) for hw in g["shapes"]]

    class CpuFunction:
        @staticmethod
        def apply(value, shapes, level_start, loc, attn, im2col_step):
            return msda_gridsample(value, levels, loc, attn)

    class MaskDropout(torch.nn.Module):
        def __init__(self, m):
            super().__init__()
            self.m, self.p = m, p                                          # .p: the layer's routing reads it

        def forward(self, t):
            return t * self.m.view(t.shape)

    ref.dropout1, ref.dropout2, ref.dropout3 = (MaskDropout(m) for m in masks)
    monkeypatch.setattr(mod, "MSDeformAttnFunction", CpuFunction)
    want = _run(ref.train(), x64, go.cpu().double())
    for k, what in enumerate(("out", "grad_src", "grad_pos")):
        _close(got[k], want[k], what)
    for n in want[3]:
        _close(got[3][n], want[3][n], n)
