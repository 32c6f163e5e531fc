"""CPU tests of the encoder layer's training kernels' surface (include/dynmask_hip.h, uninext_amd/csrc/layer_train.hip): the keep
function's layout against a plain-Python Philox, properties of the masks, the float64 restatements of tests/layer_train_cases.py
against torch float64 autograd, that the measure has teeth (wrong variants leave the bound), the binding's rows and exported
symbols, and that the module keeps the composition where the kernels cannot run.  No GPU work."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layer_train_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dropout_add_layernorm_hip_train_f32", "dropout_add_layernorm_hip_backward_workspace_bytes",
               "dropout_add_layernorm_hip_backward_f32", "relu_dropout_hip_f32", "relu_dropout_hip_backward_f32",
               "row_dropout_hip_keep_u8")


def _philox_python(counter, key):
    """Philox4x32-10 in Python integers, written from the paper, not from the numpy port."""
    c, k = list(counter), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


@pytest.mark.parametrize("row,col", [(0, 0), (0, 3), (0, 4), (2, 255), (256, 259), (1030, 4095)])
def test_mask_layout_against_plain_python_philox(row, col):
    seed = LC.seed_of("layer_train/layout")
    sd, off = (int(v) for v in seed.view(np.uint64))
    for p in (0.1, 0.5):
        words = _philox_python((off & 0xFFFFFFFF, off >> 32, row, col // 4), (sd & 0xFFFFFFFF, sd >> 32))
        want = words[col % 4] >= LC.threshold_of(p)
        assert bool(LC.keep_mask(seed, p, row + 1, 4 * (col // 4) + 4)[row, col]) == want


def test_mask_properties():
    seed = LC.seed_of("layer_train/properties")
    assert LC.keep_mask(seed, 0.0, 7, 260).all()
    base = LC.keep_mask(seed, 0.5, 7, 260)
    other_seed, other_offset = seed.copy(), seed.copy()
    other_seed[0] += 1
    other_offset[1] += 1
    assert not np.array_equal(base, LC.keep_mask(other_seed, 0.5, 7, 260))
    assert not np.array_equal(base, LC.keep_mask(other_offset, 0.5, 7, 260))
    assert not np.array_equal(base[0], base[1])
    assert np.array_equal(base[:, :256], LC.keep_mask(seed, 0.5, 7, 256))          # no geometry enters: a prefix is a prefix
    assert np.array_equal(base[:3], LC.keep_mask(seed, 0.5, 3, 260))


def test_kept_share_within_five_sigma():
    n, p = 257 * 1024, 0.1
    kept = int(LC.keep_mask(LC.seed_of("layer_train/share"), p, 257, 1024).sum())
    assert abs(kept - n * (1 - p)) <= 5.0 * np.sqrt(n * p * (1 - p)), kept


SMALL_LN = [c for c in LC.LN_CASES if c[0] * c[1] <= 70000]
SMALL_RELU = [c for c in LC.RELU_CASES if c[0] * c[1] <= 70000]


def _t(a, grad=False):
    return None if a is None else torch.from_numpy(np.asarray(a, dtype=np.float64)).requires_grad_(grad)


@pytest.mark.parametrize("case", SMALL_LN, ids=LC.ln_name)
def test_layernorm_restatement_against_float64_autograd(case):
    x = LC.ln_inputs(case)
    rows, f, p = case[:3]
    keep = LC.keep_mask(x["seed"], p, rows, f)
    mine = LC.ln_forward(x["x"], x["res"], x["gamma"], x["beta"], x["eps"], keep, p)
    xs, res, gamma, beta = _t(x["x"], True), _t(x["res"], True), _t(x["gamma"], True), _t(x["beta"], True)
    cm = torch.from_numpy(keep.astype(np.float64) * float(LC.scale_of(p)))
    z = cm * xs if res is None else res + cm * xs
    out = F.layer_norm(z, (f,), gamma, beta, x["eps"])
    assert np.abs(mine["z"] - z.detach().numpy()).max() <= 1e-12
    assert np.abs(mine["out"] - out.detach().numpy()).max() <= 1e-11
    # the backward restates from a GIVEN z: differentiate LayerNorm at z, then chain through z = res + c m x by hand
    zl = z.detach().clone().requires_grad_(True)
    F.layer_norm(zl, (f,), gamma, beta, x["eps"]).backward(_t(x["go"]))
    back = LC.ln_backward(x["go"], z.detach().numpy(), x["gamma"], x["eps"], keep, p)
    scale = max(1.0, float(np.abs(back["gres"]).max()))
    assert np.abs(back["gres"] - zl.grad.numpy()).max() <= 1e-11 * scale
    assert np.abs(back["gx"] - (cm * zl.grad).numpy()).max() <= 1e-11 * scale
    if gamma is not None:
        assert np.abs(back["ggamma"] - gamma.grad.numpy()).max() <= 1e-10 * max(1.0, float(np.abs(back["ggamma"]).max()))
        assert np.abs(back["gbeta"] - beta.grad.numpy()).max() <= 1e-10 * max(1.0, float(np.abs(back["gbeta"]).max()))


@pytest.mark.parametrize("case", SMALL_RELU, ids=LC.relu_name)
def test_relu_dropout_restatement_against_float64_autograd(case):
    x = LC.relu_inputs(case)
    rows, f, p = case
    keep = LC.keep_mask(x["seed"], p, rows, f)
    h = _t(x["h"], True)
    out = torch.from_numpy(keep.astype(np.float64) * float(LC.scale_of(p))) * torch.relu(h)
    out.backward(_t(x["go"]))
    mine = LC.relu_forward(x["h"], keep, p)
    assert np.array_equal(mine["out"], out.detach().numpy())
    assert np.array_equal(LC.relu_backward(x["go"], mine["out"], p)["gh"], h.grad.numpy())


def _ln_case_terms(case):
    x = LC.ln_inputs(case)
    rows, f, p = case[:3]
    keep = LC.keep_mask(x["seed"], p, rows, f)
    z = LC.ln_forward(x["x"], x["res"], x["gamma"], x["beta"], x["eps"], keep, p, np.float32)["z"]
    args = (x["go"], z, x["gamma"], x["eps"], keep, p)
    return args, LC.ln_backward(*args), LC.ln_backward(*args, dt=np.float32)


def test_composition_is_inside_its_own_bound_and_wrong_variants_leave_it():
    case = (257, 256, 0.1, True, True)
    args, want, comp = _ln_case_terms(case)
    assert LC.passes(comp, want, comp, LC.LN_GRADS)
    for variant in LC.LN_VARIANTS:
        wrong = LC.ln_backward(*args, variant=variant)
        assert not LC.passes(wrong, want, comp, LC.LN_GRADS), variant
    x = LC.relu_inputs((5, 252, 0.5))
    keep = LC.keep_mask(x["seed"], 0.5, 5, 252)
    out = LC.relu_forward(x["h"], keep, 0.5)["out"]
    want, comp = LC.relu_backward(x["go"], out, 0.5), LC.relu_backward(x["go"], out, 0.5, np.float32)
    assert LC.passes(comp, want, comp, ("gh",))
    assert not LC.passes(LC.relu_backward(x["go"], out, 0.5, variant="gate_from_grad_out"), want, comp, ("gh",))


def test_forward_without_the_mask_leaves_the_bound():
    case = (5, 252, 0.1, False, True)
    x = LC.ln_inputs(case)
    keep = LC.keep_mask(x["seed"], 0.1, 5, 252)
    f = lambda k, dt: LC.ln_forward(x["x"], x["res"], x["gamma"], x["beta"], x["eps"], k, 0.1, dt)
    want, comp = f(keep, np.float64), f(keep, np.float32)
    assert LC.passes(comp, want, comp, LC.LN_OUTPUTS)
    assert not LC.passes(f(np.ones_like(keep), np.float64), want, comp, LC.LN_OUTPUTS)


def test_binding_rows():
    from uninext_amd import _lib
    i, p, f, z, ll = ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_size_t, ctypes.c_longlong
    rows = _lib._SIGNATURES["dynmask_hip.h"]          # declared there: layernorm_hip.h's prototypes are the add_layernorm family alone
    assert set(NEW_SYMBOLS) <= set(rows) and set(NEW_SYMBOLS) <= set(_lib.DYNMASK_EXPORTS)
    assert rows["dropout_add_layernorm_hip_train_f32"] == (i, [p, p, p, p, f, ll, i, f, p, p, p, p])
    assert rows["dropout_add_layernorm_hip_backward_workspace_bytes"] == (z, [ll, i])
    assert rows["dropout_add_layernorm_hip_backward_f32"] == (i, [p, p, p, f, ll, i, f, p, p, p, p, p, p, z, p])
    assert rows["relu_dropout_hip_f32"] == (i, [p, ll, i, f, p, p, p])
    assert rows["relu_dropout_hip_backward_f32"] == (i, [p, p, ll, i, f, p, p])
    assert rows["row_dropout_hip_keep_u8"] == (i, [p, f, ll, i, p, p])
    assert _lib._SIGNATURES["layernorm_hip.h"] == {"add_layernorm_hip_f32": (i, [p, p, p, p, f, ll, i, p, p])}      # unchanged


def test_library_exports_the_symbols_and_refuses_without_a_gpu():
    from uninext_amd import _lib
    lib = _lib.load()
    for sym in NEW_SYMBOLS:
        assert hasattr(lib, sym), sym
    one = 16
    train, bwd = lib.dropout_add_layernorm_hip_train_f32, lib.dropout_add_layernorm_hip_backward_f32
    assert train(one, None, None, None, 1e-5, 10, 6, 0.0, None, one, one, None) == _lib.LAYERNORM_ERR_UNSUPPORTED
    assert train(one, None, None, None, 1e-5, 10, 4100, 0.0, None, one, one, None) == _lib.LAYERNORM_ERR_UNSUPPORTED
    assert train(one, None, None, None, 1e-5, 10, 256, 1.0, one, one, one, None) == _lib.LAYERNORM_ERR_BAD_DIMS
    assert train(one, None, None, None, 1e-5, 10, 256, -0.1, one, one, one, None) == _lib.LAYERNORM_ERR_BAD_DIMS
    assert train(one, None, None, None, 1e-5, 10, 256, 0.1, None, one, one, None) == _lib.LAYERNORM_ERR_NULL_POINTER
    assert "seed" in _lib.last_error()
    assert train(one, None, None, None, 1e-5, 10, 256, 0.0, None, None, one, None) == _lib.LAYERNORM_ERR_NULL_POINTER
    assert train(one, None, None, None, 1e-5, 1 << 32, 256, 0.0, None, one, one, None) == _lib.LAYERNORM_ERR_BAD_DIMS
    assert train(None, None, None, None, 1e-5, 0, 256, 0.0, None, None, None, None) == 0
    need = lib.dropout_add_layernorm_hip_backward_workspace_bytes(1031, 256)
    assert need == 33 * 2 * 256 * 8 and lib.dropout_add_layernorm_hip_backward_workspace_bytes(0, 256) == 0
    assert bwd(one, one, None, 1e-5, 1031, 256, 0.0, None, one, one, one, one, one, need - 1, None) == _lib.LAYERNORM_ERR_WORKSPACE
    assert bwd(one, one, None, 1e-5, 1031, 256, 0.0, None, one, one, one, one, None, need, None) == _lib.LAYERNORM_ERR_NULL_POINTER
    assert bwd(None, one, None, 1e-5, 10, 256, 0.0, None, one, one, None, None, None, 0, None) == _lib.LAYERNORM_ERR_NULL_POINTER
    assert bwd(one, one, None, 1e-5, 10, 258, 0.0, None, one, one, None, None, None, 0, None) == _lib.LAYERNORM_ERR_UNSUPPORTED
    assert bwd(None, None, None, 1e-5, 0, 256, 0.0, None, None, None, None, None, None, 0, None) == 0
    assert lib.relu_dropout_hip_f32(one, 10, 65540, 0.0, None, one, None) == _lib.LAYERNORM_ERR_UNSUPPORTED
    assert lib.relu_dropout_hip_f32(one, 10, 2048, 0.5, None, one, None) == _lib.LAYERNORM_ERR_NULL_POINTER
    assert lib.relu_dropout_hip_f32(None, 0, 2048, 0.5, one, None, None) == 0
    assert lib.relu_dropout_hip_backward_f32(one, None, 10, 2048, 0.5, one, None) == _lib.LAYERNORM_ERR_NULL_POINTER
    assert lib.relu_dropout_hip_backward_f32(one, one, 10, 2046, 0.5, one, None) == _lib.LAYERNORM_ERR_UNSUPPORTED
    assert lib.row_dropout_hip_keep_u8(None, 0.5, 10, 256, one, None) == _lib.LAYERNORM_ERR_NULL_POINTER
    assert lib.row_dropout_hip_keep_u8(one, 1.5, 10, 256, one, None) == _lib.LAYERNORM_ERR_BAD_DIMS


def test_functions_are_exported():
    from uninext_amd import functions
    from uninext_amd.functions.layer_train import DropoutAddLayerNormFunction, ReluDropoutFunction
    assert functions.DropoutAddLayerNormFunction is DropoutAddLayerNormFunction
    assert functions.ReluDropoutFunction is ReluDropoutFunction


def test_cpu_float64_module_keeps_the_composition_with_either_flag(monkeypatch):
    """On the CPU and in float64 no kernel can run: with either flag set the layer is the composition, bit for bit, and its
    state-dict keys are the reference's."""
    from golden_util import enclayer_names, load_golden
    from oracle.msda_gridsample import msda_gridsample
    from uninext_amd.functions import layer_train
    from uninext_amd.modules import DeformableTransformerEncoderLayer, DeformableTransformerEncoderVL
    from uninext_amd.modules import ms_deform_attn as mod
    assert DeformableTransformerEncoderLayer.own_training is False and DeformableTransformerEncoderLayer.own_dropout is False
    g = load_golden(enclayer_names()[0])
    params = {k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p:")}
    d_model, d_ffn = params["linear1.weight"].shape[1], params["linear1.weight"].shape[0]
    layer = DeformableTransformerEncoderLayer(d_model=d_model, d_ffn=d_ffn, dropout=0.0, n_heads=d_model // 32).double()
    assert sorted(layer.state_dict()) == sorted(params)
    layer.load_state_dict(params)
    enc = DeformableTransformerEncoderVL(torch.nn.Identity(), layer, torch.nn.Identity(), 2, num_vl_layers=0)
    assert enc.set_own_training(True, dropout=True) is enc
    assert all(lyr.own_training and lyr.own_dropout for lyr in enc.layers)
    enc.set_own_training(True)
    assert all(lyr.own_training and not lyr.own_dropout for lyr in enc.layers)
    enc.set_own_training(False, dropout=True)
    assert not any(lyr.own_training or lyr.own_dropout for lyr in enc.layers)
    assert sorted(enc.layers[0].state_dict()) == sorted(params)
    levels = [tuple(int(v) for v in hw) for hw in g["shapes"]]

    class CpuFunction:
        @staticmethod
        def apply(value, shapes, level_start, loc, attn, im2col_step):
            return msda_gridsample(value, levels, loc, attn)

    def no_kernel(*args):
        raise AssertionError("the HIP function was called on the CPU")

    monkeypatch.setattr(mod, "MSDeformAttnFunction", CpuFunction)
    monkeypatch.setattr(layer_train.DropoutAddLayerNormFunction, "apply", staticmethod(no_kernel))
    monkeypatch.setattr(layer_train.ReluDropoutFunction, "apply", staticmethod(no_kernel))
    args = [torch.from_numpy(g[k]) for k in ("pos", "ref", "shapes", "lsi")]
    mask = torch.from_numpy(g["mask"]) if "mask" in g else None
    outs = []
    for own, drop in ((False, False), (True, False), (True, True)):
        layer.own_training, layer.own_dropout = own, drop
        src = torch.from_numpy(g["src"]).clone().requires_grad_(True)
        out = layer.train()(src, *args, mask)
        out.sum().backward()
        outs.append((out.detach(), src.grad))
    for out, grad in outs[1:]:
        assert torch.equal(out, outs[0][0]) and torch.equal(grad, outs[0][1])
