"""The reference's own Python layers on top of this repository's drop-in module, checked against what the reference computes.

The reference's ops/functions/ms_deform_attn_func.py does `import MultiScaleDeformableAttention as MSDA` (:18) and calls
`MSDA.ms_deform_attn_forward / ms_deform_attn_backward`; with this repository on sys.path that import resolves to
./MultiScaleDeformableAttention.py, i.e. to uninext_amd.ext and the C ABI.  CPU tensors are served by the host-pointer
variants (msda_host_*).  What the reference computes is stored under tests/golden/reference_glue/
(tests/golden/make_reference_glue_golden.py runs the reference's own files to mint it): the names the reference binds,
ops/test.py's inputs with `ms_deform_attn_core_pytorch`'s output, and the reference's `MSDeformAttn` in float64 -- its
outputs and gradients on parameters and inputs that the fixture's generator draws from a seed and the test draws again."""
import importlib
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLUE = os.path.join(ROOT, "tests", "golden", "reference_glue")


def _npz(name):
    with np.load(os.path.join(GLUE, name)) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


def test_reference_function_binds_to_this_library():
    with open(os.path.join(GLUE, "binding.json")) as f:
        binding = json.load(f)
    from uninext_amd import ext
    msda = importlib.import_module(binding["module"])                 # what ms_deform_attn_func.py:18 imports as MSDA
    assert msda.__name__ == "MultiScaleDeformableAttention"
    assert os.path.dirname(os.path.abspath(msda.__file__)) == ROOT     # this repository's drop-in, not a compiled extension
    assert sorted(binding["functions"]) == ["ms_deform_attn_backward", "ms_deform_attn_forward"]
    assert msda.ms_deform_attn_forward is ext.ms_deform_attn_forward
    assert msda.ms_deform_attn_backward is ext.ms_deform_attn_backward


def test_reference_function_forward_equals_its_pytorch_path():
    """check_forward_equal_with_pytorch_double / _float (ops/test.py:31-57): the Function against the stored output of the
    reference's `ms_deform_attn_core_pytorch` on the same inputs."""
    from uninext_amd.functions import MSDeformAttnFunction
    g = _npz("testpy.npz")
    for tag, tol in (("f64", 1e-12), ("f32", 1e-6)):
        want = g["want_" + tag]
        got = MSDeformAttnFunction.apply(g["value_" + tag], g["shapes"], g["lsi"], g["loc_" + tag], g["attn_" + tag], 2)
        assert got.dtype == want.dtype
        assert torch.allclose(got, want, rtol=1e-2, atol=1e-3)          # the reference's own criterion
        assert (got - want).abs().max().item() < tol


def test_reference_function_gradcheck():
    """check_gradient_numerical (ops/test.py:60-76), channels 30 and 32."""
    from uninext_amd.functions import MSDeformAttnFunction
    for D in (30, 32):
        N, M, Lq, L, P = 1, 2, 2, 2, 2
        shapes = torch.as_tensor([(6, 4), (3, 2)], dtype=torch.long)
        lsi = torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))
        S = int(shapes.prod(1).sum())
        torch.manual_seed(3)
        value = (torch.rand(N, S, M, D, dtype=torch.float64) * 0.01).requires_grad_(True)
        loc = torch.rand(N, Lq, M, L, P, 2, dtype=torch.float64).requires_grad_(True)
        attn = torch.rand(N, Lq, M, L, P, dtype=torch.float64) + 1e-5
        attn = (attn / attn.sum(-1, keepdim=True).sum(-2, keepdim=True)).requires_grad_(True)
        assert torch.autograd.gradcheck(MSDeformAttnFunction.apply, (value, shapes, lsi, loc, attn, 2))


def _recipes():
    """tests/golden/make_reference_glue_golden.py: the seeded parameter and input draws the fixtures were minted on."""
    spec = importlib.util.spec_from_file_location(
        "make_reference_glue_golden", os.path.join(ROOT, "tests", "golden", "make_reference_glue_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_reference_module_runs_on_this_library_and_matches_the_mirror():
    """The class the reference's transformer constructs (deformable_transformer_dino.py:338,380): uninext_amd.modules.MSDeformAttn
    takes its state_dict and reproduces its outputs and gradients (stored: the reference module in float64).  Every weight
    gradient is compared element by element with the reference's dW = dy^T x, rebuilt from the stored factors."""
    from uninext_amd.modules import MSDeformAttn
    gen = _recipes()
    c = gen.module_case(torch.float32)
    g = _npz("module.npz")
    assert abs(c["digest"] - float(g["digest"])) < 1e-9 * float(g["digest"]), "parameter generator drifted from the fixture"
    ours = MSDeformAttn(256, 4, 8, 4)
    assert set(c["params"]) == set(ours.state_dict())
    ours.load_state_dict(c["params"])                       # reference checkpoints load unchanged
    src, refpts, shapes, lsi, mask = c["src"], c["refpts"], c["shapes"], c["lsi"], c["mask"]
    qb = src.clone().requires_grad_(True)
    b = ours(qb, refpts, src, shapes, lsi, mask)
    assert (g["out"] - b).abs().max().item() < 1e-5
    b.sum().backward()
    want_q = g["grad_query"]
    assert (want_q - qb.grad).abs().max().item() < 1e-4 * max(1.0, want_q.abs().max().item())
    inputs = {"sampling_offsets": src, "attention_weights": src, "value_proj": src, "output_proj": g["x:output_proj"]}
    checked = set()
    for name, x in inputs.items():
        dy = g["dy:" + name].double()
        dy, x = dy.reshape(-1, dy.shape[-1]), x.double().reshape(-1, x.shape[-1])
        lin = getattr(ours, name)
        for pname, p, r in ((name + ".weight", lin.weight, dy.t() @ x), (name + ".bias", lin.bias, dy.sum(0))):
            assert (p.grad.double() - r).abs().max().item() < 1e-4 * max(1.0, r.abs().max().item()), pname
            checked.add(pname)
    assert checked == {n for n, _ in ours.named_parameters()}
    # decoder form: 4-d reference boxes
    assert (g["out4"] - ours(c["query4"], c["ref4"], src, shapes, lsi, None)).abs().max().item() < 1e-5
    with pytest.raises(ValueError):
        ours(c["query4"], torch.rand(2, 11, 4, 3), src, shapes, lsi, None)
