"""The reference's config entry points and its encoder layer, against this repository (BASELINE.json north_star: "... the
detectron2 META_ARCH_REGISTRY/config entry points so projects/UNINEXT configs load unchanged").

What the reference's own code makes is stored under tests/golden/reference_glue/ (tests/golden/make_reference_glue_golden.py
runs the reference's detectron2.config, uninext/config.py and deformable_transformer_dino.py to mint it):

  1. configs.json: `detectron2.config.get_cfg()` + `uninext/config.py::add_uninext_config` + `merge_from_file` of
     projects/UNINEXT/configs/image_joint_r50.yaml and obj365v2_32g_r50.yaml -- the meta-architecture, the matcher, and
     the geometry the HIP path is specialised for, which this repository's defaults must equal;
  2. enclayer_d512.npz: the `DeformableTransformerEncoderLayer` the reference's transformer builds
     (deformable_transformer_dino.py:330-370, self_attn = MSDeformAttn(...) at :338) in float64 -- its output on
     parameters and inputs that tests/golden/make_reference_glue_golden.py::enclayer_case draws from a seed -- which the
     mirror in uninext_amd.modules, on the C ABI of libmsda_hip.so (host-pointer variants here), reproduces from the same
     state_dict.
"""
import importlib.util
import inspect
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLUE = os.path.join(ROOT, "tests", "golden", "reference_glue")


@pytest.mark.parametrize("yaml_name", ["image_joint_r50.yaml", "obj365v2_32g_r50.yaml"])
def test_projects_uninext_configs_load_unchanged(yaml_name):
    with open(os.path.join(GLUE, "configs.json")) as f:
        cfg = json.load(f)[yaml_name]
    assert cfg["MODEL.META_ARCHITECTURE"] == "UNINEXT_IMG"
    dd = cfg["MODEL.DDETRS"]
    assert dd["NUM_OBJECT_QUERIES"] == 900 and cfg["MODEL.OTA"] is True
    # the geometry the HIP path is specialised for (d_model 256, 8 heads, 4 levels, 4 points, 6 + 6 layers)
    assert (dd["HIDDEN_DIM"], dd["NHEADS"], dd["NUM_FEATURE_LEVELS"], dd["ENC_N_POINTS"], dd["DEC_N_POINTS"], dd["ENC_LAYERS"],
            dd["DEC_LAYERS"]) == (256, 8, 4, 4, 4, 6, 6)
    assert cfg["frozen_refuses_assignment"] is True                            # frozen, like any detectron2 config
    # ... and it is this repository's geometry
    import bench
    from uninext_amd import workloads
    from uninext_amd.modules import DeformableTransformerEncoderLayer, MSDeformAttn
    assert (workloads.HEADS * workloads.HEAD_DIM, workloads.HEADS, len(workloads.R50_LEVELS_INFER), workloads.POINTS) == \
        (dd["HIDDEN_DIM"], dd["NHEADS"], dd["NUM_FEATURE_LEVELS"], dd["ENC_N_POINTS"])
    assert workloads.WORKLOADS["r50_infer_decoder"]["num_query"] == dd["NUM_OBJECT_QUERIES"]
    assert (bench.ENC_LAYERS, bench.DEC_LAYERS) == (dd["ENC_LAYERS"], dd["DEC_LAYERS"])
    defaults = {k: v.default for k, v in inspect.signature(MSDeformAttn.__init__).parameters.items()}
    assert (defaults["d_model"], defaults["n_levels"], defaults["n_heads"], defaults["n_points"]) == \
        (dd["HIDDEN_DIM"], dd["NUM_FEATURE_LEVELS"], dd["NHEADS"], dd["DEC_N_POINTS"])
    defaults = {k: v.default for k, v in inspect.signature(DeformableTransformerEncoderLayer.__init__).parameters.items()}
    assert (defaults["d_model"], defaults["n_levels"], defaults["n_heads"], defaults["n_points"]) == \
        (dd["HIDDEN_DIM"], dd["NUM_FEATURE_LEVELS"], dd["NHEADS"], dd["ENC_N_POINTS"])


def test_transformer_layer_runs_on_this_repositorys_module():
    """deformable_transformer_dino.py:330-370 (stored in float64) against uninext_amd.modules with the same state_dict."""
    from uninext_amd.modules import DeformableTransformerEncoderLayer
    spec = importlib.util.spec_from_file_location(
        "make_reference_glue_golden", os.path.join(ROOT, "tests", "golden", "make_reference_glue_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    c = gen.enclayer_case(torch.float32)                   # the seeded parameters and inputs the fixture was minted on
    with np.load(os.path.join(GLUE, "enclayer_d512.npz")) as z:
        want, digest = torch.from_numpy(z["out"]), float(z["digest"])
    assert abs(c["digest"] - digest) < 1e-9 * digest, "parameter generator drifted from the fixture"
    ours = DeformableTransformerEncoderLayer(d_model=256, d_ffn=512, dropout=0.0, n_heads=8).eval()
    assert set(c["params"]) == set(ours.state_dict())
    ours.load_state_dict(c["params"])                                             # same parameter names
    b = ours(c["src"], c["pos"], c["ref"], c["shapes"], c["lsi"], c["mask"])
    assert (want - b).abs().max().item() < 1e-5
