"""Registers and scratch of the kernels of uninext_amd/csrc/biattn_bwd.hip, in the style of tests/test_kernel_resources_cpu.py:
what they compiled to when the file was written.  No kernel of the file may use scratch: the image-owner and text-owner passes
live at one wave per SIMD, and a spill there is traffic on the MFMA chain."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

# (VGPRs at most, scratch bytes per lane)
PINNED = {
    "biattn_bwd::image_train<1>": (184, 0), "biattn_bwd::image_train<2>": (202, 0), "biattn_bwd::image_train<4>": (235, 0),
    "biattn_bwd::image_train<8>": (256, 0),
    "biattn_bwd::text_stats": (19, 0), "biattn_bwd::row_dots": (18, 0), "biattn_bwd::bwd_combine": (17, 0),
    "biattn_bwd::bwd_image<false>": (256, 0), "biattn_bwd::bwd_image<true>": (204, 0),
    "biattn_bwd::bwd_text<0>": (256, 0), "biattn_bwd::bwd_text<1>": (256, 0), "biattn_bwd::bwd_text<2>": (256, 0),
}


@pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None, reason="needs hipcc")
def test_biattn_bwd_kernels_keep_their_registers_and_use_no_scratch():
    got = kernel_resources.resources(os.path.join(ROOT, "uninext_amd", "csrc", "biattn_bwd.hip"))
    assert set(PINNED) <= set(got), sorted(set(PINNED) - set(got))
    for name, r in got.items():
        assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0, (name, r)
    for name, (vgprs, scratch) in PINNED.items():
        assert got[name]["vgprs"] <= vgprs and got[name]["scratch"] == scratch, (name, got[name])
