"""CPU: every launcher that reports through the library's shared last-error slot (msda::set_error, launch_glue.hpp) answers a
refused call with the code and the exact message it answered before the launchers' host code was gathered into that header.

tests/golden/rejections.json holds the calls and the answers, recorded from a build of the commit before that change by
tests/golden/make_rejections_golden.py; every call in it is refused -- or answered 0 as an empty problem -- before any HIP
runtime call, so no GPU is needed or touched."""
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_rejections_golden as gen  # noqa: E402

CASES = json.load(open(os.path.join(GOLDEN, "rejections.json")))


@pytest.fixture(scope="module")
def lib():
    from uninext_amd import build, _lib
    build.build()
    return _lib.load()


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_rejection_answers_as_recorded(lib, case):
    """One entry point, one refused (or empty) call: the returned code and msda_hip_last_error() are the recorded ones.

    Covered: every entry point of biattn, conv3x3, conv3x3_bwd, convnext, dec_attn, det_post, dynmask, dynmask_bwd, layernorm,
    linear, lsap, matcher_cost, msda_prologue, ota, patch_embed, patch_embed_bwd, qdtrack, query_select, tracker and vit_attn
    that can refuse a call; every message of theirs that is reachable without a HIP runtime call; one case per pointer of
    every 16-byte alignment check (that pointer off by 4 bytes, the others aligned); the empty-problem returns; the 0 that
    track_hip_state_offset / qdtrack_hip_state_offset answer a geometry they refuse (recorded from the commit before the two
    trackers' bank code moved into track_bank.hpp).

    Left out, because they sit behind a HIP runtime call (the LDS opt-in hipFuncSetAttribute, or a launch):
      "convnext_dwconv_ln: cannot reserve LDS", "layernorm_cf: cannot reserve LDS",
      "detpost_nms: cannot reserve the kernel's LDS", "ffn: dynamic LDS opt-in failed",
      and the hipGetErrorString texts of a failed launch or memset (launch_status)."""
    assert case["code"] <= 0      # a recorded HIP error code would mean the call had reached the runtime
    code, message = gen.run(lib, case)
    assert (code, message) == (case["code"], case["message"])


def test_fixture_matches_the_generator_table():
    """The committed calls are the generator's table: a case added there without re-recording, or edited here by hand, shows."""
    assert [(c["id"], c["fn"], c["args"]) for c in CASES] == [(c["id"], c["fn"], c["args"]) for c in gen.all_cases()]
    for fn, names in gen.ALIGNED16.items():
        for name in names:
            assert any(c["id"] == "%s-misaligned-%s" % (fn, name) and "aligned" in c["message"] for c in CASES), (fn, name)
