"""CPU: registers and scratch of the contract kernels, as the compiler reports them for gfx950 (tools/kernel_resources.py).

These kernels live at occupancy limits chosen on purpose (msda_fwd_lg3: 64 VGPRs = 8 waves per SIMD, msda_fwd_win2: 80 = 6,
msda_fwd_win: 128 = 4, the one-workgroup-per-CU kernels: 168 = 3), and a change that costs a few more live values does not
fail -- it spills, and the spill sits on the critical path of every work item (round 3: three registers too many in
msda_fwd_lg3 cost 13 % of its time and 20 % more HBM traffic before the evidence pass caught it).  The numbers here are upper
bounds on what the shipped sources compile to; raise one only with the measurement that justifies it."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "uninext_amd", "csrc")

# file -> {kernel: (max VGPRs, max scratch bytes per lane)}
LIMITS = {
    # msda_fwd_fused<REFD>: the users of lane_ops.hpp's group_max / group_sum, at what they compiled to before that header existed
    "msda_fwd.hip": {"msda::msda_fwd_lg3<0>": (64, 0), "msda::msda_fwd_lanegroup<8, 16>": (64, 0),
                     "msda::msda_fwd_fused<2>": (64, 0), "msda::msda_fwd_fused<4>": (64, 0)},
    "msda_fwd_win.hip": {"msda::msda_fwd_win<0, false>": (128, 8), "msda::msda_fwd_win<0, true>": (128, 8)},
    "experiments/msda_fwd_win2.hip": {"msda::msda_fwd_win2": (80, 0)},
    "experiments/msda_fwd_win3.hip": {"msda::msda_fwd_win3": (168, 0)},
    "msda_bwd_win.hip": {"msda::msda_bwd_win": (168, 0)},
    "msda_bwd_tiled.hip": {"msda::msda_bwd_tiled": (168, 0)},
    # msda_bwd_lanegroup<8, 16> (lane_ops.hpp's group_sum<G>) spilled 44 registers into 180 B of scratch before the header existed,
    # and is pinned there: the bound keeps the refactor honest, it does not call the spill good
    "msda_bwd.hip": {"msda::msda_bwd_generic<float, 1>": (96, 0), "msda::msda_bwd_lanegroup<8, 16>": (128, 180)},
    "msda_bwd_q.hip": {"msda::msda_bwd_q": (64, 0)},
    # round 4: the lane-parallel prefetch of a pair's inputs keeps 9 values in scratch across the query loop's head; measured WITH
    # them: 80 us against 88 for the version without (profiles/r04_backward_decoder.txt)
    "msda_bwd_dec.hip": {"msda::msda_bwd_dec": (128, 36)},
    # round 6: two 512-thread workgroups per CU = 4 waves per SIMD; the loads of 5 scan steps / 5 record pairs travel together
    "msda_bwd_dst.hip": {"msda::msda_bwd_dst": (128, 0)},
    # the LayerNorm-epilogue kernels of linear.hip (lane_ops.hpp's group_sum<32> over a half-wave): what they compiled to when the
    # shared header was introduced.  ffn_packed<true, 8> is 8 registers short of the whole file
    "linear.hip": {"linear::linear_packed<4, 64, false, 1, true>": (236, 0), "linear::ffn_packed<true, 8>": (248, 0),
                   "linear::ffn_packed<true, 4>": (234, 0)},
    # the streamed-attention cores (attn_tile.hpp): what they compiled to when the shared header was introduced.  biattn_text and
    # biattn_image<8> use the whole register file; one more live value there is a spill.  biattn_image<NJ> is a thin kernel around
    # biattn_common.hpp's image_fwd<NJ, false>, so these are also the bounds of the text it shares with biattn_bwd::image_train
    "biattn.hip": {"biattn::biattn_text": (256, 0), "biattn::biattn_image<1>": (180, 0), "biattn::biattn_image<2>": (202, 0),
                   "biattn::biattn_image<4>": (234, 0), "biattn::biattn_image<8>": (256, 0)},
    "vit_attn.hip": {"vit_attn::attn<64, false>": (177, 0), "vit_attn::attn<64, true>": (180, 0),
                     "vit_attn::attn<80, false>": (164, 0), "vit_attn::attn<80, true>": (186, 0)},
    "dec_attn.hip": {"dec_attn::attn<0>": (123, 0), "dec_attn::attn<2>": (130, 0), "dec_attn::attn<3>": (130, 0)},
    # the attention training kernels (attn_bwd_tile.hpp, dec_attn_launch.hpp, the device pieces of vit_attn_launch.hpp): what they
    # compiled to when the shared headers were introduced.  vit_attn_bwd::bwd_kv<80, *> uses the whole register file
    "vit_attn_bwd.hip": {"vit_attn_bwd::attn_lse<64, false>": (178, 0), "vit_attn_bwd::attn_lse<64, true>": (181, 0),
                         "vit_attn_bwd::attn_lse<80, false>": (165, 0), "vit_attn_bwd::attn_lse<80, true>": (187, 0),
                         "vit_attn_bwd::bwd_q<64, false>": (150, 0), "vit_attn_bwd::bwd_q<64, true>": (196, 0),
                         "vit_attn_bwd::bwd_q<80, false>": (201, 0), "vit_attn_bwd::bwd_q<80, true>": (247, 0),
                         "vit_attn_bwd::bwd_kv<64, false>": (242, 0), "vit_attn_bwd::bwd_kv<64, true>": (254, 0),
                         "vit_attn_bwd::bwd_kv<80, false>": (256, 0), "vit_attn_bwd::bwd_kv<80, true>": (256, 0)},
    "dec_attn_bwd.hip": {"dec_attn_bwd::attn_lse<0>": (123, 0), "dec_attn_bwd::attn_lse<2>": (130, 0),
                         "dec_attn_bwd::attn_lse<3>": (130, 0), "dec_attn_bwd::bwd_q<0>": (122, 0),
                         "dec_attn_bwd::bwd_q<2>": (140, 0), "dec_attn_bwd::bwd_q<3>": (140, 0),
                         "dec_attn_bwd::bwd_kv<0>": (160, 0), "dec_attn_bwd::bwd_kv<2>": (162, 0),
                         "dec_attn_bwd::bwd_kv<3>": (164, 0)},
}


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
@pytest.mark.parametrize("name", sorted(LIMITS))
def test_contract_kernels_fit_their_register_budgets(name):
    import kernel_resources
    got = kernel_resources.resources(os.path.join(CSRC, name))
    for kernel, (max_vgprs, max_scratch) in LIMITS[name].items():
        assert kernel in got, (kernel, sorted(got))
        r = got[kernel]
        print("%-40s vgprs %d scratch %d B/lane occupancy %d" % (kernel, r["vgprs"], r["scratch"], r["occupancy"]))
        assert r["vgprs"] <= max_vgprs, (kernel, r)
        assert r["scratch"] <= max_scratch, (kernel, r)
