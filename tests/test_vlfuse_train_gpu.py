"""The training route of the bi-directional attention core on the GPU: the C ABI (biattn_hip_train_f32,
biattn_hip_backward_f32) driven with exactly sized, NaN-filled buffers and held per entry to parity_measure.entry_bound against
the float64 restatement of tests/vlfuse_train_cases.py, and the module route (BiMultiHeadAttention.own_training)."""
import os

import numpy as np
import pytest
import torch

import vlfuse_train_cases as VC

pytestmark = pytest.mark.gpu

WORST = {}


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _kind(mask):
    from uninext_amd import _lib
    if mask is None:
        return _lib.BIATTN_MASK_NONE
    return _lib.BIATTN_MASK_INT64 if mask.dtype == np.int64 else _lib.BIATTN_MASK_F32


def run(x, stream=None, inference=False):
    """Drives the C ABI on the case's inputs; returns numpy results and the device inputs (to see them unchanged)."""
    from uninext_amd import _lib
    lib = _lib.load()
    B, H, S, T = x["B"], x["H"], x["S"], x["T"]
    E = H * VC.D
    t = {n: _dev(x[n]) for n in ("q", "k", "vv", "vl", "gv", "gl")}
    mask = _dev(x["mask"])
    mptr = None if mask is None else mask.data_ptr()
    kind = _kind(x["mask"])
    SP, TP = (S + 31) // 32 * 32, (T + 31) // 32 * 32
    out_v, out_l = _nan(B, S, E), _nan(B, T, E)
    stat_v, stat_l = _nan(B * H, 2, SP), _nan(B * H, 2, TP)
    nf = lib.biattn_hip_workspace_bytes(B, H, S, T, VC.D)
    nb = lib.biattn_hip_backward_workspace_bytes(B, H, S, T, VC.D)
    assert nf > 0 and nb > 0
    wf = torch.full((nf,), 0xFF, dtype=torch.uint8, device="cuda")          # NaN patterns
    wb = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda")
    sp = None if stream is None else stream.cuda_stream
    torch.cuda.synchronize()
    rc = lib.biattn_hip_train_f32(t["q"].data_ptr(), t["k"].data_ptr(), t["vv"].data_ptr(), t["vl"].data_ptr(), mptr, kind, B, H, S,
                                  T, VC.D, x["scale"], out_v.data_ptr(), out_l.data_ptr(), stat_v.data_ptr(), stat_l.data_ptr(),
                                  wf.data_ptr(), nf, sp)
    assert rc == 0, _lib.last_error()
    res = {}
    if inference:
        fv, fl = _nan(B, S, E), _nan(B, T, E)
        rc = lib.biattn_hip_forward_f32(t["q"].data_ptr(), t["k"].data_ptr(), t["vv"].data_ptr(), t["vl"].data_ptr(), mptr, kind, B,
                                        H, S, T, VC.D, x["scale"], fv.data_ptr(), fl.data_ptr(), wf.data_ptr(), nf, sp)
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        res.update(fwd_v=fv.cpu().numpy(), fwd_l=fl.cpu().numpy())
    dq, dvv, dk, dvl = _nan(B, S, E), _nan(B, S, E), _nan(B, T, E), _nan(B, T, E)
    rc = lib.biattn_hip_backward_f32(t["q"].data_ptr(), t["k"].data_ptr(), t["vv"].data_ptr(), t["vl"].data_ptr(), mptr, kind,
                                     out_v.data_ptr(), out_l.data_ptr(), stat_v.data_ptr(), stat_l.data_ptr(), t["gv"].data_ptr(),
                                     t["gl"].data_ptr(), B, H, S, T, VC.D, x["scale"], dq.data_ptr(), dk.data_ptr(), dvv.data_ptr(),
                                     dvl.data_ptr(), wb.data_ptr(), nb, sp)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    for n in ("q", "k", "vv", "vl", "gv", "gl"):
        assert np.array_equal(t[n].cpu().numpy().view(np.uint32), x[n].view(np.uint32)), (x["name"], n, "input changed")
    res.update(out_v=out_v, out_l=out_l, stat_v=stat_v, stat_l=stat_l, dq=dq, dk=dk, dvv=dvv, dvl=dvl)
    return {n: (v.cpu().numpy() if torch.is_tensor(v) else v) for n, v in res.items()}


def check_stats(got, x):
    """The kept statistics within parity_measure.entry_bound of the restatement's, with the magnitudes of
    vlfuse_train_cases.core and no composition term (nothing but the derived term); columns past S / T hold 0."""
    want = VC.core(x)
    B, H, S, T = x["B"], x["H"], x["S"], x["T"]
    sv, sl = got["stat_v"].reshape(B, H, 2, -1).astype(np.float64), got["stat_l"].reshape(B, H, 2, -1).astype(np.float64)
    assert not sv[..., S:].any() and not sl[..., T:].any()
    for name, have in (("max_v", sv[:, :, 0, :S]), ("logsum_v", sv[:, :, 1, :S]), ("M", sl[:, :, 0, :T]), ("logL", sl[:, :, 1, :T])):
        VC.PM.errors(have, want[name], want["mag_" + name], np.full(have.shape, np.nan)).check(x["name"], name)


CASES = [(S, T, bh, VC.MASKS[(si + ti + bi) % len(VC.MASKS)])
         for si, S in enumerate(VC.SS) for ti, T in enumerate(VC.TS) for bi, bh in enumerate(VC.BHS)]


@pytest.mark.parametrize("S,T,bh,mask", CASES, ids=["S%d_T%d_%dx%d_%s" % (S, T, bh[0], bh[1], m) for S, T, bh, m in CASES])
def test_sweep(S, T, bh, mask):
    x = VC.make(bh[0], bh[1], S, T, mask)
    got = run(x)
    VC.check(got, x, x["name"], worst=WORST)
    check_stats(got, x)


@pytest.mark.parametrize("mask", VC.MASKS)
def test_every_mask_at_the_tile_edges(mask):
    x = VC.make(2, 3, 129, 65, mask)
    got = run(x)
    VC.check(got, x, x["name"], worst=WORST)


def test_more_tiles_than_ranges_with_an_uneven_split():
    x = VC.make(1, 1, VC.S_UNEVEN, 33, "i64")
    got = run(x)
    VC.check(got, x, x["name"], worst=WORST)


def test_scores_beyond_the_clamp_get_no_gradient_and_leave_the_rest_alone():
    x = VC.make(1, 1, 33, 33, "none", "beyond")
    want = VC.core(x)
    assert want["r"][0, 0, 0, 0] > VC.CLAMP and want["r"][0, 0, -1, -1] < -VC.CLAMP and want["dr"][0, 0, 0, 0] == 0.0
    got = run(x)
    VC.check(got, x, x["name"], worst=WORST)


def test_a_score_of_exactly_50000_passes_the_gradient():
    x = VC.make(1, 1, 33, 33, "none", "equal")
    want = VC.core(x)
    assert want["r"][0, 0, 0, 0] == VC.CLAMP and want["dr"][0, 0, 0, 0] != 0.0
    assert VC.core(x, variant="gate_exclusive")["dr"][0, 0, 0, 0] == 0.0
    got = run(x)
    VC.check(got, x, x["name"], worst=WORST)


def test_a_column_below_the_inner_clamp():
    x = VC.make(1, 1, 33, 33, "none", "inner")
    want = VC.core(x)
    assert (want["e"][0, 0, :, 0] == -VC.CLAMP).all()
    got = run(x)
    VC.check(got, x, x["name"], worst=WORST)


def test_training_forward_is_the_inference_forward_bitwise():
    """Both image-side kernels are one text (biattn_common.hpp's image_fwd); the cases reach its four NJ instantiations
    (T = 256 -> 8, 65 -> 4, 33 -> 2, 32 / 31 / 1 -> 1) and the tails of both sides."""
    for S, T, bh, mask in ((257, 256, (2, 3), "i64"), (129, 33, (1, 1), "f32"), (33, 65, (2, 3), "allmasked"),
                           (33, 32, (1, 1), "none"), (1, 1, (1, 1), "i64"), (128, 31, (2, 3), "f32")):
        x = VC.make(bh[0], bh[1], S, T, mask)
        got = run(x, inference=True)
        assert np.array_equal(got["out_v"].view(np.uint32), got["fwd_v"].view(np.uint32))
        assert np.array_equal(got["out_l"].view(np.uint32), got["fwd_l"].view(np.uint32))


def test_two_runs_and_a_second_stream_give_the_same_bits():
    x = VC.make(2, 3, 257, 129, "f32")
    a, b = run(x), run(x)
    c = run(x, stream=torch.cuda.Stream())
    for n in VC.GRADS + ("out_v", "out_l", "stat_v", "stat_l"):
        assert np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)), n
        assert np.array_equal(a[n].view(np.uint32), c[n].view(np.uint32)), n


def test_rejected_calls_touch_nothing_and_an_empty_batch_returns_0():
    from uninext_amd import _lib
    lib = _lib.load()
    B, H, S, T = 1, 1, 33, 33
    E = H * VC.D
    bufs = [_nan(B, n, E) for n in (S, T, S, T)] + [_nan(B, S, E), _nan(B, T, E), _nan(B * H, 2, 64), _nan(B * H, 2, 64)] + \
           [_nan(B, S, E), _nan(B, T, E)] + [_nan(B, S, E), _nan(B, T, E), _nan(B, S, E), _nan(B, T, E)]
    nb = lib.biattn_hip_backward_workspace_bytes(B, H, S, T, VC.D)
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda")
    p = [t.data_ptr() for t in bufs]

    def call(B=B, H=H, S=S, T=T, D=VC.D, kind=0, nbytes=nb, shift=0):
        return lib.biattn_hip_backward_f32(p[0], p[1], p[2], p[3], None, kind, p[4], p[5], p[6], p[7], p[8], p[9], B, H, S, T, D, 0.0625,
                                           p[10] + shift, p[11], p[12], p[13], ws.data_ptr(), nbytes, None)

    assert call(D=128) == -5 and call(T=257) == -5 and call(S=0) == -2 and call(kind=7) == -5
    assert call(kind=1) == -1                                     # a mask kind without a mask
    assert call(nbytes=nb - 1) == -6 and call(shift=4) == -5
    assert lib.biattn_hip_backward_workspace_bytes(1, 1, 33, 257, VC.D) == 0 and lib.biattn_hip_backward_workspace_bytes(1, 1, 0, 3, VC.D) == 0
    assert call(B=0) == 0
    torch.cuda.synchronize()
    for t in bufs:
        assert bool(torch.isnan(t).all())
    assert bool((ws == 0xFF).all())


def test_rejected_training_forward_calls_touch_nothing_and_an_empty_batch_returns_0():
    from uninext_amd import _lib
    lib = _lib.load()
    B, H, S, T = 1, 1, 33, 33
    E = H * VC.D
    bufs = [_nan(B, n, E) for n in (S, T, S, T)] + [_nan(B, S, E), _nan(B, T, E), _nan(B * H, 2, 64), _nan(B * H, 2, 64)]
    nf = lib.biattn_hip_workspace_bytes(B, H, S, T, VC.D)
    ws = torch.full((nf,), 0xFF, dtype=torch.uint8, device="cuda")
    p = [t.data_ptr() for t in bufs]

    def call(B=B, H=H, S=S, T=T, D=VC.D, kind=0, nbytes=nf, stat_v=p[6], stat_l=p[7]):
        return lib.biattn_hip_train_f32(p[0], p[1], p[2], p[3], None, kind, B, H, S, T, D, 0.0625, p[4], p[5], stat_v, stat_l,
                                        ws.data_ptr(), nbytes, None)

    assert call(D=128) == -5 and call(T=257) == -5 and call(S=0) == -2 and call(H=0) == -2 and call(kind=7) == -5
    assert call(kind=1) == -1                                     # a mask kind without a mask
    assert call(stat_v=None) == -1 and call(stat_l=None) == -1
    assert call(nbytes=nf - 1) == -6
    assert call(B=0) == 0
    torch.cuda.synchronize()
    for t in bufs:
        assert bool(torch.isnan(t).all())
    assert bool((ws == 0xFF).all())


# ---------------------------------------------------------------------------------------------------------------- the module

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vlfuse_train")
FIXTURES = ("t1_nomask", "t37_partial", "t33_nomask", "t256_partial")
# a gradient group: the two inputs, and the parameters of one module together (a projection's weight and bias)
GROUPS = ("visual", "hidden", "layer_norm_v", "layer_norm_l", "gamma_v", "gamma_l", "attn.v_proj", "attn.l_proj",
          "attn.values_v_proj", "attn.values_l_proj", "attn.out_v_proj", "attn.out_l_proj")


def _group_of(name):
    for g in GROUPS:
        if name == g or name.startswith(g + "."):
            return g
    raise AssertionError(name)


@pytest.mark.parametrize("name", FIXTURES)
def test_block_on_the_own_route_matches_the_reference_fixtures(name):
    """BiAttentionBlockForCheckpoint with the flag on against the reference's float64 outputs and gradients
    (tests/golden/make_vlfuse_train_golden.py): per gradient group, max abs error <= C.TOL of the group's max abs."""
    import types
    import decoder_cases as C
    from uninext_amd import _lib
    from uninext_amd.modules import vl_fusion
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    fuse = types.SimpleNamespace(STABLE_SOFTMAX_2D=False, CLAMP_MIN_FOR_UNDERFLOW=True, CLAMP_MAX_FOR_OVERFLOW=True)
    cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(DYHEAD=types.SimpleNamespace(FUSE_CONFIG=fuse)))
    state = {k[len("state."):]: torch.from_numpy(d[k]).float() for k in d.files if k.startswith("state.")}
    heads = int(d["num_heads"])
    block = vl_fusion.BiAttentionBlockForCheckpoint(v_dim=d["visual"].shape[2], l_dim=d["hidden"].shape[2], embed_dim=heads * VC.D,
                                                    num_heads=heads, dropout=0.1, init_values=float(d["init_values"]), cfg=cfg)
    block.load_state_dict(state, strict=True)
    block = block.cuda().eval()                                     # dropout 0.1, inactive: the fixtures' condition
    block.attn.own_training = True
    v = torch.from_numpy(d["visual"]).float().cuda().requires_grad_()
    l = torch.from_numpy(d["hidden"]).float().cuda().requires_grad_()
    mask = torch.from_numpy(d["masks"]).cuda() if "masks" in d.files else None
    entered = []
    orig = vl_fusion.BiAttentionFunction.apply
    vl_fusion.BiAttentionFunction.apply = lambda *a: entered.append(1) or orig(*a)
    try:
        ov, ol = block(v, l, mask)
        ((ov * torch.from_numpy(d["w_visual"]).float().cuda()).sum() + (ol * torch.from_numpy(d["w_hidden"]).float().cuda()).sum()).backward()
    finally:
        vl_fusion.BiAttentionFunction.apply = orig
    assert entered == [1] and "biattn_bwd_image" in _lib.last_kernel("biattn_bwd")
    for key, have in (("out_visual", ov), ("out_hidden", ol)):
        err = np.abs(have.detach().cpu().numpy() - d[key]).max() / np.abs(d[key]).max()
        print(name, key, "%.2e" % err)
        assert err <= C.TOL, (key, err)
    got = {"visual": v.grad, "hidden": l.grad}
    got.update({n: p.grad for n, p in block.named_parameters()})
    assert sorted("grad." + n for n in got) == sorted(k for k in d.files if k.startswith("grad."))
    err, size = dict.fromkeys(GROUPS, 0.0), dict.fromkeys(GROUPS, 0.0)
    for n, t in got.items():
        g, want = _group_of(n), d["grad." + n]
        err[g] = max(err[g], float(np.abs(t.detach().cpu().numpy() - want).max()))
        size[g] = max(size[g], float(np.abs(want).max()))
    for g in GROUPS:
        print(name, g, "%.2e" % (err[g] / size[g]))
        assert size[g] > 0 and err[g] <= C.TOL * size[g], (g, err[g] / size[g])



def _block(dropout=0.0):
    import types
    from uninext_amd.modules.vl_fusion import BiAttentionBlockForCheckpoint
    fuse = types.SimpleNamespace(STABLE_SOFTMAX_2D=False, CLAMP_MIN_FOR_UNDERFLOW=True, CLAMP_MAX_FOR_OVERFLOW=True)
    cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(DYHEAD=types.SimpleNamespace(FUSE_CONFIG=fuse)))
    torch.manual_seed(5)
    return BiAttentionBlockForCheckpoint(v_dim=64, l_dim=48, embed_dim=512, num_heads=2, dropout=dropout, init_values=0.25,
                                         cfg=cfg).cuda()


def _step(block, own, checkpointed=False):
    """One forward + backward of the block; returns outputs and gradients as numpy."""
    import torch.utils.checkpoint as checkpoint
    block.attn.own_training = own
    g = torch.Generator().manual_seed(11)
    v = torch.randn(2, 70, 64, generator=g).cuda().requires_grad_()
    l = torch.randn(2, 9, 48, generator=g).cuda().requires_grad_()
    mask = (torch.arange(9)[None, :] < torch.tensor([9, 5])[:, None]).long().cuda()
    block.zero_grad(set_to_none=True)
    if checkpointed:
        ov, ol = checkpoint.checkpoint(block, v, l, mask, None, use_reentrant=False)
    else:
        ov, ol = block(v, l, mask)
    wv = torch.randn(ov.shape, generator=g).cuda()
    wl = torch.randn(ol.shape, generator=g).cuda()
    ((ov * wv).sum() + (ol * wl).sum()).backward()
    out = {"out_v": ov, "out_l": ol, "grad_v": v.grad, "grad_l": l.grad}
    out.update({"grad." + n: p.grad for n, p in block.named_parameters()})
    return {n: t.detach().cpu().numpy() for n, t in out.items()}


def test_module_route_agrees_with_the_composition_and_checkpointing_gives_the_same_bits():
    import decoder_cases as C
    from uninext_amd import _lib
    block = _block()
    block.train()                                                   # dropout 0: the own route still serves
    ref = _step(block, own=False)
    own = _step(block, own=True)
    assert "biattn_bwd_image" in _lib.last_kernel("biattn_bwd")
    ckpt = _step(block, own=True, checkpointed=True)
    for n in ref:
        scale = max(np.abs(ref[n]).max(), 1e-30)
        assert np.abs(own[n] - ref[n]).max() <= C.TOL * scale, (n, np.abs(own[n] - ref[n]).max() / scale)
        assert np.array_equal(own[n].view(np.uint32), ckpt[n].view(np.uint32)), n
    off = _step(block, own=False)
    for n in ref:
        assert np.array_equal(off[n].view(np.uint32), ref[n].view(np.uint32)), n


def test_train_mode_with_dropout_falls_back_to_the_composition():
    from uninext_amd.modules import vl_fusion
    block = _block(dropout=0.1)
    block.train()
    block.attn.own_training = True
    v = torch.randn(1, 40, 64, device="cuda", requires_grad=True)
    l = torch.randn(1, 5, 48, device="cuda", requires_grad=True)
    assert not block.attn._own_training(block.layer_norm_v(v), block.layer_norm_l(l), None)
    calls = []
    orig = vl_fusion.BiAttentionFunction.apply
    vl_fusion.BiAttentionFunction.apply = lambda *a: calls.append(1) or orig(*a)
    try:
        ov, ol = block(v, l, None)
        (ov.sum() + ol.sum()).backward()
    finally:
        vl_fusion.BiAttentionFunction.apply = orig
    assert not calls
    block.eval()
    assert block.attn._own_training(block.layer_norm_v(v), block.layer_norm_l(l), None)


def test_report_worst_entries():
    """Prints the worst entry per output of the sweep that ran in this process (kernel err, composition err, bound, ratio)."""
    for name in sorted(WORST):
        print("WORST %s" % WORST[name][1])
