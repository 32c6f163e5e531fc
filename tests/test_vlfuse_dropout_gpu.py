"""The attention dropout inside the bi-directional attention core on the GPU: the keep decisions written out by
biattn_hip_dropout_keep_u8 against the numpy masks of tests/vlfuse_dropout_cases.py byte for byte, the C ABI
(biattn_hip_train_dropout_f32, biattn_hip_backward_dropout_f32) driven with exactly sized, NaN-filled buffers and held per entry
to parity_measure.entry_bound against the float64 restatement under the same masks, the bitwise facts the header states, the
refusals, and the module route (BiMultiHeadAttention.own_dropout).  One process, no tools."""
import types

import numpy as np
import pytest
import torch

import test_vlfuse_train_gpu as TG
import vlfuse_dropout_cases as DC
import vlfuse_train_cases as VC

pytestmark = pytest.mark.gpu

WORST = {}
NAMES = DC.OUTPUTS + ("stat_v", "stat_l")


def _seed(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def export(seed, p, B, H, S, T):
    from uninext_amd import _lib
    lib = _lib.load()
    sd = _seed(seed)
    kv = torch.full((B * H, S, T), 0xFF, dtype=torch.uint8, device="cuda")
    kl = torch.full((B * H, T, S), 0xFF, dtype=torch.uint8, device="cuda")
    rc = lib.biattn_hip_dropout_keep_u8(sd.data_ptr(), p, B, H, S, T, kv.data_ptr(), kl.data_ptr(), None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return kv.cpu().numpy(), kl.cpu().numpy()


def run(x, p, seed, stream=None, dropout=True):
    """Drives the C ABI on the case's inputs -- the entry points with dropout, or (dropout=False) those without -- and returns
    numpy results; the inputs and the seed are seen unchanged."""
    from uninext_amd import _lib
    lib = _lib.load()
    B, H, S, T = x["B"], x["H"], x["S"], x["T"]
    E = H * VC.D
    t = {n: TG._dev(x[n]) for n in ("q", "k", "vv", "vl", "gv", "gl")}
    mask = TG._dev(x["mask"])
    mptr = None if mask is None else mask.data_ptr()
    kind = TG._kind(x["mask"])
    sd = _seed(seed)
    SP, TP = (S + 31) // 32 * 32, (T + 31) // 32 * 32
    out_v, out_l = TG._nan(B, S, E), TG._nan(B, T, E)
    stat_v, stat_l = TG._nan(B * H, 2, SP), TG._nan(B * H, 2, TP)
    nf = lib.biattn_hip_workspace_bytes(B, H, S, T, VC.D)
    nb = lib.biattn_hip_backward_workspace_bytes(B, H, S, T, VC.D)
    assert nf > 0 and nb > 0
    wf = torch.full((nf,), 0xFF, dtype=torch.uint8, device="cuda")
    wb = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda")
    sp = None if stream is None else stream.cuda_stream
    torch.cuda.synchronize()
    fwd = (t["q"].data_ptr(), t["k"].data_ptr(), t["vv"].data_ptr(), t["vl"].data_ptr(), mptr, kind, B, H, S, T, VC.D, x["scale"],
           out_v.data_ptr(), out_l.data_ptr(), stat_v.data_ptr(), stat_l.data_ptr(), wf.data_ptr(), nf)
    rc = lib.biattn_hip_train_dropout_f32(*fwd, p, sd.data_ptr(), sp) if dropout else lib.biattn_hip_train_f32(*fwd, sp)
    assert rc == 0, _lib.last_error()
    dq, dvv, dk, dvl = TG._nan(B, S, E), TG._nan(B, S, E), TG._nan(B, T, E), TG._nan(B, T, E)
    bwd = (t["q"].data_ptr(), t["k"].data_ptr(), t["vv"].data_ptr(), t["vl"].data_ptr(), mptr, kind, out_v.data_ptr(), out_l.data_ptr(),
           stat_v.data_ptr(), stat_l.data_ptr(), t["gv"].data_ptr(), t["gl"].data_ptr(), B, H, S, T, VC.D, x["scale"], dq.data_ptr(),
           dk.data_ptr(), dvv.data_ptr(), dvl.data_ptr(), wb.data_ptr(), nb)
    rc = lib.biattn_hip_backward_dropout_f32(*bwd, p, sd.data_ptr(), sp) if dropout else lib.biattn_hip_backward_f32(*bwd, sp)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    for n in ("q", "k", "vv", "vl", "gv", "gl"):
        assert np.array_equal(t[n].cpu().numpy().view(np.uint32), x[n].view(np.uint32)), (x["name"], n, "input changed")
    assert np.array_equal(sd.cpu().numpy(), seed)
    res = dict(out_v=out_v, out_l=out_l, stat_v=stat_v, stat_l=stat_l, dq=dq, dk=dk, dvv=dvv, dvl=dvl)
    return {n: v.cpu().numpy() for n, v in res.items()}


def same_bits(a, b, names=NAMES):
    for n in names:
        assert np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)), n


def sweep_case(x, p):
    """One case of the sweep: the six outputs per entry against the restatement under the numpy masks, and the statistics
    bitwise those of biattn_hip_train_f32."""
    seed = DC.seed_of(x["name"])
    kv, kl = DC.case_masks(x, p, seed)
    got = run(x, p, seed)
    who = "%s p%.1f" % (x["name"], p)
    DC.check(got, x, kv, kl, p, who, worst=WORST)
    plain = run(x, 0.0, seed, dropout=False)
    same_bits(got, plain, ("stat_v", "stat_l"))


# ---------------------------------------------------------------------------------------------------------------- the export

@pytest.mark.parametrize("S", [1, 33, 129, 257])
def test_export_is_the_numpy_masks_byte_for_byte(S):
    for T in (1, 33, 65, 256):
        for p in (0.1, 0.5):
            seed = DC.seed_of("export/%d/%d" % (S, T))
            kv, kl = export(seed, p, 2, 3, S, T)
            wv, wl = DC.keep_masks(seed, p, 6, S, T)
            assert np.array_equal(kv, wv.astype(np.uint8)) and np.array_equal(kl, wl.astype(np.uint8)), (S, T, p)


def test_export_with_more_tiles_than_ranges_and_without_dropout():
    seed = DC.seed_of("export/uneven")
    kv, kl = export(seed, 0.1, 1, 1, VC.S_UNEVEN, 33)
    wv, wl = DC.keep_masks(seed, 0.1, 1, VC.S_UNEVEN, 33)
    assert np.array_equal(kv, wv.astype(np.uint8)) and np.array_equal(kl, wl.astype(np.uint8))
    kv, kl = export(seed, 0.0, 2, 3, 33, 33)
    assert (kv == 1).all() and (kl == 1).all()


# ------------------------------------------------------------------------------------------------------------------ the C ABI

SS, TS = (1, 32, 33, 128, 129, 257), (1, 32, 33, 65, 256)
CASES = [(S, T, bh, VC.MASKS[(si + ti + bi + pi) % len(VC.MASKS)], p)
         for si, S in enumerate(SS) for ti, T in enumerate(TS) for bi, bh in enumerate(VC.BHS) for pi, p in enumerate((0.1, 0.5))]


@pytest.mark.parametrize("S,T,bh,mask,p", CASES,
                         ids=["S%d_T%d_%dx%d_%s_p%.1f" % (S, T, bh[0], bh[1], m, p) for S, T, bh, m, p in CASES])
def test_sweep(S, T, bh, mask, p):
    sweep_case(VC.make(bh[0], bh[1], S, T, mask), p)


def test_more_tiles_than_ranges_with_an_uneven_split():
    sweep_case(VC.make(1, 1, VC.S_UNEVEN, 33, "i64"), 0.1)


@pytest.mark.parametrize("special", VC.SPECIALS)
def test_specials_under_dropout(special):
    sweep_case(VC.make(1, 1, 33, 33, "none", special), 0.5)


def test_report_worst_entries():
    """Prints the worst entry per output of the sweep that ran in this process (kernel err, composition err, bound, ratio)."""
    for name in sorted(WORST):
        print("WORST %s" % WORST[name][1])


# ------------------------------------------------------------------------------------------------------------ bitwise checks

@pytest.mark.parametrize("shape,mask", [((2, 3, 257, 129), "f32"), ((1, 1, 33, 32), "i64")])
def test_without_dropout_the_new_entry_points_give_the_old_ones_bits(shape, mask):
    x = VC.make(*shape, mask)
    seed = DC.seed_of(x["name"])
    same_bits(run(x, 0.0, seed), run(x, 0.0, seed, dropout=False))


def test_two_runs_and_a_second_stream_give_the_same_bits_and_another_seed_does_not():
    x = VC.make(2, 3, 257, 129, "f32")
    seed = DC.seed_of(x["name"])
    a, b = run(x, 0.1, seed), run(x, 0.1, seed)
    c = run(x, 0.1, seed, stream=torch.cuda.Stream())
    same_bits(a, b)
    same_bits(a, c)
    d = run(x, 0.1, DC.seed_of("another"))
    assert not np.array_equal(a["out_v"].view(np.uint32), d["out_v"].view(np.uint32))
    same_bits(a, d, ("stat_v", "stat_l"))


# ------------------------------------------------------------------------------------------------------------------ refusals

def test_rejected_calls_touch_nothing_and_an_empty_batch_returns_0():
    from uninext_amd import _lib
    lib = _lib.load()
    B, H, S, T = 1, 1, 33, 33
    E = H * VC.D
    nan = TG._nan
    bufs = [nan(B, n, E) for n in (S, T, S, T)] + [nan(B, S, E), nan(B, T, E), nan(B * H, 2, 64), nan(B * H, 2, 64)] + \
           [nan(B, S, E), nan(B, T, E)] + [nan(B, S, E), nan(B, T, E), nan(B, S, E), nan(B, T, E)]
    nf = lib.biattn_hip_workspace_bytes(B, H, S, T, VC.D)
    nb = lib.biattn_hip_backward_workspace_bytes(B, H, S, T, VC.D)
    wf = torch.full((nf,), 0xFF, dtype=torch.uint8, device="cuda")
    wb = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda")
    seed = _seed(DC.seed_of("refusals"))
    ptr = [t.data_ptr() for t in bufs]

    def fwd(B=B, T=T, D=VC.D, nbytes=nf, p=0.1, sd=seed.data_ptr()):
        return lib.biattn_hip_train_dropout_f32(ptr[0], ptr[1], ptr[2], ptr[3], None, 0, B, H, S, T, D, 0.0625, ptr[4], ptr[5], ptr[6],
                                                ptr[7], wf.data_ptr(), nbytes, p, sd, None)

    def bwd(B=B, T=T, D=VC.D, nbytes=nb, p=0.1, sd=seed.data_ptr()):
        return lib.biattn_hip_backward_dropout_f32(ptr[0], ptr[1], ptr[2], ptr[3], None, 0, ptr[4], ptr[5], ptr[6], ptr[7], ptr[8],
                                                   ptr[9], B, H, S, T, D, 0.0625, ptr[10], ptr[11], ptr[12], ptr[13], wb.data_ptr(),
                                                   nbytes, p, sd, None)

    for call, n in ((fwd, nf), (bwd, nb)):
        assert call(sd=None) == -1
        assert call(p=1.0) == -2 and call(p=-0.1) == -2 and call(p=float("nan")) == -2
        assert call(D=128) == -5 and call(T=257) == -5 and call(nbytes=n - 1) == -6
        assert call(B=0) == 0
    kv = torch.full((B * H, S, T), 0xFF, dtype=torch.uint8, device="cuda")
    keep = lambda sd=seed.data_ptr(), p=0.1, T=T, B=B, out=kv.data_ptr(): lib.biattn_hip_dropout_keep_u8(
        sd, p, B, H, S, T, out, wf.data_ptr(), None)
    assert keep(sd=None) == -1 and keep(p=1.0) == -2 and keep(p=float("nan")) == -2 and keep(T=257) == -5 and keep(out=None) == -1
    assert keep(B=0) == 0
    torch.cuda.synchronize()
    for t in bufs:
        assert bool(torch.isnan(t).all())
    assert bool((wf == 0xFF).all()) and bool((wb == 0xFF).all()) and bool((kv == 0xFF).all())


# ---------------------------------------------------------------------------------------------------------------- the module

def _flags(block, training, dropout):
    block.attn.own_training, block.attn.own_dropout = training, dropout


def _step(block, own, checkpointed=False):
    dropout = block.attn.own_dropout                              # TG._step sets own_training alone
    out = TG._step(block, own, checkpointed)
    assert block.attn.own_dropout == dropout
    return out


def test_module_route_with_dropout_agrees_with_the_composition_on_the_exported_masks():
    import decoder_cases as C
    from uninext_amd import _lib, ext
    from uninext_amd.modules import vl_fusion
    block = TG._block(dropout=0.1)
    block.train()
    fixed = _seed(DC.seed_of("module"))
    kv, kl = ext.bi_attention_dropout_keep(fixed, 0.1, 2, 2, 70, 9)          # TG._step's shapes: B 2, heads 2, S 70, T 9
    assert np.array_equal(kv.cpu().numpy(), DC.keep_masks(DC.seed_of("module"), 0.1, 4, 70, 9)[0].astype(np.uint8))
    c = float(DC.scale_of(0.1))
    masks = []
    real_F, real_seed, real_apply = vl_fusion.F, ext.bi_attention_seed, vl_fusion.BiAttentionFunction.apply

    def dropout_on_masks(w, p, training):
        assert training and p == 0.1
        return w * masks.pop(0).to(w.dtype) * c

    entered = []
    vl_fusion.F = types.SimpleNamespace(softmax=real_F.softmax, dropout=dropout_on_masks)
    ext.bi_attention_seed = lambda device: fixed
    vl_fusion.BiAttentionFunction.apply = lambda *a: entered.append(len(a)) or real_apply(*a)
    try:
        block.attn.own_dropout = False
        masks[:] = [kv, kl]                                                  # _core_torch drops p_v first, then p_l
        ref = _step(block, own=True)                                        # own_dropout off: the composition serves
        assert not entered and not masks
        block.attn.own_dropout = True
        own = _step(block, own=True)
        assert entered == [9] and "biattn_bwd_image_dropout" in _lib.last_kernel("biattn_bwd")
    finally:
        vl_fusion.F, ext.bi_attention_seed, vl_fusion.BiAttentionFunction.apply = real_F, real_seed, real_apply
    for n in ref:
        scale = max(np.abs(ref[n]).max(), 1e-30)
        print(n, "%.2e" % (np.abs(own[n] - ref[n]).max() / scale))
        assert np.abs(own[n] - ref[n]).max() <= C.TOL * scale, (n, np.abs(own[n] - ref[n]).max() / scale)


def test_checkpointing_redraws_the_forwards_seed():
    """Without replacing the seed helper: torch.manual_seed before each step, and the recompute of
    checkpoint(..., use_reentrant=False) restores the generator, so outputs and gradients are bitwise the plain step's."""
    block = TG._block(dropout=0.1)
    block.train()
    block.attn.own_dropout = True
    torch.manual_seed(21)
    plain = _step(block, own=True)
    torch.manual_seed(21)
    ckpt = _step(block, own=True, checkpointed=True)
    torch.manual_seed(22)
    other = _step(block, own=True)
    for n in plain:
        assert np.array_equal(plain[n].view(np.uint32), ckpt[n].view(np.uint32)), n
    assert not np.array_equal(plain["out_v"].view(np.uint32), other["out_v"].view(np.uint32))


def test_eval_mode_keeps_its_routes():
    from uninext_amd import _lib
    from uninext_amd.modules import vl_fusion
    block = TG._block(dropout=0.1)
    block.eval()
    _flags(block, True, True)
    v, l = torch.randn(1, 40, 64, device="cuda"), torch.randn(1, 5, 48, device="cuda")
    entered = []
    real_apply = vl_fusion.BiAttentionFunction.apply
    vl_fusion.BiAttentionFunction.apply = lambda *a: entered.append(len(a)) or real_apply(*a)
    try:
        with torch.no_grad():
            block(v, l, None)
        assert not entered and "biattn_image" in _lib.last_kernel("biattn")    # the inference route
        ov, ol = block(v.requires_grad_(), l, None)
        (ov.sum() + ol.sum()).backward()
        assert entered == [7] and "dropout" not in _lib.last_kernel("biattn_bwd")   # under autograd: the kernels without dropout
    finally:
        vl_fusion.BiAttentionFunction.apply = real_apply
