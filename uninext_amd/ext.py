"""The two functions of the reference's pybind module `MultiScaleDeformableAttention`
(ops/src/vision.cpp:13-16), same names / argument order / error behaviour, implemented by
calling the C ABI of libmsda_hip.so with raw device pointers and PyTorch's current stream.

Reference host code mirrored: ops/src/ms_deform_attn.h:21-61 (device dispatch: CPU tensors
raise "Not implemented on the CPU") and ops/src/cuda/ms_deform_attn_cuda.cu:28-52
(contiguity / device / im2col_step checks), :54 and :121-123 (output allocation).
"""
import contextlib
import ctypes
import os
import threading

import torch

from . import _lib
from ._cache import CheckedOnce, tensor_version

_SUFFIX = {torch.float32: "f32", torch.float64: "f64"}
# CPU tensors: the reference raises "Not implemented on the CPU" (ops/src/ms_deform_attn.h:35-38).  This library has
# host-pointer variants of the operator (include/msda_hip.h: msda_host_*, csrc/msda_host.cpp), so
# CPU tensors are served by them -- BASELINE configs[0], the model's plumbing on a GPU-less box, then runs through the
# same `MSDeformAttnFunction` instead of ms_deform_attn_core_pytorch.  MSDA_HIP_STRICT_DEVICE=1 restores the
# reference's error.  GPU tensors never take this route: they go to the HIP kernels or fail loudly.
STRICT_DEVICE = os.environ.get("MSDA_HIP_STRICT_DEVICE", "0") == "1"
HOST_THREADS = int(os.environ.get("MSDA_HOST_THREADS", "0"))   # 0: all hardware threads
# Backward workspace (include/msda_hip.h: msda_hip_backward_workspace_bytes / msda_hip_backward_ws_f32): "1" (the default since
# round 6) lends the library a buffer from PyTorch's caching allocator for every fp32 backward call that may need one -- stream-
# ordered, no hipMalloc / device synchronisation inside the library, capturable, and visible to torch.cuda.memory_stats(); the
# block (~0.7 GB at the R50 training shapes) is cached by the allocator and handed out again call after call.  "0" leaves the
# library its own per-device workspace behind the allocator's back, allocated (hipMalloc, grown with a device sync, never freed)
# only when msda_bwd_regions is actually chosen: eight ranks of a node each did that.
TORCH_WORKSPACE = os.environ.get("MSDA_HIP_TORCH_WORKSPACE", "1") != "0"


# ---- call context of the automatic forward-kernel choice (include/msda_hip.h: msda_hip_set_call_context) ----------------
CTX_GEOMETRY_CHECKED, CTX_DETERMINISTIC = 1, 2
_site = threading.local()
_geometry_checks = CheckedOnce()


@contextlib.contextmanager
def call_site(site):
    """Forward calls made inside the block belong to call site `site` (0..63): the library chooses between its two
    encoder-forward kernels PER SITE.  MSDeformAttn modules wrap their operator calls in their own.  Outside of any block
    the site is derived from the call sequence (`_auto_site`)."""
    prev = getattr(_site, "value", None)
    _site.value = int(site)
    try:
        yield
    finally:
        _site.value = prev


def current_call_site():
    """The call site of the enclosing call_site() block (0 outside of one)."""
    v = getattr(_site, "value", None)
    return 0 if v is None else int(v)


def explicit_call_site():
    """The call site of the enclosing call_site() block, None outside of one -- autograd functions record it in forward
    and re-enter it in backward, which runs on another thread (`reenter`)."""
    v = getattr(_site, "value", None)
    return None if v is None else int(v)


def reenter(site):
    """Context manager for a backward: the forward's explicit call site again, or nothing when it had none (the call is
    then matched to its forward by the derived-site rules below)."""
    return call_site(site) if site is not None else contextlib.nullcontext()


# ---- call sites for callers that pass none: the reference's UNMODIFIED module on top (INTEGRATION.md option A) --------------
# ops/modules/ms_deform_attn.py:113 calls MSDeformAttnFunction.apply with no notion of a call site, from six encoder layers
# (dino.py:338,363) that sample differently.  Deformable-DETR builds `spatial_shapes` once per forward pass of the transformer
# and hands the SAME tensor object to every layer, so the ordinal of an encoder-shaped call since that object was first seen
# is the layer index: site = AUTO_SITE_BASE + ordinal % AUTO_SITES.  The backward of such a call arrives on the autograd
# thread with the forward's saved tensors: it is matched to its forward by the storage of `sampling_loc` (a tensor the
# layer made for this call alone and autograd keeps alive until then).  A caller that repeats ONE call in a loop on the same
# shapes object walks through the 16 derived slots (each settles on its kernel at its third visit): wrap such loops in
# call_site().  This repository's own modules pass explicit sites 1..47 from a counter of instances (the derived range 48..63
# is reserved: round 6); unmatched_backward_calls() counts the backward calls that found no forward.
AUTO_SITE_BASE, AUTO_SITES = 48, 16
_AUTO_BWD_KEEP = 256                      # forward calls remembered for their backward (inference never consumes them)


class _AutoSites:
    def __init__(self):
        self.lock = threading.Lock()
        self.shapes_ref = None            # weak reference to the spatial_shapes object of the current pass
        self.shapes_version = -1
        self.ordinal = 0
        self.by_loc = {}                  # (sampling_loc.data_ptr(), its shape) -> site, insertion-ordered
        self.last = -1                    # the site the last context carried (tests, bench)
        self.unmatched = 0                # backward calls whose forward was not found (they take the history-free kernel)

    def forward(self, spatial_shapes, sampling_loc):
        import weakref
        with self.lock:
            cur = self.shapes_ref() if self.shapes_ref is not None else None
            # (tensor_version: -1 for inference tensors -- a shapes tensor built under torch.inference_mode(), as Deformable-DETR
            # does, has no version counter and `_version` raises on it)
            version = tensor_version(spatial_shapes)
            if cur is not spatial_shapes or self.shapes_version != version:
                self.shapes_ref = weakref.ref(spatial_shapes)
                self.shapes_version = version
                self.ordinal = 0
            site = AUTO_SITE_BASE + self.ordinal % AUTO_SITES
            self.ordinal += 1
            if sampling_loc is not None:
                # (address AND shape: the caching allocator hands a freed address out again -- an inference pass's leftover entry must
                # not vouch for a later tensor of another call)
                self.by_loc[(int(sampling_loc.data_ptr()), tuple(sampling_loc.shape))] = site
                while len(self.by_loc) > _AUTO_BWD_KEEP:
                    self.by_loc.pop(next(iter(self.by_loc)))
            return site

    def backward(self, sampling_loc):
        with self.lock:
            site = self.by_loc.pop((int(sampling_loc.data_ptr()), tuple(sampling_loc.shape)), None)
            if site is None:
                self.unmatched += 1
            return site


_auto = _AutoSites()


def reset_auto_sites(forget_history=False):
    """Start a new pass for the derived call sites: the next encoder-shaped call without a call_site() block is layer 0.
    Only needed by a caller that REUSES one spatial_shapes tensor object across forward passes (the reference rebuilds it).
    forget_history=True also clears what the derived slots' earlier calls reported (msda_hip_reset_call_site): for a process
    that puts another model or checkpoint behind them."""
    with _auto.lock:
        _auto.shapes_ref, _auto.shapes_version, _auto.ordinal = None, -1, 0
        _auto.by_loc.clear()
    if forget_history:
        lib = _lib.load()
        for site in range(AUTO_SITE_BASE, AUTO_SITE_BASE + AUTO_SITES):
            lib.msda_hip_reset_call_site(site)


def _auto_site(spatial_shapes, sampling_loc, backward=False):
    """Site of an encoder-shaped call made outside of every call_site() block (see above).  A backward call whose forward is
    unknown gets -1: no history, the library's history-free kernel."""
    if backward:
        site = _auto.backward(sampling_loc)
        return -1 if site is None else site
    return _auto.forward(spatial_shapes, sampling_loc)


def unmatched_backward_calls():
    """How many encoder-shaped backward calls made outside call_site() blocks could not be matched to their forward (a cast or
    contiguous copy of sampling_loc, activation checkpointing, a forward older than the last 256): those calls are correct
    but take the history-free backward kernel.  A count that grows with the steps says the integration should pass sites."""
    return _auto.unmatched


def last_call_site():
    """The call site the last encoder-shaped call of this process carried (explicit or derived); -1 before the first."""
    return _auto.last


def _geometry_checked(spatial_shapes, level_start_index, spatial_size):
    """sum_l H_l * W_l == spatial_size and level_start_index == the prefix sums -- the precondition of the window kernels,
    which the reference operator itself does not require.  A device -> host copy, done once per shapes TENSOR OBJECT (weak
    reference + version, tests/test_cache_cpu.py) and never during a stream capture (a capture only sees earlier verdicts)."""
    extra = (int(spatial_size), id(level_start_index), int(level_start_index.data_ptr()))
    if _geometry_checks.hit(spatial_shapes, extra):
        return True
    if torch.cuda.is_current_stream_capturing():
        return False
    hw = (spatial_shapes[:, 0] * spatial_shapes[:, 1]).cpu()
    lsi = level_start_index.cpu()
    ok = bool((spatial_shapes.cpu() > 0).all()) and int(hw.sum()) == int(spatial_size) and lsi.shape[0] == hw.shape[0] \
        and bool((lsi == torch.cat((hw.new_zeros(1), hw.cumsum(0)[:-1]))).all())
    if ok:
        _geometry_checks.add(spatial_shapes, extra)
    return ok


def _set_call_context(lib, value_dtype, spatial_shapes, level_start_index, S, M_D, L, Lq, P, sampling_loc=None, backward=False):
    """Describe the coming forward or backward call to the library.  Only encoder-shaped fp32 calls have a choice to make; for
    everything else no context is set (and nothing is copied to the host)."""
    if value_dtype != torch.float32 or Lq != S or S < 1024 or L != 4 or P != 4 or M_D != 32:
        return
    flags = CTX_GEOMETRY_CHECKED if _geometry_checked(spatial_shapes, level_start_index, S) else 0
    if torch.are_deterministic_algorithms_enabled():
        flags |= CTX_DETERMINISTIC
    site = getattr(_site, "value", None)
    if site is None:
        site = _auto_site(spatial_shapes, sampling_loc, backward)
    _auto.last = int(site)
    lib.msda_hip_set_call_context(int(site), flags)



# ---- what every launcher below is made of --------------------------------------------------------------------------------
def _check(name, t, dev):
    if not t.is_contiguous():
        raise RuntimeError("%s tensor has to be contiguous" % name)
    if not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor" % name)  # "CUDA" == the HIP device on PyTorch-ROCm
    if t.device != dev:
        raise RuntimeError("%s is on %s but value is on %s" % (name, t.device, dev))


def _check_host(name, t, dev=None):
    """_check for an all-CPU call."""
    if not t.is_contiguous():
        raise RuntimeError("%s tensor has to be contiguous" % name)
    if t.is_cuda:
        raise RuntimeError("%s is on %s but value is on the CPU" % (name, t.device))


def _check_f32(name, t, dev, shape=None, message=None):
    """`t` is None or a contiguous float32 tensor on `dev`, of `shape` when one is given.  A wrong dtype or shape is refused
    with `message` ("<name> must be float32" without one)."""
    if t is None:
        return
    _check(name, t, dev)
    if t.dtype != torch.float32 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise RuntimeError(message or "%s must be float32" % name)


def _raise(rc):
    raise RuntimeError("MultiScaleDeformableAttention (HIP): %s [code %d]" % (_lib.last_error(), rc))


def _ptr(t):
    """Address of an optional tensor: None is the C ABI's NULL."""
    return None if t is None else t.data_ptr()


def _stream():
    """PyTorch's current stream of the current device as the `void* stream` of the C ABI."""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _launch(dev, fn, *args):
    """Call one device entry point on PyTorch's current stream of `dev` (the stream is the last parameter of every one); a
    non-zero return code raises."""
    with torch.cuda.device(dev):
        rc = fn(*args, _stream())
    if rc != 0:
        _raise(rc)


def _workspace(nbytes, dev):
    """Scratch memory lent to the library for one call, from PyTorch's caching allocator (never an empty tensor)."""
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)


def _pack_weight(weight, ok, dims, nbytes_fn, pack_fn, expected, refusal=None):
    """The body of every weight packer: `weight` is a float32 GPU tensor and `ok` (else `expected` is raised); size query on
    `dims`, `refusal` raised when it answers 0, allocation, launch.  Returns the opaque uint8 tensor."""
    _check("weight", weight, weight.device)
    if weight.dtype != torch.float32 or not ok:
        raise RuntimeError(expected)
    nbytes = nbytes_fn(*dims)
    if refusal is not None and nbytes == 0:
        raise RuntimeError(refusal)
    packed = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    _launch(weight.device, pack_fn, weight.data_ptr(), *dims, packed.data_ptr())
    return packed


def _dims(value, spatial_shapes, sampling_loc, im2col_step):
    if value.dim() != 4 or sampling_loc.dim() != 6 or spatial_shapes.dim() != 2:
        raise RuntimeError("expected value [N,S,M,D], spatial_shapes [L,2], sampling_loc [N,Lq,M,L,P,2]")
    batch, spatial_size, num_heads, channels = value.shape
    num_levels = spatial_shapes.shape[0]
    num_query, num_point = sampling_loc.shape[1], sampling_loc.shape[4]
    step = min(batch, int(im2col_step))
    if batch > 0 and (step <= 0 or batch % step != 0):
        raise RuntimeError("batch(%d) must divide im2col_step(%d)" % (batch, step))
    return batch, spatial_size, num_heads, channels, num_levels, num_query, num_point


def _validated(check, dev, value, spatial_shapes, level_start_index, sampling_loc, attn_weight, extra):
    """What _host_args and _prep share: the dtype of value, `check(name, t, dev)` on every tensor, the other dtypes."""
    if value.dtype not in _SUFFIX:
        raise RuntimeError("ms_deform_attn: unsupported dtype %s (float32/float64 only)" % value.dtype)
    named = (("value", value), ("spatial_shapes", spatial_shapes), ("level_start_index", level_start_index),
             ("sampling_loc", sampling_loc), ("attn_weight", attn_weight)) + tuple(extra)
    for name, t in named:
        check(name, t, dev)
    for name, t in named[3:]:
        if t.dtype != value.dtype:
            raise RuntimeError("%s has dtype %s, value has %s" % (name, t.dtype, value.dtype))
    if spatial_shapes.dtype != torch.int64 or level_start_index.dtype != torch.int64:
        raise RuntimeError("spatial_shapes and level_start_index must be int64")
    return _lib.load(), _SUFFIX[value.dtype]


def _host_args(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, extra=()):
    """Validation of an all-CPU call (same contiguity / dtype rules as the device path)."""
    if STRICT_DEVICE:
        raise RuntimeError("Not implemented on the CPU")  # ops/src/ms_deform_attn.h:38
    return _validated(_check_host, None, value, spatial_shapes, level_start_index, sampling_loc, attn_weight, extra)


def _prep(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, extra=()):
    if not value.is_cuda:
        raise RuntimeError("Not implemented on the CPU")  # ops/src/ms_deform_attn.h:38 (fused / device-only entry points)
    return _validated(_check, value.device, value, spatial_shapes, level_start_index, sampling_loc, attn_weight, extra)


def ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step):
    host = not value.is_cuda   # CPU tensors: the host-pointer variant of the C ABI
    lib, suf = (_host_args if host else _prep)(value, spatial_shapes, level_start_index, sampling_loc, attn_weight)
    N, S, M, D, L, Lq, P = _dims(value, spatial_shapes, sampling_loc, im2col_step)
    out = torch.empty((N, Lq, M * D), dtype=value.dtype, device=value.device)  # kernel writes every element
    args = (value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(), sampling_loc.data_ptr(),
            attn_weight.data_ptr(), N, S, M, D, L, Lq, P, out.data_ptr())
    if host:
        rc = getattr(lib, "msda_host_forward_" + suf)(*args, HOST_THREADS)
    else:
        with torch.cuda.device(value.device):
            _set_call_context(lib, value.dtype, spatial_shapes, level_start_index, S, D, L, Lq, P, sampling_loc)
            rc = getattr(lib, "msda_hip_forward_" + suf)(*args, _stream())
    if rc != 0:
        _raise(rc)
    return out


def ms_deform_attn_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output,
                            im2col_step):
    host = not value.is_cuda   # CPU tensors: the host-pointer variant of the C ABI
    lib, suf = (_host_args if host else _prep)(value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                                               extra=(("grad_output", grad_output),))
    N, S, M, D, L, Lq, P = _dims(value, spatial_shapes, sampling_loc, im2col_step)
    grad_value = torch.zeros_like(value)               # accumulated with atomics
    grad_loc = torch.empty_like(sampling_loc)          # every element written by the kernel
    grad_attn = torch.empty_like(attn_weight)
    args = (grad_output.data_ptr(), value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(),
            sampling_loc.data_ptr(), attn_weight.data_ptr(), N, S, M, D, L, Lq, P, grad_value.data_ptr(),
            grad_loc.data_ptr(), grad_attn.data_ptr())
    if host:
        rc = getattr(lib, "msda_host_backward_" + suf)(*args, HOST_THREADS)
    else:
        with torch.cuda.device(value.device):
            ws_bytes = int(lib.msda_hip_backward_workspace_bytes(N, S, M, D, L, Lq, P)) if TORCH_WORKSPACE and suf == "f32" else 0
            _set_call_context(lib, value.dtype, spatial_shapes, level_start_index, S, D, L, Lq, P, sampling_loc, backward=True)
            if ws_bytes > 0:
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=value.device)   # freed (to the cache) in stream order
                rc = lib.msda_hip_backward_ws_f32(*args, ws.data_ptr(), ws_bytes, _stream())
            else:
                rc = getattr(lib, "msda_hip_backward_" + suf)(*args, _stream())
    if rc != 0:
        _raise(rc)
    return [grad_value, grad_loc, grad_attn]


ERR_UNSUPPORTED = -5   # MSDA_ERR_UNSUPPORTED in include/msda_hip.h


def fused_forward_supported(value, reference_points, num_levels, num_points):
    """Geometry the fused-prologue kernel covers (include/msda_hip.h): fp32 on the GPU, 32 channels per head,
    levels * points == 16, 2-d or 4-d reference points."""
    return (value.is_cuda and value.dtype == torch.float32 and value.dim() == 4 and value.shape[3] == 32
            and num_levels * num_points == 16 and num_points % 2 == 0 and reference_points.shape[-1] in (2, 4))


def fused_forward_hm_supported(value_shape, num_levels, num_points, num_query):
    """Geometry msda_hip_forward_fused_hm_f32 covers: 32 channels per head, 4 levels x 4 points, encoder-sized calls."""
    return value_shape[-1] == 32 and num_levels == 4 and num_points == 4 and num_query >= 1024


def ms_deform_attn_forward_fused(value, spatial_shapes, level_start_index, reference_points, sampling_offsets,
                                 attention_logits, num_points, value_head_major=False):
    """MSDeformAttn.forward's softmax + sampling-location arithmetic + sampling in ONE kernel
    (ops/modules/ms_deform_attn.py:99-113).  `sampling_offsets` [N, Lq, M*L*P*2] and `attention_logits`
    [N, Lq, M*L*P] are the raw Linear outputs, `reference_points` [N, Lq, L, 2|4].  Inference only (no autograd).
    value_head_major: `value` is [N, M, S, D] (linear_packed_forward(..., head_major_rows=S)) instead of [N, S, M, D].
    Raises RuntimeError for unsupported geometry -- check fused_forward_supported() first."""
    lib, _ = _prep(value, spatial_shapes, level_start_index, sampling_offsets, attention_logits,
                   extra=(("reference_points", reference_points),))
    if value_head_major:
        N, M, S, D = value.shape
    else:
        N, S, M, D = value.shape
    L = spatial_shapes.shape[0]
    Lq = sampling_offsets.shape[1]
    P = int(num_points)
    if sampling_offsets.shape != (N, Lq, M * L * P * 2) or attention_logits.shape != (N, Lq, M * L * P) \
            or reference_points.shape[:3] != (N, Lq, L):
        raise RuntimeError("ms_deform_attn_forward_fused: inconsistent shapes")
    out = torch.empty((N, Lq, M * D), dtype=value.dtype, device=value.device)
    fn = lib.msda_hip_forward_fused_hm_f32 if value_head_major else lib.msda_hip_forward_fused_f32
    with torch.cuda.device(value.device):
        _set_call_context(lib, value.dtype, spatial_shapes, level_start_index, S, D, L, Lq, P)
        rc = fn(value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(), reference_points.data_ptr(),
                int(reference_points.shape[-1]), sampling_offsets.data_ptr(), attention_logits.data_ptr(),
                N, S, M, D, L, Lq, P, out.data_ptr(), _stream())
    if rc != 0:
        _raise(rc)
    return out


# ---- dynamic mask head (include/dynmask_hip.h) -------------------------------------------------------------
def msda_prologue(spatial_shapes, reference_points, sampling_offsets, attention_logits, num_heads, num_points):
    """(sampling_locations [N, Lq, M, L, P, 2], attention_weights [N, Lq, M, L, P]) from the raw Linear outputs and the reference
    points -- ops/modules/ms_deform_attn.py:99-112 in one kernel (include/msda_hip.h: msda_hip_prologue_f32).  fp32, GPU."""
    lib = _lib.load()
    dev = sampling_offsets.device
    N, Lq = sampling_offsets.shape[:2]
    L, M, P = spatial_shapes.shape[0], int(num_heads), int(num_points)
    for name, t in (("reference_points", reference_points), ("sampling_offsets", sampling_offsets), ("attention_logits", attention_logits)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == dev):
            raise RuntimeError("msda_prologue: %s must be a contiguous float32 tensor on the GPU" % name)
    if sampling_offsets.numel() != N * Lq * M * L * P * 2 or attention_logits.numel() != N * Lq * M * L * P \
            or tuple(reference_points.shape[:3]) != (N, Lq, L) or reference_points.shape[-1] not in (2, 4):
        raise RuntimeError("msda_prologue: inconsistent shapes")
    loc = torch.empty((N, Lq, M, L, P, 2), dtype=torch.float32, device=dev)
    attn = torch.empty((N, Lq, M, L, P), dtype=torch.float32, device=dev)
    _launch(dev, lib.msda_hip_prologue_f32, spatial_shapes.data_ptr(), reference_points.data_ptr(),
            int(reference_points.shape[-1]), sampling_offsets.data_ptr(), attention_logits.data_ptr(), N, M, L, Lq, P,
            loc.data_ptr(), attn.data_ptr())
    return loc, attn


def msda_prologue_backward(spatial_shapes, reference_points, sampling_offsets, attention_weights, grad_loc, grad_attn,
                           need_grad_reference=False, inplace=False):
    """(grad_sampling_offsets, grad_attention_logits, grad_reference_points | None) -- the backward of msda_prologue in one kernel
    (+ one small one for the reference points).  Shapes as the raw tensors: [N, Lq, M*L*P*2], [N, Lq, M*L*P], [N, Lq, L, 2|4].
    inplace: the results overwrite grad_loc / grad_attn (returned as views of the raw shapes)."""
    lib = _lib.load()
    dev = attention_weights.device
    N, Lq, M, L, P = attention_weights.shape
    for name, t in (("reference_points", reference_points), ("sampling_offsets", sampling_offsets), ("attention_weights", attention_weights),
                    ("grad_loc", grad_loc), ("grad_attn", grad_attn)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == dev):
            raise RuntimeError("msda_prologue_backward: %s must be a contiguous float32 tensor on the GPU" % name)
    g_off = grad_loc.view(N, Lq, M * L * P * 2) if inplace else torch.empty((N, Lq, M * L * P * 2), dtype=torch.float32, device=dev)
    g_logits = grad_attn.view(N, Lq, M * L * P) if inplace else torch.empty((N, Lq, M * L * P), dtype=torch.float32, device=dev)
    g_ref = torch.empty_like(reference_points) if need_grad_reference else None
    _launch(dev, lib.msda_hip_prologue_backward_f32, spatial_shapes.data_ptr(), reference_points.data_ptr(),
            int(reference_points.shape[-1]), sampling_offsets.data_ptr(), attention_weights.data_ptr(), grad_loc.data_ptr(),
            grad_attn.data_ptr(), N, M, L, Lq, P, g_off.data_ptr(), g_logits.data_ptr(), _ptr(g_ref))
    return g_off, g_logits, g_ref


def dynmask_supported(mask_feats):
    return mask_feats.is_cuda and mask_feats.dtype == torch.float32 and mask_feats.dim() == 4 and mask_feats.shape[1] == 8


def dynmask_forward(mask_feats, inst_xy, params, num_insts, stride, rel_coord=True):
    """Per-instance 3-layer 1x1 dynamic conv (ddetrs_dn.py:734-752 on the inputs of :765-808) -> [n_inst, H, W]."""
    lib = _lib.load()
    dev = mask_feats.device
    for name, t in (("mask_feats", mask_feats), ("inst_xy", inst_xy), ("params", params)):
        _check_f32(name, t, dev)
    N, C, H, W = mask_feats.shape
    counts = [int(n) for n in num_insts]
    n_all = sum(counts)
    want = (C + 2 if rel_coord else C) * 8 + 8 * 8 + 8 + 8 + 8 + 1
    if len(counts) != N or inst_xy.shape != (n_all, 2) or params.shape != (n_all, want):
        raise RuntimeError("dynmask_forward: inconsistent shapes")
    out = torch.empty((n_all, H, W), dtype=torch.float32, device=dev)
    arr = (ctypes.c_int * max(N, 1))(*counts)
    _launch(dev, lib.dynmask_hip_forward_f32, mask_feats.data_ptr(), inst_xy.data_ptr(), params.data_ptr(), arr, N, C, H, W,
            int(stride), int(bool(rel_coord)), out.data_ptr())
    return out


def aligned_bilinear_forward(x, factor):
    """aligned_bilinear (ddetrs_dn.py:1174-1196) of a [n, 1, h, w] or [n, h, w] fp32 GPU tensor."""
    lib = _lib.load()
    _check_f32("tensor", x, x.device)
    squeeze = x.dim() == 4
    if squeeze and x.shape[1] != 1:
        raise RuntimeError("aligned_bilinear_forward: expected [n, 1, h, w]")
    n, h, w = x.shape[0], x.shape[-2], x.shape[-1]
    f = int(factor)
    out = torch.empty((n, 1, f * h, f * w) if squeeze else (n, f * h, f * w), dtype=torch.float32, device=x.device)
    _launch(x.device, lib.aligned_bilinear_hip_f32, x.data_ptr(), n, h, w, f, out.data_ptr())
    return out


def dynmask_backward(mask_feats, inst_xy, params, num_insts, stride, rel_coord, grad_logits, need_xy=True, need_feats=True,
                     need_params=True):
    """Backward of dynmask_forward (include/dynmask_hip.h: dynmask_hip_backward_f32): grad_logits [n_inst, H, W] ->
    (grad_mask_feats [N, 8, H, W], grad_params [n_inst, P], grad_inst_xy [n_inst, 2] or None).  need_feats / need_params /
    need_xy = False: that gradient is None and its kernels are not launched (round 6).  Deterministic (no float
    atomics); the activations are recomputed, the workspace (partial sums of the pixel slices) comes from PyTorch's
    caching allocator for the duration of the call."""
    lib = _lib.load()
    dev = mask_feats.device
    for name, t in (("mask_feats", mask_feats), ("inst_xy", inst_xy), ("params", params), ("grad_logits", grad_logits)):
        _check_f32(name, t, dev)
    N, C, H, W = mask_feats.shape
    counts = [int(n) for n in num_insts]
    n_all = sum(counts)
    want = (C + 2 if rel_coord else C) * 8 + 8 * 8 + 8 + 8 + 8 + 1
    if len(counts) != N or inst_xy.shape != (n_all, 2) or params.shape != (n_all, want) or grad_logits.shape != (n_all, H, W):
        raise RuntimeError("dynmask_backward: inconsistent shapes")
    if N > _lib.DYNMASK_BWD_MAX_BATCH:
        raise RuntimeError("dynmask_backward: at most %d images per call" % _lib.DYNMASK_BWD_MAX_BATCH)
    g_feats = torch.empty_like(mask_feats) if need_feats else None
    g_params = torch.empty_like(params) if (need_params or need_xy) else None     # (the reference points' gradient comes out of the same pass)
    g_xy = torch.empty_like(inst_xy) if need_xy else None
    ws_bytes = int(lib.dynmask_hip_backward_workspace_bytes(n_all, H, W)) if g_params is not None else 0
    ws = _workspace(ws_bytes, dev)
    arr = (ctypes.c_int * max(N, 1))(*counts)
    _launch(dev, lib.dynmask_hip_backward_f32, mask_feats.data_ptr(), inst_xy.data_ptr(), params.data_ptr(), arr, N, C, H, W,
            int(stride), int(bool(rel_coord)), grad_logits.data_ptr(), _ptr(g_feats), _ptr(g_params), _ptr(g_xy),
            ws.data_ptr(), ws_bytes)
    return g_feats, (g_params if need_params else None), g_xy


def aligned_bilinear_backward(grad_out, factor):
    """Backward of aligned_bilinear_forward: grad_out [n, 1, f h, f w] or [n, f h, f w] -> the input's gradient."""
    lib = _lib.load()
    _check_f32("grad_out", grad_out, grad_out.device)
    squeeze = grad_out.dim() == 4
    if squeeze and grad_out.shape[1] != 1:
        raise RuntimeError("aligned_bilinear_backward: expected [n, 1, H, W]")
    f = int(factor)
    n, oh, ow = grad_out.shape[0], grad_out.shape[-2], grad_out.shape[-1]
    if f < 1 or oh % f or ow % f:
        raise RuntimeError("aligned_bilinear_backward: the gradient's size is not a multiple of the factor")
    h, w = oh // f, ow // f
    out = torch.empty((n, 1, h, w) if squeeze else (n, h, w), dtype=torch.float32, device=grad_out.device)
    _launch(grad_out.device, lib.aligned_bilinear_hip_backward_f32, grad_out.data_ptr(), n, h, w, f, out.data_ptr())
    return out


def _check_conv_args(x, weight, bias):
    """x, weight and the optional bias of a convolution: contiguous on the device of x, all of them, then float32."""
    named = (("x", x), ("weight", weight), ("bias", bias))
    for name, t in named:
        if t is not None:
            _check(name, t, x.device)
    for name, t in named:
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError("%s must be float32" % name)


def patch_embed_supported(x, weight, stride, padding):
    """True when include/patch_embed_hip.h has a kernel for this convolution (fp32, GPU, kernel == stride, no pad)."""
    if not (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.dim() == 4 and weight.dim() == 4):
        return False
    k = weight.shape[2]
    pad = tuple(padding) if isinstance(padding, (tuple, list)) else (padding, padding)
    st = tuple(stride) if isinstance(stride, (tuple, list)) else (stride, stride)
    return (weight.shape[3] == k and st == (k, k) and pad == (0, 0) and k in (2, 4, 8, 16)
            and (weight.shape[1] * k * k) % 16 == 0 and x.shape[1] == weight.shape[1])


def patch_embed_forward(x, weight, bias=None, channels_last=True):
    """Non-overlapping-patch convolution (kernel == stride, no padding) on the matrix cores, exact fp32.

    x [B, C, H, W], weight [E, C, k, k] (nn.Conv2d layout), bias [E] or None ->
    [B, H // k, W // k, E] if channels_last (ViT PatchEmbed.forward, backbone/utils.py:182-186)
    else [B, E, H // k, W // k] (nn.Conv2d, ConvNeXt stem / downsample convs, backbone/convnext.py:80,87).
    Forward only; under autograd backbone.PatchEmbedFunction pairs it with patch_embed_backward.
    """
    lib = _lib.load()
    _check_conv_args(x, weight, bias)
    if x.dim() != 4 or weight.dim() != 4 or weight.shape[2] != weight.shape[3] or x.shape[1] != weight.shape[1]:
        raise RuntimeError("patch_embed_forward: expected x [B, C, H, W] and weight [E, C, k, k]")
    if bias is not None and bias.shape != (weight.shape[0],):
        raise RuntimeError("patch_embed_forward: bias must be [E]")
    B, C, H, W = x.shape
    E, k = weight.shape[0], weight.shape[2]
    shape = (B, H // k, W // k, E) if channels_last else (B, E, H // k, W // k)
    out = torch.empty(shape, dtype=torch.float32, device=x.device)
    _launch(x.device, lib.patch_embed_hip_f32, x.data_ptr(), weight.data_ptr(), _ptr(bias), B, C, H, W, E, k,
            int(bool(channels_last)), out.data_ptr())
    return out


def patch_embed_backward(x, weight, grad_out, channels_last, need_input=True, need_weight=True, need_bias=True):
    """Backward of patch_embed_forward (include/patch_embed_hip.h: patch_embed_hip_backward_f32): exact fp32, fixed order,
    bitwise repeatable.  x [B, C, H, W] (read only for need_weight), weight [E, C, k, k] (read only for need_input), grad_out in
    the forward's output layout ([B, H // k, W // k, E] if channels_last, else [B, E, H // k, W // k]), contiguous.  Returns
    (grad_x [B, C, H, W], grad_weight [E, C, k, k], grad_bias [E]); a part that is not needed is None and its kernels are not
    launched.  The workspace comes from PyTorch's caching allocator on the current stream for the duration of the call."""
    lib = _lib.load()
    dev = grad_out.device
    _check("grad_out", grad_out, dev)
    if x.dim() != 4 or weight.dim() != 4 or weight.shape[2] != weight.shape[3] or x.shape[1] != weight.shape[1]:
        raise RuntimeError("patch_embed_backward: expected x [B, C, H, W] and weight [E, C, k, k]")
    for name, t in (("x", x), ("weight", weight), ("grad_out", grad_out)):
        if t.dtype != torch.float32:
            raise RuntimeError("%s must be float32" % name)
    B, C, H, W = x.shape
    E, k = weight.shape[0], weight.shape[2]
    shape = (B, H // k, W // k, E) if channels_last else (B, E, H // k, W // k)
    if tuple(grad_out.shape) != shape:
        raise RuntimeError("patch_embed_backward: grad_out must be %s" % (list(shape),))
    if need_weight:
        _check("x", x, dev)
    if need_input:
        _check("weight", weight, dev)
    g_x = torch.empty((B, C, H, W), dtype=torch.float32, device=dev) if need_input else None
    g_w = torch.empty((E, C, k, k), dtype=torch.float32, device=dev) if need_weight else None
    g_b = torch.empty((E,), dtype=torch.float32, device=dev) if need_bias else None
    ws_bytes = int(lib.patch_embed_hip_backward_workspace_bytes(B, C, H, W, E, k)) if (need_weight or need_bias) else 0
    ws = _workspace(ws_bytes, dev)
    _launch(dev, lib.patch_embed_hip_backward_f32, _ptr(x if need_weight else None), _ptr(weight if need_input else None),
            grad_out.data_ptr(), B, C, H, W, E, k, int(bool(channels_last)), _ptr(g_x), _ptr(g_w), _ptr(g_b),
            ws.data_ptr(), ws_bytes)
    return g_x, g_w, g_b


CONVNEXT_MAX_DIM = 1536   # include/patch_embed_hip.h: patch_embed_hip_convnext_dwconv_ln_f32 takes C % 32 == 0, 32 <= C <= 1536


def convnext_dwconv_ln_supported(x, dw_weight):
    """True when patch_embed_hip_convnext_dwconv_ln_f32 (include/patch_embed_hip.h) covers this block head: contiguous fp32 GPU tensors,
    x [B, C, H, W], dw_weight [C, 1, 7, 7], C a multiple of 32 between 32 and 1536."""
    if not (x.is_cuda and x.dtype == torch.float32 and dw_weight.dtype == torch.float32 and x.dim() == 4 and dw_weight.dim() == 4
            and x.is_contiguous() and dw_weight.is_contiguous()):
        return False
    C = x.shape[1]
    return tuple(dw_weight.shape) == (C, 1, 7, 7) and C % 32 == 0 and 32 <= C <= CONVNEXT_MAX_DIM


def convnext_dwconv_ln(x, dw_weight, dw_bias, ln_weight, ln_bias, eps):
    """The ConvNeXt block's head in one kernel (backbone/convnext.py:46-48): depthwise 7x7 convolution (padding 3) of
    x [B, C, H, W] with dw_weight [C, 1, 7, 7] + dw_bias [C] (or None), then LayerNorm over C with ln_weight / ln_bias [C]:
    [B, H, W, C].  Exact fp32, bitwise repeatable.  Unsupported arguments raise: callers ask convnext_dwconv_ln_supported first."""
    lib = _lib.load()
    if not convnext_dwconv_ln_supported(x, dw_weight):
        raise RuntimeError("convnext_dwconv_ln: unsupported arguments (contiguous fp32 GPU x [B, C, H, W] and weight [C, 1, 7, 7], "
                           "C a multiple of 32, 32 <= C <= %d)" % CONVNEXT_MAX_DIM)
    B, C, H, W = x.shape
    _check("dw_weight", dw_weight, x.device)
    for name, t in (("dw_bias", dw_bias), ("ln_weight", ln_weight), ("ln_bias", ln_bias)):
        _check_f32(name, t, x.device, (C,), "convnext_dwconv_ln: %s must be float32 [C]" % name)
    if ln_weight is None or ln_bias is None:
        raise RuntimeError("convnext_dwconv_ln: ln_weight and ln_bias are required")
    out = torch.empty((B, H, W, C), dtype=torch.float32, device=x.device)
    if out.numel() == 0:
        return out
    _launch(x.device, lib.patch_embed_hip_convnext_dwconv_ln_f32, x.data_ptr(), dw_weight.data_ptr(), _ptr(dw_bias), ln_weight.data_ptr(),
            ln_bias.data_ptr(), float(eps), B, C, H, W, out.data_ptr())
    return out


def convnext_scale_residual(y, gamma, input):
    """The ConvNeXt block's tail in one kernel (backbone/convnext.py:52-56): `input + (gamma * y).permute(0, 3, 1, 2)` for
    y [B, H, W, C], gamma [C] or None, input [B, C, H, W] -> [B, C, H, W], bitwise what PyTorch's two operations give."""
    lib = _lib.load()
    _check("y", y, y.device)
    _check("input", input, y.device)
    if y.dtype != torch.float32 or input.dtype != torch.float32 or y.dim() != 4 or input.dim() != 4:
        raise RuntimeError("convnext_scale_residual: expected float32 y [B, H, W, C] and input [B, C, H, W]")
    B, H, W, C = y.shape
    if tuple(input.shape) != (B, C, H, W):
        raise RuntimeError("convnext_scale_residual: input must be [%d, %d, %d, %d]" % (B, C, H, W))
    _check_f32("gamma", gamma, y.device, (C,), "convnext_scale_residual: gamma must be float32 [C]")
    out = torch.empty_like(input)
    if out.numel():
        _launch(y.device, lib.patch_embed_hip_convnext_scale_residual_f32, y.data_ptr(), _ptr(gamma), input.data_ptr(), B, C, H, W,
                out.data_ptr())
    return out


def convnext_dwconv_ln_backward(x, dw_weight, dw_bias, ln_weight, eps, grad_out, need_input=True, need_dw_weight=True,
                                need_dw_bias=True, need_ln_weight=True, need_ln_bias=True):
    """Backward of convnext_dwconv_ln (patch_embed_hip_convnext_dwconv_ln_backward_f32): exact fp32, fixed order, bitwise repeatable.
    x [B, C, H, W], dw_weight [C, 1, 7, 7], dw_bias [C] or None, ln_weight [C], grad_out [B, H, W, C]; the convolution output is
    recomputed from x.  Returns (grad_x, grad_dw_weight, grad_dw_bias, grad_ln_weight, grad_ln_bias); a part that is not needed is
    None and is not computed.  The workspace comes from PyTorch's caching allocator on the current stream; a grad_out or ln_weight
    that does not start on a multiple of 16 bytes is copied once."""
    lib = _lib.load()
    if not convnext_dwconv_ln_supported(x, dw_weight):
        raise RuntimeError("convnext_dwconv_ln_backward: unsupported arguments (contiguous fp32 GPU x [B, C, H, W] and weight "
                           "[C, 1, 7, 7], C a multiple of 32, 32 <= C <= %d)" % CONVNEXT_MAX_DIM)
    B, C, H, W = x.shape
    dev = x.device
    _check("dw_weight", dw_weight, dev)
    for name, t in (("dw_bias", dw_bias), ("ln_weight", ln_weight)):
        _check_f32(name, t, dev, (C,), "convnext_dwconv_ln_backward: %s must be float32 [C]" % name)
    if ln_weight is None:
        raise RuntimeError("convnext_dwconv_ln_backward: ln_weight is required")
    _check_f32("grad_out", grad_out, dev, (B, H, W, C), "convnext_dwconv_ln_backward: grad_out must be float32 [%d, %d, %d, %d]" % (B, H, W, C))
    new = lambda need, *shape: torch.empty(shape, dtype=torch.float32, device=dev) if need else None
    g_x, g_w, g_b = new(need_input, B, C, H, W), new(need_dw_weight, C, 1, 7, 7), new(need_dw_bias and dw_bias is not None, C)
    g_lw, g_lb = new(need_ln_weight, C), new(need_ln_bias, C)
    if x.numel() == 0:   # the gradients of a sum over no pixels (an empty tensor has no address to hand over)
        return (g_x,) + tuple(None if g is None else g.zero_() for g in (g_w, g_b, g_lw, g_lb))
    # the kernel reads grad_out and ln_weight 16 bytes at once; autograd may hand over a view at any offset: one copy then, same values
    grad_out, ln_weight = (t if t.data_ptr() % 16 == 0 else t.clone() for t in (grad_out, ln_weight))
    ws_bytes = int(lib.patch_embed_hip_convnext_dwconv_ln_backward_workspace_bytes(B, C, H, W))
    ws = _workspace(ws_bytes, dev)
    _launch(dev, lib.patch_embed_hip_convnext_dwconv_ln_backward_f32, x.data_ptr(), dw_weight.data_ptr(), _ptr(dw_bias),
            ln_weight.data_ptr(), float(eps), grad_out.data_ptr(), B, C, H, W, _ptr(g_x), _ptr(g_w), _ptr(g_b), _ptr(g_lw), _ptr(g_lb),
            ws.data_ptr(), ws_bytes)
    return g_x, g_w, g_b, g_lw, g_lb


def convnext_scale_residual_drop(y, gamma, sample_scale, input):
    """convnext_scale_residual with stochastic depth: `input + ((gamma * y) * sample_scale.view(B, 1, 1, 1)).permute(0, 3, 1, 2)`,
    bitwise PyTorch's three operations; sample_scale [B] (0 or 1 / keep per sample) or None: convnext_scale_residual itself."""
    if sample_scale is None:
        return convnext_scale_residual(y, gamma, input)
    lib = _lib.load()
    _check("y", y, y.device)
    _check("input", input, y.device)
    if y.dtype != torch.float32 or input.dtype != torch.float32 or y.dim() != 4 or input.dim() != 4:
        raise RuntimeError("convnext_scale_residual_drop: expected float32 y [B, H, W, C] and input [B, C, H, W]")
    B, H, W, C = y.shape
    if tuple(input.shape) != (B, C, H, W):
        raise RuntimeError("convnext_scale_residual_drop: input must be [%d, %d, %d, %d]" % (B, C, H, W))
    _check_f32("gamma", gamma, y.device, (C,), "convnext_scale_residual_drop: gamma must be float32 [C]")
    _check_f32("sample_scale", sample_scale, y.device, (B,), "convnext_scale_residual_drop: sample_scale must be float32 [B]")
    out = torch.empty_like(input)
    if out.numel():
        _launch(y.device, lib.patch_embed_hip_convnext_scale_residual_drop_f32, y.data_ptr(), _ptr(gamma), sample_scale.data_ptr(),
                input.data_ptr(), B, C, H, W, out.data_ptr())
    return out


def convnext_scale_residual_backward(grad_out, y, gamma, sample_scale, need_y=True, need_gamma=True):
    """Backward of the tail (patch_embed_hip_convnext_scale_residual_backward_f32) from grad_out [B, C, H, W]: returns
    (grad_y [B, H, W, C] = ((grad_out * sample_scale) * gamma) permuted, bitwise; grad_gamma [C] = sum (grad_out * sample_scale) * y),
    None for a part that is not needed (grad_gamma also without gamma).  The gradient of `input` is grad_out itself: the caller's."""
    lib = _lib.load()
    dev = grad_out.device
    _check("grad_out", grad_out, dev)
    if grad_out.dtype != torch.float32 or grad_out.dim() != 4:
        raise RuntimeError("convnext_scale_residual_backward: expected a float32 grad_out [B, C, H, W]")
    B, C, H, W = grad_out.shape
    need_gamma = bool(need_gamma and gamma is not None)
    _check_f32("gamma", gamma, dev, (C,), "convnext_scale_residual_backward: gamma must be float32 [C]")
    _check_f32("sample_scale", sample_scale, dev, (B,), "convnext_scale_residual_backward: sample_scale must be float32 [B]")
    if need_gamma:
        _check_f32("y", y, dev, (B, H, W, C), "convnext_scale_residual_backward: y must be float32 [%d, %d, %d, %d]" % (B, H, W, C))
        if y is None:
            raise RuntimeError("convnext_scale_residual_backward: y is required for grad_gamma")
    g_y = torch.empty((B, H, W, C), dtype=torch.float32, device=dev) if need_y else None
    g_g = torch.empty((C,), dtype=torch.float32, device=dev) if need_gamma else None
    if grad_out.numel() == 0:
        return g_y, (None if g_g is None else g_g.zero_())
    ws_bytes = int(lib.patch_embed_hip_convnext_scale_residual_backward_workspace_bytes(B, C, H, W)) if need_gamma else 0
    ws = _workspace(ws_bytes, dev)
    _launch(dev, lib.patch_embed_hip_convnext_scale_residual_backward_f32, grad_out.data_ptr(), _ptr(y if need_gamma else None), _ptr(gamma),
            _ptr(sample_scale), B, C, H, W, _ptr(g_y), _ptr(g_g), ws.data_ptr(), ws_bytes)
    return g_y, g_g


def layernorm_channels_first_backward(x, weight, eps, grad_out, need_input=True, need_weight=True, need_bias=True):
    """Backward of layernorm_channels_first (patch_embed_hip_layernorm_cf_backward_f32): x, grad_out [B, C, H, W], weight [C] ->
    (grad_x [B, C, H, W], grad_weight [C], grad_bias [C]), None for a part that is not needed."""
    lib = _lib.load()
    dev = x.device
    _check("x", x, dev)
    if x.dtype != torch.float32 or x.dim() != 4:
        raise RuntimeError("layernorm_channels_first_backward: expected a float32 x [B, C, H, W]")
    B, C, H, W = x.shape
    if weight is None:
        raise RuntimeError("layernorm_channels_first_backward: weight is required")
    _check_f32("weight", weight, dev, (C,), "layernorm_channels_first_backward: weight must be float32 [C]")
    _check_f32("grad_out", grad_out, dev, (B, C, H, W), "layernorm_channels_first_backward: grad_out must be float32 [%d, %d, %d, %d]" % (B, C, H, W))
    g_x = torch.empty_like(x) if need_input else None
    g_w = torch.empty((C,), dtype=torch.float32, device=dev) if need_weight else None
    g_b = torch.empty((C,), dtype=torch.float32, device=dev) if need_bias else None
    if x.numel() == 0:
        return g_x, (None if g_w is None else g_w.zero_()), (None if g_b is None else g_b.zero_())
    ws_bytes = int(lib.patch_embed_hip_layernorm_cf_backward_workspace_bytes(B, C, H, W)) if (need_weight or need_bias) else 0
    ws = _workspace(ws_bytes, dev)
    _launch(dev, lib.patch_embed_hip_layernorm_cf_backward_f32, x.data_ptr(), weight.data_ptr(), float(eps), grad_out.data_ptr(), B, C, H, W,
            _ptr(g_x), _ptr(g_w), _ptr(g_b), ws.data_ptr(), ws_bytes)
    return g_x, g_w, g_b


def layernorm_channels_first(x, weight, bias, eps):
    """LayerNorm over the channels of x [B, C, H, W] in one kernel (backbone/convnext.py:189-194); weight, bias [C]."""
    lib = _lib.load()
    _check("x", x, x.device)
    if x.dtype != torch.float32 or x.dim() != 4:
        raise RuntimeError("layernorm_channels_first: expected a float32 x [B, C, H, W]")
    B, C, H, W = x.shape
    for name, t in (("weight", weight), ("bias", bias)):
        if t is None:
            raise RuntimeError("layernorm_channels_first: %s is required" % name)
        _check_f32(name, t, x.device, (C,), "layernorm_channels_first: %s must be float32 [C]" % name)
    out = torch.empty_like(x)
    if out.numel():
        _launch(x.device, lib.patch_embed_hip_layernorm_cf_f32, x.data_ptr(), weight.data_ptr(), bias.data_ptr(), float(eps), B, C, H, W,
                out.data_ptr())
    return out


def vit_attention_supported(qkv, rel_h_table, rel_w_table, num_heads, q_hw):
    """True when patch_embed_hip_vit_attn_f32 (include/patch_embed_hip.h) covers this attention core: qkv a contiguous fp32 GPU
    tensor [B', S, 3 * num_heads * D] with S = q_h * q_w and D in {64, 80}; the tables both None or contiguous fp32
    [2 * q_h - 1, D] and [2 * q_w - 1, D] on qkv's device; 16-byte aligned storage; sizes inside the header's limits."""
    if not (qkv.is_cuda and qkv.dtype == torch.float32 and qkv.dim() == 3 and qkv.is_contiguous()):
        return False
    q_h, q_w = int(q_hw[0]), int(q_hw[1])
    B, S, E3 = qkv.shape
    if num_heads <= 0 or q_h <= 0 or q_w <= 0 or S != q_h * q_w or E3 % (3 * num_heads) != 0:
        return False
    D = E3 // (3 * num_heads)
    if D not in _lib.VIT_ATTN_HEAD_DIMS:
        return False
    SP = (S + 31) // 32 * 32
    if (q_h > _lib.VIT_ATTN_MAX_SIDE or q_w > _lib.VIT_ATTN_MAX_SIDE or S > _lib.VIT_ATTN_MAX_TOKENS or (q_h + q_w) * SP >= 1 << 31
            or B * num_heads * ((S + 127) // 128) >= 1 << 31 or B * num_heads * (q_h + q_w) * SP >= 1 << 40 or B * S * E3 >= 1 << 42):
        return False
    if (rel_h_table is None) != (rel_w_table is None):
        return False
    for t, rows in ((rel_h_table, 2 * q_h - 1), (rel_w_table, 2 * q_w - 1)):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == qkv.device
                                  and tuple(t.shape) == (rows, D)):
            return False
    return all(t is None or t.data_ptr() % 16 == 0 for t in (qkv, rel_h_table, rel_w_table))   # the kernels load 16 bytes at once


def vit_attention(qkv, rel_h_table, rel_w_table, num_heads, q_hw, scale):
    """The core of the ViT blocks' Attention.forward at inference (include/patch_embed_hip.h: patch_embed_hip_vit_attn_f32):
    qkv [B', S, 3 * num_heads * D] is the `qkv` Linear's output, read in place; rel_h_table [2 * q_h - 1, D] and rel_w_table
    [2 * q_w - 1, D] are the relative-position tables at exactly these lengths, or both None.  Returns [B', S, num_heads * D],
    token-major, the input of `proj`.  Exact fp32, bitwise repeatable; the [B' * heads, S, S] scores are never written.  The
    workspace comes from PyTorch's caching allocator on the current stream for the duration of the call.  Unsupported arguments
    raise: callers ask vit_attention_supported first."""
    lib = _lib.load()
    if not vit_attention_supported(qkv, rel_h_table, rel_w_table, num_heads, q_hw):
        raise RuntimeError("vit_attention: unsupported arguments (contiguous fp32 GPU qkv [B, q_h * q_w, 3 * heads * D], D in %s, "
                           "tables [2 * q_h - 1, D] and [2 * q_w - 1, D] or both None)" % (_lib.VIT_ATTN_HEAD_DIMS,))
    q_h, q_w = int(q_hw[0]), int(q_hw[1])
    B, S, E3 = qkv.shape
    D = E3 // (3 * num_heads)
    for name, t in (("rel_h_table", rel_h_table), ("rel_w_table", rel_w_table)):
        _check_f32(name, t, qkv.device)
    out = torch.empty((B, S, num_heads * D), dtype=torch.float32, device=qkv.device)
    if B == 0:
        return out
    ws_bytes = int(lib.patch_embed_hip_vit_attn_workspace_bytes(B, num_heads, q_h, q_w, D))
    ws = _workspace(ws_bytes, qkv.device)
    _launch(qkv.device, lib.patch_embed_hip_vit_attn_f32, qkv.data_ptr(), _ptr(rel_h_table), _ptr(rel_w_table), B, num_heads, q_h, q_w,
            D, float(scale), out.data_ptr(), ws.data_ptr(), ws_bytes)
    return out


def vit_attention_train_supported(qkv, rel_h_table, rel_w_table, num_heads, q_hw):
    """vit_attention_supported, and q_w inside the training kernels' limit (include/patch_embed_hip.h)."""
    return vit_attention_supported(qkv, rel_h_table, rel_w_table, num_heads, q_hw) and int(q_hw[1]) <= _lib.VIT_ATTN_TRAIN_MAX_W


def _vit_train_args(name, qkv, rel_h_table, rel_w_table, num_heads, q_hw):
    if not vit_attention_train_supported(qkv, rel_h_table, rel_w_table, num_heads, q_hw):
        raise RuntimeError("%s: unsupported arguments (contiguous fp32 GPU qkv [B, q_h * q_w, 3 * heads * D], D in %s, q_w <= %d, "
                           "tables [2 * q_h - 1, D] and [2 * q_w - 1, D] or both None)"
                           % (name, _lib.VIT_ATTN_HEAD_DIMS, _lib.VIT_ATTN_TRAIN_MAX_W))
    B, S, E3 = qkv.shape
    return int(q_hw[0]), int(q_hw[1]), B, S, E3 // (3 * num_heads)


def vit_attention_train(qkv, rel_h_table, rel_w_table, num_heads, q_hw, scale):
    """vit_attention for the training route (patch_embed_hip_vit_attn_train_f32): returns (out, lse) with `out` bitwise
    vit_attention's and lse [B' * num_heads, roundup(S, 32)] the row log-sum-exp of the scores, which vit_attention_backward
    takes.  Same arguments, same refusals (and q_w <= 256)."""
    lib = _lib.load()
    q_h, q_w, B, S, D = _vit_train_args("vit_attention_train", qkv, rel_h_table, rel_w_table, num_heads, q_hw)
    out = torch.empty((B, S, num_heads * D), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((B * num_heads, (S + 31) // 32 * 32), dtype=torch.float32, device=qkv.device)
    if B == 0:
        return out, lse
    ws_bytes = int(lib.patch_embed_hip_vit_attn_workspace_bytes(B, num_heads, q_h, q_w, D))
    ws = _workspace(ws_bytes, qkv.device)
    _launch(qkv.device, lib.patch_embed_hip_vit_attn_train_f32, qkv.data_ptr(), _ptr(rel_h_table), _ptr(rel_w_table), B, num_heads, q_h,
            q_w, D, float(scale), out.data_ptr(), lse.data_ptr(), ws.data_ptr(), ws_bytes)
    return out, lse


def vit_attention_backward(qkv, rel_h_table, rel_w_table, out, lse, grad_out, num_heads, q_hw, scale):
    """The backward of vit_attention_train (patch_embed_hip_vit_attn_backward_f32): (grad_qkv, grad_rel_h_table,
    grad_rel_w_table), the table gradients None without tables.  The probabilities are recomputed from qkv and lse tile by tile;
    the [B' * heads, S, S] scores are never written.  Exact fp32, bitwise repeatable.  A grad_out that is not contiguous or not
    16-byte aligned is staged by one copy; the workspace comes from PyTorch's caching allocator for the duration of the call."""
    lib = _lib.load()
    q_h, q_w, B, S, D = _vit_train_args("vit_attention_backward", qkv, rel_h_table, rel_w_table, num_heads, q_hw)
    dev = qkv.device
    _check_f32("out", out, dev, (B, S, num_heads * D), "vit_attention_backward: out must be float32 [B, S, heads * D]")
    _check_f32("lse", lse, dev, (B * num_heads, (S + 31) // 32 * 32), "vit_attention_backward: lse must be float32 [B * heads, roundup(S, 32)]")
    if not (grad_out.is_cuda and grad_out.device == dev and grad_out.dtype == torch.float32 and tuple(grad_out.shape) == tuple(out.shape)):
        raise RuntimeError("vit_attention_backward: grad_out must be float32 [B, S, heads * D] on qkv's device")
    if not grad_out.is_contiguous() or grad_out.data_ptr() % 16 != 0:
        grad_out = grad_out.clone(memory_format=torch.contiguous_format)
    grad_qkv = torch.empty_like(qkv)
    has_rel = rel_h_table is not None
    if B == 0:     # empty gradients for qkv, zero ones for the tables
        return grad_qkv, (torch.zeros_like(rel_h_table) if has_rel else None), (torch.zeros_like(rel_w_table) if has_rel else None)
    grad_th = torch.empty_like(rel_h_table) if has_rel else None
    grad_tw = torch.empty_like(rel_w_table) if has_rel else None
    ws_bytes = int(lib.patch_embed_hip_vit_attn_backward_workspace_bytes(B, num_heads, q_h, q_w, D))
    ws = _workspace(ws_bytes, dev)
    _launch(dev, lib.patch_embed_hip_vit_attn_backward_f32, qkv.data_ptr(), _ptr(rel_h_table), _ptr(rel_w_table), out.data_ptr(),
            lse.data_ptr(), grad_out.data_ptr(), B, num_heads, q_h, q_w, D, float(scale), grad_qkv.data_ptr(), _ptr(grad_th),
            _ptr(grad_tw), ws.data_ptr(), ws_bytes)
    return grad_qkv, grad_th, grad_tw


def bi_attention_supported(q, k, vv, vl, mask, num_heads):
    """True when include/biattn_hip.h has a kernel: contiguous fp32 GPU tensors q, vv [B, S, E] and k, vl [B, T, E] with
    E / num_heads == 256, 1 <= T <= 256, S >= 1, and a mask that is absent, int64 or fp32 [B, T] (contiguous, same device)."""
    ts = (q, k, vv, vl)
    if not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 3 and t.device == q.device for t in ts):
        return False
    B, S, E = q.shape
    T = k.shape[1]
    if tuple(vv.shape) != (B, S, E) or tuple(k.shape) != (B, T, E) or tuple(vl.shape) != (B, T, E):
        return False
    if num_heads <= 0 or E != num_heads * _lib.BIATTN_HEAD_DIM or not (1 <= T <= _lib.BIATTN_MAX_TEXT) or S < 1:
        return False
    if mask is not None and not (mask.dtype in (torch.int64, torch.float32) and mask.is_cuda and mask.device == q.device
                                 and mask.is_contiguous() and tuple(mask.shape) == (B, T)):
        return False
    return True


def _bi_attention_args(name, q, k, vv, vl, mask, num_heads):
    """(B, S, T, head_dim, mask kind of the C ABI), or the one refusal of the three bi-attention wrappers"""
    if not bi_attention_supported(q, k, vv, vl, mask, num_heads):
        raise RuntimeError("%s: unsupported arguments (contiguous fp32 GPU tensors, head_dim 256, "
                           "1 <= T <= 256, mask int64 / fp32 / None)" % name)
    B, S, E = q.shape
    kind = _lib.BIATTN_MASK_NONE if mask is None else (_lib.BIATTN_MASK_INT64 if mask.dtype == torch.int64 else _lib.BIATTN_MASK_F32)
    return B, S, k.shape[1], E // num_heads, kind


def bi_attention_forward(q, k, vv, vl, mask, num_heads, q_scale):
    """The core of BiMultiHeadAttention.forward at inference (include/biattn_hip.h: biattn_hip_forward_f32): q = v_proj(v) (NOT
    scaled) and vv = values_v_proj(v) [B, S, E], k = l_proj(l) and vl = values_l_proj(l) [B, T, E], mask [B, T] int64 / fp32 or
    None.  Returns (out_v [B, S, E], out_l [B, T, E]), token-major, the inputs of out_v_proj / out_l_proj.  Exact fp32, bitwise
    repeatable; the [B * H, S, T] attention matrix is never written.  The workspace comes from PyTorch's caching allocator on
    the current stream for the duration of the call.  Unsupported arguments raise: callers ask bi_attention_supported first."""
    lib = _lib.load()
    B, S, T, D, kind = _bi_attention_args("bi_attention_forward", q, k, vv, vl, mask, num_heads)
    out_v = torch.empty_like(q)
    out_l = torch.empty_like(k)
    if B == 0:
        return out_v, out_l
    ws_bytes = int(lib.biattn_hip_workspace_bytes(B, num_heads, S, T, D))
    ws = _workspace(ws_bytes, q.device)
    _launch(q.device, lib.biattn_hip_forward_f32, q.data_ptr(), k.data_ptr(), vv.data_ptr(), vl.data_ptr(), _ptr(mask), kind,
            B, num_heads, S, T, D, float(q_scale), out_v.data_ptr(), out_l.data_ptr(), ws.data_ptr(), ws_bytes)
    return out_v, out_l


def bi_attention_train_supported(q, k, vv, vl, mask, num_heads):
    """True when the training route (biattn_hip_train_f32 / biattn_hip_backward_f32) covers this core: the inference kernels'
    conditions, and 16-byte aligned tensors."""
    return bi_attention_supported(q, k, vv, vl, mask, num_heads) and all(t.data_ptr() % 16 == 0 for t in (q, k, vv, vl))


def bi_attention_seed(device):
    """The (seed, offset) pair of one dropout draw: two int64 on `device`, drawn ON the device from torch's CUDA generator, so
    torch.cuda.manual_seed governs it, nothing is copied to the host and nothing synchronises; the recompute of
    checkpoint(..., use_reentrant=False), which restores the generator's state, draws the same pair again.  Module-level so
    that a test can replace it."""
    return torch.empty(2, dtype=torch.int64, device=device).random_()


def _bi_attention_dropout(name, dropout_p, seed, dev):
    """The checked (p, seed) of the wrappers below: p in [0, 1), the seed two int64 on `dev`."""
    p = float(dropout_p)
    if not (0.0 <= p < 1.0):
        raise RuntimeError("%s: dropout_p must be in [0, 1)" % name)
    if not (torch.is_tensor(seed) and seed.dtype == torch.int64 and seed.is_cuda and seed.device == dev and seed.is_contiguous()
            and seed.numel() == 2):
        raise RuntimeError("%s: seed must be two contiguous int64 (seed, offset) on q's device" % name)
    return p, seed


def bi_attention_train(q, k, vv, vl, mask, num_heads, q_scale, dropout_p=0.0, seed=None):
    """bi_attention_forward for the training route (biattn_hip_train_f32): returns (out_v, out_l, stat_v, stat_l) with out_v and
    out_l bitwise bi_attention_forward's, stat_v [B * num_heads, 2, roundup(S, 32)] and stat_l [B * num_heads, 2,
    roundup(T, 32)] the maximum and the log of the sum of every softmax row, which bi_attention_backward takes.  Same arguments,
    same refusals.  With a `seed` (bi_attention_seed's two int64 on the device) the call is biattn_hip_train_dropout_f32:
    dropout with probability dropout_p on both attention probabilities, decided inside the kernels; without one dropout_p must
    be 0 and the call is the one above, bit for bit."""
    lib = _lib.load()
    if seed is None and float(dropout_p) != 0.0:
        raise RuntimeError("bi_attention_train: dropout_p > 0 needs a seed (bi_attention_seed)")
    B, S, T, D, kind = _bi_attention_args("bi_attention_train", q, k, vv, vl, mask, num_heads)
    out_v = torch.empty_like(q)
    out_l = torch.empty_like(k)
    stat_v = torch.empty((B * num_heads, 2, (S + 31) // 32 * 32), dtype=torch.float32, device=q.device)
    stat_l = torch.empty((B * num_heads, 2, (T + 31) // 32 * 32), dtype=torch.float32, device=q.device)
    if B == 0:
        return out_v, out_l, stat_v, stat_l
    ws_bytes = int(lib.biattn_hip_workspace_bytes(B, num_heads, S, T, D))
    ws = _workspace(ws_bytes, q.device)
    args = (q.data_ptr(), k.data_ptr(), vv.data_ptr(), vl.data_ptr(), _ptr(mask), kind, B, num_heads, S, T, D, float(q_scale),
            out_v.data_ptr(), out_l.data_ptr(), stat_v.data_ptr(), stat_l.data_ptr(), ws.data_ptr(), ws_bytes)
    if seed is None:
        _launch(q.device, lib.biattn_hip_train_f32, *args)
    else:
        p, seed = _bi_attention_dropout("bi_attention_train", dropout_p, seed, q.device)
        _launch(q.device, lib.biattn_hip_train_dropout_f32, *args, p, seed.data_ptr())
    return out_v, out_l, stat_v, stat_l


def bi_attention_backward(q, k, vv, vl, mask, out_v, out_l, stat_v, stat_l, grad_out_v, grad_out_l, num_heads, q_scale,
                          dropout_p=0.0, seed=None):
    """The backward of bi_attention_train (biattn_hip_backward_f32): (grad_q, grad_k, grad_vv, grad_vl).  Both probabilities are
    recomputed from q, k, the mask and the kept row statistics tile by tile; the [B * H, S, T] matrix is never written and the
    mask gets no gradient.  Exact fp32, bitwise repeatable.  A gradient that is not contiguous or not 16-byte aligned is staged
    by one copy; the workspace comes from PyTorch's caching allocator for the duration of the call.  dropout_p and seed as given
    to bi_attention_train (biattn_hip_backward_dropout_f32): the forward's keep decisions are recomputed, not stored."""
    lib = _lib.load()
    if seed is None and float(dropout_p) != 0.0:
        raise RuntimeError("bi_attention_backward: dropout_p > 0 needs the forward's seed")
    B, S, T, D, kind = _bi_attention_args("bi_attention_backward", q, k, vv, vl, mask, num_heads)
    dev, E = q.device, q.shape[2]
    _check_f32("out_v", out_v, dev, (B, S, E), "bi_attention_backward: out_v must be float32 [B, S, E]")
    _check_f32("out_l", out_l, dev, (B, T, E), "bi_attention_backward: out_l must be float32 [B, T, E]")
    _check_f32("stat_v", stat_v, dev, (B * num_heads, 2, (S + 31) // 32 * 32),
               "bi_attention_backward: stat_v must be float32 [B * heads, 2, roundup(S, 32)]")
    _check_f32("stat_l", stat_l, dev, (B * num_heads, 2, (T + 31) // 32 * 32),
               "bi_attention_backward: stat_l must be float32 [B * heads, 2, roundup(T, 32)]")
    grads = []
    for name, g, ref in (("grad_out_v", grad_out_v, out_v), ("grad_out_l", grad_out_l, out_l)):
        if not (g.is_cuda and g.device == dev and g.dtype == torch.float32 and tuple(g.shape) == tuple(ref.shape)):
            raise RuntimeError("bi_attention_backward: %s must be float32 of its output's shape on q's device" % name)
        if not g.is_contiguous() or g.data_ptr() % 16 != 0:
            g = g.clone(memory_format=torch.contiguous_format)
        grads.append(g)
    grad_q, grad_vv = torch.empty_like(q), torch.empty_like(vv)
    grad_k, grad_vl = torch.empty_like(k), torch.empty_like(vl)
    if B == 0:
        return grad_q, grad_k, grad_vv, grad_vl
    ws_bytes = int(lib.biattn_hip_backward_workspace_bytes(B, num_heads, S, T, D))
    ws = _workspace(ws_bytes, dev)
    args = (q.data_ptr(), k.data_ptr(), vv.data_ptr(), vl.data_ptr(), _ptr(mask), kind, out_v.data_ptr(), out_l.data_ptr(),
            stat_v.data_ptr(), stat_l.data_ptr(), grads[0].data_ptr(), grads[1].data_ptr(), B, num_heads, S, T, D, float(q_scale),
            grad_q.data_ptr(), grad_k.data_ptr(), grad_vv.data_ptr(), grad_vl.data_ptr(), ws.data_ptr(), ws_bytes)
    if seed is None:
        _launch(dev, lib.biattn_hip_backward_f32, *args)
    else:
        p, seed = _bi_attention_dropout("bi_attention_backward", dropout_p, seed, dev)
        _launch(dev, lib.biattn_hip_backward_dropout_f32, *args, p, seed.data_ptr())
    return grad_q, grad_k, grad_vv, grad_vl


def bi_attention_dropout_keep(seed, p, B, H, S, T):
    """FOR TESTS AND TOOLS (biattn_hip_dropout_keep_u8): the keep decisions of bi_attention_train's dropout for `seed` written
    out, (keep_v [B * H, S, T], keep_l [B * H, T, S]) uint8 with 1 = kept -- the only place where a mask of full size exists."""
    lib = _lib.load()
    p, seed = _bi_attention_dropout("bi_attention_dropout_keep", p, seed, seed.device if torch.is_tensor(seed) else None)
    keep_v = torch.empty((B * H, S, T), dtype=torch.uint8, device=seed.device)
    keep_l = torch.empty((B * H, T, S), dtype=torch.uint8, device=seed.device)
    if B * H == 0:
        return keep_v, keep_l
    _launch(seed.device, lib.biattn_hip_dropout_keep_u8, seed.data_ptr(), p, B, H, S, T, keep_v.data_ptr(), keep_l.data_ptr())
    return keep_v, keep_l


def _dec_attn_view(t):
    """[B, L, E] fp32 GPU view whose last dimension is contiguous and whose batches lie L rows apart, as the C ABI reads it."""
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 3):
        return False
    B, L, E = t.shape
    s = _dec_attn_stride(t)
    return ((E == 1 or t.stride(2) == 1) and ((L == 1 and B <= 1) or (s >= E and s % 4 == 0))
            and (B <= 1 or t.stride(0) == L * s) and t.data_ptr() % 16 == 0)


def _dec_attn_stride(t):
    B, L, E = t.shape
    if L > 1:
        return t.stride(1)
    return t.stride(0) if B > 1 else max(E, 4)   # one row a batch: the batches' distance; one row in all: no stride to speak of


def decoder_self_attention_supported(q, k, v, num_heads, attn_mask):
    """True when biattn_hip_self_forward_f32 (include/biattn_hip.h) covers this self-attention core: q, k, v fp32 GPU views
    [B, L, E] of one device with a contiguous last dimension (row strides multiples of 4, 16-byte aligned), E / num_heads == 32,
    1 <= L <= 65535, and a mask that is absent or a contiguous [L, L] bool or fp32 tensor on that device."""
    if not all(_dec_attn_view(t) and t.device == q.device and t.shape == q.shape for t in (q, k, v)):
        return False
    B, L, E = q.shape
    if num_heads <= 0 or E != num_heads * _lib.DEC_ATTN_HEAD_DIM or not (1 <= L <= _lib.DEC_ATTN_MAX_LEN):
        return False
    if B * num_heads * ((L + 31) // 32) >= 1 << 31 or any(B * L * _dec_attn_stride(t) >= 1 << 42 for t in (q, k, v)):
        return False
    if attn_mask is not None and not (attn_mask.dtype in (torch.bool, torch.float32) and attn_mask.is_cuda
                                      and attn_mask.device == q.device and attn_mask.is_contiguous()
                                      and tuple(attn_mask.shape) == (L, L)):
        return False
    return True


def _dec_attn_args(name, q, k, v, num_heads, attn_mask):
    """(B, L, E, head_dim), or the one refusal of the three decoder attention wrappers"""
    if not decoder_self_attention_supported(q, k, v, num_heads, attn_mask):
        raise RuntimeError("%s: unsupported arguments (fp32 GPU views [B, L, heads * 32] with a contiguous last dimension, "
                           "1 <= L <= 65535, mask [L, L] bool / fp32 / None)" % name)
    B, L, E = q.shape
    return B, L, E, E // num_heads


def _dec_attn_mask(attn_mask, dev):
    """(mask kind of the C ABI, the tensor whose address goes with it)"""
    if attn_mask is None:
        return _lib.BIATTN_MASK_NONE, None
    if attn_mask.dtype == torch.bool:
        return _lib.BIATTN_MASK_BOOL, attn_mask.view(torch.uint8)     # the same bytes
    _check_f32("attn_mask", attn_mask, dev)
    return _lib.BIATTN_MASK_F32, attn_mask


def decoder_self_attention(q, k, v, num_heads, attn_mask=None, q_scale=None):
    """The core of nn.MultiheadAttention among the decoder's queries at inference (include/biattn_hip.h:
    biattn_hip_self_forward_f32): q, k, v [B, L, E] are the three input projections (q NOT scaled; views of a wider projection
    output are read in place), attn_mask [L, L] bool (True = may not attend) or fp32 (added; may hold -inf) or None, q_scale
    head_dim ** -0.5 unless given.  Returns [B, L, E], token-major, the input of out_proj.  Exact fp32, bitwise repeatable; the
    [B * heads, L, L] attention matrix is never written.  A query with every key excluded is NaN, as in PyTorch.  Unsupported
    arguments raise: callers ask decoder_self_attention_supported first."""
    lib = _lib.load()
    B, L, E, D = _dec_attn_args("decoder_self_attention", q, k, v, num_heads, attn_mask)
    out = torch.empty((B, L, E), dtype=torch.float32, device=q.device)
    if B == 0:
        return out
    kind, mask = _dec_attn_mask(attn_mask, q.device)
    scale = float(D) ** -0.5 if q_scale is None else float(q_scale)
    _launch(q.device, lib.biattn_hip_self_forward_f32, q.data_ptr(), k.data_ptr(), v.data_ptr(), _dec_attn_stride(q),
            _dec_attn_stride(k), _dec_attn_stride(v), _ptr(mask), kind, B, num_heads, L, D, scale, out.data_ptr())
    return out


def _bert_mask(mask, B, T, dev):
    """(mask kind of the C ABI, the tensor whose address goes with it) of a keep mask, or None for one without a kernel:
    None, [B, T] int64 / bool / uint8, or [B, T, T] bool / uint8 indexed [b, query, key]; contiguous, on `dev`."""
    if mask is None:
        return _lib.BERT_MASK_NONE, None
    if not (mask.is_cuda and mask.device == dev and mask.is_contiguous()):
        return None
    byte = mask.dtype in (torch.bool, torch.uint8)
    if tuple(mask.shape) == (B, T) and mask.dtype == torch.int64:
        return _lib.BERT_MASK_KEY_I64, mask
    if tuple(mask.shape) == (B, T) and byte:
        return _lib.BERT_MASK_KEY_U8, mask.view(torch.uint8)          # the same bytes
    if tuple(mask.shape) == (B, T, T) and byte:
        return _lib.BERT_MASK_FULL_U8, mask.view(torch.uint8)
    return None


def bert_self_attention_supported(q, k, v, num_heads, mask):
    """True when bert_hip_self_attention_f32 (include/dynmask_hip.h) covers this core: q, k, v fp32 GPU views [B, T, E] of one
    device with a contiguous last dimension (row strides multiples of 4, 16-byte aligned), E / num_heads == 64, 1 <= T <= 512,
    and a keep mask that _bert_mask knows."""
    if not all(_dec_attn_view(t) and t.device == q.device and t.shape == q.shape for t in (q, k, v)):
        return False
    B, T, E = q.shape
    if num_heads <= 0 or E != num_heads * _lib.BERT_HEAD_DIM or not (1 <= T <= _lib.BERT_MAX_LEN):
        return False
    if B * num_heads * ((T + 31) // 32) >= 1 << 31 or any(B * T * _dec_attn_stride(t) >= 1 << 42 for t in (q, k, v)):
        return False
    return _bert_mask(mask, B, T, q.device) is not None


def bert_self_attention(q, k, v, num_heads, mask=None, q_scale=None):
    """The core of BertSelfAttention at inference (include/dynmask_hip.h: bert_hip_self_attention_f32): q, k, v [B, T, E] are
    the three projections (q NOT scaled; views of one [B, T, 3 E] projection output are read in place), mask a KEEP mask (see
    _bert_mask; non-zero = the key takes part), q_scale head_dim ** -0.5 unless given.  Returns [B, T, E], token-major, the input
    of attention.output.dense.  Exact fp32, bitwise repeatable; the [B * heads, T, T] matrix is never written.  A query that
    keeps no key is a row of zeros.  Unsupported arguments raise: callers ask bert_self_attention_supported first."""
    lib = _lib.load()
    if not bert_self_attention_supported(q, k, v, num_heads, mask):
        raise RuntimeError("bert_self_attention: unsupported arguments (fp32 GPU views [B, T, heads * 64] with a contiguous last "
                           "dimension, 1 <= T <= 512, keep mask [B, T] int64 / bool / uint8, [B, T, T] bool / uint8 or None)")
    B, T, E = q.shape
    out = torch.empty((B, T, E), dtype=torch.float32, device=q.device)
    if B == 0:
        return out
    kind, m = _bert_mask(mask, B, T, q.device)
    D = E // num_heads
    scale = float(D) ** -0.5 if q_scale is None else float(q_scale)
    _launch(q.device, lib.bert_hip_self_attention_f32, q.data_ptr(), k.data_ptr(), v.data_ptr(), _dec_attn_stride(q),
            _dec_attn_stride(k), _dec_attn_stride(v), _ptr(m), kind, B, num_heads, T, D, scale, out.data_ptr())
    return out


def bert_self_attention_train_supported(q, k, v, num_heads, mask, dropout_p=0.0):
    """True when the training route (bert_hip_self_attention_train_f32 / bert_hip_self_attention_backward_f32) covers this
    core: the inference kernel's conditions, a dropout probability in [0, 1) and, with dropout, B * num_heads <= 65535."""
    p = float(dropout_p)
    if not (0.0 <= p < 1.0) or not bert_self_attention_supported(q, k, v, num_heads, mask):
        return False
    return p == 0.0 or q.shape[0] * num_heads <= _lib.BERT_DROPOUT_MAX_BH


def _bert_train_args(name, q, k, v, num_heads, mask, dropout_p, seed):
    """(B, T, E, mask kind, mask tensor, p, seed or None), or the one refusal of the training wrappers"""
    if not bert_self_attention_train_supported(q, k, v, num_heads, mask, dropout_p):
        raise RuntimeError("%s: unsupported arguments (fp32 GPU views [B, T, heads * 64] with a contiguous last dimension, "
                           "1 <= T <= 512, keep mask [B, T] int64 / bool / uint8, [B, T, T] bool / uint8 or None, dropout_p in "
                           "[0, 1), B * heads <= 65535 with dropout)" % name)
    p = float(dropout_p)
    if seed is None:
        if p != 0.0:
            raise RuntimeError("%s: dropout_p > 0 needs a seed (bi_attention_seed)" % name)
    else:
        p, seed = _bi_attention_dropout(name, p, seed, q.device)
    B, T, E = q.shape
    kind, m = _bert_mask(mask, B, T, q.device)
    return B, T, E, kind, m, p, seed


def bert_self_attention_train(q, k, v, num_heads, mask=None, q_scale=None, dropout_p=0.0, seed=None):
    """bert_self_attention for the training route (bert_hip_self_attention_train_f32): returns (out, lse) with lse
    [B * num_heads, roundup(T, 32)] the row log-sum-exp of the scaled scores over the kept keys (-inf for a query that keeps no
    key, 0 past T), which bert_self_attention_backward takes.  With dropout_p > 0 the attention dropout is decided inside the
    kernel from `seed` (bi_attention_seed's two int64 on the device) and applied after the normalisation; with dropout_p == 0
    `out` is bitwise bert_self_attention's, with or without a seed.  Same arguments, same refusals."""
    lib = _lib.load()
    B, T, E, kind, m, p, seed = _bert_train_args("bert_self_attention_train", q, k, v, num_heads, mask, dropout_p, seed)
    out = torch.empty((B, T, E), dtype=torch.float32, device=q.device)
    lse = torch.empty((B * num_heads, (T + 31) // 32 * 32), dtype=torch.float32, device=q.device)
    if B == 0:
        return out, lse
    D = E // num_heads
    scale = float(D) ** -0.5 if q_scale is None else float(q_scale)
    _launch(q.device, lib.bert_hip_self_attention_train_f32, q.data_ptr(), k.data_ptr(), v.data_ptr(), _dec_attn_stride(q),
            _dec_attn_stride(k), _dec_attn_stride(v), _ptr(m), kind, B, num_heads, T, D, scale, out.data_ptr(), lse.data_ptr(), p,
            _ptr(seed))
    return out, lse


def bert_self_attention_backward(q, k, v, out, lse, grad_out, num_heads, mask=None, q_scale=None, dropout_p=0.0, seed=None):
    """The backward of bert_self_attention_train (bert_hip_self_attention_backward_f32): ONE [B, T, 3 E] tensor that carries
    dq | dk | dv when q, k and v are the three thirds of one [B, T, 3 E] tensor (as the layer's projection gives them), else
    (grad_q, grad_k, grad_v).  The probabilities and the forward's keep decisions are recomputed from q, k, the mask, lse and the
    seed tile by tile; no [B * heads, T, T] tensor is written, and the mask gets no gradient.  Exact fp32, bitwise repeatable.
    A query that keeps no key gets a zero row in grad_q and adds nothing to grad_k and grad_v; an excluded key gets zero rows
    (include/dynmask_hip.h).  A grad_out that is not contiguous or not 16-byte aligned is staged by one copy; the workspace comes
    from PyTorch's caching allocator for the duration of the call."""
    lib = _lib.load()
    B, T, E, kind, m, p, seed = _bert_train_args("bert_self_attention_backward", q, k, v, num_heads, mask, dropout_p, seed)
    dev = q.device
    _check_f32("out", out, dev, (B, T, E), "bert_self_attention_backward: out must be float32 [B, T, heads * 64]")
    _check_f32("lse", lse, dev, (B * num_heads, (T + 31) // 32 * 32),
               "bert_self_attention_backward: lse must be float32 [B * heads, roundup(T, 32)]")
    if not (grad_out.is_cuda and grad_out.device == dev and grad_out.dtype == torch.float32 and tuple(grad_out.shape) == (B, T, E)):
        raise RuntimeError("bert_self_attention_backward: grad_out must be float32 [B, T, heads * 64] on q's device")
    if not grad_out.is_contiguous() or grad_out.data_ptr() % 16 != 0:
        grad_out = grad_out.clone(memory_format=torch.contiguous_format)
    thirds = (q.untyped_storage().data_ptr() == k.untyped_storage().data_ptr() == v.untyped_storage().data_ptr()
              and k.data_ptr() == q.data_ptr() + 4 * E and v.data_ptr() == q.data_ptr() + 8 * E
              and all(_dec_attn_stride(t) == 3 * E for t in (q, k, v)))
    if thirds:
        result = torch.empty((B, T, 3 * E), dtype=torch.float32, device=dev)
        grads = (result[..., :E], result[..., E:2 * E], result[..., 2 * E:])
        stride = 3 * E
    else:
        result = grads = tuple(torch.empty((B, T, E), dtype=torch.float32, device=dev) for _ in range(3))
        stride = E
    if B == 0:
        return result
    D = E // num_heads
    scale = float(D) ** -0.5 if q_scale is None else float(q_scale)
    ws_bytes = int(lib.bert_hip_self_attention_backward_workspace_bytes(B, num_heads, T, D))
    ws = _workspace(ws_bytes, dev)
    _launch(dev, lib.bert_hip_self_attention_backward_f32, q.data_ptr(), k.data_ptr(), v.data_ptr(), _dec_attn_stride(q),
            _dec_attn_stride(k), _dec_attn_stride(v), _ptr(m), kind, out.data_ptr(), lse.data_ptr(), grad_out.data_ptr(), B, num_heads,
            T, D, scale, grads[0].data_ptr(), grads[1].data_ptr(), grads[2].data_ptr(), stride, stride, stride, ws.data_ptr(), ws_bytes,
            p, _ptr(seed))
    return result


def bert_dropout_keep(seed, p, B, H, T):
    """FOR TESTS AND TOOLS (bert_hip_dropout_keep_u8): the keep decisions of bert_self_attention_train's dropout for `seed`
    written out, [B * H, T, T] uint8 indexed [b * H + h, query, key] with 1 = kept -- the only place where a mask of full size
    exists."""
    lib = _lib.load()
    p, seed = _bi_attention_dropout("bert_dropout_keep", p, seed, seed.device if torch.is_tensor(seed) else None)
    keep = torch.empty((B * H, T, T), dtype=torch.uint8, device=seed.device)
    if B * H == 0:
        return keep
    _launch(seed.device, lib.bert_hip_dropout_keep_u8, seed.data_ptr(), p, B, H, T, keep.data_ptr())
    return keep


def bert_embed_layernorm_supported(input_ids, token_type_ids, word, position, type_table, ln_weight, ln_bias):
    """True when bert_hip_embed_layernorm_f32 covers these embeddings: ids (and type ids, if given) contiguous int64 [B, T] on
    the GPU, contiguous fp32 tables of one hidden size (a multiple of 4, at most 4096) there, T within the position table."""
    if not (input_ids.is_cuda and input_ids.dtype == torch.int64 and input_ids.dim() == 2 and input_ids.is_contiguous()):
        return False
    dev = input_ids.device
    if token_type_ids is not None and not (token_type_ids.dtype == torch.int64 and token_type_ids.device == dev
                                           and token_type_ids.shape == input_ids.shape and token_type_ids.is_contiguous()):
        return False
    tables = (word, position, type_table)
    if not all(t.dim() == 2 and t.dtype == torch.float32 and t.device == dev and t.is_contiguous() for t in tables):
        return False
    H = word.shape[1]
    if not all(t.shape[1] == H for t in tables) or H % 4 != 0 or not (0 < H <= _lib.BERT_MAX_HIDDEN):
        return False
    if not all(t is not None and t.dtype == torch.float32 and t.device == dev and tuple(t.shape) == (H,) and t.is_contiguous()
               for t in (ln_weight, ln_bias)):
        return False
    return 1 <= input_ids.shape[1] <= position.shape[0] and all(t.shape[0] < 1 << 31 for t in tables)


def bert_embed_layernorm(input_ids, token_type_ids, word, position, type_table, ln_weight, ln_bias, eps):
    """BertEmbeddings at inference in one launch (include/dynmask_hip.h: bert_hip_embed_layernorm_f32):
    LayerNorm(word[ids] + type[token_type_ids] + position[t]) -> [B, T, hidden]; token_type_ids None = type 0.  A row whose id is
    out of range is NaN.  Unsupported arguments raise: callers ask bert_embed_layernorm_supported first."""
    lib = _lib.load()
    if not bert_embed_layernorm_supported(input_ids, token_type_ids, word, position, type_table, ln_weight, ln_bias):
        raise RuntimeError("bert_embed_layernorm: unsupported arguments (int64 GPU ids [B, T], contiguous fp32 tables of one hidden "
                           "size that is a multiple of 4 and at most 4096, T within the position table)")
    B, T = input_ids.shape
    H = word.shape[1]
    out = torch.empty((B, T, H), dtype=torch.float32, device=input_ids.device)
    if B == 0:
        return out
    _launch(input_ids.device, lib.bert_hip_embed_layernorm_f32, input_ids.data_ptr(), _ptr(token_type_ids), word.data_ptr(),
            position.data_ptr(), type_table.data_ptr(), ln_weight.data_ptr(), ln_bias.data_ptr(), float(eps), B, T, H, word.shape[0],
            position.shape[0], type_table.shape[0], out.data_ptr())
    return out


def decoder_self_attention_train_supported(q, k, v, num_heads, attn_mask):
    """True when the training route (biattn_hip_self_train_f32 / biattn_hip_self_backward_f32) covers this core: the inference
    kernel's conditions, which are the training kernels' too."""
    return decoder_self_attention_supported(q, k, v, num_heads, attn_mask)


def decoder_self_attention_train(q, k, v, num_heads, attn_mask=None, q_scale=None):
    """decoder_self_attention for the training route (biattn_hip_self_train_f32): returns (out, lse) with `out` bitwise
    decoder_self_attention's and lse [B * num_heads, roundup(L, 32)] the row log-sum-exp of the masked scores (-inf for a query
    with every key excluded), which decoder_self_attention_backward takes.  Same arguments, same refusals."""
    lib = _lib.load()
    B, L, E, D = _dec_attn_args("decoder_self_attention_train", q, k, v, num_heads, attn_mask)
    out = torch.empty((B, L, E), dtype=torch.float32, device=q.device)
    lse = torch.empty((B * num_heads, (L + 31) // 32 * 32), dtype=torch.float32, device=q.device)
    if B == 0:
        return out, lse
    kind, mask = _dec_attn_mask(attn_mask, q.device)
    scale = float(D) ** -0.5 if q_scale is None else float(q_scale)
    _launch(q.device, lib.biattn_hip_self_train_f32, q.data_ptr(), k.data_ptr(), v.data_ptr(), _dec_attn_stride(q),
            _dec_attn_stride(k), _dec_attn_stride(v), _ptr(mask), kind, B, num_heads, L, D, scale, out.data_ptr(), lse.data_ptr())
    return out, lse


def decoder_self_attention_backward(q, k, v, out, lse, grad_out, num_heads, attn_mask=None, q_scale=None):
    """The backward of decoder_self_attention_train (biattn_hip_self_backward_f32): (grad_qk, grad_v) with grad_qk ONE
    [B, L, 2 E] tensor that carries dq | dk when q and k are the two halves of one [B, L, 2 E] tensor (as the layer's q | k
    projection gives them), else (grad_q, grad_k, grad_v).  The probabilities are recomputed from q, k, the mask and lse tile by
    tile; the [B * heads, L, L] scores are never written, and the mask gets no gradient.  Exact fp32, bitwise repeatable.  A
    query with every key excluded gets a NaN row in grad_q and adds nothing to grad_k and grad_v (include/biattn_hip.h).  A
    grad_out that is not contiguous or not 16-byte aligned is staged by one copy; the workspace comes from PyTorch's caching
    allocator for the duration of the call."""
    lib = _lib.load()
    B, L, E, D = _dec_attn_args("decoder_self_attention_backward", q, k, v, num_heads, attn_mask)
    dev = q.device
    _check_f32("out", out, dev, (B, L, E), "decoder_self_attention_backward: out must be float32 [B, L, heads * 32]")
    _check_f32("lse", lse, dev, (B * num_heads, (L + 31) // 32 * 32),
               "decoder_self_attention_backward: lse must be float32 [B * heads, roundup(L, 32)]")
    if not (grad_out.is_cuda and grad_out.device == dev and grad_out.dtype == torch.float32 and tuple(grad_out.shape) == (B, L, E)):
        raise RuntimeError("decoder_self_attention_backward: grad_out must be float32 [B, L, heads * 32] on q's device")
    if not grad_out.is_contiguous() or grad_out.data_ptr() % 16 != 0:
        grad_out = grad_out.clone(memory_format=torch.contiguous_format)
    halves = (q.untyped_storage().data_ptr() == k.untyped_storage().data_ptr() and k.data_ptr() == q.data_ptr() + 4 * E
              and _dec_attn_stride(q) == 2 * E and _dec_attn_stride(k) == 2 * E)
    grad_v = torch.empty((B, L, E), dtype=torch.float32, device=dev)
    if halves:
        grad_qk = torch.empty((B, L, 2 * E), dtype=torch.float32, device=dev)
        grad_q, grad_k = grad_qk[..., :E], grad_qk[..., E:]
        gq_stride = gk_stride = 2 * E
    else:
        grad_q, grad_k = torch.empty_like(grad_v), torch.empty_like(grad_v)
        gq_stride = gk_stride = E
    result = (grad_qk, grad_v) if halves else (grad_q, grad_k, grad_v)
    if B == 0:
        return result
    kind, mask = _dec_attn_mask(attn_mask, dev)
    scale = float(D) ** -0.5 if q_scale is None else float(q_scale)
    ws_bytes = int(lib.biattn_hip_self_backward_workspace_bytes(B, num_heads, L, D))
    ws = _workspace(ws_bytes, dev)
    _launch(dev, lib.biattn_hip_self_backward_f32, q.data_ptr(), k.data_ptr(), v.data_ptr(), _dec_attn_stride(q), _dec_attn_stride(k),
            _dec_attn_stride(v), _ptr(mask), kind, out.data_ptr(), lse.data_ptr(), grad_out.data_ptr(), B, num_heads, L, D, scale,
            grad_q.data_ptr(), grad_k.data_ptr(), grad_v.data_ptr(), gq_stride, gk_stride, E, ws.data_ptr(), ws_bytes)
    return result


def conv3x3_supported(x, weight):
    """True when include/conv3x3_hip.h has a kernel: fp32 GPU tensors, weight [cout, cin, 3, 3], 9 * cin % 16 == 0."""
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.dim() == 4
            and weight.dim() == 4 and tuple(weight.shape[2:]) == (3, 3) and x.shape[1] == weight.shape[1]
            and (9 * weight.shape[1]) % 16 == 0)


def conv3x3_forward(x, weight, bias=None, relu=False, precision=0):
    """3x3 convolution, stride 1, zero padding 1, + bias (+ ReLU) on the matrix cores: the
    `F.relu(self.layN(x))` steps of MaskHeadSmallConv.forward (ddetrs_dn.py:991-1025).  NCHW in, NCHW out; forward
    only (inference).  precision 0: exact fp32 MFMA; 1: split-bf16 products with fp32 accumulation (~2e-5 of the
    output scale, see include/conv3x3_hip.h)."""
    lib = _lib.load()
    _check_conv_args(x, weight, bias)
    if x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or x.shape[1] != weight.shape[1]:
        raise RuntimeError("conv3x3_forward: expected x [B, C, H, W] and weight [E, C, 3, 3]")
    if bias is not None and bias.shape != (weight.shape[0],):
        raise RuntimeError("conv3x3_forward: bias must be [E]")
    B, C, H, W = x.shape
    E = weight.shape[0]
    out = torch.empty((B, E, H, W), dtype=torch.float32, device=x.device)
    _launch(x.device, lib.conv3x3_hip_f32, x.data_ptr(), weight.data_ptr(), _ptr(bias), B, C, H, W, E, int(bool(relu)),
            int(precision), out.data_ptr())
    return out


def conv3x3_pack_weight(weight, exact=False):
    """Split + re-order a [cout, cin, 3, 3] fp32 GPU weight once for conv3x3_packed_forward (cin % 16 == 0).
    exact: the fp32 re-ordering of the exact kernel (conv3x3_hip_pack_weight_exact_f32) instead of the bf16 hi / lo split.
    Returns an opaque uint8 tensor on the same device."""
    lib = _lib.load()
    return _pack_weight(weight, weight.dim() == 4 and tuple(weight.shape[2:]) == (3, 3), tuple(weight.shape[:2]),
                        lib.conv3x3_hip_packed_exact_weight_bytes if exact else lib.conv3x3_hip_packed_weight_bytes,
                        lib.conv3x3_hip_pack_weight_exact_f32 if exact else lib.conv3x3_hip_pack_weight_f32,
                        "conv3x3_pack_weight: expected a float32 [cout, cin, 3, 3] weight",
                        "conv3x3_pack_weight: cin must be a multiple of 16")


def conv3x3_packed_forward(x, packed, cout, bias=None, relu=False, exact=False):
    """3x3 / padding 1 convolution + bias (+ ReLU) from weights prepared by conv3x3_pack_weight: split-bf16 products
    with fp32 accumulation (~2e-5 of the output scale), or -- exact=True, weights packed with exact=True -- exact fp32 products
    on v_mfma_f32_32x32x2_f32; both halo-tiled (include/conv3x3_hip.h)."""
    lib = _lib.load()
    nbytes_fn = lib.conv3x3_hip_packed_exact_weight_bytes if exact else lib.conv3x3_hip_packed_weight_bytes
    run = lib.conv3x3_hip_packed_exact_f32 if exact else lib.conv3x3_hip_packed_f32
    _check("x", x, x.device)
    _check("packed", packed, x.device)
    _check_f32("bias", bias, x.device, (cout,), "conv3x3_packed_forward: bias must be float32 [cout]")
    if x.dtype != torch.float32 or x.dim() != 4:
        raise RuntimeError("conv3x3_packed_forward: expected a float32 x [B, C, H, W]")
    B, C, H, W = x.shape
    if packed.dtype != torch.uint8 or packed.numel() != nbytes_fn(int(cout), C):
        raise RuntimeError("conv3x3_packed_forward: `packed` does not belong to a [%d, %d, 3, 3] weight" % (cout, C))
    out = torch.empty((B, int(cout), H, W), dtype=torch.float32, device=x.device)
    _launch(x.device, run, x.data_ptr(), packed.data_ptr(), _ptr(bias), B, C, H, W, int(cout), int(bool(relu)), out.data_ptr())
    return out


def conv3x3_pack_weight_dgrad(weight):
    """Re-order a [cout, cin, 3, 3] fp32 GPU weight once for the grad-input half of conv3x3_backward: the transposed, flipped
    weights W'[c, n, ky, kx] = W[n, c, 2 - ky, 2 - kx] in the exact forward kernel's layout, cout padded to a multiple of 16
    (conv3x3_hip_pack_weight_exact_dgrad_f32).  Opaque uint8 tensor on the same device."""
    lib = _lib.load()
    return _pack_weight(weight, weight.dim() == 4 and tuple(weight.shape[2:]) == (3, 3), tuple(weight.shape[:2]),
                        lib.conv3x3_hip_packed_exact_dgrad_weight_bytes, lib.conv3x3_hip_pack_weight_exact_dgrad_f32,
                        "conv3x3_pack_weight_dgrad: expected a float32 [cout, cin, 3, 3] weight")


def conv3x3_backward(x, packed_dgrad, out, grad_out, cout, relu=True, need_input=True, need_weight=True, need_bias=True):
    """Backward of `relu(conv3x3(x, W) + bias)` (include/conv3x3_hip.h: conv3x3_hip_backward_exact_f32): exact fp32, fixed
    order, bitwise repeatable.  x [B, cin, H, W]; out / grad_out [B, cout, H, W] (out is read only when relu);
    packed_dgrad from conv3x3_pack_weight_dgrad (needed only for need_input).  Returns (grad_x, grad_weight [cout, cin, 3, 3],
    grad_bias [cout]); a part that is not needed is None and its kernels are not launched.  The workspace comes from
    PyTorch's caching allocator for the duration of the call."""
    lib = _lib.load()
    dev = grad_out.device
    _check("grad_out", grad_out, dev)
    if x.dim() != 4 or grad_out.dim() != 4 or x.dtype != torch.float32 or grad_out.dtype != torch.float32:
        raise RuntimeError("conv3x3_backward: expected float32 x [B, C, H, W] and grad_out [B, cout, H, W]")
    B, C, H, W = x.shape
    cout = int(cout)
    if tuple(grad_out.shape) != (B, cout, H, W):
        raise RuntimeError("conv3x3_backward: grad_out must be [%d, %d, %d, %d]" % (B, cout, H, W))
    if need_weight:
        _check("x", x, dev)
    if relu:
        _check_f32("out", out, dev, (B, cout, H, W), "conv3x3_backward: out must be float32 like grad_out")
    if need_input:
        _check("packed_dgrad", packed_dgrad, dev)
        if packed_dgrad.dtype != torch.uint8 or packed_dgrad.numel() != lib.conv3x3_hip_packed_exact_dgrad_weight_bytes(cout, C):
            raise RuntimeError("conv3x3_backward: `packed_dgrad` does not belong to a [%d, %d, 3, 3] weight" % (cout, C))
    g_in = torch.empty_like(x) if need_input else None
    g_w = torch.empty((cout, C, 3, 3), dtype=torch.float32, device=dev) if need_weight else None
    g_b = torch.empty((cout,), dtype=torch.float32, device=dev) if need_bias else None
    ws_bytes = int(lib.conv3x3_hip_backward_workspace_bytes(B, C, H, W, cout))
    ws = _workspace(ws_bytes, dev)
    _launch(dev, lib.conv3x3_hip_backward_exact_f32, _ptr(x if need_weight else None), _ptr(packed_dgrad if need_input else None),
            _ptr(out if relu else None), grad_out.data_ptr(), B, C, H, W, cout, int(bool(relu)), _ptr(g_in), _ptr(g_w), _ptr(g_b),
            ws.data_ptr(), ws_bytes)
    return g_in, g_w, g_b


def patch_embed_packed_supported(weight):
    """True when the split-bf16 packed path of include/patch_embed_hip.h covers this [E, C, k, k] weight."""
    return (weight.dim() == 4 and weight.shape[2] == weight.shape[3] and
            _lib.load().patch_embed_hip_packed_weight_bytes(weight.shape[0], weight.shape[1], weight.shape[2]) > 0)


def patch_embed_pack_weight(weight):
    """Split + re-order an [E, C, k, k] fp32 GPU weight once for patch_embed_packed_forward.  Opaque uint8 tensor."""
    lib = _lib.load()
    return _pack_weight(weight, weight.dim() == 4 and weight.shape[2] == weight.shape[3], tuple(weight.shape[:3]),
                        lib.patch_embed_hip_packed_weight_bytes, lib.patch_embed_hip_pack_weight_f32,
                        "patch_embed_pack_weight: expected a float32 [E, C, k, k] weight",
                        "patch_embed_pack_weight: needs k in {2, 4, 8, 16} and C * k * k a multiple of 48")


def patch_embed_packed_forward(x, packed, embed_dim, patch, bias=None, channels_last=True):
    """patch_embed_forward with split-bf16 products (~2e-5 of the output scale) from weights prepared by
    patch_embed_pack_weight."""
    lib = _lib.load()
    _check("x", x, x.device)
    _check("packed", packed, x.device)
    if x.dtype != torch.float32 or x.dim() != 4:
        raise RuntimeError("patch_embed_packed_forward: expected a float32 x [B, C, H, W]")
    B, C, H, W = x.shape
    E, k = int(embed_dim), int(patch)
    _check_f32("bias", bias, x.device, (E,), "patch_embed_packed_forward: bias must be float32 [E]")
    if packed.dtype != torch.uint8 or packed.numel() == 0 or packed.numel() != lib.patch_embed_hip_packed_weight_bytes(E, C, k):
        raise RuntimeError("patch_embed_packed_forward: `packed` does not belong to a [%d, %d, %d, %d] weight" % (E, C, k, k))
    shape = (B, H // k, W // k, E) if channels_last else (B, E, H // k, W // k)
    out = torch.empty(shape, dtype=torch.float32, device=x.device)
    _launch(x.device, lib.patch_embed_hip_packed_f32, x.data_ptr(), packed.data_ptr(), _ptr(bias), B, C, H, W, E, k,
            int(bool(channels_last)), out.data_ptr())
    return out


def linear_packed_supported(x, weight):
    """True when include/linear_hip.h covers `F.linear(x, weight)`: fp32 GPU tensors, in_features % 64 == 0."""
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and weight.dim() == 2
            and x.shape[-1] == weight.shape[1] and weight.shape[1] % 64 == 0)


def linear_pack_weight(weight):
    """Split + re-order an [out_features, in_features] fp32 GPU weight once for linear_packed_forward."""
    lib = _lib.load()
    return _pack_weight(weight, weight.dim() == 2, tuple(weight.shape), lib.linear_hip_packed_weight_bytes,
                        lib.linear_hip_pack_weight_f32, "linear_pack_weight: expected a float32 [out_features, in_features] weight",
                        "linear_pack_weight: in_features must be a multiple of 64")


def linear_packed_split_forward(x, packed, split_col, out_features, bias=None, x_add=None):
    """Two Linear layers on the same input as one product (include/linear_hip.h: linear_hip_packed_split_f32): `packed`
    belongs to the row-wise concatenation [W_a; W_b] ([out_features, in_features]), `bias` to the concatenated biases;
    returns (x' W_a^T + b_a  [..., split_col],  x' W_b^T + b_b  [..., out_features - split_col]) with x' = x + x_add."""
    lib = _lib.load()
    _check("x", x, x.device)
    _check("packed", packed, x.device)
    if x.dtype != torch.float32 or x.dim() < 1:
        raise RuntimeError("linear_packed_split_forward: expected a float32 x [..., in_features]")
    k, n, sc = x.shape[-1], int(out_features), int(split_col)
    rows = x.numel() // k if k else 0
    _check_f32("bias", bias, x.device, (n,), "linear_packed_split_forward: bias must be float32 [out_features]")
    _check_f32("x_add", x_add, x.device, x.shape, "linear_packed_split_forward: x_add must be float32 with the shape of x")
    if packed.dtype != torch.uint8 or packed.numel() == 0 or packed.numel() != lib.linear_hip_packed_weight_bytes(n, k):
        raise RuntimeError("linear_packed_split_forward: `packed` does not belong to a [%d, %d] weight" % (n, k))
    out_a = torch.empty(x.shape[:-1] + (sc,), dtype=torch.float32, device=x.device)
    out_b = torch.empty(x.shape[:-1] + (n - sc,), dtype=torch.float32, device=x.device)
    if rows:
        _launch(x.device, lib.linear_hip_packed_split_f32, x.data_ptr(), _ptr(x_add), packed.data_ptr(), _ptr(bias), rows, k, n, sc,
                out_a.data_ptr(), out_b.data_ptr())
    return out_a, out_b


def linear_packed_forward(x, packed, out_features, bias=None, row_mask=None, head_major_rows=0, x_add=None, relu=False):
    """`F.linear(x, W, bias)` with split-bf16 products (~2e-5 of the output scale) from weights prepared by
    linear_pack_weight; rows whose `row_mask` entry is True are written as zeros (the masked_fill of
    ops/modules/ms_deform_attn.py:96-97).  x [..., in_features] contiguous -> [..., out_features].
    head_major_rows = S > 0: x is [N, S, in_features] and the result is [N, out_features // 32, S, 32] (head-major
    `value` for ms_deform_attn_forward_fused(..., value_head_major=True)).
    x_add (same shape as x): the layer's input is x + x_add, added while the operand is loaded (`with_pos_embed`);
    relu: ReLU in the epilogue.  Neither combines with head_major_rows."""
    lib = _lib.load()
    _check("x", x, x.device)
    _check("packed", packed, x.device)
    if x.dtype != torch.float32 or x.dim() < 1:
        raise RuntimeError("linear_packed_forward: expected a float32 x [..., in_features]")
    k, n = x.shape[-1], int(out_features)
    rows = x.numel() // k if k else 0
    _check_f32("bias", bias, x.device, (n,), "linear_packed_forward: bias must be float32 [out_features]")
    if row_mask is not None:
        _check("row_mask", row_mask, x.device)
        if row_mask.dtype not in (torch.bool, torch.uint8) or row_mask.numel() != rows:
            raise RuntimeError("linear_packed_forward: row_mask must be bool / uint8 with one entry per row")
    if packed.dtype != torch.uint8 or packed.numel() == 0 or packed.numel() != lib.linear_hip_packed_weight_bytes(n, k):
        raise RuntimeError("linear_packed_forward: `packed` does not belong to a [%d, %d] weight" % (n, k))
    hm = int(head_major_rows)
    _check_f32("x_add", x_add, x.device, x.shape, "linear_packed_forward: x_add must be float32 with the shape of x")
    if hm and (x_add is not None or relu):
        raise RuntimeError("linear_packed_forward: head-major output does not combine with x_add / relu")
    if hm:
        if x.dim() != 3 or x.shape[1] != hm or n % 32:
            raise RuntimeError("linear_packed_forward: head-major output needs x [N, S, in_features] and out_features % 32 == 0")
        out = torch.empty((x.shape[0], n // 32, hm, 32), dtype=torch.float32, device=x.device)
        _launch(x.device, lib.linear_hip_packed_hm_f32, x.data_ptr(), packed.data_ptr(), _ptr(bias), _ptr(row_mask), rows, k, n, hm,
                out.data_ptr())
        return out
    out = torch.empty(x.shape[:-1] + (n,), dtype=torch.float32, device=x.device)
    if x_add is not None or relu:
        _launch(x.device, lib.linear_hip_packed_ex_f32, x.data_ptr(), _ptr(x_add), packed.data_ptr(), _ptr(bias), _ptr(row_mask),
                rows, k, n, int(bool(relu)), out.data_ptr())
    else:
        _launch(x.device, lib.linear_hip_packed_f32, x.data_ptr(), packed.data_ptr(), _ptr(bias), _ptr(row_mask), rows, k, n,
                out.data_ptr())
    return out


def add_layernorm_supported(x, normalized_shape):
    return (x.is_cuda and x.dtype == torch.float32 and len(normalized_shape) == 1 and x.shape[-1] == normalized_shape[0]
            and x.shape[-1] % 4 == 0 and x.shape[-1] <= 4096)


def add_layernorm(x, residual, weight, bias, eps):
    """LayerNorm(x + residual) over the last dimension in one pass (include/layernorm_hip.h); residual may be None."""
    lib = _lib.load()
    _check("x", x, x.device)
    for name, t in (("residual", residual), ("weight", weight), ("bias", bias)):
        _check_f32(name, t, x.device)
    if x.dtype != torch.float32:
        raise RuntimeError("x must be float32")
    d = x.shape[-1]
    if residual is not None and residual.shape != x.shape:
        raise RuntimeError("add_layernorm: residual must have the shape of x")
    for name, t in (("weight", weight), ("bias", bias)):
        if t is not None and t.shape != (d,):
            raise RuntimeError("add_layernorm: %s must be [features]" % name)
    out = torch.empty_like(x)
    rows = x.numel() // d if d else 0
    _launch(x.device, lib.add_layernorm_hip_f32, x.data_ptr(), _ptr(residual), _ptr(weight), _ptr(bias), float(eps), rows, d,
            out.data_ptr())
    return out


# ---- the training route of the same blocks (include/dynmask_hip.h, csrc/layer_train.hip) ---------------------------------
def _row_dropout(name, p, seed, dev):
    """The checked (p, seed) of the wrappers below: p in [0, 1); the seed two int64 on `dev` (bi_attention_seed), None only at
    p == 0."""
    p = float(p)
    if not (0.0 <= p < 1.0):
        raise RuntimeError("%s: p must be in [0, 1)" % name)
    if seed is None:
        if p != 0.0:
            raise RuntimeError("%s: p > 0 needs a seed (bi_attention_seed)" % name)
        return p, None
    return _bi_attention_dropout(name, p, seed, dev)


def _rows_of(name, x, limit):
    """(rows, features) of a contiguous fp32 GPU tensor whose last dimension the kernels take."""
    _check(name, x, x.device)
    d = x.shape[-1] if x.dim() else 0
    if x.dtype != torch.float32 or d == 0 or d % 4 != 0 or d > limit or x.data_ptr() % 16 != 0:
        raise RuntimeError("%s must be float32, 16-byte aligned, its last dimension a multiple of 4 and at most %d" % (name, limit))
    return x.numel() // d, d


def dropout_add_layernorm_train_supported(x, normalized_shape):
    """True when dropout_add_layernorm_train / _backward cover LayerNorm(normalized_shape) of x: add_layernorm's conditions, a
    contiguous and 16-byte aligned x."""
    return add_layernorm_supported(x, normalized_shape) and x.is_contiguous() and x.data_ptr() % 16 == 0 and x.numel() > 0


dropout_add_layernorm_backward_supported = dropout_add_layernorm_train_supported


def dropout_add_layernorm_train(x, residual, weight, bias, eps, p=0.0, seed=None):
    """(out, z) of dropout_add_layernorm_hip_train_f32: z = residual + dropout(x), out = LayerNorm(z) over the last dimension;
    z is what dropout_add_layernorm_backward takes.  residual, weight and bias may be None.  `seed`: bi_attention_seed's two
    int64 on the device, needed when p > 0; the keep decisions are made inside the kernel.  At p == 0 out is add_layernorm's
    bit for bit."""
    lib = _lib.load()
    rows, d = _rows_of("x", x, _lib.LAYERNORM_MAX_FEATURES)
    dev = x.device
    _check_f32("residual", residual, dev, x.shape, "dropout_add_layernorm_train: residual must be float32 of the shape of x")
    for name, t in (("weight", weight), ("bias", bias)):
        _check_f32(name, t, dev, (d,), "dropout_add_layernorm_train: %s must be float32 [features]" % name)
    p, seed = _row_dropout("dropout_add_layernorm_train", p, seed, dev)
    z, out = torch.empty_like(x), torch.empty_like(x)
    _launch(dev, lib.dropout_add_layernorm_hip_train_f32, x.data_ptr(), _ptr(residual), _ptr(weight), _ptr(bias), float(eps), rows, d,
            p, _ptr(seed), z.data_ptr(), out.data_ptr())
    return out, z


def dropout_add_layernorm_backward(grad_out, z, weight, eps, p=0.0, seed=None, need_x=True, need_residual=True, need_weight=True,
                                   need_bias=True):
    """(grad_x, grad_residual, grad_weight, grad_bias) of dropout_add_layernorm_hip_backward_f32, None where not needed.  Mean
    and rstd are recomputed from z and the keep decisions from `seed`; the parameter gradients are float64 sums in a fixed
    order (bitwise repeatable).  At p == 0 grad_x IS grad_residual (one tensor, written once).  A gradient that is not
    contiguous or not 16-byte aligned is staged by one copy; the workspace comes from PyTorch's caching allocator."""
    lib = _lib.load()
    rows, d = _rows_of("z", z, _lib.LAYERNORM_MAX_FEATURES)
    dev = z.device
    if not (grad_out.is_cuda and grad_out.device == dev and grad_out.dtype == torch.float32 and grad_out.shape == z.shape):
        raise RuntimeError("dropout_add_layernorm_backward: grad_out must be float32 of the shape of z on its device")
    if not grad_out.is_contiguous() or grad_out.data_ptr() % 16 != 0:
        grad_out = grad_out.clone(memory_format=torch.contiguous_format)
    _check_f32("weight", weight, dev, (d,), "dropout_add_layernorm_backward: weight must be float32 [features]")
    p, seed = _row_dropout("dropout_add_layernorm_backward", p, seed, dev)
    shared = p == 0.0 and need_x and need_residual
    grad_res = torch.empty_like(z) if need_residual or shared else None
    grad_x = torch.empty_like(z) if need_x and not shared else None
    grad_w = torch.empty(d, dtype=torch.float32, device=dev) if need_weight else None
    grad_b = torch.empty(d, dtype=torch.float32, device=dev) if need_bias else None
    ws_bytes = int(lib.dropout_add_layernorm_hip_backward_workspace_bytes(rows, d)) if need_weight or need_bias else 0
    ws = _workspace(ws_bytes, dev) if ws_bytes else None
    _launch(dev, lib.dropout_add_layernorm_hip_backward_f32, grad_out.data_ptr(), z.data_ptr(), _ptr(weight), float(eps), rows, d, p,
            _ptr(seed), _ptr(grad_x), _ptr(grad_res), _ptr(grad_w), _ptr(grad_b), _ptr(ws), ws_bytes)
    return (grad_res if shared else grad_x), (grad_res if need_residual else None), grad_w, grad_b


def relu_dropout_supported(h):
    """True when relu_dropout / relu_dropout_backward cover h."""
    return (h.is_cuda and h.dtype == torch.float32 and h.is_contiguous() and h.dim() >= 1 and h.numel() > 0
            and h.shape[-1] % 4 == 0 and h.shape[-1] <= _lib.RELU_DROPOUT_MAX_FEATURES and h.data_ptr() % 16 == 0)


relu_dropout_backward_supported = relu_dropout_supported


def relu_dropout(h, p=0.0, seed=None):
    """dropout(relu(h)) in one pass (relu_dropout_hip_f32), the keep decisions made inside the kernel from `seed`
    (bi_attention_seed's two int64, needed when p > 0).  The result is all relu_dropout_backward takes."""
    lib = _lib.load()
    rows, d = _rows_of("h", h, _lib.RELU_DROPOUT_MAX_FEATURES)
    p, seed = _row_dropout("relu_dropout", p, seed, h.device)
    out = torch.empty_like(h)
    _launch(h.device, lib.relu_dropout_hip_f32, h.data_ptr(), rows, d, p, _ptr(seed), out.data_ptr())
    return out


def relu_dropout_backward(grad_out, out, p=0.0):
    """grad_h of relu_dropout from its result alone (relu_dropout_hip_backward_f32): grad_out / (1 - p) where out > 0."""
    lib = _lib.load()
    rows, d = _rows_of("out", out, _lib.RELU_DROPOUT_MAX_FEATURES)
    p = float(p)
    if not (0.0 <= p < 1.0):
        raise RuntimeError("relu_dropout_backward: p must be in [0, 1)")
    if not (grad_out.is_cuda and grad_out.device == out.device and grad_out.dtype == torch.float32 and grad_out.shape == out.shape):
        raise RuntimeError("relu_dropout_backward: grad_out must be float32 of the shape of out on its device")
    if not grad_out.is_contiguous() or grad_out.data_ptr() % 16 != 0:
        grad_out = grad_out.clone(memory_format=torch.contiguous_format)
    grad_h = torch.empty_like(out)
    _launch(out.device, lib.relu_dropout_hip_backward_f32, grad_out.data_ptr(), out.data_ptr(), rows, d, p, grad_h.data_ptr())
    return grad_h


def row_dropout_keep(seed, p, rows, features):
    """FOR TESTS AND TOOLS (row_dropout_hip_keep_u8): the keep decisions of the two ops above for `seed` written out, uint8
    [rows, features] with 1 = kept -- the only place where a mask of full size exists."""
    lib = _lib.load()
    p, seed = _bi_attention_dropout("row_dropout_keep", p, seed, seed.device if torch.is_tensor(seed) else None)
    keep = torch.empty((rows, features), dtype=torch.uint8, device=seed.device)
    _launch(seed.device, lib.row_dropout_hip_keep_u8, seed.data_ptr(), p, rows, features, keep.data_ptr())
    return keep


def _qsel_geometry(who, memory, padding_mask, spatial_shapes, valid_wh, enc_weight, enc_bias, ln_weight, ln_bias):
    """Checks of the arguments qsel_scores and qsel_boxes share; (B, S, d, n_levels)."""
    dev = memory.device
    _check("memory", memory, dev)
    if memory.dtype != torch.float32 or memory.dim() != 3:
        raise RuntimeError("%s: memory must be float32 [B, S, d_model]" % who)
    B, S, d = memory.shape
    _check("padding_mask", padding_mask, dev)
    if padding_mask.dtype != torch.bool or tuple(padding_mask.shape) != (B, S):
        raise RuntimeError("%s: padding_mask must be bool [B, S]" % who)
    _check("spatial_shapes", spatial_shapes, dev)
    if spatial_shapes.dtype != torch.long or spatial_shapes.dim() != 2 or spatial_shapes.shape[1] != 2:
        raise RuntimeError("%s: spatial_shapes must be int64 [n_levels, 2]" % who)
    L = spatial_shapes.shape[0]
    _check_f32("valid_wh", valid_wh, dev, (B, L, 2), "%s: valid_wh must be float32 [B, n_levels, 2]" % who)
    _check_f32("enc_weight", enc_weight, dev, (d, d), "%s: enc_weight must be float32 [d_model, d_model]" % who)
    for name, t in (("enc_bias", enc_bias), ("ln_weight", ln_weight), ("ln_bias", ln_bias)):
        _check_f32(name, t, dev, (d,), "%s: %s must be float32 [d_model]" % (who, name))
    return B, S, d, L


def qsel_scores(memory, padding_mask, spatial_shapes, valid_wh, enc_weight, enc_bias, ln_weight, ln_bias, eps, class_vec,
                class_bias, scale=None, clamp=0.0, want_memory=False):
    """Class score of every row of the encoder memory for two-stage query selection (include/dynmask_hip.h:
    qsel_scores_hip_f32): LayerNorm(row @ enc_weight^T + enc_bias) . class_vec[b] / scale + class_bias[b], clamped to +-clamp
    when clamp > 0; padded rows and rows with an invalid proposal count as zeros.  class_vec [B, d] or [1, d] / [d] (one head
    for every image), class_bias [B] or [1]; scale None or a DEVICE tensor of one float (never read on the host).  Returns
    logits [B, S], or (logits, output_memory [B, S, d]) with want_memory."""
    lib = _lib.load()
    B, S, d, L = _qsel_geometry("qsel_scores", memory, padding_mask, spatial_shapes, valid_wh, enc_weight, enc_bias, ln_weight,
                                ln_bias)
    dev = memory.device
    class_vec = class_vec.view(1, -1) if class_vec.dim() == 1 else class_vec
    if class_vec.dim() != 2 or class_vec.shape[0] not in (1, B) or class_vec.shape[1] != d:
        raise RuntimeError("qsel_scores: class_vec must be float32 [B, d_model] or [1, d_model]")
    _check_f32("class_vec", class_vec, dev)
    if class_bias.dim() != 1 or class_bias.shape[0] not in (1, B):
        raise RuntimeError("qsel_scores: class_bias must be float32 [B] or [1]")
    _check_f32("class_bias", class_bias, dev)
    if scale is not None and scale.numel() != 1:
        raise RuntimeError("qsel_scores: scale must hold one float")
    _check_f32("scale", scale, dev)
    logits = torch.empty((B, S), dtype=torch.float32, device=dev)
    out_mem = torch.empty((B, S, d), dtype=torch.float32, device=dev) if want_memory else None
    _launch(dev, lib.qsel_scores_hip_f32, memory.data_ptr(), padding_mask.data_ptr(), spatial_shapes.data_ptr(), L,
            valid_wh.data_ptr(), enc_weight.data_ptr(), enc_bias.data_ptr(), ln_weight.data_ptr(), ln_bias.data_ptr(), float(eps),
            class_vec.data_ptr(), d if class_vec.shape[0] == B and B > 1 else 0, class_bias.data_ptr(),
            1 if class_bias.shape[0] == B and B > 1 else 0, _ptr(scale), float(clamp), B, S, d, logits.data_ptr(), _ptr(out_mem))
    return (logits, out_mem) if want_memory else logits


def qsel_boxes(memory, padding_mask, spatial_shapes, valid_wh, enc_weight, enc_bias, ln_weight, ln_bias, eps, idx, w1, b1, w2,
               b2, w3, b3):
    """Boxes of the rows idx [B, K] (int64, as torch.topk returns them) for two-stage query selection (include/dynmask_hip.h:
    qsel_boxes_hip_f32): the 3-layer box MLP on LayerNorm(row @ enc_weight^T + enc_bias) plus the logit of the row's proposal
    (+inf on padded and invalid rows).  Returns (coords_unact [B, K, 4], reference_points = its sigmoid)."""
    lib = _lib.load()
    B, S, d, L = _qsel_geometry("qsel_boxes", memory, padding_mask, spatial_shapes, valid_wh, enc_weight, enc_bias, ln_weight,
                                ln_bias)
    dev = memory.device
    _check("idx", idx, dev)
    if idx.dtype != torch.long or idx.dim() != 2 or idx.shape[0] != B:
        raise RuntimeError("qsel_boxes: idx must be int64 [B, K]")
    K = idx.shape[1]
    for name, t, shape in (("w1", w1, (d, d)), ("b1", b1, (d,)), ("w2", w2, (d, d)), ("b2", b2, (d,)), ("w3", w3, (4, d)),
                           ("b3", b3, (4,))):
        _check_f32(name, t, dev, shape, "qsel_boxes: %s must be float32 %s" % (name, shape))
    coords = torch.empty((B, K, 4), dtype=torch.float32, device=dev)
    points = torch.empty((B, K, 4), dtype=torch.float32, device=dev)
    _launch(dev, lib.qsel_boxes_hip_f32, memory.data_ptr(), padding_mask.data_ptr(), spatial_shapes.data_ptr(), L,
            valid_wh.data_ptr(), enc_weight.data_ptr(), enc_bias.data_ptr(), ln_weight.data_ptr(), ln_bias.data_ptr(), float(eps),
            idx.data_ptr(), K, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), w3.data_ptr(), b3.data_ptr(), B, S, d,
            coords.data_ptr(), points.data_ptr())
    return coords, points


def pred_heads(hs, tokens, token_bias, scale, clamp, reference, box_mlp, iou=None, controller=None):
    """Class logits, boxes, IoU logit and mask-head parameters of every query of one decoder level in one launch
    (include/dynmask_hip.h: pred_heads_hip_f32).  hs [B, Q, d_model]; tokens [B, T, d_model] or [1, T, d_model] (one text for
    every image) with token_bias [B, T] or [1, T]; scale None or a DEVICE tensor of one float (never read on the host);
    reference [B, Q, 2 | 4] in sigmoid space; box_mlp the six tensors (w1, b1, w2, b2, w3 [4, d_model], b3); iou None or
    (weight [1, d_model] or [d_model], bias [1]); controller None or its six tensors, w3 [P, d_model].
    Returns (logits [B, Q, T], boxes [B, Q, 4], iou [B, Q] or None, params [B, Q, P] or None)."""
    lib = _lib.load()
    dev = hs.device
    _check("hs", hs, dev)
    if hs.dtype != torch.float32 or hs.dim() != 3:
        raise RuntimeError("pred_heads: hs must be float32 [B, Q, d_model]")
    B, Q, d = hs.shape
    if tokens.dim() != 3 or tokens.shape[0] not in (1, B) or tokens.shape[2] != d:
        raise RuntimeError("pred_heads: tokens must be float32 [B, T, d_model] or [1, T, d_model]")
    _check_f32("tokens", tokens, dev)
    T = tokens.shape[1]
    _check_f32("token_bias", token_bias, dev, (tokens.shape[0], T), "pred_heads: token_bias must be float32 [B, T] like tokens")
    if scale is not None and scale.numel() != 1:
        raise RuntimeError("pred_heads: scale must hold one float")
    _check_f32("scale", scale, dev)
    if reference.dim() != 3 or tuple(reference.shape[:2]) != (B, Q) or reference.shape[2] not in (2, 4):
        raise RuntimeError("pred_heads: reference must be float32 [B, Q, 2] or [B, Q, 4]")
    _check_f32("reference", reference, dev)

    def mlp(who, tensors, out):
        if len(tensors) != 6:
            raise RuntimeError("pred_heads: %s must be (w1, b1, w2, b2, w3, b3)" % who)
        for name, t, shape in zip(("w1", "b1", "w2", "b2", "w3", "b3"), tensors, ((d, d), (d,), (d, d), (d,), (out, d), (out,))):
            _check_f32(name, t, dev, shape, "pred_heads: %s %s must be float32 %s" % (who, name, shape))
        return [t.data_ptr() for t in tensors]

    box = mlp("box_mlp", box_mlp, 4)
    iou_ptrs, iou_out = [None, None], None
    if iou is not None:
        iou_w, iou_b = iou
        if iou_w.numel() != d:
            raise RuntimeError("pred_heads: iou weight must be float32 [1, d_model]")
        _check_f32("iou weight", iou_w, dev)
        _check_f32("iou bias", iou_b, dev, (1,), "pred_heads: iou bias must be float32 [1]")
        iou_ptrs, iou_out = [iou_w.data_ptr(), iou_b.data_ptr()], torch.empty((B, Q), dtype=torch.float32, device=dev)
    ctrl, P, params = [None] * 6, 0, None
    if controller is not None:
        if len(controller) != 6 or controller[4].dim() != 2:
            raise RuntimeError("pred_heads: controller must be (w1, b1, w2, b2, w3 [P, d_model], b3)")
        P = controller[4].shape[0]
        ctrl = mlp("controller", controller, P)
        params = torch.empty((B, Q, P), dtype=torch.float32, device=dev)
    per_image = tokens.shape[0] == B and B > 1
    logits = torch.empty((B, Q, T), dtype=torch.float32, device=dev)
    boxes = torch.empty((B, Q, 4), dtype=torch.float32, device=dev)
    _launch(dev, lib.pred_heads_hip_f32, hs.data_ptr(), tokens.data_ptr(), T * d if per_image else 0, token_bias.data_ptr(),
            T if per_image else 0, _ptr(scale), float(clamp), reference.data_ptr(), reference.shape[2], *box, *iou_ptrs, *ctrl, P,
            B, Q, T, d, logits.data_ptr(), boxes.data_ptr(), _ptr(iou_out), _ptr(params))
    return logits, boxes, iou_out, params


def pred_heads_set_variant(variant):
    """The grid of pred_heads: "auto", "split" or "tile" (include/dynmask_hip.h: pred_heads_hip_set_variant); for A/B runs."""
    if _lib.load().pred_heads_hip_set_variant(_lib.PRED_HEADS_VARIANTS.index(variant)) != 0:
        raise ValueError(_lib.last_error())


def detpost_supported(num_queries, num_classes, num_tokens):
    """The sizes the detpost_* kernels accept (include/dynmask_hip.h)."""
    return (0 < num_queries <= _lib.DETPOST_MAX_QUERIES and 0 < num_classes <= _lib.DETPOST_MAX_CLASSES
            and 0 < num_tokens <= _lib.DETPOST_MAX_TOKENS)


def _i32(name, t, dev, shape):
    _check(name, t, dev)
    if t.dtype != torch.int32 or tuple(t.shape) != tuple(shape):
        raise RuntimeError("%s must be int32 %s" % (name, tuple(shape)))


def detpost_scores(logits, iou_logits, cls_ptr, tok_idx, score_thres=0.0, out=None):
    """Per-class scores of every decoder query (include/dynmask_hip.h: detpost_scores_hip_f32).  logits [B, Q, T] fp32,
    iou_logits [B, Q] fp32 or None, the positive map as CSR (cls_ptr [C + 1], tok_idx [nnz], int32 on the device).  Returns
    (prob [B, Q, C], row_max [B, Q], row_arg [B, Q] int32, row_valid [B, Q] int32); `out` may supply the four to write."""
    lib = _lib.load()
    dev = logits.device
    _check("logits", logits, dev)
    if logits.dtype != torch.float32 or logits.dim() != 3:
        raise RuntimeError("detpost_scores: logits must be float32 [B, Q, T]")
    B, Q, T = logits.shape
    _check_f32("iou_logits", iou_logits, dev, (B, Q), "detpost_scores: iou_logits must be float32 [B, Q]")
    _check("cls_ptr", cls_ptr, dev)
    _check("tok_idx", tok_idx, dev)
    if cls_ptr.dtype != torch.int32 or tok_idx.dtype != torch.int32 or cls_ptr.dim() != 1 or tok_idx.dim() != 1 \
            or cls_ptr.numel() < 2:
        raise RuntimeError("detpost_scores: cls_ptr [C + 1] and tok_idx [nnz] must be int32")
    C = cls_ptr.numel() - 1
    if out is None:
        out = (torch.empty((B, Q, C), dtype=torch.float32, device=dev), torch.empty((B, Q), dtype=torch.float32, device=dev),
               torch.empty((B, Q), dtype=torch.int32, device=dev), torch.empty((B, Q), dtype=torch.int32, device=dev))
    prob, row_max, row_arg, row_valid = out
    _check_f32("prob", prob, dev, (B, Q, C), "detpost_scores: prob must be float32 [B, Q, C]")
    _check_f32("row_max", row_max, dev, (B, Q), "detpost_scores: row_max must be float32 [B, Q]")
    _i32("row_arg", row_arg, dev, (B, Q))
    _i32("row_valid", row_valid, dev, (B, Q))
    _launch(dev, lib.detpost_scores_hip_f32, logits.data_ptr(), _ptr(iou_logits), cls_ptr.data_ptr(), tok_idx.data_ptr(),
            tok_idx.numel(), float(score_thres), B, Q, C, T, prob.data_ptr(), row_max.data_ptr(), row_arg.data_ptr(),
            row_valid.data_ptr())
    return prob, row_max, row_arg, row_valid


def detpost_nms(boxes, row_max, row_arg, iou_threshold, per_class=False, out=None):
    """Class-aware NMS of every image's queries (include/dynmask_hip.h: detpost_nms_hip_f32).  boxes [B, Q, 4] fp32 cxcywh,
    row_max [B, Q] fp32 the scores, row_arg [B, Q] int32 the classes.  Returns (keep [B, Q] int32, the kept queries by
    decreasing score padded with -1; n_keep [B] int32; kept_mask [B, Q] uint8); `out` may supply the three to write."""
    lib = _lib.load()
    dev = boxes.device
    _check("boxes", boxes, dev)
    if boxes.dtype != torch.float32 or boxes.dim() != 3 or boxes.shape[2] != 4:
        raise RuntimeError("detpost_nms: boxes must be float32 [B, Q, 4]")
    B, Q, _ = boxes.shape
    _check_f32("row_max", row_max, dev, (B, Q), "detpost_nms: row_max must be float32 [B, Q]")
    _i32("row_arg", row_arg, dev, (B, Q))
    if out is None:
        out = (torch.empty((B, Q), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev),
               torch.empty((B, Q), dtype=torch.uint8, device=dev))
    keep, n_keep, kept_mask = out
    _i32("keep", keep, dev, (B, Q))
    _i32("n_keep", n_keep, dev, (B,))
    _check("kept_mask", kept_mask, dev)
    if kept_mask.dtype != torch.uint8 or tuple(kept_mask.shape) != (B, Q):
        raise RuntimeError("detpost_nms: kept_mask must be uint8 [B, Q]")
    _launch(dev, lib.detpost_nms_hip_f32, boxes.data_ptr(), row_max.data_ptr(), row_arg.data_ptr(), float(iou_threshold),
            1 if per_class else 0, B, Q, keep.data_ptr(), n_keep.data_ptr(), kept_mask.data_ptr())
    return keep, n_keep, kept_mask


def maskpost_supported(h, w, stride, crop, out_size, thres, num_queries=1, n=1):
    """The sizes maskpost_binarize accepts (include/dynmask_hip.h)."""
    big = 1 << 24
    return (stride in _lib.MASKPOST_STRIDES and 0.0 < thres < 1.0 and 0 < w <= _lib.MASKPOST_MAX_WIDTH and h > 0
            and 1 <= crop[0] <= h * stride <= big and 1 <= crop[1] <= w * stride <= big
            and 1 <= out_size[0] <= big and 1 <= out_size[1] <= big
            and num_queries * h * w < 1 << 31 and n * out_size[0] * out_size[1] < 1 << 31)


def _maskpost_planes(who, logits, rows):
    dev = logits.device
    _check("logits", logits, dev)
    if logits.dtype != torch.float32 or logits.dim() != 3:
        raise RuntimeError("%s: logits must be float32 [Q, h, w]" % who)
    _check("rows", rows, dev)
    if rows.dtype != torch.int64 or rows.dim() != 1:
        raise RuntimeError("%s: rows must be int64 [n]" % who)
    return dev, logits.shape[0], logits.shape[1], logits.shape[2], rows.shape[0]


def maskpost_binarize(logits, rows, stride, crop, out_size, thres, out=None):
    """Binarised masks at the output size (include/dynmask_hip.h: maskpost_binarize_hip_f32): logits [Q, h, w] fp32, rows [n]
    int64 the instances' rows of Q; bilinear x `stride`, sigmoid, > thres, crop to `crop` (height, width), nearest to
    `out_size`.  Returns [n, out_h, out_w] uint8 of 0 / 1; `out` may supply it."""
    lib = _lib.load()
    dev, Q, h, w, n = _maskpost_planes("maskpost_binarize", logits, rows)
    shape = (n, int(out_size[0]), int(out_size[1]))
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    _check("out", out, dev)
    if out.dtype != torch.uint8 or tuple(out.shape) != shape:
        raise RuntimeError("maskpost_binarize: out must be uint8 %s" % (shape,))
    _launch(dev, lib.maskpost_binarize_hip_f32, logits.data_ptr(), rows.data_ptr(), Q, h, w, n, int(stride), int(crop[0]),
            int(crop[1]), shape[1], shape[2], float(thres), out.data_ptr())
    return out


def maskpost_pack(logits, rows, out=None):
    """Bit-packed low-resolution masks (include/dynmask_hip.h: maskpost_pack_hip_f32): logits [Q, h, w] fp32, rows [n] int64.
    Returns (bits [n, ceil(h w / 32)] int32 holding the words, area [n] int32); `out` may supply the two."""
    lib = _lib.load()
    dev, Q, h, w, n = _maskpost_planes("maskpost_pack", logits, rows)
    words = (h * w + 31) // 32
    if out is None:
        out = (torch.empty((n, words), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev))
    bits, area = out
    _i32("bits", bits, dev, (n, words))
    _i32("area", area, dev, (n,))
    _launch(dev, lib.maskpost_pack_hip_f32, logits.data_ptr(), rows.data_ptr(), Q, h, w, n, bits.data_ptr(), area.data_ptr())
    return bits, area


def maskpost_nms(bits, area, nms_thr, out=None):
    """Greedy mask NMS in the given order (include/dynmask_hip.h: maskpost_nms_hip_u32): bits [n, words] int32 and area [n] int32
    as maskpost_pack returns them.  Returns (inter [n, n] int32 the pairs' common pixels, keep [n] uint8); `out` may supply the
    two."""
    lib = _lib.load()
    dev = bits.device
    if bits.dim() != 2:
        raise RuntimeError("maskpost_nms: bits must be int32 [n, words]")
    n, words = bits.shape
    _i32("bits", bits, dev, (n, words))
    _i32("area", area, dev, (n,))
    if out is None:
        out = (torch.empty((n, n), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.uint8, device=dev))
    inter, keep = out
    _i32("inter", inter, dev, (n, n))
    _check("keep", keep, dev)
    if keep.dtype != torch.uint8 or tuple(keep.shape) != (n,):
        raise RuntimeError("maskpost_nms: keep must be uint8 [n]")
    _launch(dev, lib.maskpost_nms_hip_u32, bits.data_ptr(), area.data_ptr(), n, words, float(nms_thr), inter.data_ptr(), keep.data_ptr())
    return inter, keep


class _BankState:
    """One memory bank of a tracker's kernels: a zeroed device buffer laid out by `offset(field, *geometry)` and a view of each
    field of `fields` ((name, dtype, geometry -> shape), ...)."""

    def __init__(self, fields, offset, geometry, device):
        self.geometry = tuple(int(g) for g in geometry)
        at = [offset(k, *self.geometry) for k in range(len(fields) + 1)]
        self.buffer = torch.zeros(at[-1], dtype=torch.uint8, device=device)
        for k, (name, dtype, shape) in enumerate(fields):
            shape = shape(*self.geometry)
            nbytes = torch.empty((), dtype=dtype).element_size() * int(torch.Size(shape).numel())
            assert at[k] % 16 == 0 and at[k] + nbytes <= at[k + 1]
            setattr(self, name, self.buffer[at[k]:at[k] + nbytes].view(dtype).view(shape))


def _bank_pair(who, state, next_state):
    """The device of `state`; next_state (None: the call writes no bank) must be another buffer like it."""
    if next_state is not None and (next_state.geometry != state.geometry or next_state.buffer.device != state.buffer.device
                                   or next_state.buffer.data_ptr() == state.buffer.data_ptr()):
        raise RuntimeError("%s: the next state must be another buffer of the same geometry on the same device" % who)
    return state.buffer.device


def _bank_flags(name, flags, dev, n):
    _check(name, flags, dev)
    if flags.dtype != torch.uint8 or tuple(flags.shape) != (n,):
        raise RuntimeError("%s must be uint8 [n]" % name)


def _bank_i64(what, t, dev, count, text):
    """`t` is int64 [count] on dev, or RuntimeError("<what> must be int64 [<text>]"); `what` may carry the caller's "who: "."""
    _check(what.split(" ")[-1], t, dev)
    if t.dtype != torch.int64 or tuple(t.shape) != (count,):
        raise RuntimeError("%s must be int64 [%s]" % (what, text))


TRACK_STATE_FIELDS = (("meta", torch.int64, lambda C, D, L: (2,)), ("id", torch.int64, lambda C, D, L: (C,)),
                      ("label", torch.int64, lambda C, D, L: (C,)), ("bbox", torch.float32, lambda C, D, L: (C, 5)),
                      ("velocity", torch.float32, lambda C, D, L: (C, 5)), ("last_frame", torch.int32, lambda C, D, L: (C,)),
                      ("acc_frame", torch.int32, lambda C, D, L: (C,)), ("exist_frame", torch.int32, lambda C, D, L: (C,)),
                      ("long_len", torch.int32, lambda C, D, L: (C,)), ("long_score", torch.float32, lambda C, D, L: (C, L)),
                      ("embed", torch.float32, lambda C, D, L: (C, D)), ("long_embed", torch.float32, lambda C, D, L: (C, L, D)))


def track_supported(n, capacity, D, memory_len):
    """The sizes the track_hip_* kernels accept (include/dynmask_hip.h)."""
    return (0 <= n <= _lib.MASKPOST_MAX_MASKS and 1 <= capacity <= _lib.TRACK_MAX_CAPACITY and 1 <= D <= _lib.TRACK_MAX_DIM
            and 1 <= memory_len <= _lib.TRACK_MAX_MEMORY_LEN)


class TrackState(_BankState):
    """One memory bank of the tracker kernels (include/dynmask_hip.h: track_hip_state_offset): a zeroed device buffer and a
    view of each of its fields (`meta`, `id`, `label`, `bbox`, `velocity`, `last_frame`, `acc_frame`, `exist_frame`,
    `long_len`, `long_score`, `embed`, `long_embed`) for capacity C, width D and ring length L."""

    def __init__(self, capacity, D, memory_len, device):
        lib = _lib.load()
        if not track_supported(0, capacity, D, memory_len):
            raise RuntimeError("TrackState: capacity %d, width %d, ring %d are beyond the kernels' sizes" % (capacity, D, memory_len))
        assert len(TRACK_STATE_FIELDS) == _lib.TRACK_STATE_FIELDS
        super().__init__(TRACK_STATE_FIELDS, lib.track_hip_state_offset, (capacity, D, memory_len), device)


def _track_args(who, state, next_state, n):
    C, D, L = state.geometry
    dev = _bank_pair(who, state, next_state)
    if not track_supported(n, C, D, L):
        raise RuntimeError("%s: %d detections are beyond the kernels' sizes" % (who, n))
    return dev, C, D, L


def track_scores(embeds, keep, state, M, long_match=False, temporal=None):
    """Bi-softmax scores of the kept detections against the M live slots (include/dynmask_hip.h: track_hip_scores_f32): embeds
    [n, D] fp32, keep [n] uint8, `temporal` the [L + 1, L] fp32 table or None.  Returns scores [n, M] fp32 (rows the pre-NMS
    dropped are not written)."""
    lib = _lib.load()
    n = embeds.shape[0]
    dev, C, D, L = _track_args("track_scores", state, None, n)
    _check_f32("embeds", embeds, dev, (n, D))
    _bank_flags("keep", keep, dev, n)
    _check_f32("temporal", temporal, dev, (L + 1, L))
    if not 0 <= M <= C:
        raise RuntimeError("track_scores: M must lie in [0, capacity]")
    scores = torch.empty((n, M), dtype=torch.float32, device=dev)
    memo = torch.empty((max(M, 1), D), dtype=torch.float32, device=dev) if long_match else None
    stats = torch.empty((2 * max(n, 1),), dtype=torch.float32, device=dev)
    _launch(dev, lib.track_hip_scores_f32, embeds.data_ptr(), keep.data_ptr(), state.buffer.data_ptr(), _ptr(temporal),
            1 if long_match else 0, n, int(M), C, D, L, _ptr(memo), stats.data_ptr(), scores.data_ptr())
    return scores


def track_associate(scores, keep, bboxes, inter, area, state, next_state, M, frame_weight, match_score_thr, new_score_thr,
                    nms_thr_post, frame_id, memo_tracklet_frames):
    """The association of one frame (include/dynmask_hip.h: track_hip_associate_f32).  Returns (plan [2 C + n] int32, result
    [3 n + 2] int64: keep flags, ids, the next count, the next num_tracklets, the kept rows); writes next_state.meta."""
    lib = _lib.load()
    n = bboxes.shape[0]
    dev, C, D, L = _track_args("track_associate", state, next_state, n)
    _check_f32("bboxes", bboxes, dev, (n, 5))
    _bank_flags("keep", keep, dev, n)
    _i32("inter", inter, dev, (n, n))
    _i32("area", area, dev, (n,))
    if M > 0:
        _check_f32("scores", scores, dev, (n, M))
    plan = torch.empty((2 * C + n,), dtype=torch.int32, device=dev)
    result = torch.empty((3 * n + 2,), dtype=torch.int64, device=dev)
    _launch(dev, lib.track_hip_associate_f32, _ptr(scores if M > 0 else None), keep.data_ptr(), bboxes.data_ptr(), inter.data_ptr(),
            area.data_ptr(), state.buffer.data_ptr(), next_state.buffer.data_ptr(), n, int(M), C, D, L, 1 if frame_weight else 0,
            float(match_score_thr), float(new_score_thr), float(nms_thr_post), int(frame_id), int(memo_tracklet_frames),
            plan.data_ptr(), result.data_ptr())
    return plan, result


def track_update(embeds, bboxes, labels, plan, result, state, next_state, M, momentum, frame_id):
    """The memory update of one frame (include/dynmask_hip.h: track_hip_update_f32): writes next_state from state, the plan and
    the result of track_associate."""
    lib = _lib.load()
    n = embeds.shape[0]
    dev, C, D, L = _track_args("track_update", state, next_state, n)
    _check_f32("embeds", embeds, dev, (n, D))
    _check_f32("bboxes", bboxes, dev, (n, 5))
    _bank_i64("track_update: labels", labels, dev, n, "n")
    _i32("plan", plan, dev, (2 * C + n,))
    _bank_i64("track_update: result", result, dev, 3 * n + 2, "3 n + 2")
    _launch(dev, lib.track_hip_update_f32, embeds.data_ptr(), bboxes.data_ptr(), labels.data_ptr(), plan.data_ptr(), result.data_ptr(),
            state.buffer.data_ptr(), next_state.buffer.data_ptr(), n, int(M), C, D, L, float(1 - momentum), float(momentum),
            int(frame_id))


_QD = lambda shape: (lambda C, D, B, K: shape(C, D, B, max(K, 1)))
QDTRACK_STATE_FIELDS = (("meta", torch.int64, _QD(lambda C, D, B, K: (2 + _lib.QDTRACK_MAX_BACKDROP_FRAMES,))),
                        ("id", torch.int64, _QD(lambda C, D, B, K: (C,))), ("label", torch.int64, _QD(lambda C, D, B, K: (C,))),
                        ("bbox", torch.float32, _QD(lambda C, D, B, K: (C, 5))), ("velocity", torch.float32, _QD(lambda C, D, B, K: (C, 5))),
                        ("last_frame", torch.int32, _QD(lambda C, D, B, K: (C,))), ("acc_frame", torch.int32, _QD(lambda C, D, B, K: (C,))),
                        ("embed", torch.float32, _QD(lambda C, D, B, K: (C, D))),
                        ("backdrop_label", torch.int64, _QD(lambda C, D, B, K: (K, B))),
                        ("backdrop_bbox", torch.float32, _QD(lambda C, D, B, K: (K, B, 5))),
                        ("backdrop_embed", torch.float32, _QD(lambda C, D, B, K: (K, B, D))))
del _QD


def qdtrack_supported(n, capacity, D, backdrop_capacity, backdrop_frames):
    """The sizes the qdtrack_hip_* kernels accept (include/dynmask_hip.h)."""
    return (0 <= n <= _lib.MASKPOST_MAX_MASKS and 1 <= capacity <= _lib.TRACK_MAX_CAPACITY and 1 <= D <= _lib.TRACK_MAX_DIM
            and 1 <= backdrop_capacity <= _lib.QDTRACK_MAX_BACKDROPS and 0 <= backdrop_frames <= _lib.QDTRACK_MAX_BACKDROP_FRAMES)


class QDTrackState(_BankState):
    """One memory bank of the QuasiDense tracker's kernels (include/dynmask_hip.h: qdtrack_hip_state_offset): a zeroed device
    buffer and a view of each of its fields (`meta`, `id`, `label`, `bbox`, `velocity`, `last_frame`, `acc_frame`, `embed`,
    `backdrop_label`, `backdrop_bbox`, `backdrop_embed`) for capacity C, width D and B backdrops in each of K frames."""

    def __init__(self, capacity, D, backdrop_capacity, backdrop_frames, device):
        lib = _lib.load()
        if not qdtrack_supported(0, capacity, D, backdrop_capacity, backdrop_frames):
            raise RuntimeError("QDTrackState: capacity %d, width %d, %d backdrops in %d frames are beyond the kernels' sizes"
                               % (capacity, D, backdrop_capacity, backdrop_frames))
        assert len(QDTRACK_STATE_FIELDS) == _lib.QDTRACK_STATE_FIELDS
        super().__init__(QDTRACK_STATE_FIELDS, lib.qdtrack_hip_state_offset, (capacity, D, backdrop_capacity, backdrop_frames), device)


def _qdtrack_args(who, state, next_state, n, M, backdrops):
    """(device, C, D, B, K, the four backdrop counts) of a call on `state` with M live slots and `backdrops` rows per frame."""
    C, D, B, K = state.geometry
    dev = _bank_pair(who, state, next_state)
    if not qdtrack_supported(n, C, D, B, K):
        raise RuntimeError("%s: %d detections are beyond the kernels' sizes" % (who, n))
    backdrops = [int(b) for b in backdrops]
    if not 0 <= M <= C or len(backdrops) > K or any(not 0 <= b <= B for b in backdrops):
        raise RuntimeError("%s: M must lie in [0, capacity], and at most backdrop_frames counts in [0, backdrop_capacity]" % who)
    return dev, C, D, B, K, backdrops + [0] * (_lib.QDTRACK_MAX_BACKDROP_FRAMES - len(backdrops))


def qdtrack_prepare(bboxes, obj_score_thr, nms_backdrop_iou_thr, nms_class_iou_thr):
    """The score order, the box IoU of the sorted rows and the pre-NMS' flags (include/dynmask_hip.h: qdtrack_hip_prepare_f32):
    bboxes [n, 5] fp32.  Returns (order [n] int32, iou [n, n] fp32, valid [n] uint8)."""
    lib = _lib.load()
    dev = bboxes.device
    _check("bboxes", bboxes, dev)
    if bboxes.dtype != torch.float32 or bboxes.dim() != 2 or bboxes.shape[1] != 5:
        raise RuntimeError("qdtrack_prepare: bboxes must be float32 [n, 5]")
    n = bboxes.shape[0]
    if n > _lib.MASKPOST_MAX_MASKS:
        raise RuntimeError("qdtrack_prepare: %d detections are beyond the kernels' sizes" % n)
    order = torch.empty((n,), dtype=torch.int32, device=dev)
    iou = torch.empty((n, n), dtype=torch.float32, device=dev)
    valid = torch.empty((n,), dtype=torch.uint8, device=dev)
    _launch(dev, lib.qdtrack_hip_prepare_f32, bboxes.data_ptr(), n, float(obj_score_thr), float(nms_backdrop_iou_thr),
            float(nms_class_iou_thr), order.data_ptr(), iou.data_ptr(), valid.data_ptr())
    return order, iou, valid


def qdtrack_scores(embeds, labels, order, valid, state, M, backdrops, with_cats=True):
    """Bi-softmax scores of the valid sorted rows against the memory's columns, the M live slots and then `backdrops` (a list
    of at most backdrop_frames counts, newest first) rows of the backdrop frames (include/dynmask_hip.h: qdtrack_hip_scores_f32).
    Returns scores [n, M + sum(backdrops)] fp32 (rows the pre-NMS dropped are not written)."""
    lib = _lib.load()
    n = embeds.shape[0]
    dev, C, D, B, K, b = _qdtrack_args("qdtrack_scores", state, None, n, M, backdrops)
    _check_f32("embeds", embeds, dev, (n, D))
    _bank_i64("labels", labels, dev, n, "n")
    _i32("order", order, dev, (n,))
    _bank_flags("valid", valid, dev, n)
    scores = torch.empty((n, int(M) + sum(b)), dtype=torch.float32, device=dev)
    stats = torch.empty((2 * max(n, 1),), dtype=torch.float32, device=dev)
    _launch(dev, lib.qdtrack_hip_scores_f32, embeds.data_ptr(), labels.data_ptr(), order.data_ptr(), valid.data_ptr(),
            state.buffer.data_ptr(), n, int(M), b[0], b[1], b[2], b[3], C, D, B, K, 1 if with_cats else 0, stats.data_ptr(),
            scores.data_ptr())
    return scores


def qdtrack_associate(scores, valid, order, bboxes, iou, state, next_state, M, backdrops, match_score_thr, obj_score_thr,
                      nms_conf_thr, init_score_thr, nms_backdrop_iou_thr, frame_id, memo_tracklet_frames):
    """The association of one frame (include/dynmask_hip.h: qdtrack_hip_associate_f32).  Returns (plan [2 C + 2 n] int32, result
    [4 n + 4] int64: the valid rows' detections, their ids, their sorted rows, the valid count, the next count, the next num_tracklets, the rows of
    the new backdrop frame, the ids by sorted row); writes next_state.meta."""
    lib = _lib.load()
    n = bboxes.shape[0]
    dev, C, D, B, K, b = _qdtrack_args("qdtrack_associate", state, next_state, n, M, backdrops)
    _check_f32("bboxes", bboxes, dev, (n, 5))
    _i32("order", order, dev, (n,))
    _bank_flags("valid", valid, dev, n)
    _check_f32("iou", iou, dev, (n, n))
    if M > 0 and n > 0:
        _check_f32("scores", scores, dev, (n, int(M) + sum(b)))
    plan = torch.empty((2 * C + 2 * n,), dtype=torch.int32, device=dev)
    result = torch.empty((4 * n + 4,), dtype=torch.int64, device=dev)
    _launch(dev, lib.qdtrack_hip_associate_f32, _ptr(scores if M > 0 and n > 0 else None), valid.data_ptr(), order.data_ptr(),
            bboxes.data_ptr(), iou.data_ptr(), state.buffer.data_ptr(), next_state.buffer.data_ptr(), n, int(M), b[0], b[1], b[2], b[3],
            C, D, B, K, float(match_score_thr), float(obj_score_thr), float(nms_conf_thr), float(init_score_thr),
            float(nms_backdrop_iou_thr), int(frame_id), int(memo_tracklet_frames), plan.data_ptr(), result.data_ptr())
    return plan, result


def qdtrack_update(embeds, bboxes, labels, order, plan, result, state, next_state, M, backdrops, momentum, frame_id):
    """The memory update of one frame (include/dynmask_hip.h: qdtrack_hip_update_f32): writes next_state from state, the plan
    and the result of qdtrack_associate."""
    lib = _lib.load()
    n = embeds.shape[0]
    dev, C, D, B, K, b = _qdtrack_args("qdtrack_update", state, next_state, n, M, backdrops)
    _check_f32("embeds", embeds, dev, (n, D))
    _check_f32("bboxes", bboxes, dev, (n, 5))
    _bank_i64("labels", labels, dev, n, "n")
    _i32("order", order, dev, (n,))
    _i32("plan", plan, dev, (2 * C + 2 * n,))
    _bank_i64("qdtrack_update: result", result, dev, 4 * n + 4, "4 n + 4")
    _launch(dev, lib.qdtrack_hip_update_f32, embeds.data_ptr(), bboxes.data_ptr(), labels.data_ptr(), order.data_ptr(), plan.data_ptr(),
            result.data_ptr(), state.buffer.data_ptr(), next_state.buffer.data_ptr(), n, int(M), b[0], b[1], b[2], b[3], C, D, B, K,
            float(1 - momentum), float(momentum), int(frame_id))


def encoder_input_supported(convs, image_mask, num_groups=32):
    """What the encprep_hip_* kernels accept (include/dynmask_hip.h): contiguous fp32 [B, 256, H, W] convolution outputs of at most
    8 levels on one GPU, GroupNorm(32, 256), a bool [B, Hi, Wi] image mask on the same device."""
    if not convs or len(convs) > _lib.ENCPREP_MAX_LEVELS or num_groups != _lib.ENCPREP_GROUPS:
        return False
    dev, B = convs[0].device, convs[0].shape[0]
    return (all(c.is_cuda and c.device == dev and c.dtype == torch.float32 and c.dim() == 4 and c.shape[0] == B
                and c.shape[1] == _lib.ENCPREP_CHANNELS and c.is_contiguous() and c.numel() > 0 for c in convs)
            and image_mask.is_cuda and image_mask.device == dev and image_mask.dtype == torch.bool and image_mask.dim() == 3
            and image_mask.shape[0] == B and image_mask.numel() > 0)


def _encprep_pointers(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def encoder_input_prepare(convs, image_mask, sources, gn_weights, gn_biases, gn_eps, level_embed, dim_t, scale, eps=1e-6,
                          return_stats=False):
    """The encoder's inputs from the input_proj convolutions' outputs in four launches (include/dynmask_hip.h: encprep_hip_*).
    convs: per level [B, 256, H, W] fp32; image_mask [B, Hi, Wi] bool; sources: per level -1 (its mask is resized from the image
    mask) or the earlier level it is resized from; gn_weights / gn_biases: per level [256] fp32, gn_eps per level; level_embed
    [>= L, 256] fp32; dim_t [128] fp32.  Returns (src_flatten [B, S, 256], mask_flatten [B, S] bool, lvl_pos_embed_flatten
    [B, S, 256], valid_ratios [B, L, 2], reference_points [B, S, L, 2]), and (mean, rstd) [B, L, 32] with return_stats."""
    lib = _lib.load()
    if not encoder_input_supported(convs, image_mask):
        raise RuntimeError("encoder_input_prepare: fp32 [B, 256, H, W] levels (at most 8) and a bool [B, Hi, Wi] mask on one GPU")
    dev, B, L, C = convs[0].device, convs[0].shape[0], len(convs), _lib.ENCPREP_CHANNELS
    if not (len(sources) == len(gn_weights) == len(gn_biases) == len(gn_eps) == L):
        raise RuntimeError("encoder_input_prepare: one source, weight, bias and eps per level")
    image_mask = image_mask.contiguous()
    for t in list(gn_weights) + list(gn_biases):
        _check_f32("GroupNorm weight / bias", t, dev, (C,))
    _check_f32("level_embed", level_embed, dev)
    _check_f32("dim_t", dim_t, dev, (C // 2,))
    if level_embed.dim() != 2 or level_embed.shape[0] < L or level_embed.shape[1] != C:
        raise RuntimeError("encoder_input_prepare: level_embed must be [>= levels, 256]")
    flat = []
    for c, src in zip(convs, sources):
        flat += [int(c.shape[2]), int(c.shape[3]), int(src)]
    levels = (ctypes.c_int * len(flat))(*flat)
    S = sum(c.shape[2] * c.shape[3] for c in convs)
    T = sum(c.shape[2] + c.shape[3] for c in convs)
    f32 = dict(dtype=torch.float32, device=dev)
    mask_flatten = torch.empty((B, S), dtype=torch.bool, device=dev)
    valid_ratios = torch.empty((B, L, 2), **f32)
    yx_embed, totals = torch.empty((B, S, 2), **f32), torch.empty((B, T), **f32)
    pos, src_flatten = torch.empty((B, S, C), **f32), torch.empty((B, S, C), **f32)
    reference_points = torch.empty((B, S, L, 2), **f32)
    mean, rstd = torch.empty((B, L, _lib.ENCPREP_GROUPS), **f32), torch.empty((B, L, _lib.ENCPREP_GROUPS), **f32)
    nbytes = lib.encprep_hip_workspace_bytes(B, levels, L)
    partials = _workspace(nbytes, dev)
    xs, ws, bs = _encprep_pointers(convs), _encprep_pointers(gn_weights), _encprep_pointers(gn_biases)
    eps_all = (ctypes.c_float * L)(*[float(e) for e in gn_eps])
    _launch(dev, lib.encprep_hip_masks_u8, image_mask.data_ptr(), B, image_mask.shape[1], image_mask.shape[2], levels, L,
            mask_flatten.data_ptr(), valid_ratios.data_ptr(), yx_embed.data_ptr(), totals.data_ptr())
    _launch(dev, lib.encprep_hip_pos_f32, yx_embed.data_ptr(), totals.data_ptr(), valid_ratios.data_ptr(), level_embed.data_ptr(),
            dim_t.data_ptr(), B, levels, L, C, float(scale), float(eps), pos.data_ptr(), reference_points.data_ptr())
    _launch(dev, lib.encprep_hip_gn_stats_f32, xs, B, levels, L, C, _lib.ENCPREP_GROUPS, partials.data_ptr(), nbytes)
    _launch(dev, lib.encprep_hip_gn_apply_f32, xs, ws, bs, eps_all, partials.data_ptr(), nbytes, B, levels, L, C, _lib.ENCPREP_GROUPS,
            src_flatten.data_ptr(), mean.data_ptr(), rstd.data_ptr())
    out = (src_flatten, mask_flatten, pos, valid_ratios, reference_points)
    return out + (mean, rstd) if return_stats else out


def token_focal_loss_supported(logits, targets_all, gamma=2.0):
    """What the criterion_hip_token_focal_* kernels accept (include/dynmask_hip.h): contiguous fp32 [B, Q, T] logits on a GPU,
    at most 256 tokens, fp32 positive maps, gamma 2."""
    return (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 3 and logits.is_contiguous()
            and 0 < logits.shape[2] <= _lib.CRITERION_MAX_TOKENS and float(gamma) == 2.0
            and (targets_all is None or targets_all.dtype == torch.float32))


def _token_focal_args(who, logits, text_mask, row_target, positive_map_all):
    dev = logits.device
    _check("logits", logits, dev)
    if logits.dtype != torch.float32 or logits.dim() != 3:
        raise RuntimeError("%s: logits must be float32 [B, Q, T]" % who)
    B, Q, T = logits.shape
    _i32("row_target", row_target, dev, (B, Q))
    kind = _lib.CRITERION_MASK_NONE
    if text_mask is not None:
        _check("text_mask", text_mask, dev)
        if tuple(text_mask.shape) != (B, T) or text_mask.dtype not in (torch.int64, torch.bool, torch.uint8):
            raise RuntimeError("%s: text_mask must be int64, bool or uint8 [B, T]" % who)
        kind = _lib.CRITERION_MASK_INT64 if text_mask.dtype == torch.int64 else _lib.CRITERION_MASK_BOOL
    G = 0
    if positive_map_all is not None and positive_map_all.numel():
        G = positive_map_all.shape[0]
        _check_f32("positive_map_all", positive_map_all, dev, (G, T), "%s: positive_map_all must be float32 [G, T]" % who)
    return dev, B, Q, T, kind, G, (positive_map_all.data_ptr() if G else None)


def token_focal_loss_forward(logits, text_mask, row_target, positive_map_all, alpha, out=None, workspace=None):
    """Sum of the token focal loss (gamma 2) over the counted tokens (include/dynmask_hip.h:
    criterion_hip_token_focal_forward_f32).  logits [B, Q, T] fp32; text_mask [B, T] int64 / bool / uint8 or None; row_target [B, Q]
    int32, a row of positive_map_all [G, T] fp32 or -1.  Returns a [1] fp32 tensor; `out` may supply it, `workspace` the scratch."""
    lib = _lib.load()
    dev, B, Q, T, kind, G, pm = _token_focal_args("token_focal_loss_forward", logits, text_mask, row_target, positive_map_all)
    if out is None:
        out = torch.empty((1,), dtype=torch.float32, device=dev)
    _check_f32("out", out, dev, (1,), "token_focal_loss_forward: out must be float32 [1]")
    nbytes = lib.criterion_hip_workspace_bytes(_lib.CRITERION_TOKEN_FOCAL, B * Q, T)
    ws = _workspace(nbytes, dev) if workspace is None else workspace
    _launch(dev, lib.criterion_hip_token_focal_forward_f32, logits.data_ptr(), _ptr(text_mask), kind, row_target.data_ptr(), pm, G,
            float(alpha), B, Q, T, out.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size())
    return out


def token_focal_loss_backward(logits, text_mask, row_target, positive_map_all, alpha, scale, out=None):
    """grad_logits [B, Q, T] = scale * d loss / d logits (criterion_hip_token_focal_backward_f32); `scale` is a [1] fp32 tensor on the
    device.  Exactly 0.0 at masked tokens; every element is written."""
    lib = _lib.load()
    dev, B, Q, T, kind, G, pm = _token_focal_args("token_focal_loss_backward", logits, text_mask, row_target, positive_map_all)
    _check_f32("scale", scale, dev, (1,), "token_focal_loss_backward: scale must be float32 [1]")
    if out is None:
        out = torch.empty_like(logits)
    _check_f32("grad_logits", out, dev, (B, Q, T), "token_focal_loss_backward: grad_logits must be float32 [B, Q, T]")
    _launch(dev, lib.criterion_hip_token_focal_backward_f32, logits.data_ptr(), _ptr(text_mask), kind, row_target.data_ptr(), pm, G,
            float(alpha), scale.data_ptr(), B, Q, T, out.data_ptr())
    return out


def mask_losses_supported(src, gt):
    """What the criterion_hip_mask_losses_* kernels accept: contiguous fp32 [n, F, h, w] logits on a GPU and contiguous bool / uint8
    [B, G_max, H_im, W_im] padded masks on the same one."""
    return (src.is_cuda and src.dtype == torch.float32 and src.dim() == 4 and src.is_contiguous() and gt.device == src.device
            and gt.dtype in (torch.bool, torch.uint8) and gt.is_contiguous())


def _mask_losses_args(who, src, gt, gt_row, stride):
    dev = src.device
    _check("src", src, dev)
    if src.dtype != torch.float32 or src.dim() != 4:
        raise RuntimeError("%s: src must be float32 [n, F, h, w]" % who)
    n, F, h, w = src.shape
    _check("gt", gt, dev)
    if gt.dtype not in (torch.bool, torch.uint8) or gt.dim() < 3:
        raise RuntimeError("%s: gt must be bool or uint8 [..., H_im, W_im]" % who)
    H_im, W_im = gt.shape[-2:]
    R = gt.numel() // max(H_im * W_im, 1)
    _i32("gt_row", gt_row, dev, (n,))
    return dev, n, F, h, w, R, H_im, W_im, int(stride)


def mask_losses_forward(src, gt, gt_row, stride, num_boxes, out=None, workspace=None):
    """Focal and dice loss of instance masks against strided pixels of the padded ground truth (include/dynmask_hip.h:
    criterion_hip_mask_losses_forward_f32).  src [n, F, h, w] fp32; gt bool / uint8 [R, H_im, W_im] (leading dimensions flattened);
    gt_row [n] int32, the first of an instance's F rows.  Returns (losses [2] = (loss_mask, loss_dice), sums [n, 4]); `out` may
    supply the two, `workspace` the scratch."""
    lib = _lib.load()
    dev, n, F, h, w, R, H_im, W_im, stride = _mask_losses_args("mask_losses_forward", src, gt, gt_row, stride)
    if out is None:
        out = (torch.empty((2,), dtype=torch.float32, device=dev), torch.empty((n, 4), dtype=torch.float32, device=dev))
    losses, sums = out
    _check_f32("losses", losses, dev, (2,), "mask_losses_forward: losses must be float32 [2]")
    _check_f32("sums", sums, dev, (n, 4), "mask_losses_forward: sums must be float32 [n, 4]")
    nbytes = lib.criterion_hip_workspace_bytes(_lib.CRITERION_MASK_LOSSES, n, F * h * w)
    ws = _workspace(nbytes, dev) if workspace is None else workspace
    _launch(dev, lib.criterion_hip_mask_losses_forward_f32, src.data_ptr(), gt.data_ptr(), gt_row.data_ptr(), n, F, h, w, R, H_im,
            W_im, stride, float(num_boxes), sums.data_ptr(), losses.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size())
    return losses, sums


def mask_losses_backward(src, gt, gt_row, stride, num_boxes, sums, grad_mask, grad_dice, out=None):
    """grad_src [n, F, h, w] of both losses in one pass (criterion_hip_mask_losses_backward_f32); grad_mask and grad_dice are [1] fp32
    tensors on the device, sums the forward's [n, 4].  Every element is written."""
    lib = _lib.load()
    dev, n, F, h, w, R, H_im, W_im, stride = _mask_losses_args("mask_losses_backward", src, gt, gt_row, stride)
    _check_f32("sums", sums, dev, (n, 4), "mask_losses_backward: sums must be float32 [n, 4]")
    _check_f32("grad_mask", grad_mask, dev, (1,), "mask_losses_backward: grad_mask must be float32 [1]")
    _check_f32("grad_dice", grad_dice, dev, (1,), "mask_losses_backward: grad_dice must be float32 [1]")
    if out is None:
        out = torch.empty_like(src)
    _check_f32("grad_src", out, dev, (n, F, h, w), "mask_losses_backward: grad_src must be float32 [n, F, h, w]")
    _launch(dev, lib.criterion_hip_mask_losses_backward_f32, src.data_ptr(), gt.data_ptr(), gt_row.data_ptr(), sums.data_ptr(),
            grad_mask.data_ptr(), grad_dice.data_ptr(), n, F, h, w, R, H_im, W_im, stride, float(num_boxes), out.data_ptr())
    return out


def box_bitmasks(boxes, height, width, out=None):
    """bool [G, height, width]: pixel (y, x) of box g set where int(y1) <= y < int(y2 + 1) and int(x1) <= x < int(x2 + 1)
    (include/dynmask_hip.h: criterion_hip_box_bitmasks).  boxes [G, 4] fp32 xyxy in pixels, >= 0; nothing is copied to the host."""
    lib = _lib.load()
    dev = boxes.device
    G = boxes.shape[0]
    _check_f32("boxes", boxes, dev, (G, 4), "box_bitmasks: boxes must be float32 [G, 4]")
    if out is None:
        out = torch.empty((G, height, width), dtype=torch.bool, device=dev)
    _check("out", out, dev)
    if out.dtype not in (torch.bool, torch.uint8) or tuple(out.shape) != (G, height, width):
        raise RuntimeError("box_bitmasks: out must be bool or uint8 [G, height, width]")
    _launch(dev, lib.criterion_hip_box_bitmasks, boxes.data_ptr(), G, int(height), int(width), out.data_ptr())
    return out


_SRGB_TABLES = {}


def srgb_linear_table(dev):
    """float64 [256] on `dev`: the sRGB linearisation of byte / 255, computed on the host once per device."""
    if dev not in _SRGB_TABLES:
        c = torch.arange(256, dtype=torch.float64) / 255
        _SRGB_TABLES[dev] = torch.where(c > 0.04045, ((c + 0.055) / 1.055) ** 2.4, c / 12.92).to(dev)
    return _SRGB_TABLES[dev]


def color_similarity(images, image_masks, stride, dilation, out=None, lab=None):
    """fp32 [bs, 8, H / stride, W / stride]: the colour similarity of every pooled pixel with its 8 neighbours at `dilation`, times
    the neighbour's mask (include/dynmask_hip.h: criterion_hip_color_similarity_f32).  images [bs, 3, H, W] BGR, uint8 or fp32 holding
    integers; image_masks [bs, H, W] bool / uint8.  `lab` ([bs, 3, h, w] fp32) receives the Lab image when given."""
    lib = _lib.load()
    dev = images.device
    _check("images", images, dev)
    if images.dtype not in (torch.uint8, torch.float32) or images.dim() != 4 or images.shape[1] != 3:
        raise RuntimeError("color_similarity: images must be uint8 or float32 [bs, 3, H, W]")
    bs, _, H, W = images.shape
    _check("image_masks", image_masks, dev)
    if image_masks.dtype not in (torch.bool, torch.uint8) or tuple(image_masks.shape) != (bs, H, W):
        raise RuntimeError("color_similarity: image_masks must be bool or uint8 [bs, H, W]")
    stride = int(stride)
    if stride <= 0 or H % stride or W % stride:
        raise RuntimeError("color_similarity: H and W must be multiples of the stride")
    h, w = H // stride, W // stride
    if out is None:
        out = torch.empty((bs, 8, h, w), dtype=torch.float32, device=dev)
    _check_f32("out", out, dev, (bs, 8, h, w), "color_similarity: out must be float32 [bs, 8, h, w]")
    _check_f32("lab", lab, dev, (bs, 3, h, w), "color_similarity: lab must be float32 [bs, 3, h, w]")
    kind = _lib.CRITERION_IMAGE_U8 if images.dtype == torch.uint8 else _lib.CRITERION_IMAGE_F32
    _launch(dev, lib.criterion_hip_color_similarity_f32, images.data_ptr(), kind, image_masks.data_ptr(), srgb_linear_table(dev).data_ptr(),
            bs, H, W, stride, int(dilation), out.data_ptr(), _ptr(lab))
    return out


def boxinst_losses_supported(src, gt, sim, dilation):
    """What the criterion_hip_boxinst_* kernels accept: contiguous fp32 [N, 1, h, w] logits on a GPU, contiguous bool / uint8 padded
    masks and a contiguous fp32 [B, 8, h, w] similarity on the same one, 1 <= dilation <= 8, rows that fit the LDS tile."""
    return (src.is_cuda and src.dtype == torch.float32 and src.dim() == 4 and src.shape[1] == 1 and src.is_contiguous()
            and gt.device == src.device and gt.dtype in (torch.bool, torch.uint8) and gt.is_contiguous()
            and sim.device == src.device and sim.dtype == torch.float32 and sim.dim() == 4 and sim.is_contiguous()
            and tuple(sim.shape[1:]) == (8,) + tuple(src.shape[2:]) and 1 <= int(dilation) <= _lib.BOXINST_MAX_DILATION
            and (_lib.BOXINST_BAND + 2 * int(dilation)) * 9 * src.shape[3] <= _lib.BOXINST_LDS_BYTES)


def _boxinst_args(who, src, inst, gt, gt_row, sim, img, warmup):
    dev = src.device
    _check("src", src, dev)
    if src.dtype != torch.float32 or src.dim() != 4:
        raise RuntimeError("%s: src must be float32 [N, F, h, w]" % who)
    N_all, F, h, w = src.shape
    _check("gt", gt, dev)
    if gt.dtype not in (torch.bool, torch.uint8) or gt.dim() < 3:
        raise RuntimeError("%s: gt must be bool or uint8 [..., H_im, W_im]" % who)
    H_im, W_im = gt.shape[-2:]
    R = gt.numel() // max(H_im * W_im, 1)
    n = inst.numel()
    _i32("inst", inst, dev, (n,))
    _i32("gt_row", gt_row, dev, (n,))
    _i32("img", img, dev, (n,))
    _check("sim", sim, dev)
    if sim.dtype != torch.float32 or sim.dim() != 4 or tuple(sim.shape[1:]) != (8, h, w):
        raise RuntimeError("%s: sim must be float32 [B, 8, h, w]" % who)
    _check_f32("warmup", warmup, dev, (1,), "%s: warmup must be float32 [1]" % who)
    return dev, n, N_all, F, h, w, R, H_im, W_im, sim.shape[0]


def boxinst_losses_forward(src, inst, gt, gt_row, stride, sim, img, thresh, dilation, warmup, out=None, workspace=None):
    """(loss_prj, loss_pairwise) of BoxInst in one pass over the kept instances (include/dynmask_hip.h:
    criterion_hip_boxinst_forward_f32).  src [N, 1, h, w] fp32; inst [n] int32, the row of src an instance reads; gt / gt_row / stride
    as in mask_losses_forward; sim [B, 8, h, w] fp32 and img [n] int32; warmup a [1] fp32 tensor on the device.  Returns (losses [2],
    saved) with saved = (pos int32 [n, h + w], tmax uint8 [n, h + w], sums float64 [n, 4], totals float64 [2]) for the backward; `out` may supply
    (losses, pos, tmax, sums, totals), `workspace` the scratch."""
    lib = _lib.load()
    dev, n, N_all, F, h, w, R, H_im, W_im, B = _boxinst_args("boxinst_losses_forward", src, inst, gt, gt_row, sim, img, warmup)
    if out is None:
        out = (torch.empty((2,), dtype=torch.float32, device=dev), torch.empty((n, h + w), dtype=torch.int32, device=dev),
               torch.empty((n, h + w), dtype=torch.uint8, device=dev), torch.empty((n, 4), dtype=torch.float64, device=dev),
               torch.empty((2,), dtype=torch.float64, device=dev))
    losses, pos, tmax, sums, totals = out
    _check_f32("losses", losses, dev, (2,), "boxinst_losses_forward: losses must be float32 [2]")
    _i32("pos", pos, dev, (n, h + w))
    _check("tmax", tmax, dev)
    _check("totals", totals, dev)
    _check("sums", sums, dev)
    if tmax.dtype != torch.uint8 or tuple(tmax.shape) != (n, h + w) or totals.dtype != torch.float64 or tuple(totals.shape) != (2,) \
            or sums.dtype != torch.float64 or tuple(sums.shape) != (n, 4):
        raise RuntimeError("boxinst_losses_forward: tmax must be uint8 [n, h + w], sums float64 [n, 4] and totals float64 [2]")
    nbytes = lib.criterion_hip_workspace_bytes(_lib.CRITERION_BOXINST, n, F * h * w)
    ws = _workspace(nbytes, dev) if workspace is None else workspace
    _launch(dev, lib.criterion_hip_boxinst_forward_f32, src.data_ptr(), inst.data_ptr(), gt.data_ptr(), gt_row.data_ptr(), sim.data_ptr(),
            img.data_ptr(), warmup.data_ptr(), n, N_all, F, h, w, R, H_im, W_im, int(stride), B, float(thresh), int(dilation),
            pos.data_ptr(), tmax.data_ptr(), sums.data_ptr(), totals.data_ptr(), losses.data_ptr(), ws.data_ptr(),
            ws.numel() * ws.element_size())
    return losses, (pos, tmax, sums, totals)


def boxinst_losses_backward(src, inst, gt, gt_row, stride, sim, img, thresh, dilation, warmup, saved, grad_prj, grad_pairwise, out=None):
    """grad_src [N, 1, h, w] of both losses in one pass (criterion_hip_boxinst_backward_f32): every element written, exactly 0.0 in the
    rows `inst` does not name.  grad_prj and grad_pairwise are [1] fp32 tensors on the device, `saved` the forward's."""
    lib = _lib.load()
    dev, n, N_all, F, h, w, R, H_im, W_im, B = _boxinst_args("boxinst_losses_backward", src, inst, gt, gt_row, sim, img, warmup)
    pos, tmax, sums, totals = saved
    _i32("pos", pos, dev, (n, h + w))
    _check("tmax", tmax, dev)
    _check("totals", totals, dev)
    _check("sums", sums, dev)
    if tmax.dtype != torch.uint8 or tuple(tmax.shape) != (n, h + w) or totals.dtype != torch.float64 or tuple(totals.shape) != (2,) \
            or sums.dtype != torch.float64 or tuple(sums.shape) != (n, 4):
        raise RuntimeError("boxinst_losses_backward: tmax must be uint8 [n, h + w], sums float64 [n, 4] and totals float64 [2]")
    _check_f32("grad_prj", grad_prj, dev, (1,), "boxinst_losses_backward: grad_prj must be float32 [1]")
    _check_f32("grad_pairwise", grad_pairwise, dev, (1,), "boxinst_losses_backward: grad_pairwise must be float32 [1]")
    if out is None:
        out = torch.empty_like(src)
    _check_f32("grad_src", out, dev, (N_all, F, h, w), "boxinst_losses_backward: grad_src must be float32 [N, F, h, w]")
    _launch(dev, lib.criterion_hip_boxinst_backward_f32, src.data_ptr(), inst.data_ptr(), gt.data_ptr(), gt_row.data_ptr(), sim.data_ptr(),
            img.data_ptr(), warmup.data_ptr(), pos.data_ptr(), tmax.data_ptr(), sums.data_ptr(), totals.data_ptr(), grad_prj.data_ptr(),
            grad_pairwise.data_ptr(), n, N_all, F, h, w, R, H_im, W_im, int(stride), B, float(thresh), int(dilation), out.data_ptr())
    return out


def matcher_cost(logits, boxes, tgt_boxes, positive_map, w_class, w_bbox, w_giou):
    """[num_pred, num_gt] fp32 cost matrix of HungarianMatcherVL.forward in one kernel (include/matcher_cost_hip.h): the same
    float32 operations in the same order as the PyTorch composition of matcher.py:476-498.  logits [num_pred, T], boxes
    [num_pred, 4], tgt_boxes [num_gt, 4] fp32 on one GPU; positive_map [num_gt, T] bool (or 0 / 1)."""
    lib = _lib.load()
    dev = logits.device
    for name, t in (("logits", logits), ("boxes", boxes), ("tgt_boxes", tgt_boxes)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.device == dev):
            raise RuntimeError("matcher_cost: %s has to be a 2-d float32 tensor on the GPU of the logits" % name)
    num_pred, T = logits.shape
    G = tgt_boxes.shape[0]
    if boxes.shape != (num_pred, 4) or tgt_boxes.shape[1] != 4 or tuple(positive_map.shape) != (G, T):
        raise RuntimeError("matcher_cost: shapes do not fit together")
    logits, boxes, tgt_boxes = logits.contiguous(), boxes.contiguous(), tgt_boxes.contiguous()
    pm = positive_map.to(device=dev) != 0
    # CSR of the positive map, built on the device (nonzero() of a row-major mask lists the tokens of a target in order)
    tok_idx = pm.nonzero()[:, 1].to(torch.int32).contiguous()
    tok_off = torch.zeros(G + 1, dtype=torch.int32, device=dev)
    tok_off[1:] = pm.sum(1).cumsum(0).to(torch.int32)
    cost = torch.empty((num_pred, G), dtype=torch.float32, device=dev)
    _launch(dev, lib.matcher_cost_hip_f32, logits.data_ptr(), boxes.data_ptr(), tgt_boxes.data_ptr(), tok_off.data_ptr(),
            _ptr(tok_idx if tok_idx.numel() else None), num_pred, T, G, float(w_class), float(w_bbox), float(w_giou),
            cost.data_ptr())
    return cost


def _batch_offsets(sizes):
    """Per-image counts -> (offsets as a Python list, the same as the int32 host array the ota_* entry points take)."""
    off = [0]
    for n in sizes:
        off.append(off[-1] + int(n))
    return off, (ctypes.c_int32 * len(off))(*off)


def ota_assign(class_table, boxes, tgt_boxes, positive_map, sizes, max_rounds=10000):
    """simOTA assignment of a whole batch on the device (include/ota_hip.h): two kernels, nothing returns to the host.
    class_table [bs, Q, T] fp32 (the focal table pos - neg of matcher.py:327-330), boxes [bs, Q, 4] cxcywh, tgt_boxes
    [G_total, 4], positive_map [G_total, T] bool / uint8 -- targets of all images concatenated, `sizes` their counts per image
    (Python ints).  Returns device tensors (sel_query [bs, Q] int64, sel_gt [bs, Q] int64, matched_query [G_total] int64,
    num_selected [bs] int32, status [bs] int32): image b's assignment is sel_query[b, :num_selected[b]] (ascending) with the
    target sel_gt[b, :num_selected[b]] each, and matched_query[off_b : off_b + G_b] the cheapest own query of every target."""
    lib = _lib.load()
    dev = class_table.device
    bs, Q, T = class_table.shape
    if bs > _lib.OTA_MAX_BATCH:
        raise RuntimeError("ota_assign: at most %d images per call" % _lib.OTA_MAX_BATCH)
    for name, t, shape in (("class_table", class_table, (bs, Q, T)), ("boxes", boxes, (bs, Q, 4)), ("tgt_boxes", tgt_boxes, (sum(sizes), 4))):
        if not (t.is_cuda and t.device == dev and t.dtype == torch.float32 and tuple(t.shape) == shape):
            raise RuntimeError("ota_assign: %s has to be a float32 tensor of shape %s on the GPU of the table" % (name, (shape,)))
    if tuple(positive_map.shape) != (sum(sizes), T) or positive_map.dtype not in (torch.bool, torch.uint8) or positive_map.device != dev:
        raise RuntimeError("ota_assign: positive_map has to be [G_total, T] bool / uint8 on the same GPU")
    class_table, boxes, tgt_boxes = class_table.contiguous(), boxes.contiguous(), tgt_boxes.contiguous()
    pm = positive_map.contiguous().view(torch.uint8)
    off, gt_off = _batch_offsets(sizes)
    G = off[-1]
    cost = torch.empty(Q * G, dtype=torch.float32, device=dev)
    iou = torch.empty(Q * G, dtype=torch.float32, device=dev)
    flags = torch.empty(Q * G, dtype=torch.uint8, device=dev)
    matching = torch.empty(Q * G, dtype=torch.uint8, device=dev)
    sel_q = torch.empty((bs, Q), dtype=torch.int64, device=dev)
    sel_g = torch.empty((bs, Q), dtype=torch.int64, device=dev)
    matched = torch.empty(G, dtype=torch.int64, device=dev)
    count = torch.empty(bs, dtype=torch.int32, device=dev)
    status = torch.empty(bs, dtype=torch.int32, device=dev)
    # without targets (G == 0) everything sized by G is passed as NULL
    tgt_p, pm_p, cost_p, iou_p, flags_p, matching_p, matched_p = (
        _ptr(t if G else None) for t in (tgt_boxes, pm, cost, iou, flags, matching, matched))
    with torch.cuda.device(dev):    # both kernels under one guard, on one stream
        stream = _stream()
        rc = lib.ota_cost_hip_f32(class_table.data_ptr(), boxes.data_ptr(), tgt_p, pm_p, gt_off, bs, Q, T, cost_p, iou_p, flags_p,
                                  stream)
        if rc != 0:
            _raise(rc)
        rc = lib.ota_dynamic_k_hip(cost_p, iou_p, flags_p, matching_p, gt_off, bs, Q, int(max_rounds), sel_q.data_ptr(),
                                   sel_g.data_ptr(), matched_p, count.data_ptr(), status.data_ptr(), stream)
        if rc != 0:
            _raise(rc)
    return sel_q, sel_g, matched, count, status


def lsap_batch(costs, check=True):
    """Linear sum assignment of each 2-d fp32 GPU cost matrix in `costs` (row-major views with any row stride, e.g.
    column slices of one big matrix) on the device, with SciPy's result index for index (include/lsap_hip.h).
    Returns a list of (row_ind, col_ind) int64 GPU tensors.  check=True synchronises once at the end and raises
    ValueError where SciPy would (NaN / -inf entries, infeasible matrix); check=False never leaves the stream."""
    lib = _lib.load()
    if not costs:
        return []
    dev = costs[0].device
    for c in costs:
        if not (c.is_cuda and c.device == dev and c.dtype == torch.float32 and c.dim() == 2):
            raise RuntimeError("lsap_batch: expected 2-d float32 tensors on one GPU")
        if c.numel() and (c.stride(1) != 1 or c.stride(0) < c.shape[1]):
            raise RuntimeError("lsap_batch: rows must be contiguous (row stride >= cols, column stride 1)")
    results, keep = [], []
    status = torch.full((len(costs),), -1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = _stream()
        for lo in range(0, len(costs), _lib.LSAP_MAX_BATCH):
            chunk = costs[lo:lo + _lib.LSAP_MAX_BATCH]
            n = len(chunk)
            P, LL, I = ctypes.c_void_p * n, ctypes.c_longlong * n, ctypes.c_int * n
            rows = [c.shape[0] for c in chunk]
            cols = [c.shape[1] for c in chunk]
            outs = [(torch.empty(min(r, k), dtype=torch.int64, device=dev), torch.empty(min(r, k), dtype=torch.int64, device=dev))
                    for r, k in zip(rows, cols)]
            ws = [torch.empty(lib.lsap_hip_workspace_bytes(r, k), dtype=torch.uint8, device=dev) for r, k in zip(rows, cols)]
            keep.append(ws)
            rc = lib.lsap_hip_batch_f32(
                n, P(*[_ptr(c if c.numel() else None) for c in chunk]),
                LL(*[c.stride(0) if c.numel() else max(k, 1) for c, k in zip(chunk, cols)]), I(*rows), I(*cols),
                P(*[_ptr(o[0] if o[0].numel() else None) for o in outs]),
                P(*[_ptr(o[1] if o[1].numel() else None) for o in outs]), P(*[w.data_ptr() for w in ws]),
                P(*[status[lo + k:].data_ptr() for k in range(n)]), stream)
            if rc != 0:
                _raise(rc)
            results += outs
    if check:
        st = status.cpu().tolist()      # also keeps the workspaces alive until the kernels are done
        if any(s == 1 for s in st):
            raise ValueError("matrix contains invalid numeric entries")
        if any(s == 2 for s in st):
            raise ValueError("cost matrix is infeasible")
    else:
        for ws in keep:                 # the caching allocator may hand the workspace out again: tie it to the stream
            for w in ws:
                w.record_stream(torch.cuda.current_stream())
    return results


def lsap(cost, check=True):
    """scipy.optimize.linear_sum_assignment(cost) for one 2-d fp32 GPU matrix, on the device."""
    return lsap_batch([cost], check)[0]


def upsample_add(skip, low):
    """`skip + F.interpolate(low, size=skip.shape[-2:], mode="nearest")` in one pass (include/conv3x3_hip.h)."""
    lib = _lib.load()
    _check("skip", skip, skip.device)
    _check("low", low, skip.device)
    if skip.dtype != torch.float32 or low.dtype != torch.float32 or skip.dim() != 4 or low.dim() != 4 \
            or skip.shape[:2] != low.shape[:2]:
        raise RuntimeError("upsample_add: expected float32 skip [B, C, H, W] and low [B, C, h, w]")
    B, C, H, W = skip.shape
    out = torch.empty_like(skip)
    _launch(skip.device, lib.upsample_add_hip_f32, skip.data_ptr(), low.data_ptr(), B, C, H, W, low.shape[2], low.shape[3],
            out.data_ptr())
    return out


def linear_packed_ln_supported(x, weight, norm_shape):
    return linear_packed_supported(x, weight) and weight.shape[0] == 256 and tuple(norm_shape) == (256,)


def linear_packed_ln(x, packed, bias, residual, ln_weight, ln_bias, eps):
    """LayerNorm(residual + F.linear(x, W, bias)) * ln_weight + ln_bias with the add and the normalisation in the
    Linear's epilogue (include/linear_hip.h; out_features == 256).  x [..., in_features] -> [..., 256]."""
    lib = _lib.load()
    _check("x", x, x.device)
    _check("packed", packed, x.device)
    k, n = x.shape[-1], 256
    rows = x.numel() // k if k else 0
    for name, t, shape in (("bias", bias, (n,)), ("ln_weight", ln_weight, (n,)), ("ln_bias", ln_bias, (n,)),
                           ("residual", residual, x.shape[:-1] + (n,))):
        _check_f32(name, t, x.device, shape, "linear_packed_ln: %s must be float32 %s" % (name, tuple(shape)))
    if x.dtype != torch.float32 or packed.dtype != torch.uint8 or packed.numel() != lib.linear_hip_packed_weight_bytes(n, k) \
            or packed.numel() == 0:
        raise RuntimeError("linear_packed_ln: expected float32 x and the packed copy of a [256, %d] weight" % k)
    out = torch.empty(x.shape[:-1] + (n,), dtype=torch.float32, device=x.device)
    _launch(x.device, lib.linear_hip_packed_ln_f32, x.data_ptr(), packed.data_ptr(), _ptr(bias), _ptr(residual), _ptr(ln_weight),
            _ptr(ln_bias), float(eps), rows, k, n, out.data_ptr())
    return out


def ffn_packed_supported(x, weight1, weight2, norm_shape=None):
    """True when linear_hip_packed_ffn_f32 covers `linear2(relu(linear1(x)))` (+ residual, + LayerNorm): fp32 GPU
    tensors, d_model == 256, d_ffn a multiple of 128."""
    return (x.is_cuda and x.dtype == torch.float32 and x.shape[-1] == 256
            and weight1.dtype == torch.float32 and weight2.dtype == torch.float32
            and weight1.dim() == 2 and weight2.dim() == 2 and weight1.shape[1] == 256 and weight2.shape[0] == 256
            and weight1.shape[0] == weight2.shape[1] and weight1.shape[0] % 128 == 0
            and (norm_shape is None or tuple(norm_shape) == (256,)))


def ffn_packed(x, packed1, bias1, packed2, bias2, d_ffn, residual=None, ln_weight=None, ln_bias=None, eps=1e-5,
               layer_norm=True):
    """[LayerNorm](residual + F.linear(relu(F.linear(x, W1, bias1)), W2, bias2)) in one kernel: the hidden activations
    stay on the CU (include/linear_hip.h).  packed1 / packed2 = linear_pack_weight(W1 [d_ffn, 256]) / (W2 [256, d_ffn]).
    Bitwise equal to linear_packed_forward(..., relu=True) followed by linear_packed_ln / linear_packed_forward."""
    lib = _lib.load()
    _check("x", x, x.device)
    _check("packed1", packed1, x.device)
    _check("packed2", packed2, x.device)
    k, n = x.shape[-1], 256
    rows = x.numel() // k if k else 0
    for name, t, shape in (("bias1", bias1, (d_ffn,)), ("bias2", bias2, (n,)), ("ln_weight", ln_weight, (n,)),
                           ("ln_bias", ln_bias, (n,)), ("residual", residual, tuple(x.shape))):
        _check_f32(name, t, x.device, shape, "ffn_packed: %s must be float32 %s" % (name, tuple(shape)))
    if (x.dtype != torch.float32 or k != n or d_ffn <= 0 or d_ffn % 128 != 0 or packed1.dtype != torch.uint8
            or packed2.dtype != torch.uint8 or packed1.numel() != lib.linear_hip_packed_weight_bytes(d_ffn, k)
            or packed2.numel() != lib.linear_hip_packed_weight_bytes(n, d_ffn)):
        raise RuntimeError("ffn_packed: expected float32 x [..., 256] and the packed copies of [%d, 256] and [256, %d] "
                           "weights (d_ffn a multiple of 128)" % (d_ffn, d_ffn))
    out = torch.empty_like(x)
    _launch(x.device, lib.linear_hip_packed_ffn_f32, x.data_ptr(), packed1.data_ptr(), _ptr(bias1), packed2.data_ptr(), _ptr(bias2),
            _ptr(residual), _ptr(ln_weight), _ptr(ln_bias), float(eps), 1 if layer_norm else 0, rows, k, d_ffn, out.data_ptr())
    return out


# ---- re-ID contrastive training (include/ota_hip.h: ota_reid_*; uninext_amd/reid.py) ----------------------------------------------
def _reid_out(out, shapes, dev):
    """The output tensors: `out` (a tuple given by the caller, checked) or fresh ones of (shape, dtype)."""
    if out is None:
        return tuple(torch.empty(shape, dtype=dtype, device=dev) for shape, dtype in shapes)
    if len(out) != len(shapes):
        raise RuntimeError("reid: expected %d output tensors" % len(shapes))
    for t, (shape, dtype) in zip(out, shapes):
        if not (t.is_cuda and t.device == dev and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous()):
            raise RuntimeError("reid: an output tensor has to be contiguous %s of shape %s on the inputs' GPU" % (dtype, tuple(shape)))
    return tuple(out)


def reid_select(class_table, boxes, tgt_boxes, positive_map, valid, key_index, sizes, num_key_queries, max_rounds=10000, out=None):
    """Positive / negative selection of a whole batch on the device (include/ota_hip.h: ota_cost_hip_f32, ota_reid_select_hip): two
    kernels, nothing returns to the host.  class_table [bs, Q, T] fp32 (the focal table of pos_neg_select.py:113-114), boxes
    [bs, Q, 4], tgt_boxes [G_total, 4], positive_map [G_total, T] bool / uint8, valid [G_total] uint8, key_index [G_total] int64,
    `sizes` the targets per image.  Returns device tensors (cost, iou, flags, matching_pos, matching_neg, words): the byte
    matrices in the batch layout and words int32 [2 * G_total + bs] = the (n_pos, n_neg) pairs, then the status of every image."""
    lib = _lib.load()
    dev = class_table.device
    bs, Q, T = class_table.shape
    off, gt_off = _batch_offsets(sizes)
    G = off[-1]
    if len(sizes) != bs or not 0 < bs <= _lib.OTA_MAX_BATCH or G == 0:
        raise RuntimeError("reid_select: 1 .. %d images with at least one target" % _lib.OTA_MAX_BATCH)
    for name, t, shape, dtypes in (("class_table", class_table, (bs, Q, T), (torch.float32,)), ("boxes", boxes, (bs, Q, 4), (torch.float32,)),
                                   ("tgt_boxes", tgt_boxes, (G, 4), (torch.float32,)), ("positive_map", positive_map, (G, T), (torch.bool, torch.uint8)),
                                   ("valid", valid, (G,), (torch.uint8,)), ("key_index", key_index, (G,), (torch.int64,))):
        if not (t.is_cuda and t.device == dev and t.dtype in dtypes and tuple(t.shape) == shape and t.is_contiguous()):
            raise RuntimeError("reid_select: %s has to be a contiguous %s tensor of shape %s on the table's GPU" % (name, dtypes[0], shape))
    cost, iou, flags, mpos, mneg, words = _reid_out(out, [((Q * G,), torch.float32), ((Q * G,), torch.float32), ((Q * G,), torch.uint8),
                                                          ((Q * G,), torch.uint8), ((Q * G,), torch.uint8), ((2 * G + bs,), torch.int32)], dev)
    pm = positive_map.view(torch.uint8)
    with torch.cuda.device(dev):
        stream = _stream()
        rc = lib.ota_cost_hip_f32(class_table.data_ptr(), boxes.data_ptr(), tgt_boxes.data_ptr(), pm.data_ptr(), gt_off, bs, Q, T,
                                  cost.data_ptr(), iou.data_ptr(), flags.data_ptr(), stream)
        if rc != 0:
            _raise(rc)
        rc = lib.ota_reid_select_hip(cost.data_ptr(), iou.data_ptr(), flags.data_ptr(), valid.data_ptr(), key_index.data_ptr(), gt_off, bs, Q,
                                 int(num_key_queries), int(max_rounds), mpos.data_ptr(), mneg.data_ptr(), words.data_ptr(),
                                 words.data_ptr() + 8 * G, stream)
        if rc != 0:
            _raise(rc)
    return cost, iou, flags, mpos, mneg, words


def reid_scores(ref_embeds, key_embeds, key_index, valid, sizes, out=None):
    """dot, cos [Q * G_total] (batch layout), ref_norm [bs, Q], key_norm [G_total] of include/ota_hip.h: ota_reid_scores_hip_f32."""
    lib = _lib.load()
    dev = ref_embeds.device
    bs, Q, C = ref_embeds.shape
    Qk = key_embeds.shape[1]
    off, gt_off = _batch_offsets(sizes)
    G = off[-1]
    for name, t, shape, dtype in (("ref_embeds", ref_embeds, (bs, Q, C), torch.float32), ("key_embeds", key_embeds, (bs, Qk, C), torch.float32),
                                  ("key_index", key_index, (G,), torch.int64), ("valid", valid, (G,), torch.uint8)):
        if not (t.is_cuda and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()):
            raise RuntimeError("reid_scores: %s has to be a contiguous %s tensor of shape %s on one GPU" % (name, dtype, shape))
    if len(sizes) != bs or G == 0:
        raise RuntimeError("reid_scores: one size per image, at least one target")
    dot, cos, ref_norm, key_norm = _reid_out(out, [((Q * G,), torch.float32), ((Q * G,), torch.float32), ((bs, Q), torch.float32),
                                                   ((G,), torch.float32)], dev)
    _launch(dev, lib.ota_reid_scores_hip_f32, ref_embeds.data_ptr(), key_embeds.data_ptr(), key_index.data_ptr(), valid.data_ptr(), gt_off, bs,
            Q, Qk, C, dot.data_ptr(), cos.data_ptr(), ref_norm.data_ptr(), key_norm.data_ptr())
    return dot, cos, ref_norm, key_norm


def reid_loss_forward(dot, cos, matching_pos, matching_neg, item_meta, ranks, sizes, num_queries, out=None):
    """(losses [2] = loss_reid, loss_reid_aux; roles uint8 [n_items, Q]; item_stats float64 [n_items, 6]) of ota_reid_loss_hip_f32.
    item_meta int32 [n_items, 5], ranks int32 (at least one element, also when nothing is sampled)."""
    lib = _lib.load()
    dev = dot.device
    off, gt_off = _batch_offsets(sizes)
    Q, G, n = int(num_queries), off[-1], item_meta.shape[0]
    for name, t, shape, dtype in (("dot", dot, (Q * G,), torch.float32), ("cos", cos, (Q * G,), torch.float32),
                                  ("matching_pos", matching_pos, (Q * G,), torch.uint8), ("matching_neg", matching_neg, (Q * G,), torch.uint8),
                                  ("item_meta", item_meta, (n, _lib.REID_META), torch.int32), ("ranks", ranks, (ranks.numel(),), torch.int32)):
        if not (t.is_cuda and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()):
            raise RuntimeError("reid_loss_forward: %s has to be a contiguous %s tensor of shape %s on one GPU" % (name, dtype, shape))
    if n == 0 or ranks.numel() == 0:
        raise RuntimeError("reid_loss_forward: at least one item and one element of ranks")
    losses, roles, stats = _reid_out(out, [((2,), torch.float32), ((n, Q), torch.uint8), ((n, _lib.REID_STATS), torch.float64)], dev)
    _launch(dev, lib.ota_reid_loss_hip_f32, dot.data_ptr(), cos.data_ptr(), matching_pos.data_ptr(), matching_neg.data_ptr(), item_meta.data_ptr(),
            ranks.data_ptr(), gt_off, len(sizes), Q, n, roles.data_ptr(), stats.data_ptr(), losses.data_ptr())
    return losses, roles, stats


def reid_loss_backward(ref_embeds, key_embeds, key_index, dot, cos, ref_norm, key_norm, roles, item_stats, item_meta, item_counts,
                       grad_losses, sizes, out=None, workspace=None):
    """(grad_ref [bs, Q, C], grad_key [bs, Qk, C]) of ota_reid_loss_bwd_hip_f32.  item_counts: the items per image (Python ints);
    grad_losses [2] fp32 on the device; workspace: (coef [2, n_items, Q], key_item_grad [n_items, C]) or None."""
    lib = _lib.load()
    dev = ref_embeds.device
    bs, Q, C = ref_embeds.shape
    Qk = key_embeds.shape[1]
    off, gt_off = _batch_offsets(sizes)
    ioff, item_off = _batch_offsets(item_counts)
    G, n = off[-1], ioff[-1]
    for name, t, shape, dtype in (("ref_embeds", ref_embeds, (bs, Q, C), torch.float32), ("key_embeds", key_embeds, (bs, Qk, C), torch.float32),
                                  ("key_index", key_index, (G,), torch.int64), ("dot", dot, (Q * G,), torch.float32), ("cos", cos, (Q * G,), torch.float32),
                                  ("ref_norm", ref_norm, (bs, Q), torch.float32), ("key_norm", key_norm, (G,), torch.float32),
                                  ("roles", roles, (n, Q), torch.uint8), ("item_stats", item_stats, (n, _lib.REID_STATS), torch.float64),
                                  ("item_meta", item_meta, (n, _lib.REID_META), torch.int32), ("grad_losses", grad_losses, (2,), torch.float32)):
        if not (t.is_cuda and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()):
            raise RuntimeError("reid_loss_backward: %s has to be a contiguous %s tensor of shape %s on one GPU" % (name, dtype, shape))
    if len(sizes) != bs or len(item_counts) != bs or n == 0:
        raise RuntimeError("reid_loss_backward: one size and one item count per image, at least one item")
    grad_ref, grad_key = _reid_out(out, [((bs, Q, C), torch.float32), ((bs, Qk, C), torch.float32)], dev)
    coef, key_item_grad = _reid_out(workspace, [((2, n, Q), torch.float32), ((n, C), torch.float32)], dev)
    _launch(dev, lib.ota_reid_loss_bwd_hip_f32, ref_embeds.data_ptr(), key_embeds.data_ptr(), key_index.data_ptr(), dot.data_ptr(), cos.data_ptr(),
            ref_norm.data_ptr(), key_norm.data_ptr(), roles.data_ptr(), item_stats.data_ptr(), item_meta.data_ptr(), item_off,
            grad_losses.data_ptr(), gt_off, bs, Q, Qk, C, n, coef.data_ptr(), key_item_grad.data_ptr(), grad_ref.data_ptr(), grad_key.data_ptr())
    return grad_ref, grad_key
