"""ctypes binding of libmsda_hip.so: the C ABI declared by the ten headers under include/.  Loading never falls back
to anything: if the HIP library is absent the import of the op fails loudly (there is no CPU or eager path).

To add an operator: declare its prototype in a header under include/, give it one row in `_SIGNATURES` below under that
header (tests/test_binding_signatures_cpu.py holds every row to the header), and write its launcher in ext.py."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MSDA_HIP_LIB points the binding at another build of the SAME library (A/B builds of experimental kernels)
LIB_PATH = os.environ.get("MSDA_HIP_LIB") or os.path.join(_HERE, "lib", "libmsda_hip.so")

ABI_VERSION = 2   # include/msda_hip.h: MSDA_HIP_ABI_VERSION (what each number added: docs/DESIGN_HISTORY.md)

i, p, s, f = ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_float
u, z, ll, dp = ctypes.c_uint, ctypes.c_size_t, ctypes.c_longlong, ctypes.POINTER(ctypes.c_double)
_FWD = [p, p, p, p, p, i, i, i, i, i, i, i, p]                # msda forward / backward up to the outputs; then the stream
_BWD = [p, p, p, p, p, p, i, i, i, i, i, i, i, p, p, p]       # (device entry points) or the number of threads (host)

# header under include/ -> {exported function: (restype, argtypes)}, the whole C ABI.  The stream is the last parameter of
# every device entry point.
_SIGNATURES = {
    "msda_hip.h": {
        "msda_hip_abi_version": (i, []),
        "msda_hip_last_error": (s, []),
        "msda_hip_forward_f32": (i, _FWD + [p]),
        "msda_hip_forward_f64": (i, _FWD + [p]),
        "msda_hip_backward_f32": (i, _BWD + [p]),
        "msda_hip_backward_workspace_bytes": (z, [i, i, i, i, i, i, i]),
        "msda_hip_backward_ws_f32": (i, _BWD + [p, z, p]),
        "msda_hip_backward_f64": (i, _BWD + [p]),
        "msda_hip_forward_fused_f32": (i, [p, p, p, p, i, p, p, i, i, i, i, i, i, i, p, p]),
        "msda_hip_forward_fused_hm_f32": (i, [p, p, p, p, i, p, p, i, i, i, i, i, i, i, p, p]),
        "msda_hip_prologue_f32": (i, [p, p, i, p, p, i, i, i, i, i, p, p, p]),
        "msda_hip_prologue_backward_f32": (i, [p, p, i, p, p, p, p, i, i, i, i, i, p, p, p, p]),
        "msda_host_forward_f32": (i, _FWD + [i]),
        "msda_host_forward_f64": (i, _FWD + [i]),
        "msda_host_backward_f32": (i, _BWD + [i]),
        "msda_host_backward_f64": (i, _BWD + [i]),
        "msda_host_last_num_threads": (i, []),
        "msda_hip_set_variant": (i, [i, i]),
        "msda_hip_get_variant": (i, [i]),
        "msda_hip_variant_name": (s, [i, i]),
        "msda_hip_last_kernel": (s, [i]),
        "msda_hip_set_call_context": (None, [i, u]),
        "msda_hip_forward_locality": (i, [dp]),
        "msda_hip_reset_call_site": (None, [i]),
        "msda_hip_set_lanegroup_general": (None, [i]),
    },
    "dynmask_hip.h": {
        "dynmask_hip_forward_f32": (i, [p, p, p, p, i, i, i, i, i, i, p, p]),
        "aligned_bilinear_hip_f32": (i, [p, i, i, i, i, p, p]),
        "dynmask_hip_set_variant": (i, [i]),
        "dynmask_hip_last_kernel": (s, []),
        "dynmask_hip_backward_workspace_bytes": (z, [i, i, i]),
        "dynmask_hip_backward_parts": (i, [i, i, i]),
        "dynmask_hip_backward_f32": (i, [p, p, p, p, i, i, i, i, i, i, p, p, p, p, p, z, p]),
        "aligned_bilinear_hip_backward_f32": (i, [p, i, i, i, i, p, p]),
        "qsel_scores_hip_f32": (i, [p, p, p, i, p, p, p, p, p, f, p, ll, p, ll, p, f, i, ll, i, p, p, p]),
        "qsel_boxes_hip_f32": (i, [p, p, p, i, p, p, p, p, p, f, p, ll, p, p, p, p, p, p, i, ll, i, p, p, p]),
        "qsel_hip_last_kernel": (s, []),
        "pred_heads_hip_f32": (i, [p, p, ll, p, ll, p, f, p, i] + [p] * 14 + [i, i, ll, i, i, p, p, p, p, p]),
        "pred_heads_hip_set_variant": (i, [i]),
        "pred_heads_hip_last_kernel": (s, []),
        "detpost_scores_hip_f32": (i, [p, p, p, p, i, f, i, i, i, i, p, p, p, p, p]),
        "detpost_nms_hip_f32": (i, [p, p, p, f, i, i, i, p, p, p, p]),
        "detpost_hip_last_kernel": (s, []),
        "maskpost_binarize_hip_f32": (i, [p, p, i, i, i, i, i, i, i, i, i, f, p, p]),
        "maskpost_pack_hip_f32": (i, [p, p, i, i, i, i, p, p, p]),
        "maskpost_nms_hip_u32": (i, [p, p, i, i, f, p, p, p]),
        "maskpost_hip_last_kernel": (s, []),
        "track_hip_state_offset": (z, [i, i, i, i]),
        "track_hip_scores_f32": (i, [p, p, p, p, i, i, i, i, i, i, p, p, p, p]),
        "track_hip_associate_f32": (i, [p, p, p, p, p, p, p, i, i, i, i, i, i, f, f, f, i, i, p, p, p]),
        "track_hip_update_f32": (i, [p, p, p, p, p, p, p, i, i, i, i, i, f, f, i, p]),
        "track_hip_last_kernel": (s, []),
        "qdtrack_hip_state_offset": (z, [i, i, i, i, i]),
        "qdtrack_hip_prepare_f32": (i, [p, i, f, f, f, p, p, p, p]),
        "qdtrack_hip_scores_f32": (i, [p, p, p, p, p, i, i, i, i, i, i, i, i, i, i, i, p, p, p]),
        "qdtrack_hip_associate_f32": (i, [p, p, p, p, p, p, p, i, i, i, i, i, i, i, i, i, i, f, f, f, f, f, i, i, p, p, p]),
        "qdtrack_hip_update_f32": (i, [p, p, p, p, p, p, p, p, i, i, i, i, i, i, i, i, i, i, f, f, i, p]),
        "qdtrack_hip_last_kernel": (s, []),
        "criterion_hip_workspace_bytes": (z, [i, ll, ll]),
        "criterion_hip_last_kernel": (s, []),
        "criterion_hip_token_focal_forward_f32": (i, [p, p, i, p, p, i, f, i, i, i, p, p, z, p]),
        "criterion_hip_token_focal_backward_f32": (i, [p, p, i, p, p, i, f, p, i, i, i, p, p]),
        "criterion_hip_mask_losses_forward_f32": (i, [p, p, p, i, i, i, i, i, i, i, i, f, p, p, p, z, p]),
        "criterion_hip_mask_losses_backward_f32": (i, [p, p, p, p, p, p, i, i, i, i, i, i, i, i, f, p, p]),
        "criterion_hip_box_bitmasks": (i, [p, i, i, i, p, p]),
        "criterion_hip_color_similarity_f32": (i, [p, i, p, p, i, i, i, i, i, p, p, p]),
        "criterion_hip_boxinst_forward_f32": (i, [p] * 7 + [i] * 10 + [f, i] + [p] * 6 + [z, p]),
        "criterion_hip_boxinst_backward_f32": (i, [p] * 13 + [i] * 10 + [f, i, p, p]),
        "encprep_hip_workspace_bytes": (z, [i, p, i]),
        "encprep_hip_masks_u8": (i, [p, i, i, i, p, i, p, p, p, p, p]),
        "encprep_hip_pos_f32": (i, [p, p, p, p, p, i, p, i, i, f, f, p, p, p]),
        "encprep_hip_gn_stats_f32": (i, [p, i, p, i, i, i, p, z, p]),
        "encprep_hip_gn_apply_f32": (i, [p, p, p, p, p, z, i, p, i, i, i, p, p, p, p]),
        "encprep_hip_last_kernel": (s, []),
        "bert_hip_self_attention_f32": (i, [p, p, p, ll, ll, ll, p, i, i, i, i, i, f, p, p]),
        "bert_hip_embed_layernorm_f32": (i, [p, p, p, p, p, p, p, f, i, i, i, i, i, i, p, p]),
        "bert_hip_attention_last_kernel": (s, []),
        "bert_hip_embed_last_kernel": (s, []),
        "bert_hip_self_attention_train_f32": (i, [p, p, p, ll, ll, ll, p, i, i, i, i, i, f, p, p, f, p, p]),
        "bert_hip_self_attention_backward_workspace_bytes": (z, [i, i, i, i]),
        "bert_hip_self_attention_backward_f32": (i, [p, p, p, ll, ll, ll, p, i, p, p, p, i, i, i, i, f, p, p, p, ll, ll, ll, p, z, f, p, p]),
        "bert_hip_dropout_keep_u8": (i, [p, f, i, i, i, p, p]),
        "bert_hip_attention_train_last_kernel": (s, []),
        "bert_hip_attention_backward_last_kernel": (s, []),
        "dropout_add_layernorm_hip_train_f32": (i, [p, p, p, p, f, ll, i, f, p, p, p, p]),
        "dropout_add_layernorm_hip_backward_workspace_bytes": (z, [ll, i]),
        "dropout_add_layernorm_hip_backward_f32": (i, [p, p, p, f, ll, i, f, p, p, p, p, p, p, z, p]),
        "relu_dropout_hip_f32": (i, [p, ll, i, f, p, p, p]),
        "relu_dropout_hip_backward_f32": (i, [p, p, ll, i, f, p, p]),
        "row_dropout_hip_keep_u8": (i, [p, f, ll, i, p, p]),
    },
    "patch_embed_hip.h": {
        "patch_embed_hip_f32": (i, [p, p, p, i, i, i, i, i, i, i, p, p]),
        "patch_embed_hip_packed_weight_bytes": (z, [i, i, i]),
        "patch_embed_hip_pack_weight_f32": (i, [p, i, i, i, p, p]),
        "patch_embed_hip_packed_f32": (i, [p, p, p, i, i, i, i, i, i, i, p, p]),
        "patch_embed_hip_backward_workspace_bytes": (z, [i, i, i, i, i, i]),
        "patch_embed_hip_backward_f32": (i, [p, p, p, i, i, i, i, i, i, i, p, p, p, p, z, p]),
        "patch_embed_hip_convnext_dwconv_ln_f32": (i, [p, p, p, p, p, f, i, i, i, i, p, p]),
        "patch_embed_hip_convnext_scale_residual_f32": (i, [p, p, p, i, i, i, i, p, p]),
        "patch_embed_hip_layernorm_cf_f32": (i, [p, p, p, f, i, i, i, i, p, p]),
        "patch_embed_hip_convnext_last_kernel": (s, []),
        "patch_embed_hip_convnext_scale_residual_drop_f32": (i, [p, p, p, p, i, i, i, i, p, p]),
        "patch_embed_hip_convnext_dwconv_ln_backward_workspace_bytes": (z, [i, i, i, i]),
        "patch_embed_hip_convnext_dwconv_ln_backward_f32": (i, [p, p, p, p, f, p, i, i, i, i, p, p, p, p, p, p, z, p]),
        "patch_embed_hip_convnext_scale_residual_backward_workspace_bytes": (z, [i, i, i, i]),
        "patch_embed_hip_convnext_scale_residual_backward_f32": (i, [p, p, p, p, i, i, i, i, p, p, p, z, p]),
        "patch_embed_hip_layernorm_cf_backward_workspace_bytes": (z, [i, i, i, i]),
        "patch_embed_hip_layernorm_cf_backward_f32": (i, [p, p, f, p, i, i, i, i, p, p, p, p, z, p]),
        "patch_embed_hip_vit_attn_workspace_bytes": (z, [i, i, i, i, i]),
        "patch_embed_hip_vit_attn_f32": (i, [p, p, p, i, i, i, i, i, f, p, p, z, p]),
        "patch_embed_hip_vit_attn_last_kernel": (s, []),
        "patch_embed_hip_vit_attn_train_f32": (i, [p, p, p, i, i, i, i, i, f, p, p, p, z, p]),
        "patch_embed_hip_vit_attn_backward_workspace_bytes": (z, [i, i, i, i, i]),
        "patch_embed_hip_vit_attn_backward_f32": (i, [p, p, p, p, p, p, i, i, i, i, i, f, p, p, p, p, z, p]),
        "patch_embed_hip_vit_attn_backward_last_kernel": (s, []),
    },
    "linear_hip.h": {
        "linear_hip_packed_weight_bytes": (z, [i, i]),
        "linear_hip_pack_weight_f32": (i, [p, i, i, p, p]),
        "linear_hip_packed_f32": (i, [p, p, p, p, ll, i, i, p, p]),
        "linear_hip_packed_hm_f32": (i, [p, p, p, p, ll, i, i, i, p, p]),
        "linear_hip_packed_ex_f32": (i, [p, p, p, p, p, ll, i, i, i, p, p]),
        "linear_hip_packed_split_f32": (i, [p, p, p, p, ll, i, i, i, p, p, p]),
        "linear_hip_packed_ln_f32": (i, [p, p, p, p, p, p, f, ll, i, i, p, p]),
        "linear_hip_packed_ffn_f32": (i, [p, p, p, p, p, p, p, p, f, i, ll, i, i, p, p]),
    },
    "layernorm_hip.h": {
        "add_layernorm_hip_f32": (i, [p, p, p, p, f, ll, i, p, p]),
    },
    "lsap_hip.h": {
        "lsap_hip_workspace_bytes": (z, [i, i]),
        "lsap_hip_f32": (i, [p, ll, i, i, p, p, p, p, p]),
        "lsap_hip_batch_f32": (i, [i, p, p, p, p, p, p, p, p, p]),
    },
    "matcher_cost_hip.h": {
        "matcher_cost_hip_f32": (i, [p, p, p, p, p, i, i, i, f, f, f, p, p]),
    },
    "ota_hip.h": {
        "ota_cost_hip_f32": (i, [p, p, p, p, p, i, i, i, p, p, p, p]),
        "ota_dynamic_k_hip": (i, [p, p, p, p, p, i, i, i, p, p, p, p, p, p]),
        "ota_reid_select_hip": (i, [p, p, p, p, p, p, i, i, i, i, p, p, p, p, p]),
        "ota_reid_scores_hip_f32": (i, [p, p, p, p, p, i, i, i, i, p, p, p, p, p]),
        "ota_reid_loss_hip_f32": (i, [p, p, p, p, p, p, p, i, i, i, p, p, p, p]),
        "ota_reid_loss_bwd_hip_f32": (i, [p, p, p, p, p, p, p, p, p, p, p, p, p, i, i, i, i, i, p, p, p, p, p]),
    },
    "biattn_hip.h": {
        "biattn_hip_workspace_bytes": (z, [i, i, i, i, i]),
        "biattn_hip_forward_f32": (i, [p, p, p, p, p, i, i, i, i, i, i, f, p, p, p, z, p]),
        "biattn_hip_last_kernel": (s, []),
        "biattn_hip_backward_workspace_bytes": (z, [i, i, i, i, i]),
        "biattn_hip_train_f32": (i, [p, p, p, p, p, i, i, i, i, i, i, f, p, p, p, p, p, z, p]),
        "biattn_hip_backward_f32": (i, [p, p, p, p, p, i, p, p, p, p, p, p, i, i, i, i, i, f, p, p, p, p, p, z, p]),
        "biattn_hip_backward_last_kernel": (s, []),
        "biattn_hip_train_dropout_f32": (i, [p, p, p, p, p, i, i, i, i, i, i, f, p, p, p, p, p, z, f, p, p]),
        "biattn_hip_backward_dropout_f32": (i, [p, p, p, p, p, i, p, p, p, p, p, p, i, i, i, i, i, f, p, p, p, p, p, z, f, p, p]),
        "biattn_hip_dropout_keep_u8": (i, [p, f, i, i, i, i, p, p, p]),
        "biattn_hip_self_forward_f32": (i, [p, p, p, ll, ll, ll, p, i, i, i, i, i, f, p, p]),
        "biattn_hip_self_last_kernel": (s, []),
        "biattn_hip_self_backward_workspace_bytes": (z, [i, i, i, i]),
        "biattn_hip_self_train_f32": (i, [p, p, p, ll, ll, ll, p, i, i, i, i, i, f, p, p, p]),
        "biattn_hip_self_backward_f32": (i, [p, p, p, ll, ll, ll, p, i, p, p, p, i, i, i, i, f, p, p, p, ll, ll, ll, p, z, p]),
        "biattn_hip_self_backward_last_kernel": (s, []),
    },
    "conv3x3_hip.h": {
        "conv3x3_hip_f32": (i, [p, p, p, i, i, i, i, i, i, i, p, p]),
        "conv3x3_hip_packed_weight_bytes": (z, [i, i]),
        "conv3x3_hip_pack_weight_f32": (i, [p, i, i, p, p]),
        "conv3x3_hip_packed_f32": (i, [p, p, p, i, i, i, i, i, i, p, p]),
        "conv3x3_hip_packed_exact_weight_bytes": (z, [i, i]),
        "conv3x3_hip_pack_weight_exact_f32": (i, [p, i, i, p, p]),
        "conv3x3_hip_packed_exact_f32": (i, [p, p, p, i, i, i, i, i, i, p, p]),
        "upsample_add_hip_f32": (i, [p, p, i, i, i, i, i, i, p, p]),
        "conv3x3_hip_packed_exact_dgrad_weight_bytes": (z, [i, i]),
        "conv3x3_hip_pack_weight_exact_dgrad_f32": (i, [p, i, i, p, p]),
        "conv3x3_hip_backward_workspace_bytes": (z, [i, i, i, i, i]),
        "conv3x3_hip_backward_exact_f32": (i, [p, p, p, p, i, i, i, i, i, i, p, p, p, p, z, p]),
    },
}
del i, p, s, f, u, z, ll, dp, _FWD, _BWD   # aliases of the table only

EXPORTS = tuple(_SIGNATURES["msda_hip.h"])
DYNMASK_EXPORTS = tuple(_SIGNATURES["dynmask_hip.h"])
PATCH_EMBED_EXPORTS = tuple(_SIGNATURES["patch_embed_hip.h"])
LINEAR_EXPORTS = tuple(_SIGNATURES["linear_hip.h"])
LAYERNORM_EXPORTS = tuple(_SIGNATURES["layernorm_hip.h"])
LSAP_EXPORTS = tuple(_SIGNATURES["lsap_hip.h"])
MATCHER_COST_EXPORTS = tuple(_SIGNATURES["matcher_cost_hip.h"])
OTA_EXPORTS = tuple(_SIGNATURES["ota_hip.h"])
BIATTN_EXPORTS = tuple(_SIGNATURES["biattn_hip.h"])
CONV3X3_EXPORTS = tuple(_SIGNATURES["conv3x3_hip.h"])

DYNMASK_BWD_MAX_BATCH = 64
BIATTN_MASK_NONE, BIATTN_MASK_INT64, BIATTN_MASK_F32 = 0, 1, 2
BIATTN_MASK_BOOL = 3                    # biattn_hip_self_forward_f32 only
DEC_ATTN_HEAD_DIM, DEC_ATTN_MAX_LEN = 32, 65535
BERT_MASK_NONE, BERT_MASK_KEY_I64, BERT_MASK_KEY_U8, BERT_MASK_FULL_U8 = 0, 1, 2, 3   # bert_hip_self_attention_f32
BERT_HEAD_DIM, BERT_MAX_LEN, BERT_MAX_HIDDEN = 64, 512, 4096
BERT_ERR_WORKSPACE = -6                 # bert_hip_self_attention_backward_f32: a workspace below its workspace_bytes query
BERT_DROPOUT_MAX_BH = 65535             # batch * heads of the training route with dropout (philox.hpp's counter)
LAYERNORM_MAX_FEATURES, RELU_DROPOUT_MAX_FEATURES = 4096, 65536   # include/layernorm_hip.h
LAYERNORM_ERR_NULL_POINTER, LAYERNORM_ERR_BAD_DIMS, LAYERNORM_ERR_UNSUPPORTED, LAYERNORM_ERR_WORKSPACE = -1, -2, -5, -6
BIATTN_HEAD_DIM, BIATTN_MAX_TEXT = 256, 256
VIT_ATTN_HEAD_DIMS = (64, 80)
VIT_ATTN_MAX_SIDE, VIT_ATTN_MAX_TOKENS = 4095, 1 << 20
VIT_ATTN_TRAIN_MAX_W = 256   # q_w of the training route (the backward's width bins live in LDS)
QSEL_D_MODEL = 256
PRED_HEADS_D_MODEL, PRED_HEADS_MAX_TOKENS, PRED_HEADS_MAX_PARAMS = 256, 256, 256
PRED_HEADS_VARIANTS = ("auto", "split", "tile")   # pred_heads_hip_set_variant
DETPOST_MAX_CLASSES, DETPOST_MAX_TOKENS, DETPOST_MAX_QUERIES = 4096, 256, 1024
MASKPOST_MAX_WIDTH, MASKPOST_MAX_MASKS, MASKPOST_STRIDES = 8192, 1024, (1, 2, 4, 8)
TRACK_MAX_CAPACITY, TRACK_MAX_DIM, TRACK_MAX_MEMORY_LEN, TRACK_STATE_FIELDS = 4096, 256, 64, 12
QDTRACK_MAX_BACKDROPS, QDTRACK_MAX_BACKDROP_FRAMES, QDTRACK_STATE_FIELDS = 1024, 4, 11
CRITERION_MAX_TOKENS = 256
CRITERION_MASK_NONE, CRITERION_MASK_INT64, CRITERION_MASK_BOOL = 0, 1, 2
CRITERION_TOKEN_FOCAL, CRITERION_MASK_LOSSES, CRITERION_BOXINST = 0, 1, 2
CRITERION_IMAGE_U8, CRITERION_IMAGE_F32 = 0, 1
BOXINST_MAX_DILATION, BOXINST_BAND, BOXINST_LDS_BYTES = 8, 8, 63 * 1024
OTA_MAX_BATCH = 64
REID_MIN_QUERIES, REID_MAX_QUERIES, REID_MAX_DIM, REID_META, REID_STATS = 100, 8192, 512, 5, 6
LSAP_MAX_BATCH = 32
ENCPREP_MAX_LEVELS, ENCPREP_CHANNELS, ENCPREP_GROUPS, ENCPREP_PIXEL_TILE = 8, 256, 32, 32

_lib = None


def load():
    """Return the loaded library (cached).  Raises RuntimeError when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "MultiScaleDeformableAttention: %s not found. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C uninext_amd/csrc` "
            "(hipcc, gfx950). There is no fallback implementation." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for group in _SIGNATURES.values():
        for name, (restype, argtypes) in group.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    got = lib.msda_hip_abi_version()
    if got != ABI_VERSION:
        raise RuntimeError("libmsda_hip.so ABI version %d, binding expects %d: rebuild" % (got, ABI_VERSION))
    _lib = lib
    return lib


def last_error():
    return load().msda_hip_last_error().decode()


def set_variant(which, variant):
    """which: 'forward' | 'backward'; variant: int or name (see variants())."""
    w = {"forward": 0, "backward": 1}[which]
    if isinstance(variant, str):
        variant = variants(which).index(variant)
    if load().msda_hip_set_variant(w, int(variant)) != 0:
        raise ValueError(last_error())


def set_lanegroup_general(on):
    """Diagnostic (include/msda_hip.h): L = P = 4 lane-group calls take the general instance while `on` is true."""
    load().msda_hip_set_lanegroup_general(1 if on else 0)


def variants(which):
    w = {"forward": 0, "backward": 1}[which]
    out, k = [], 0
    while True:
        n = load().msda_hip_variant_name(w, k)
        if n is None:
            return out
        out.append(n.decode())
        k += 1


def forward_locality():
    """(reports consumed so far, far fraction of the latest) on the call site used last (include/msda_hip.h); waits for the
    launches made so far on that site."""
    frac = ctypes.c_double(0.0)
    n = load().msda_hip_forward_locality(ctypes.byref(frac))
    return n, frac.value


def last_kernel(which):
    if which == "biattn":   # include/biattn_hip.h keeps its own record
        return load().biattn_hip_last_kernel().decode()
    if which == "biattn_bwd":   # and its backward
        return load().biattn_hip_backward_last_kernel().decode()
    if which == "dec_attn":   # the decoder's self-attention core, declared in the same header, likewise
        return load().biattn_hip_self_last_kernel().decode()
    if which == "dec_attn_bwd":   # and its backward
        return load().biattn_hip_self_backward_last_kernel().decode()
    if which == "bert_attn":   # the text encoder's attention core (include/dynmask_hip.h)
        return load().bert_hip_attention_last_kernel().decode()
    if which == "bert_attn_train":   # its training forward
        return load().bert_hip_attention_train_last_kernel().decode()
    if which == "bert_attn_bwd":   # and backward
        return load().bert_hip_attention_backward_last_kernel().decode()
    if which == "bert_embed":   # and its embedding kernel
        return load().bert_hip_embed_last_kernel().decode()
    if which == "qsel":   # the query-selection kernels of include/dynmask_hip.h likewise
        return load().qsel_hip_last_kernel().decode()
    if which == "pred_heads":   # and the decoder prediction heads' kernel
        return load().pred_heads_hip_last_kernel().decode()
    if which == "detpost":   # and the detection post-processing kernels
        return load().detpost_hip_last_kernel().decode()
    if which == "maskpost":   # and the mask post-processing kernels
        return load().maskpost_hip_last_kernel().decode()
    if which == "track":   # and the tracker's
        return load().track_hip_last_kernel().decode()
    if which == "qdtrack":   # and the QuasiDense tracker's
        return load().qdtrack_hip_last_kernel().decode()
    if which == "encprep":   # and the encoder input preparation's
        return load().encprep_hip_last_kernel().decode()
    if which == "criterion":   # and the training criterion's
        return load().criterion_hip_last_kernel().decode()
    if which == "convnext":   # the ConvNeXt kernels of include/patch_embed_hip.h likewise
        return load().patch_embed_hip_convnext_last_kernel().decode()
    if which == "vit_attn":   # and the ViT attention core
        return load().patch_embed_hip_vit_attn_last_kernel().decode()
    if which == "vit_attn_bwd":   # and its backward
        return load().patch_embed_hip_vit_attn_backward_last_kernel().decode()
    return load().msda_hip_last_kernel({"forward": 0, "backward": 1}[which]).decode()
