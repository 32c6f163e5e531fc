"""Writes tests/golden/rejections.json: for every launcher of the library that reports through the shared last-error slot, calls
that are refused (or answered as an empty problem) BEFORE any HIP runtime call, with the code and the message the library
answers.  tests/test_rejections_cpu.py replays the file against the library under test.

Run it against the library whose answers are to be recorded, i.e. a build of the commit BEFORE a change of the launchers'
host code:

    MSDA_HIP_LIB=/path/to/that/libmsda_hip.so python tests/golden/make_rejections_golden.py

No GPU is needed or touched: a case that gets past the argument checks would come back with a (positive) HIP error code,
and the script refuses to record it.

An argument in the file is [kind, value]: "i" int, "ll" long long, "z" size_t, "f" float, "p" pointer.  A pointer's value
is "null", "ok" (a 16-byte aligned address that is never dereferenced), "mis4" / "mis2" (that address + 4 / + 2), or a
host array that the launcher reads: {"i32": [...]}, {"i64": [...]} or {"ptrs": ["ok" | "null", ...]}."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

OK, NULL, MIS4, MIS2 = "ok", "null", "mis4", "mis2"

# entry point -> [(argument, kind, a value with which the call would be accepted)]
SPECS = {
    "conv3x3_hip_f32": [("in", "p", OK), ("weight", "p", OK), ("bias", "p", OK), ("batch", "i", 1), ("cin", "i", 16), ("height", "i", 4),
                        ("width", "i", 4), ("cout", "i", 8), ("relu", "i", 0), ("precision", "i", 0), ("out", "p", OK), ("stream", "p", NULL)],
    "conv3x3_hip_pack_weight_f32": [("weight", "p", OK), ("cout", "i", 8), ("cin", "i", 16), ("packed", "p", OK), ("stream", "p", NULL)],
    "conv3x3_hip_packed_f32": [("in", "p", OK), ("packed", "p", OK), ("bias", "p", OK), ("batch", "i", 1), ("cin", "i", 16), ("height", "i", 4),
                               ("width", "i", 4), ("cout", "i", 8), ("relu", "i", 0), ("out", "p", OK), ("stream", "p", NULL)],
    "conv3x3_hip_pack_weight_exact_f32": [("weight", "p", OK), ("cout", "i", 8), ("cin", "i", 16), ("packed", "p", OK), ("stream", "p", NULL)],
    "conv3x3_hip_packed_exact_f32": [("in", "p", OK), ("packed", "p", OK), ("bias", "p", OK), ("batch", "i", 1), ("cin", "i", 16),
                                     ("height", "i", 4), ("width", "i", 4), ("cout", "i", 8), ("relu", "i", 0), ("out", "p", OK),
                                     ("stream", "p", NULL)],
    "upsample_add_hip_f32": [("skip", "p", OK), ("low", "p", OK), ("batch", "i", 1), ("channels", "i", 2), ("height", "i", 4), ("width", "i", 4),
                             ("low_h", "i", 2), ("low_w", "i", 2), ("out", "p", OK), ("stream", "p", NULL)],
    "conv3x3_hip_pack_weight_exact_dgrad_f32": [("weight", "p", OK), ("cout", "i", 8), ("cin", "i", 16), ("packed", "p", OK),
                                                ("stream", "p", NULL)],
    "conv3x3_hip_backward_exact_f32": [("in", "p", OK), ("packed_dgrad", "p", OK), ("out", "p", OK), ("grad_out", "p", OK), ("batch", "i", 1),
                                       ("cin", "i", 16), ("height", "i", 4), ("width", "i", 4), ("cout", "i", 16), ("relu", "i", 1),
                                       ("grad_in", "p", OK), ("grad_weight", "p", OK), ("grad_bias", "p", OK), ("workspace", "p", OK),
                                       ("workspace_bytes", "z", 1 << 40), ("stream", "p", NULL)],
    "patch_embed_hip_f32": [("x", "p", OK), ("weight", "p", OK), ("bias", "p", OK), ("batch", "i", 1), ("in_chans", "i", 4), ("height", "i", 4),
                            ("width", "i", 4), ("embed_dim", "i", 8), ("patch", "i", 2), ("channels_last", "i", 0), ("out", "p", OK),
                            ("stream", "p", NULL)],
    "patch_embed_hip_pack_weight_f32": [("weight", "p", OK), ("embed_dim", "i", 8), ("in_chans", "i", 3), ("patch", "i", 4), ("packed", "p", OK),
                                        ("stream", "p", NULL)],
    "patch_embed_hip_packed_f32": [("x", "p", OK), ("packed", "p", OK), ("bias", "p", OK), ("batch", "i", 1), ("in_chans", "i", 3),
                                   ("height", "i", 8), ("width", "i", 8), ("embed_dim", "i", 8), ("patch", "i", 4), ("channels_last", "i", 0),
                                   ("out", "p", OK), ("stream", "p", NULL)],
    "patch_embed_hip_backward_f32": [("x", "p", OK), ("weight", "p", OK), ("grad_out", "p", OK), ("batch", "i", 1), ("in_chans", "i", 4),
                                     ("height", "i", 4), ("width", "i", 4), ("embed_dim", "i", 8), ("patch", "i", 2), ("channels_last", "i", 0),
                                     ("grad_x", "p", OK), ("grad_weight", "p", OK), ("grad_bias", "p", OK), ("workspace", "p", OK),
                                     ("workspace_bytes", "z", 1 << 40), ("stream", "p", NULL)],
    "patch_embed_hip_convnext_dwconv_ln_f32": [("x", "p", OK), ("dw_weight", "p", OK), ("dw_bias", "p", OK), ("ln_weight", "p", OK),
                                               ("ln_bias", "p", OK), ("eps", "f", 1e-6), ("B", "i", 1), ("C", "i", 32), ("H", "i", 8), ("W", "i", 8),
                                               ("out", "p", OK), ("stream", "p", NULL)],
    "patch_embed_hip_convnext_scale_residual_f32": [("y", "p", OK), ("gamma", "p", OK), ("input", "p", OK), ("B", "i", 1), ("C", "i", 32),
                                                    ("H", "i", 8), ("W", "i", 8), ("out", "p", OK), ("stream", "p", NULL)],
    "patch_embed_hip_layernorm_cf_f32": [("x", "p", OK), ("weight", "p", OK), ("bias", "p", OK), ("eps", "f", 1e-6), ("B", "i", 1), ("C", "i", 32),
                                         ("H", "i", 8), ("W", "i", 8), ("out", "p", OK), ("stream", "p", NULL)],
    "patch_embed_hip_vit_attn_f32": [("qkv", "p", OK), ("rel_h_table", "p", OK), ("rel_w_table", "p", OK), ("batch", "i", 1), ("num_heads", "i", 1),
                                     ("q_h", "i", 4), ("q_w", "i", 4), ("head_dim", "i", 64), ("scale", "f", 0.125), ("out", "p", OK),
                                     ("workspace", "p", OK), ("workspace_bytes", "z", 1 << 40), ("stream", "p", NULL)],
    "biattn_hip_forward_f32": [("q", "p", OK), ("k", "p", OK), ("vv", "p", OK), ("vl", "p", OK), ("mask", "p", NULL), ("mask_kind", "i", 0),
                               ("batch", "i", 1), ("num_heads", "i", 1), ("image_len", "i", 64), ("text_len", "i", 32), ("head_dim", "i", 256),
                               ("q_scale", "f", 0.0625), ("out_v", "p", OK), ("out_l", "p", OK), ("workspace", "p", OK),
                               ("workspace_bytes", "z", 1 << 40), ("stream", "p", NULL)],
    "biattn_hip_self_forward_f32": [("q", "p", OK), ("k", "p", OK), ("v", "p", OK), ("q_stride", "ll", 32), ("k_stride", "ll", 32),
                                    ("v_stride", "ll", 32), ("mask", "p", NULL), ("mask_kind", "i", 0), ("batch", "i", 1), ("num_heads", "i", 1),
                                    ("len", "i", 64), ("head_dim", "i", 32), ("q_scale", "f", 0.25), ("out", "p", OK), ("stream", "p", NULL)],
    "detpost_scores_hip_f32": [("logits", "p", OK), ("iou_logits", "p", NULL), ("cls_ptr", "p", OK), ("tok_idx", "p", OK), ("nnz", "i", 1),
                               ("score_thres", "f", 0.5), ("batch", "i", 1), ("Q", "i", 4), ("C", "i", 2), ("T", "i", 4), ("prob", "p", OK),
                               ("row_max", "p", OK), ("row_arg", "p", OK), ("row_valid", "p", OK), ("stream", "p", NULL)],
    "detpost_nms_hip_f32": [("boxes", "p", OK), ("row_max", "p", OK), ("row_arg", "p", OK), ("iou_threshold", "f", 0.5), ("per_class", "i", 0),
                            ("batch", "i", 1), ("Q", "i", 4), ("keep", "p", OK), ("n_keep", "p", OK), ("kept_mask", "p", OK), ("stream", "p", NULL)],
    "qsel_scores_hip_f32": [("memory", "p", OK), ("padding_mask", "p", OK), ("spatial_shapes", "p", OK), ("n_levels", "i", 1), ("valid_wh", "p", OK),
                            ("enc_weight", "p", OK), ("enc_bias", "p", OK), ("ln_weight", "p", OK), ("ln_bias", "p", OK), ("eps", "f", 1e-5),
                            ("class_vec", "p", OK), ("class_vec_stride", "ll", 0), ("class_bias", "p", OK), ("class_bias_stride", "ll", 0),
                            ("scale", "p", OK), ("clamp", "f", 50000.0), ("batch", "i", 1), ("S", "ll", 8), ("d_model", "i", 256),
                            ("logits", "p", OK), ("output_memory", "p", OK), ("stream", "p", NULL)],
    "qsel_boxes_hip_f32": [("memory", "p", OK), ("padding_mask", "p", OK), ("spatial_shapes", "p", OK), ("n_levels", "i", 1), ("valid_wh", "p", OK),
                           ("enc_weight", "p", OK), ("enc_bias", "p", OK), ("ln_weight", "p", OK), ("ln_bias", "p", OK), ("eps", "f", 1e-5),
                           ("idx", "p", OK), ("K", "ll", 4), ("w1", "p", OK), ("b1", "p", OK), ("w2", "p", OK), ("b2", "p", OK), ("w3", "p", OK),
                           ("b3", "p", OK), ("batch", "i", 1), ("S", "ll", 8), ("d_model", "i", 256), ("coords_unact", "p", OK),
                           ("reference_points", "p", OK), ("stream", "p", NULL)],
    "dynmask_hip_set_variant": [("variant", "i", 0)],
    "dynmask_hip_forward_f32": [("mask_feats", "p", OK), ("inst_xy", "p", OK), ("params", "p", OK), ("num_insts", "p", {"i32": [1]}),
                                ("batch", "i", 1), ("channels", "i", 8), ("H", "i", 4), ("W", "i", 4), ("stride", "i", 8), ("rel_coord", "i", 1),
                                ("out_logits", "p", OK), ("stream", "p", NULL)],
    "aligned_bilinear_hip_f32": [("in", "p", OK), ("n", "i", 1), ("h", "i", 4), ("w", "i", 4), ("factor", "i", 2), ("out", "p", OK),
                                 ("stream", "p", NULL)],
    "dynmask_hip_backward_f32": [("mask_feats", "p", OK), ("inst_xy", "p", OK), ("params", "p", OK), ("num_insts", "p", {"i32": [1]}),
                                 ("batch", "i", 1), ("channels", "i", 8), ("H", "i", 4), ("W", "i", 4), ("stride", "i", 8), ("rel_coord", "i", 1),
                                 ("grad_logits", "p", OK), ("grad_feats", "p", OK), ("grad_params", "p", OK), ("grad_xy", "p", OK),
                                 ("workspace", "p", OK), ("workspace_bytes", "z", 1 << 40), ("stream", "p", NULL)],
    "aligned_bilinear_hip_backward_f32": [("grad_out", "p", OK), ("n", "i", 1), ("h", "i", 4), ("w", "i", 4), ("factor", "i", 2),
                                          ("grad_in", "p", OK), ("stream", "p", NULL)],
    "add_layernorm_hip_f32": [("x", "p", OK), ("residual", "p", OK), ("gamma", "p", OK), ("beta", "p", OK), ("eps", "f", 1e-5), ("rows", "ll", 4),
                              ("features", "i", 256), ("out", "p", OK), ("stream", "p", NULL)],
    "linear_hip_pack_weight_f32": [("weight", "p", OK), ("out_features", "i", 64), ("in_features", "i", 64), ("packed", "p", OK),
                                   ("stream", "p", NULL)],
    "linear_hip_packed_f32": [("x", "p", OK), ("packed", "p", OK), ("bias", "p", OK), ("row_mask", "p", NULL), ("rows", "ll", 64),
                              ("in_features", "i", 64), ("out_features", "i", 64), ("out", "p", OK), ("stream", "p", NULL)],
    "linear_hip_packed_hm_f32": [("x", "p", OK), ("packed", "p", OK), ("bias", "p", OK), ("row_mask", "p", NULL), ("rows", "ll", 64),
                                 ("in_features", "i", 64), ("out_features", "i", 64), ("rows_per_image", "i", 64), ("out", "p", OK),
                                 ("stream", "p", NULL)],
    "linear_hip_packed_ln_f32": [("x", "p", OK), ("packed", "p", OK), ("bias", "p", OK), ("residual", "p", OK), ("gamma", "p", OK),
                                 ("beta", "p", OK), ("eps", "f", 1e-5), ("rows", "ll", 64), ("in_features", "i", 64), ("out_features", "i", 256),
                                 ("out", "p", OK), ("stream", "p", NULL)],
    "linear_hip_packed_ex_f32": [("x", "p", OK), ("x_add", "p", NULL), ("packed", "p", OK), ("bias", "p", OK), ("row_mask", "p", NULL),
                                 ("rows", "ll", 64), ("in_features", "i", 64), ("out_features", "i", 64), ("activation", "i", 0), ("out", "p", OK),
                                 ("stream", "p", NULL)],
    "linear_hip_packed_split_f32": [("x", "p", OK), ("x_add", "p", NULL), ("packed", "p", OK), ("bias", "p", OK), ("rows", "ll", 64),
                                    ("in_features", "i", 64), ("out_features", "i", 256), ("split_col", "i", 128), ("out_a", "p", OK),
                                    ("out_b", "p", OK), ("stream", "p", NULL)],
    "linear_hip_packed_ffn_f32": [("x", "p", OK), ("packed1", "p", OK), ("bias1", "p", OK), ("packed2", "p", OK), ("bias2", "p", OK),
                                  ("residual", "p", OK), ("gamma", "p", OK), ("beta", "p", OK), ("eps", "f", 1e-5), ("layer_norm", "i", 1),
                                  ("rows", "ll", 64), ("d_model", "i", 256), ("d_ffn", "i", 1024), ("out", "p", OK), ("stream", "p", NULL)],
    "lsap_hip_batch_f32": [("count", "i", 1), ("cost", "p", {"ptrs": [OK]}), ("ld", "p", {"i64": [4]}), ("rows", "p", {"i32": [3]}),
                           ("cols", "p", {"i32": [4]}), ("row_ind", "p", {"ptrs": [OK]}), ("col_ind", "p", {"ptrs": [OK]}),
                           ("workspace", "p", {"ptrs": [OK]}), ("status", "p", {"ptrs": [OK]}), ("stream", "p", NULL)],
    "lsap_hip_f32": [("cost", "p", OK), ("ld", "ll", 4), ("rows", "i", 3), ("cols", "i", 4), ("row_ind", "p", OK), ("col_ind", "p", OK),
                     ("workspace", "p", OK), ("status", "p", OK), ("stream", "p", NULL)],
    "matcher_cost_hip_f32": [("logits", "p", OK), ("boxes", "p", OK), ("tgt_boxes", "p", OK), ("tok_off", "p", OK), ("tok_idx", "p", OK),
                             ("num_pred", "i", 4), ("num_tokens", "i", 4), ("num_gt", "i", 2), ("w_class", "f", 2.0), ("w_bbox", "f", 5.0),
                             ("w_giou", "f", 2.0), ("cost", "p", OK), ("stream", "p", NULL)],
    "msda_hip_prologue_f32": [("spatial_shapes", "p", OK), ("reference_points", "p", OK), ("ref_dim", "i", 2), ("sampling_offsets", "p", OK),
                              ("attn_logits", "p", OK), ("batch", "i", 1), ("num_heads", "i", 8), ("num_levels", "i", 4), ("num_query", "i", 4),
                              ("num_point", "i", 4), ("sampling_loc", "p", OK), ("attn_weight", "p", OK), ("stream", "p", NULL)],
    "msda_hip_prologue_backward_f32": [("spatial_shapes", "p", OK), ("reference_points", "p", OK), ("ref_dim", "i", 2),
                                       ("sampling_offsets", "p", OK), ("attn_weight", "p", OK), ("grad_sampling_loc", "p", OK),
                                       ("grad_attn_weight", "p", OK), ("batch", "i", 1), ("num_heads", "i", 8), ("num_levels", "i", 4),
                                       ("num_query", "i", 4), ("num_point", "i", 4), ("grad_sampling_offsets", "p", OK),
                                       ("grad_attn_logits", "p", OK), ("grad_reference_points", "p", OK), ("stream", "p", NULL)],
    "ota_cost_hip_f32": [("class_table", "p", OK), ("boxes", "p", OK), ("tgt_boxes", "p", OK), ("positive_map", "p", OK),
                         ("gt_off", "p", {"i32": [0, 2]}), ("batch", "i", 1), ("num_queries", "i", 4), ("num_tokens", "i", 4), ("cost", "p", OK),
                         ("iou", "p", OK), ("flags", "p", OK), ("stream", "p", NULL)],
    "ota_dynamic_k_hip": [("cost", "p", OK), ("iou", "p", OK), ("flags", "p", OK), ("matching", "p", OK), ("gt_off", "p", {"i32": [0, 2]}),
                          ("batch", "i", 1), ("num_queries", "i", 4), ("max_rounds", "i", 4), ("sel_query", "p", OK), ("sel_gt", "p", OK),
                          ("matched_query", "p", OK), ("num_selected", "p", OK), ("status", "p", OK), ("stream", "p", NULL)],
}

BIG_IMAGE = dict(batch=1 << 15, height=256, width=256)      # 2^31 output pixels
CONVNEXT_BIG = dict(B=1 << 12, C=1024, H=1 << 10, W=1 << 10)

# (entry point, what the case is about, {argument: value}); every pointer argument of an aligned16 check gets a case of its own
# below.  "empty" cases are answered 0 without a launch.
CASES = [
    ("conv3x3_hip_f32", "precision", dict(precision=2)),
    ("conv3x3_hip_f32", "bad_dims", dict(batch=-1)),
    ("conv3x3_hip_f32", "k_multiple", dict(cin=3)),
    ("conv3x3_hip_f32", "empty", dict(batch=0)),
    ("conv3x3_hip_f32", "too_large_pixels", BIG_IMAGE),
    ("conv3x3_hip_f32", "too_large_cout", dict(cout=65535 * 64 + 1)),
    ("conv3x3_hip_f32", "null", {"in": NULL}),
    ("conv3x3_hip_pack_weight_f32", "bad_dims", dict(cout=0)),
    ("conv3x3_hip_pack_weight_f32", "cin_multiple", dict(cin=8)),
    ("conv3x3_hip_pack_weight_f32", "null", dict(weight=NULL)),
    ("conv3x3_hip_packed_f32", "bad_dims", dict(width=0)),
    ("conv3x3_hip_packed_f32", "cin_multiple", dict(cin=8)),
    ("conv3x3_hip_packed_f32", "empty", dict(batch=0)),
    ("conv3x3_hip_packed_f32", "too_large", BIG_IMAGE),
    ("conv3x3_hip_packed_f32", "null", dict(packed=NULL)),
    ("conv3x3_hip_pack_weight_exact_f32", "bad_dims", dict(cin=0)),
    ("conv3x3_hip_pack_weight_exact_f32", "cin_multiple", dict(cin=24)),
    ("conv3x3_hip_pack_weight_exact_f32", "null", dict(packed=NULL)),
    ("conv3x3_hip_packed_exact_f32", "bad_dims", dict(cout=0)),
    ("conv3x3_hip_packed_exact_f32", "cin_multiple", dict(cin=8)),
    ("conv3x3_hip_packed_exact_f32", "empty", dict(batch=0)),
    ("conv3x3_hip_packed_exact_f32", "too_large", BIG_IMAGE),
    ("conv3x3_hip_packed_exact_f32", "null", dict(out=NULL)),
    ("upsample_add_hip_f32", "bad_dims", dict(low_h=0)),
    ("upsample_add_hip_f32", "empty", dict(batch=0)),
    ("upsample_add_hip_f32", "too_large", dict(batch=1 << 16, channels=1 << 8, height=1 << 7)),
    ("upsample_add_hip_f32", "null", dict(low=NULL)),
    ("conv3x3_hip_pack_weight_exact_dgrad_f32", "bad_dims", dict(cout=0)),
    ("conv3x3_hip_pack_weight_exact_dgrad_f32", "null", dict(weight=NULL)),
    ("conv3x3_hip_backward_exact_f32", "bad_dims", dict(height=0)),
    ("conv3x3_hip_backward_exact_f32", "empty_batch_no_param_grads", dict(batch=0, grad_weight=NULL, grad_bias=NULL)),
    ("conv3x3_hip_backward_exact_f32", "too_large", BIG_IMAGE),
    ("conv3x3_hip_backward_exact_f32", "empty_no_grads", dict(grad_in=NULL, grad_weight=NULL, grad_bias=NULL)),
    ("conv3x3_hip_backward_exact_f32", "null", dict(grad_out=NULL)),
    ("conv3x3_hip_backward_exact_f32", "null_out_with_relu", dict(out=NULL)),
    ("conv3x3_hip_backward_exact_f32", "workspace_small", dict(workspace_bytes=0)),
    ("patch_embed_hip_f32", "bad_dims", dict(patch=0)),
    ("patch_embed_hip_f32", "patch_size", dict(patch=3)),
    ("patch_embed_hip_f32", "k_multiple", dict(in_chans=3)),
    ("patch_embed_hip_f32", "empty", dict(height=1, width=1)),
    ("patch_embed_hip_f32", "too_large", dict(batch=1 << 15, height=512, width=512)),
    ("patch_embed_hip_f32", "null", dict(x=NULL)),
    ("patch_embed_hip_pack_weight_f32", "unsupported", dict(in_chans=4, patch=2)),
    ("patch_embed_hip_pack_weight_f32", "null", dict(weight=NULL)),
    ("patch_embed_hip_packed_f32", "bad_dims", dict(embed_dim=0)),
    ("patch_embed_hip_packed_f32", "unsupported", dict(in_chans=4, patch=2)),
    ("patch_embed_hip_packed_f32", "empty", dict(height=2, width=2)),
    ("patch_embed_hip_packed_f32", "too_large", dict(batch=1 << 15, height=1024, width=1024)),
    ("patch_embed_hip_packed_f32", "null", dict(packed=NULL)),
    ("patch_embed_hip_backward_f32", "bad_dims", dict(in_chans=0)),
    ("patch_embed_hip_backward_f32", "patch_size", dict(patch=5)),
    ("patch_embed_hip_backward_f32", "k_multiple", dict(in_chans=3)),
    ("patch_embed_hip_backward_f32", "too_large", dict(batch=1 << 15, height=512, width=512)),
    ("patch_embed_hip_backward_f32", "empty_no_grads", dict(grad_x=NULL, grad_weight=NULL, grad_bias=NULL)),
    ("patch_embed_hip_backward_f32", "null", dict(grad_out=NULL)),
    ("patch_embed_hip_backward_f32", "null_workspace", dict(workspace=NULL)),
    ("patch_embed_hip_backward_f32", "workspace_small", dict(workspace_bytes=0)),
    ("patch_embed_hip_convnext_dwconv_ln_f32", "bad_dims", dict(C=0)),
    ("patch_embed_hip_convnext_dwconv_ln_f32", "channels", dict(C=48)),
    ("patch_embed_hip_convnext_dwconv_ln_f32", "too_large", CONVNEXT_BIG),
    ("patch_embed_hip_convnext_dwconv_ln_f32", "null", dict(x=NULL)),
    ("patch_embed_hip_convnext_dwconv_ln_f32", "empty", dict(B=0)),
    ("patch_embed_hip_convnext_scale_residual_f32", "bad_dims", dict(H=0)),
    ("patch_embed_hip_convnext_scale_residual_f32", "too_large", CONVNEXT_BIG),
    ("patch_embed_hip_convnext_scale_residual_f32", "null", dict(input=NULL)),
    ("patch_embed_hip_convnext_scale_residual_f32", "empty", dict(B=0)),
    ("patch_embed_hip_layernorm_cf_f32", "bad_dims", dict(W=-1)),
    ("patch_embed_hip_layernorm_cf_f32", "too_large", CONVNEXT_BIG),
    ("patch_embed_hip_layernorm_cf_f32", "null", dict(bias=NULL)),
    ("patch_embed_hip_layernorm_cf_f32", "empty", dict(B=0)),
    ("patch_embed_hip_vit_attn_f32", "bad_dims", dict(num_heads=0)),
    ("patch_embed_hip_vit_attn_f32", "head_dim", dict(head_dim=32)),
    ("patch_embed_hip_vit_attn_f32", "too_large_side", dict(q_h=4096)),
    ("patch_embed_hip_vit_attn_f32", "too_large_total", dict(batch=1 << 15, num_heads=1 << 10, q_h=1024, q_w=1024)),
    ("patch_embed_hip_vit_attn_f32", "empty", dict(batch=0)),
    ("patch_embed_hip_vit_attn_f32", "null", dict(qkv=NULL)),
    ("patch_embed_hip_vit_attn_f32", "two_tables_h_only", dict(rel_w_table=NULL)),
    ("patch_embed_hip_vit_attn_f32", "two_tables_w_only", dict(rel_h_table=NULL)),
    ("patch_embed_hip_vit_attn_f32", "workspace_small", dict(workspace_bytes=0)),
    ("biattn_hip_forward_f32", "bad_dims", dict(image_len=0)),
    ("biattn_hip_forward_f32", "head_dim", dict(head_dim=128)),
    ("biattn_hip_forward_f32", "text_len", dict(text_len=257)),
    ("biattn_hip_forward_f32", "too_large", dict(batch=65536)),
    ("biattn_hip_forward_f32", "mask_kind", dict(mask_kind=7)),
    ("biattn_hip_forward_f32", "null", dict(q=NULL)),
    ("biattn_hip_forward_f32", "null_mask", dict(mask_kind=2)),
    ("biattn_hip_forward_f32", "workspace_small", dict(workspace_bytes=0)),
    ("biattn_hip_forward_f32", "empty", dict(batch=0)),
    ("biattn_hip_self_forward_f32", "bad_dims", dict(num_heads=0)),
    ("biattn_hip_self_forward_f32", "len", dict(len=65536)),
    ("biattn_hip_self_forward_f32", "head_dim", dict(head_dim=64)),
    ("biattn_hip_self_forward_f32", "mask_kind", dict(mask_kind=1)),
    ("biattn_hip_self_forward_f32", "stride_small", dict(k_stride=16)),
    ("biattn_hip_self_forward_f32", "stride_multiple", dict(v_stride=34)),
    ("biattn_hip_self_forward_f32", "too_large_stride", dict(q_stride=1 << 31)),
    ("biattn_hip_self_forward_f32", "too_large_grid", dict(batch=1 << 20, len=65535)),
    ("biattn_hip_self_forward_f32", "empty", dict(batch=0)),
    ("biattn_hip_self_forward_f32", "null", dict(out=NULL)),
    ("biattn_hip_self_forward_f32", "null_mask", dict(mask_kind=3)),
    ("biattn_hip_self_forward_f32", "mask_f32_alignment", dict(mask_kind=2, mask=MIS2)),
    ("detpost_scores_hip_f32", "bad_dims", dict(C=0)),
    ("detpost_scores_hip_f32", "limits", dict(C=4097)),
    ("detpost_scores_hip_f32", "too_large", dict(batch=1 << 12, Q=1 << 10, C=1 << 10)),
    ("detpost_scores_hip_f32", "empty", dict(Q=0)),
    ("detpost_scores_hip_f32", "null", dict(logits=NULL)),
    ("detpost_nms_hip_f32", "bad_dims", dict(per_class=2)),
    ("detpost_nms_hip_f32", "limits", dict(Q=1025)),
    ("detpost_nms_hip_f32", "empty", dict(batch=0)),
    ("detpost_nms_hip_f32", "null", dict(n_keep=NULL)),
    ("qsel_scores_hip_f32", "bad_dims", dict(n_levels=0)),
    ("qsel_scores_hip_f32", "d_model", dict(d_model=128)),
    ("qsel_scores_hip_f32", "too_large", dict(S=1 << 31)),
    ("qsel_scores_hip_f32", "class_strides", dict(class_vec_stride=2)),
    ("qsel_scores_hip_f32", "empty", dict(S=0)),
    ("qsel_scores_hip_f32", "null", dict(logits=NULL)),
    ("qsel_boxes_hip_f32", "bad_dims", dict(batch=-1)),
    ("qsel_boxes_hip_f32", "d_model", dict(d_model=512)),
    ("qsel_boxes_hip_f32", "bad_k", dict(K=-1)),
    ("qsel_boxes_hip_f32", "empty", dict(K=0)),
    ("qsel_boxes_hip_f32", "null", dict(idx=NULL)),
    ("dynmask_hip_set_variant", "unknown", dict(variant=99)),
    ("dynmask_hip_forward_f32", "bad_dims", dict(H=0)),
    ("dynmask_hip_forward_f32", "channels", dict(channels=4)),
    ("dynmask_hip_forward_f32", "empty", dict(batch=0)),
    ("dynmask_hip_forward_f32", "empty_no_instances", dict(num_insts={"i32": [0]})),
    ("dynmask_hip_forward_f32", "null_counts", dict(num_insts=NULL)),
    ("dynmask_hip_forward_f32", "negative_count", dict(num_insts={"i32": [-1]})),
    ("dynmask_hip_forward_f32", "null", dict(params=NULL)),
    ("aligned_bilinear_hip_f32", "bad_dims", dict(factor=0)),
    ("aligned_bilinear_hip_f32", "empty", dict(n=0)),
    ("aligned_bilinear_hip_f32", "null", dict(out=NULL)),
    ("aligned_bilinear_hip_f32", "too_large", dict(n=1 << 20, factor=1 << 10, h=1 << 10)),
    ("dynmask_hip_backward_f32", "bad_dims", dict(stride=0)),
    ("dynmask_hip_backward_f32", "channels", dict(channels=16)),
    ("dynmask_hip_backward_f32", "max_batch", dict(batch=65, num_insts={"i32": [0] * 65})),
    ("dynmask_hip_backward_f32", "empty", dict(batch=0)),
    ("dynmask_hip_backward_f32", "null_counts", dict(num_insts=NULL)),
    ("dynmask_hip_backward_f32", "grad_xy_alone", dict(grad_params=NULL)),
    ("dynmask_hip_backward_f32", "negative_count", dict(num_insts={"i32": [-3]})),
    ("dynmask_hip_backward_f32", "null", dict(grad_logits=NULL)),
    ("dynmask_hip_backward_f32", "null_workspace", dict(workspace=NULL)),
    ("dynmask_hip_backward_f32", "workspace_small", dict(workspace_bytes=0)),
    ("aligned_bilinear_hip_backward_f32", "bad_dims", dict(w=0)),
    ("aligned_bilinear_hip_backward_f32", "empty", dict(n=0)),
    ("aligned_bilinear_hip_backward_f32", "null", dict(grad_in=NULL)),
    ("aligned_bilinear_hip_backward_f32", "too_large", dict(n=1 << 15, h=1 << 12, w=1 << 12)),
    ("add_layernorm_hip_f32", "bad_dims", dict(features=0)),
    ("add_layernorm_hip_f32", "features", dict(features=6)),
    ("add_layernorm_hip_f32", "features_max", dict(features=4100)),
    ("add_layernorm_hip_f32", "empty", dict(rows=0)),
    ("add_layernorm_hip_f32", "too_large", dict(rows=1 << 33)),
    ("add_layernorm_hip_f32", "null", dict(x=NULL)),
    ("linear_hip_pack_weight_f32", "bad_dims", dict(out_features=0)),
    ("linear_hip_pack_weight_f32", "in_features", dict(in_features=32)),
    ("linear_hip_pack_weight_f32", "null", dict(packed=NULL)),
    ("linear_hip_packed_f32", "bad_dims", dict(rows=-1)),
    ("linear_hip_packed_f32", "in_features", dict(in_features=96)),
    ("linear_hip_packed_f32", "empty", dict(rows=0)),
    ("linear_hip_packed_f32", "too_large", dict(out_features=1 << 24)),
    ("linear_hip_packed_f32", "null", dict(x=NULL)),
    ("linear_hip_packed_hm_f32", "layout", dict(rows_per_image=0)),
    ("linear_hip_packed_hm_f32", "layout_rows", dict(rows=65)),
    ("linear_hip_packed_hm_f32", "rows_per_image", dict(rows_per_image=32)),
    ("linear_hip_packed_hm_f32", "null", dict(out=NULL)),
    ("linear_hip_packed_ln_f32", "bad_dims", dict(in_features=0)),
    ("linear_hip_packed_ln_f32", "out_features", dict(out_features=128)),
    ("linear_hip_packed_ln_f32", "empty", dict(rows=0)),
    ("linear_hip_packed_ln_f32", "too_large", dict(rows=1 << 38)),
    ("linear_hip_packed_ln_f32", "null", dict(packed=NULL)),
    ("linear_hip_packed_ex_f32", "activation", dict(activation=2)),
    ("linear_hip_packed_ex_f32", "null", dict(x=NULL)),
    ("linear_hip_packed_split_f32", "split_col_sign", dict(split_col=0)),
    ("linear_hip_packed_split_f32", "split_col_multiple", dict(split_col=64)),
    ("linear_hip_packed_split_f32", "split_col_inside", dict(split_col=256)),
    ("linear_hip_packed_split_f32", "null_second_output", dict(out_b=NULL)),
    ("linear_hip_packed_ffn_f32", "bad_dims", dict(d_ffn=0)),
    ("linear_hip_packed_ffn_f32", "d_model", dict(d_model=128)),
    ("linear_hip_packed_ffn_f32", "d_ffn", dict(d_ffn=192)),
    ("linear_hip_packed_ffn_f32", "empty", dict(rows=0)),
    ("linear_hip_packed_ffn_f32", "too_large", dict(rows=1 << 40)),
    ("linear_hip_packed_ffn_f32", "null", dict(packed2=NULL)),
    ("lsap_hip_batch_f32", "count", dict(count=33)),
    ("lsap_hip_batch_f32", "empty", dict(count=0)),
    ("lsap_hip_batch_f32", "null", dict(cost=NULL)),
    ("lsap_hip_batch_f32", "bad_dims", dict(rows={"i32": [-1]})),
    ("lsap_hip_batch_f32", "bad_ld", dict(ld={"i64": [3]})),
    ("lsap_hip_batch_f32", "null_status", dict(status={"ptrs": [NULL]})),
    ("lsap_hip_batch_f32", "null_problem", dict(cost={"ptrs": [NULL]})),
    ("lsap_hip_f32", "bad_dims", dict(cols=-1)),
    ("lsap_hip_f32", "null_status", dict(status=NULL)),
    ("lsap_hip_f32", "null", dict(workspace=NULL)),
    ("matcher_cost_hip_f32", "negative", dict(num_tokens=-1)),
    ("matcher_cost_hip_f32", "empty", dict(num_gt=0)),
    ("matcher_cost_hip_f32", "null", dict(tok_idx=NULL)),
    ("matcher_cost_hip_f32", "too_large", dict(num_pred=1 << 20, num_gt=1 << 20)),
    ("msda_hip_prologue_f32", "bad_dims", dict(num_heads=0)),
    ("msda_hip_prologue_f32", "ref_dim", dict(ref_dim=3)),
    ("msda_hip_prologue_f32", "levels_points", dict(num_levels=17, num_point=8)),
    ("msda_hip_prologue_f32", "empty", dict(num_query=0)),
    ("msda_hip_prologue_f32", "null", dict(attn_weight=NULL)),
    ("msda_hip_prologue_f32", "too_large", dict(batch=1 << 15, num_query=1 << 15, num_heads=1 << 10)),
    ("msda_hip_prologue_backward_f32", "bad_dims", dict(num_point=0)),
    ("msda_hip_prologue_backward_f32", "ref_dim", dict(ref_dim=1)),
    ("msda_hip_prologue_backward_f32", "levels_points", dict(num_levels=11, num_point=13)),
    ("msda_hip_prologue_backward_f32", "empty", dict(batch=0)),
    ("msda_hip_prologue_backward_f32", "null", dict(grad_attn_logits=NULL)),
    ("msda_hip_prologue_backward_f32", "too_large", dict(batch=1 << 15, num_query=1 << 15, num_heads=1 << 10)),
    ("ota_cost_hip_f32", "negative", dict(num_tokens=-1)),
    ("ota_cost_hip_f32", "batch_range", dict(batch=65)),
    ("ota_cost_hip_f32", "null_offsets", dict(gt_off=NULL)),
    ("ota_cost_hip_f32", "offsets_start", dict(gt_off={"i32": [1, 2]})),
    ("ota_cost_hip_f32", "offsets_order", dict(batch=2, gt_off={"i32": [0, 2, 1]})),
    ("ota_cost_hip_f32", "empty", dict(batch=0)),
    ("ota_cost_hip_f32", "empty_no_targets", dict(gt_off={"i32": [0, 0]})),
    ("ota_cost_hip_f32", "null", dict(iou=NULL)),
    ("ota_cost_hip_f32", "too_large", dict(num_queries=1 << 30, gt_off={"i32": [0, 1 << 10]})),
    ("ota_dynamic_k_hip", "negative", dict(num_queries=-1)),
    ("ota_dynamic_k_hip", "batch_range", dict(batch=-1)),
    ("ota_dynamic_k_hip", "empty", dict(batch=0)),
    ("ota_dynamic_k_hip", "targets", dict(gt_off={"i32": [0, 5000]})),
    ("ota_dynamic_k_hip", "null_counts", dict(num_selected=NULL)),
    ("ota_dynamic_k_hip", "null", dict(matching=NULL)),
]

# entry point -> the pointer arguments of its 16-byte alignment check: one case each, that pointer off by 4 bytes and every other
# one aligned
ALIGNED16 = {
    "patch_embed_hip_convnext_dwconv_ln_f32": ["out", "ln_weight", "ln_bias"],
    "qsel_scores_hip_f32": ["memory", "enc_weight", "ln_weight", "ln_bias", "class_vec", "output_memory"],
    "qsel_boxes_hip_f32": ["memory", "enc_weight", "ln_weight", "ln_bias", "w1", "w2", "w3", "coords_unact", "reference_points"],
    "biattn_hip_self_forward_f32": ["q", "k", "v", "out"],
    "patch_embed_hip_vit_attn_f32": ["qkv", "rel_h_table", "rel_w_table", "out", "workspace"],
    "detpost_nms_hip_f32": ["boxes"],
}


def all_cases():
    cases = [dict(id="%s-%s" % (fn, what), fn=fn, overrides=ov) for fn, what, ov in CASES]
    for fn, names in ALIGNED16.items():
        for name in names:
            cases.append(dict(id="%s-misaligned-%s" % (fn, name), fn=fn, overrides={name: MIS4}))
    for c in cases:
        spec = SPECS[c["fn"]]
        unknown = set(c["overrides"]) - {name for name, _, _ in spec}
        assert not unknown, (c["id"], unknown)
        c["args"] = [[kind, c["overrides"].get(name, default)] for name, kind, default in spec]
        del c["overrides"]
    assert len({c["id"] for c in cases}) == len(cases)
    return cases


_BASE = 0x10000


def marshal(args, keep):
    """ctypes values of a case's arguments; `keep` receives the host arrays so that they outlive the call."""
    def address(v, k):
        return {"null": None, "ok": _BASE + 256 * k, "mis4": _BASE + 256 * k + 4, "mis2": _BASE + 256 * k + 2}[v]
    out = []
    for k, (kind, v) in enumerate(args):
        if kind == "p" and isinstance(v, dict):
            (what, items), = v.items()
            if what == "ptrs":
                arr = (ctypes.c_void_p * len(items))(*[address(x, 64 + j) for j, x in enumerate(items)])
            else:
                arr = ({"i32": ctypes.c_int32, "i64": ctypes.c_int64}[what] * len(items))(*items)
            keep.append(arr)
            out.append(ctypes.cast(arr, ctypes.c_void_p))
        elif kind == "p":
            out.append(ctypes.c_void_p(address(v, k)))
        elif kind == "f":
            out.append(ctypes.c_float(v))
        else:
            out.append({"i": ctypes.c_int, "ll": ctypes.c_longlong, "z": ctypes.c_size_t}[kind](v))
    return out


def run(lib, case):
    """(code, message) the library answers a case with; the message is "" when the call is answered 0."""
    keep = []
    code = getattr(lib, case["fn"])(*marshal(case["args"], keep))
    return code, (lib.msda_hip_last_error().decode() if code != 0 else "")


def main():
    from uninext_amd import _lib
    lib = _lib.load()
    cases = all_cases()
    for c in cases:
        c["code"], c["message"] = run(lib, c)
        empty = c["id"].split("-")[1].startswith("empty")
        assert (c["code"] == 0) == empty and c["code"] <= 0, "%s reached the HIP runtime or is mislabelled: %r" % (c["id"], (c["code"], c["message"]))
    path = os.path.join(HERE, "rejections.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in cases) + "\n]\n")
    print("wrote %s: %d cases, %d distinct messages, library %s" % (path, len(cases), len({c["message"] for c in cases}) - 1, _lib.LIB_PATH))


if __name__ == "__main__":
    main()
