"""uninext_amd -- MI355X (gfx950) native MultiScaleDeformableAttention path for UNINEXT.

Layout (only what the hot path needs):
  csrc/        hand-written HIP kernels + the C ABI (include/msda_hip.h) -> lib/libmsda_hip.so
  _lib.py      ctypes binding of the C ABI (no torch types cross the boundary)
  ext.py       `ms_deform_attn_forward/backward` with the reference pybind signatures
  functions/   MSDeformAttnFunction   (mirror of ops/functions/ms_deform_attn_func.py)
  modules/     MSDeformAttn nn.Module (mirror of ops/modules/ms_deform_attn.py)
The repo-root module `MultiScaleDeformableAttention` re-exports ext.py under the name the
reference imports (ops/functions/ms_deform_attn_func.py:18).
"""
__version__ = "0.1.0"


def __getattr__(name):
    # the trackers' public classes, imported on first use: importing the package alone loads neither torch nor the library
    if name == "IDOL_Tracker":
        from .tracker import IDOL_Tracker
        return IDOL_Tracker
    if name == "QuasiDenseEmbedTracker":
        from .tracker import QuasiDenseEmbedTracker
        return QuasiDenseEmbedTracker
    if name in ("select_pos_neg", "get_pos_idx", "get_in_boxes_info", "dynamic_k_matching", "loss_reid", "VideoSetCriterion", "VideoDINOCriterion", "PackedContrastItems", "ReidLossFunction"):
        from . import reid                       # re-ID contrastive training (uninext_amd/reid.py), likewise
        return getattr(reid, name)
    if name in ("unfold_wo_center", "compute_project_term", "compute_pairwise_term", "get_images_color_similarity", "rgb2lab",
                "boxinst_targets", "BoxInstSetCriterion", "BoxInstDINOCriterion", "BoxInstLossesFunction"):
        from . import boxinst                    # BoxInst training (uninext_amd/boxinst.py), likewise
        return getattr(boxinst, name)
    if name in ("BertConfig", "BertEmbeddings", "BertSelfAttention", "BertSelfOutput", "BertAttention", "BertIntermediate", "BertOutput",
                "BertLayer", "BertModel", "BertEncoder", "BertSelfAttentionFunction"):
        import importlib                         # the BERT prompt encoder (uninext_amd/text_encoder.py), likewise; no `transformers`
        return getattr(importlib.import_module(".text_encoder", __name__), name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
