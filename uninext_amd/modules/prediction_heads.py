"""Decoder prediction heads: the step from the decoder's hidden states to the predictions.

Host-side mirror of the head statements of `DDETRSegmUniDN.coco_inference` (projects/UNINEXT/uninext/models/ddetrs_dn.py:413-435
and :468-483) and, per decoder level, of `coco_forward` (:190-222): `class_embed[lvl]` (a VL_Align or Still_Classifier),
`bbox_embed[lvl]` (the 3-layer box MLP), `iou_head[lvl]` (one Linear) and the `controller` (the 3-layer MLP that generates the
dynamic mask head's parameters), all on the same rows `hs[lvl]`.

`DetectionHeads` holds the four under the reference's attribute names, so the state-dict keys below it are the reference's
(`class_embed.N.dot_product_projection_text.weight`, `bbox_embed.N.layers.M.*`, `iou_head.N.*`, `controller.layers.M.*`).  It
keeps the objects it is given: a `bbox_embed` shared with `DeformableTransformerDecoder.bbox_embed` stays shared.

With `fused` set (the default), at inference on contiguous fp32 GPU tensors with d_model 256, at most 256 text tokens and at
most 256 generated parameters, a level is one HIP kernel (include/dynmask_hip.h: pred_heads_hip_f32) behind `VL_Align.token_terms` of the text;
otherwise it is the reference's composition of PyTorch ops, so training gradients are PyTorch's.
"""
import torch
from torch import nn

from .. import ext as MSDA
from .decoder_layer import inverse_sigmoid
from .query_selection import Still_Classifier, VL_Align, agg_lang_feat


class DetectionHeads(nn.Module):
    """class_embed, bbox_embed, iou_head (or None): nn.ModuleLists indexed by the decoder level; controller: an MLP (or None)."""

    # The HIP route (pred_heads_hip_f32).  On by default: tools/pred_heads_bench.py shows it faster than the composition in both
    # rows on an MI355X with the p10..p90 ranges apart (profiles/r41_pred_heads.txt, README "Decoder prediction heads").
    fused = True

    def __init__(self, class_embed, bbox_embed, iou_head=None, controller=None):
        super().__init__()
        self.class_embed = class_embed
        self.bbox_embed = bbox_embed
        self.iou_head = iou_head
        self.controller = controller

    def forward_level(self, lvl, hs_lvl, reference, text, want_controller=True):
        """(pred_logits [B, Q, T], pred_boxes [B, Q, 4], pred_iou [B, Q, 1] or None, mask_head_params [B, Q, P] or None) of
        decoder level lvl.  hs_lvl [B, Q, d_model]; reference [B, Q, 4 | 2], the level's reference points in sigmoid space;
        text [B, T, lang_dim], the token features for detection or the pooled [B, 1, lang_dim] for grounding and sot."""
        want_controller = want_controller and self.controller is not None
        if self.fused and self._inference(lvl, hs_lvl, reference, text, want_controller):
            return self._level_fused(lvl, hs_lvl, reference, text, want_controller)
        return self._level_composition(lvl, hs_lvl, reference, text, want_controller)

    forward = forward_level

    def _level_composition(self, lvl, hs_lvl, reference, text, want_controller):
        reference = inverse_sigmoid(reference)
        outputs_class = self.class_embed[lvl](hs_lvl, text)
        tmp = self.bbox_embed[lvl](hs_lvl)
        pred_iou = self.iou_head[lvl](hs_lvl) if self.iou_head is not None else None
        if reference.shape[-1] == 4:
            tmp += reference
        else:
            assert reference.shape[-1] == 2
            tmp[..., :2] += reference
        return outputs_class, tmp.sigmoid(), pred_iou, self.controller(hs_lvl) if want_controller else None

    def _inference(self, lvl, hs_lvl, reference, text, want_controller):
        class_embed, bbox_embed = self.class_embed[lvl], self.bbox_embed[lvl]
        modules = [class_embed, bbox_embed] + ([self.iou_head[lvl]] if self.iou_head is not None else []) \
            + ([self.controller] if want_controller else [])
        vl = isinstance(class_embed, VL_Align)
        tensors = (hs_lvl, reference) + ((text,) if vl else ())
        if any(not isinstance(t, torch.Tensor) for t in tensors):
            return False
        if torch.is_grad_enabled() and (any(t.requires_grad for t in tensors)
                                        or any(p.requires_grad for m in modules for p in m.parameters())):
            return False
        if not all(t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.device == hs_lvl.device for t in tensors):
            return False
        d = MSDA._lib.PRED_HEADS_D_MODEL
        if hs_lvl.dim() != 3 or hs_lvl.shape[-1] != d or reference.dim() != 3 or reference.shape[:2] != hs_lvl.shape[:2] \
                or reference.shape[-1] not in (2, 4):
            return False
        if any(p.dtype != torch.float32 or p.device != hs_lvl.device or not p.is_contiguous()
               for m in modules for p in m.parameters()):
            return False

        def mlp(m, out):
            layers = getattr(m, "layers", None)
            return layers is not None and len(layers) == 3 and all(isinstance(l, nn.Linear) and l.bias is not None for l in layers) \
                and [tuple(l.weight.shape) for l in layers[:2]] == [(d, d), (d, d)] and layers[2].weight.shape[1] == d \
                and (out is None or layers[2].weight.shape[0] == out)

        if not mlp(bbox_embed, 4):
            return False
        if want_controller and not (mlp(self.controller, None)
                                    and 1 <= self.controller.layers[2].weight.shape[0] <= MSDA._lib.PRED_HEADS_MAX_PARAMS):
            return False
        if self.iou_head is not None:
            iou = self.iou_head[lvl]
            if not (isinstance(iou, nn.Linear) and tuple(iou.weight.shape) == (1, d) and iou.bias is not None):
                return False
        if vl:
            return (text.dim() == 3 and text.shape[0] == hs_lvl.shape[0] and 1 <= text.shape[1] <= MSDA._lib.PRED_HEADS_MAX_TOKENS
                    and tuple(class_embed.dot_product_projection_text.weight.shape) == (d, text.shape[2]))
        return isinstance(class_embed, Still_Classifier) and tuple(class_embed.body.weight.shape) == (1, d)

    def class_terms(self, lvl, text):
        """(tokens [B | 1, T, d], token_bias [B | 1, T], scale [1] or None, clamp) of level lvl's class head, device tensors."""
        class_embed = self.class_embed[lvl]
        if isinstance(class_embed, VL_Align):
            tokens, bias = class_embed.token_terms(text)
            return tokens.contiguous(), bias.contiguous(), class_embed.log_scale.exp(), class_embed.clamp
        return class_embed.body.weight.view(1, 1, -1), class_embed.body.bias.view(1, 1), None, 0.0

    def _level_fused(self, lvl, hs_lvl, reference, text, want_controller):
        with torch.no_grad():
            flat = lambda m: [t for l in m.layers for t in (l.weight, l.bias)]
            iou = None if self.iou_head is None else (self.iou_head[lvl].weight, self.iou_head[lvl].bias)
            logits, boxes, pred_iou, params = MSDA.pred_heads(
                hs_lvl, *self.class_terms(lvl, text), reference, flat(self.bbox_embed[lvl]), iou,
                flat(self.controller) if want_controller else None)
            return logits, boxes, None if pred_iou is None else pred_iou.unsqueeze(-1), params

    def inference(self, hs, init_reference, inter_references, language_dict_features, task, image_sizes, cls_pool_type="average"):
        """The last decoder level's predictions as `coco_inference` forms them.  hs [n_levels, B, Q, d_model]; init_reference
        [B, Q, 4 | 2] and inter_references [n, B, Q, 4 | 2] as the decoder returns them; language_dict_features with `hidden`
        [B, L, lang_dim] and `masks` [B, L]; image_sizes one (height, width) per image.  Returns a dict: pred_logits, pred_boxes,
        pred_boxious (with an IoU branch), mask_head_params [1, B * Q, P] and reference_points [1, B * Q, 2], which is
        inter_references[-2][..., :2] in the pixels of each image, (x, y)."""
        if task == "grounding" or task == "sot":
            text = agg_lang_feat(language_dict_features["hidden"], language_dict_features["masks"],
                                 pool_type=cls_pool_type).unsqueeze(1)
        elif task == "detection":
            text = language_dict_features["hidden"]
        else:
            raise ValueError("task must be detection or grounding")
        lvl = hs.shape[0] - 1
        reference = init_reference if lvl == 0 else inter_references[lvl - 1]
        logits, boxes, pred_iou, params = self.forward_level(lvl, hs[lvl], reference, text)
        outputs = {"pred_logits": logits, "pred_boxes": boxes}
        if pred_iou is not None:
            outputs["pred_boxious"] = pred_iou
        points = inter_references[-2][..., :2]
        scale = torch.stack([torch.stack([torch.as_tensor(w).to(points), torch.as_tensor(h).to(points)]) for h, w in image_sizes])
        outputs["reference_points"] = (points * scale[:, None, :]).reshape(1, -1, 2)
        if params is not None:
            outputs["mask_head_params"] = params.reshape(1, -1, params.shape[-1])
        return outputs
