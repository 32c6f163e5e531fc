"""DeformableTransformerEncoderVL (models/deformable_detr/deformable_transformer_dino.py:277-327): the loop that owns the
early-fusion layers (modules/vl_fusion.py: VLFuse), the encoder layers (modules/encoder_layer.py) and the language layers, over the
{"visual", "lang"} dict.  Child names are the reference's (`vl_layers`, `layers`, `lang_layers`), so its checkpoints load.

Not built: use_checkpoint (the reference itself raises for it) and a language layer other than nn.Identity
(USE_ADDITIONAL_BERT is False in every shipped config)."""
import copy

from torch import nn

from .encoder_input import get_reference_points


def _get_clones(module, N):
    return nn.ModuleList([copy.deepcopy(module) for i in range(N)])


def _get_clones_advanced(module, N, N_valid):
    assert N_valid <= N
    layers = []
    for i in range(N):
        if i < N_valid:
            layers.append(copy.deepcopy(module))
        else:
            layers.append(nn.Identity())
    return nn.ModuleList(layers)


class DeformableTransformerEncoderVL(nn.Module):
    def __init__(self, vl_fusion_layer, encoder_layer, lang_encoder_layer, num_layers, use_checkpoint=False, num_vl_layers=None):
        super().__init__()
        if use_checkpoint:
            raise ValueError("NOT supported for now")
        if not isinstance(lang_encoder_layer, nn.Identity):
            raise ValueError("lang_encoder_layer must be nn.Identity: the additional BERT layers (USE_ADDITIONAL_BERT) are not built")
        num_vl_layers = num_layers if num_vl_layers is None else num_vl_layers
        self.vl_layers = _get_clones_advanced(vl_fusion_layer, num_layers, num_vl_layers)
        self.layers = _get_clones(encoder_layer, num_layers)
        self.lang_layers = _get_clones(lang_encoder_layer, num_layers)
        self.num_layers = num_layers
        self.use_checkpoint = use_checkpoint

    get_reference_points = staticmethod(get_reference_points)

    def set_own_training(self, flag=True, dropout=False):
        """DeformableTransformerEncoderLayer.own_training on every encoder layer: under autograd the add + LayerNorm blocks and
        the FFN's ReLU run on the HIP training kernels (functions/layer_train.py) where they apply.  dropout=True sets own_dropout
        as well: ACTIVE dropout is then served by the kernels, whose keep masks are not F.dropout's stream.  Returns self."""
        for layer in self.layers:
            layer.own_training = bool(flag)
            layer.own_dropout = bool(flag) and bool(dropout)
        return self

    def forward(self, src, spatial_shapes, level_start_index, valid_ratios, pos=None, padding_mask=None, language_dict_features=None,
                task=None, reference_points=None):
        """The reference's forward.  `reference_points` (not in the reference): prepare_encoder_inputs' tensor, which spares the
        loop over the levels and its copy of spatial_shapes to the host."""
        output = {"visual": src, "lang": language_dict_features}
        if reference_points is None:
            reference_points = self.get_reference_points(spatial_shapes, valid_ratios, device=src.device)
        for _, (vl_layer, layer, lang_layer) in enumerate(zip(self.vl_layers, self.layers, self.lang_layers)):
            if isinstance(vl_layer, nn.Identity):
                output = vl_layer(output)
            else:
                output = vl_layer(output, task=task)
            output["visual"] = layer(output["visual"], pos, reference_points, spatial_shapes, level_start_index, padding_mask)
            output = lang_layer(output)
        return output
