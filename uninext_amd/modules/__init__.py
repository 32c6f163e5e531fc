from .ms_deform_attn import MSDeformAttn  # noqa: F401
from .encoder_layer import DeformableTransformerEncoderLayer  # noqa: F401
from .vl_fusion import BiMultiHeadAttention, BiAttentionBlockForCheckpoint, VLFuse  # noqa: F401
from .decoder_layer import (DeformableTransformerDecoderLayer, DeformableTransformerDecoder, DeformableReidHead, MLP,  # noqa: F401
                            get_sine_pos_embed, inverse_sigmoid, DecoderSelfAttentionFunction)
from .encoder_input import (PositionEmbeddingSine, NestedTensor, EncoderInputs, interpolate_mask, get_valid_ratio,  # noqa: F401
                            get_reference_points, build_input_proj, flatten_encoder_inputs, prepare_encoder_inputs)
from .encoder import DeformableTransformerEncoderVL  # noqa: F401
from .query_selection import (VL_Align, Still_Classifier, TwoStageQuerySelection, select_queries, agg_lang_feat,  # noqa: F401
                              gen_encoder_output_proposals)
from .prediction_heads import DetectionHeads  # noqa: F401
