from .ms_deform_attn_func import MSDeformAttnFunction, MSDeformAttnFusedFunction  # noqa: F401
from .layer_train import DropoutAddLayerNormFunction, ReluDropoutFunction  # noqa: F401
