from .opt import pad_length_to_make_divisible, pad_mat_to_make_divisible
from .adaptive_scaling import (
    AdaptiveScalingInferencingConfig,
    AdaptiveScalingInferencingRoughInferResult,
    AdaptiveScalingInferencingRoughTextRegions,
    AdaptiveScalingInferencingPresiceInferResult,
    AdaptiveScalingInferencingPreciseCharPolygons,
    AdaptiveScalingInferencing,
    precise_group_char_polygons,
)
from .graphs import GraphCache, param_stamp
from .regions import region_scales, text_regions_host
