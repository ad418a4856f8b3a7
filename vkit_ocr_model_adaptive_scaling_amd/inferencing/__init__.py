from .opt import pad_length_to_make_divisible, pad_mat_to_make_divisible
from .adaptive_scaling import (
    AdaptiveScalingInferencingConfig,
    AdaptiveScalingInferencingRoughInferResult,
    AdaptiveScalingInferencingRoughTextRegions,
    AdaptiveScalingInferencingPresiceInferResult,
    AdaptiveScalingInferencingPreciseCharPolygons,
    AdaptiveScalingInferencingResult,
    AdaptiveScalingInferencingBatchResult,
    AdaptiveScalingInferencing,
    precise_group_char_polygons,
)
from .graphs import GraphCache, param_stamp
from .regions import region_scales, text_regions_host
from .packing import (SIDE_MAX, axis_weights, check_placements, pack_region_labels_host, region_crops, remap_polygons,
                      resample_host, stack_regions, check_warps, remap_polygons_affine, warp_host, warp_region_labels_host,
                      check_multi_rows, pack_region_labels_multi_host, resample_pack_multi_host, stack_regions_pages)
from .quad_tables import (clamped, host_table, host_tables, pad_quads, pad_rows, pad_values, padded_sides, quad_lists,
                          require_gpu, with_capacity)
from .evaluation import (DetectionScore, QuadMatchResult, care_pairs, check_iou_thr, evaluate_quads, evaluate_quads_host,
                         evaluation_tables, match_quads_host, match_rows, quad_iou_host, quad_rows_host, result_quads)
from .nms import (QuadNmsResult, filter_result, greedy_suppression, nms_pairs, nms_quads, nms_quads_host,
                  nms_quads_lists_host, nms_tables, suppress_results)
from .lines import (QuadLinesResult, group_results, line_params, line_quads, link_pairs, quad_frames, quad_lines,
                    quad_lines_host, quad_lines_lists_host)
from .ranking import (OperatingPoint, PRCurve, RankedMatchResult, RankedPairs, RankedScore, average_precision_host,
                      evaluate_quads_ranked, evaluate_quads_ranked_host, match_quads_ranked_host,
                      match_quads_ranked_rounds_host, quad_inter2_host, ranked_matching, ranked_matching_rounds, ranked_pairs,
                      ranked_score)
from .orient import (orient_regions, oriented_rects, region_directions, region_extents_host, region_moments_host, warp_row)
from .strips import (QuadStrips, StripLayout, check_strip_rows, quad_strips_host, remap_strip_points, strip_params, strip_rows,
                     strip_table, strip_warp)
from .spines import (SpineLayout, SpineStrips, check_spine_rows, knot_status, spine_columns_host, spine_knots, spine_pixels_host,
                     spine_points, spine_polygon, spine_rows, spine_strips_host, spine_table)
from .line_strips import quad_strips, result_lines, spine_strips, spine_strips_for_results, strips_for_results
from .line_evaluation import (LineMatchResult, LineScore, check_line_thresholds, evaluate_lines, evaluate_lines_host,
                              line_pairs, match_lines_host, match_lines_rounds_host)
from .ribbon_evaluation import (evaluate_ribbons, evaluate_ribbons_host, match_ribbons_host, match_ribbons_rounds_host,
                                polygon_ribbon, quad_ribbon, result_ribbons, ribbon_inter, ribbon_list, ribbon_pairs,
                                ribbon_rows, ribbon_tables, spine_ribbon)
