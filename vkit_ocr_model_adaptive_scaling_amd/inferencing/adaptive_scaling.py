"""Tensor side of the adaptive-scaling inference path (mirror of vkit_open_model/inferencing/adaptive_scaling.py:92-188,
295-396 and the shape rules of :95-107): pad-to-32, the short-side-720 rule, the no-grad model calls and the
sigmoid / threshold / softmax / padding-mask post-processing, which runs on the device (csrc/infer.hip).  The step that
turns the precise maps into characters - the maximum-filter peaks of the char probability map and one quadrilateral per
peak (:399-465,481-491) - runs on the device too (csrc/charpoly.hip, ``precise_infer_char_polygons``), inside the same
HIP graph as the model call; ``precise_group_char_polygons`` splits its points by a caller-given region label map on the
host (the device-free half of :467-525).

The step between the passes - the text regions of the rough mask, the median character height of each and the scale that
brings it to 35 px (:190-279) - runs on the device as well (csrc/regions.hip, ``rough_infer_text_regions``), in the rough
pass's HIP graph, restated on pixels: a region is an 8-connected component of the rough mask, not an external contour (a
hole is not filled, a component inside a hole is a region of its own), and its axis-aligned box stands in for vkit's
flattened region in the scale rule (inferencing/regions.py states the rule and holds the host oracle).

The step the model is named after - cut every text region out of the page, rescale it so that its median character
height becomes 35 px and stack the cuts into the page of the precise pass (:190-293) - runs on the device too
(csrc/respack.hip, ``ops.resample_pack_u8`` / ``ops.pack_region_labels``), and ``infer`` chains all of it: image in,
characters per region in image coordinates out.  It differs from the reference where vkit and cv2 (absent here) would be
needed: a region's axis-aligned box stands in for the flattened region - unless ``precise_text_region_orient`` is set: then
an elongated, slanted region is cut out along its own axis and turned by the small angle that makes it axis-parallel
(inferencing/orient.py, csrc/orient.hip; deskewing only: no perspective, no curved lines, no polygon dilation) -; the
interpolation rule is this project's own, in integers (inferencing/packing.py); stacking is a shelf packing; and a character
of a neighbouring region inside an overlapping box is excluded through the rough label map instead of ``flattened_mask``.
``infer_batch`` does the same for a list of images at once: the rough pass runs on batches of one padded shape, and the
regions of ALL images are cut in one launch into shared pages of at most 2048 x 1536 (the multi kernels of
csrc/respack.hip; ``stack_regions_pages``), so N small images cost a few full precise passes instead of N padded ones.

Out of scope: polygons of the rough regions and flattening beyond deskewing (vkit, cv2).  Images are plain (H, W, 3) uint8 arrays instead of ``vkit.element.Image``; results carry
numpy arrays instead of ``Mask`` / ``ScoreMap`` / ``Polygon``.  The reference loads a TorchScript file (``model_jit``,
:85-90); so does this mirror (``torch.jit.save`` of ``torch.jit.script(model)``, see model/scripting.py), and it also takes
the scripted or the eager ``AdaptiveScaling`` module itself, or a state-dict file in the reference's ``RestoreState`` schema.
"""
import ctypes
import math
from typing import Optional, Sequence, Tuple, Union

import attrs
import numpy as np
import torch

from .opt import pad_mat_to_make_divisible
from .graphs import GraphCache, param_stamp
from .regions import region_scales
from .packing import (SIDE_MAX, check_multi_rows, check_warps, region_crops, remap_polygons, remap_polygons_affine,
                      stack_regions, stack_regions_pages)
from .orient import orient_regions, region_directions, warp_row
from .nms import suppress_results
from .lines import group_results
from .line_strips import spine_strips_for_results, strips_for_results
from .strips import QuadStrips
from .. import ops
from .._lib import lib, check
from ..model import AdaptiveScaling, AdaptiveScalingConfig


@attrs.define
class AdaptiveScalingInferencingConfig:
    """inferencing/adaptive_scaling.py:41-58 (tensor-side fields, same names - including the reference's spelling
    ``legnth`` - and defaults).  ``model_jit``: the path of a TorchScript file (the reference's usage) or of a state-dict
    file (then ``model_config`` is needed), a scripted module, or an eager ``AdaptiveScaling`` module - which is then
    switched to eval mode and to ``compute_dtype`` IN PLACE (pass a copy to keep a training module as it is), a scripted one
    likewise (its recipe string is rewritten)."""
    model_jit: Union[str, AdaptiveScaling, torch.jit.ScriptModule, None] = None
    device: str = 'cuda'
    backbone_downsampling_factor: int = 32
    rough_head_upsampling_factor: int = 2
    rough_downsample_short_side_legnth: int = 720
    rough_char_mask_positive_thr: float = 0.5
    rough_valid_char_height_min: float = 3.0
    precise_head_upsampling_factor: int = 2
    precise_char_mask_positive_thr: float = 0.5
    model_config: Optional[AdaptiveScalingConfig] = None  # needed to rebuild the module from a state-dict file
    compute_dtype: torch.dtype = torch.float16            # BASELINE.json configs[4]
    # replay one captured HIP graph per (pass, padded shape) instead of enqueuing its few hundred launches from Python; the
    # first call of a shape runs eagerly (inferencing/graphs.py).  Same results bit for bit.
    use_hip_graphs: bool = True
    # :58-59, read by precise_infer_char_polygons (peak threshold, compared in fp32; scipy maximum_filter size, truncated)
    precise_build_polygons_positive_char_prob_thr: float = 0.7
    precise_build_polygons_maximum_filter_size: float = 5
    # :53-54, read by rough_infer_text_regions: the median character height a text region is rescaled to, and the share of
    # it below which a rescaled region (both sides) is dropped
    precise_flattened_text_region_resized_char_height_median: int = 35
    precise_flattened_text_region_resized_ratio_min: float = 0.25
    # table rows of rough_infer_text_regions; a page with more regions reports its true count and the first rows
    rough_text_regions_max: int = 4096
    # :55-56, read by infer: the margin around the stacked page and the gap between stacked regions, in pixels
    precise_stack_flattened_text_regions_page_pad: int = 10
    precise_stack_flattened_text_regions_pad: int = 2
    # The stacked page (inferencing/packing.py::stack_regions; both multiples of 32).  Width: the long side of the
    # reference's 2048 x 1536 page - text near 35 px (scale near 1) then stacks to no more area than the source held, so
    # such a page becomes ONE page no taller than the source, and a line as wide as the source minus the two page pads
    # still fits a row.  The height is not capped - one page always - and grows in steps: a 2048-wide page between 256
    # and 1536 rows takes one of six shapes, so the HIP-graph cache (one graph per page shape) stays small, at the price
    # of up to 255 rows of padding for the precise pass.
    precise_page_width_max: int = 2048
    precise_page_height_step: int = 256
    # Read by infer_batch only (infer stays uncapped): the height of a shared page, the short side of the reference's
    # 2048 x 1536 page and a multiple of precise_page_height_step - the regions of a batch spill onto further pages of this
    # height (inferencing/packing.py::stack_regions_pages) -, and the largest batch of one rough graph: a group of images of
    # one padded rough shape is split into chunks of at most this many, so the graph cache holds one graph per (shape,
    # chunk size) and not one per arbitrary B.
    precise_page_height_max: int = 1536
    rough_batch_max: int = 8
    # Oriented text regions (inferencing/orient.py; the reference's TextRegionFlattener, deskewing only), read by infer: a
    # kept region that is slanted by at least 1 degree, whose oriented rectangle is at least this many times longer than
    # wide (the reference's typical_long_side_ratio_min) and packs smaller than its box, is cut out along its own axis.
    # Off: every result is bit for bit what it is without the feature.
    precise_text_region_orient: bool = False
    precise_text_region_flattener_typical_long_side_ratio_min: float = 3.0
    # Suppression of duplicate characters (inferencing/nms.py), read by infer and infer_batch: after the quads are mapped back
    # into the image, the characters of one image - all regions together - go through one greedy suppression at this IoU
    # threshold (in (0, 1]).  0 = off: every result is bit for bit what it is without the feature, with no extra launch or
    # copy.
    precise_char_nms_iou_thr: float = 0.0
    # Text lines (inferencing/lines.py), read by infer and infer_batch: after the suppression step (if any), the characters of
    # one image - in ``result_quads`` order, all regions together - are grouped into lines in reading order, one device call
    # for all images.  ``gap`` (along the line), ``cross`` (across it) and ``height_ratio`` are in character heights.  Off:
    # every result is bit for bit what it is without the feature, with no extra launch or copy.
    precise_char_lines: bool = False
    precise_char_line_gap: float = 1.5
    precise_char_line_cross: float = 0.5
    precise_char_line_height_ratio: float = 2.0
    # Line strips (inferencing/strips.py), read by infer and infer_batch; needs precise_char_lines: the oriented rectangle of
    # every line is cut out of its image, turned upright and brought to ``height`` rows - the recogniser's input -, all
    # lines of all images in one launch (csrc/strips.hip).  ``margin`` (around the rectangle) is in line heights; a strip is
    # at most ``width_max`` columns (a longer line is squeezed) and lies in a slot whose width is a multiple of
    # ``width_step``.  Off: every result is bit for bit what it is without the feature, with no extra launch or copy.
    precise_line_strips: bool = False
    precise_line_strip_height: int = 32
    precise_line_strip_width_max: int = 2048
    precise_line_strip_width_step: int = 64
    precise_line_strip_margin: float = 0.125
    # Curved lines (inferencing/spines.py), read by infer and infer_batch; needs precise_line_strips: every line is cut along
    # the spine through its characters (csrc/spines.hip) instead of along its chord rectangle, with the same height, widths
    # and margin; ``line_strips`` is then a ``SpineStrips`` and the results gain ``line_spines``.  ``line_polygons`` stays the
    # chord rectangle.  Off: every result is bit for bit what it is without the feature, with no extra launch or copy.
    precise_line_strip_curved: bool = False


@attrs.define
class AdaptiveScalingInferencingRoughInferResult:
    """:61-66"""
    resized_shape: Tuple[int, int]
    padded_image: np.ndarray
    rough_char_mask: np.ndarray              # (H/FDF, W/FDF) uint8
    rough_char_height_score_map: np.ndarray  # (H/FDF, W/FDF) float32


@attrs.define
class AdaptiveScalingInferencingRoughTextRegions:
    """The text regions of one page and their scales (:190-279 on pixels, see inferencing/regions.py): region r is row
    r - 1; N = min(num_regions, config.rough_text_regions_max) rows."""
    resized_shape: Tuple[int, int]
    padded_image: np.ndarray
    num_regions: int                  # the true number of regions, also when it exceeds the table
    labels: Optional[np.ndarray]      # (H/FDF, W/FDF) int32, 0 = background, regions 1..num_regions; None if not asked for
    boxes: np.ndarray                 # (N, 4) int32 inclusive (y0, x0, y1, x1) in map pixels
    areas: np.ndarray                 # (N,) int32 pixels
    valid: np.ndarray                 # (N,) int32 pixels with a valid character height
    char_height_medians: np.ndarray   # (N,) float32 median of the valid heights, as predicted (0 without any)
    scales: np.ndarray                # (N,) float64, 0 for a region without a valid height
    resized_shapes: np.ndarray        # (N, 2) int64 (height, width) of the rescaled region
    keep: np.ndarray                  # (N,) bool: False for the regions the reference skips


@attrs.define
class AdaptiveScalingInferencingPresiceInferResult:
    """:69-76 (the reference's spelling)"""
    padded_image: np.ndarray
    precise_char_mask: Optional[np.ndarray]
    precise_char_prob_score_map: np.ndarray
    precise_np_char_up_left_corner_offset: np.ndarray      # (H/FDF, W/FDF, 2)
    precise_np_char_corner_angle_distribution: np.ndarray  # (H/FDF, W/FDF, 4)
    precise_np_char_corner_distance: np.ndarray            # (H/FDF, W/FDF, 4)


@attrs.define
class AdaptiveScalingInferencingPreciseCharPolygons:
    """The characters of one page (:399-465,481-525): the peaks of the precise char probability map and their
    quadrilaterals, in np.nonzero (row-major) order."""
    padded_image: np.ndarray
    points: np.ndarray    # (N, 2) int32 (y, x) in map pixels
    probs: np.ndarray     # (N,) float32, the char probability at each point
    polygons: np.ndarray  # (N, 4, 2) float32 (y, x) in padded-image pixels: up-left, up-right, down-right, down-left


@attrs.define
class AdaptiveScalingInferencingResult:
    """``infer``: the characters of one image, grouped by text region, in the coordinates of the image as given.  Lists
    have one entry per row of ``regions`` (region r is entry r - 1; empty for a region that was not packed)."""
    image_shape: Tuple[int, int]
    regions: AdaptiveScalingInferencingRoughTextRegions  # the region table; padded_image / labels only on request
    packed: np.ndarray          # (N,) bool: the region has a placement
    too_large: np.ndarray       # (N,) bool: kept, but wider than the page or with a side above the resampling limit
    placements: np.ndarray      # (M, 8) int32 (sy, sx, sh, sw, dy, dx, dh, dw): image rectangle -> page rectangle
    placement_regions: np.ndarray  # (M,) int32: the region (1-based) of each placement
    page_shape: Tuple[int, int]
    page: Optional[np.ndarray]  # the stacked (Hp, Wp, 3) uint8 page, only on request
    region_labels: Optional[np.ndarray]  # the (Hp/FDF, Wp/FDF) int32 label page, only on request
    points: Sequence[np.ndarray]    # per region (k, 2) int32 (y, x) in the precise maps of the page
    probs: Sequence[np.ndarray]     # per region (k,) float32
    polygons: Sequence[np.ndarray]  # per region (k, 4, 2) float64 (y, x) in image pixels
    # oriented regions (config.precise_text_region_orient; empty / all False without it): ``placements`` holds the
    # axis-aligned rows only, an oriented region has a warp row instead (inferencing/packing.py), and ``regions.keep`` /
    # ``regions.resized_shapes`` are the rule's after orientation
    oriented: np.ndarray = attrs.field(factory=lambda: np.zeros((0,), bool))             # (N,) bool
    warps: np.ndarray = attrs.field(factory=lambda: np.zeros((0, 12), np.int64))         # (K, 12) int64
    warp_regions: np.ndarray = attrs.field(factory=lambda: np.zeros((0,), np.int32))     # (K,) int32, 1-based
    # infer_batch: the shared page each placement lies on (empty from infer, which has one page).  There ``page_shape`` /
    # ``page`` / ``region_labels`` are those of the image's first placement's page, which other images share
    placement_pages: np.ndarray = attrs.field(factory=lambda: np.zeros((0,), np.int32))  # (M,) int32
    # config.precise_char_nms_iou_thr: the characters the suppression removed from the lists above, and its status - 0, or 2
    # for an image with more characters than the suppression takes (8192), which is left as it is
    num_suppressed: int = 0
    nms_status: int = 0
    # config.precise_char_lines: the line of each character in ``result_quads`` order (-1 for an invalid quad), the characters
    # of each line in reading order, the lines' oriented rectangles in image pixels (``line_quads``), and the status - 0, or
    # 2 for an image with more characters than the grouping takes (8192), which gets no lines
    char_lines: np.ndarray = attrs.field(factory=lambda: np.zeros((0,), np.int32))         # (n,) int32
    line_chars: list = attrs.field(factory=list)                                          # L int32 index arrays
    line_polygons: np.ndarray = attrs.field(factory=lambda: np.zeros((0, 4, 2), np.float64))  # (L, 4, 2) float64 (y, x)
    lines_status: int = 0
    # config.precise_line_strips: for each line its index into the strips object (inferencing/strips.py::QuadStrips) - from
    # infer ``line_strips``, from infer_batch the batch result's ``line_strips``, which all its images share
    line_strip_ids: np.ndarray = attrs.field(factory=lambda: np.zeros((0,), np.int32))     # (L,) int32
    line_strips: Optional[QuadStrips] = None
    # config.precise_line_strip_curved: ``line_strips`` is a ``SpineStrips`` (inferencing/spines.py), and per line the
    # (K, 2, 2) float64 centres and down vectors of its spine in image pixels ((0, 2, 2) for a line without a strip)
    line_spines: list = attrs.field(factory=list)


@attrs.define
class AdaptiveScalingInferencingBatchResult:
    """``infer_batch``: one result per image, in input order, and the shared pages their regions were packed into."""
    results: Sequence[AdaptiveScalingInferencingResult]
    page_shapes: Sequence[Tuple[int, int]]  # per page: all of one width, all but the last of config.precise_page_height_max
    rows: np.ndarray                        # (M, 12) int32 multi rows (inferencing/packing.py), sorted by page
    # only on request, per page (none when no region was packed): (Hp, Wp, 3) uint8; (Hp/FDF, Wp/FDF) int32 global region ids
    pages: Optional[Sequence[np.ndarray]] = None
    region_labels: Optional[Sequence[np.ndarray]] = None
    line_strips: Optional[QuadStrips] = None  # config.precise_line_strips: the strips of the lines of all images


def rough_resized_shape(height: int, width: int, short_side: int) -> Tuple[int, int]:
    """:95-107: when the shorter side exceeds ``short_side`` the image is shrunk so that it equals it (the other side
    keeps the aspect ratio, rounded like vkit's ``to_resized_image``)."""
    if min(height, width) <= short_side:
        return height, width
    if height < width:
        return short_side, round(short_side * width / height)
    return round(short_side * height / width), short_side


def _as_mat(image) -> np.ndarray:
    mat = getattr(image, 'mat', image)
    mat = np.asarray(mat)
    if mat.ndim != 3 or mat.shape[2] != 3:
        raise ValueError(f'expected an (H, W, 3) RGB image, got {mat.shape}')
    return mat


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _no_characters(n: int):
    """``points, probs, polygons`` of a result for n regions, each without characters."""
    return ([np.zeros((0, 2), np.int32) for _ in range(n)], [np.zeros((0,), np.float32) for _ in range(n)],
            [np.zeros((0, 4, 2), np.float64) for _ in range(n)])


class AdaptiveScalingInferencing:
    """:79-188,295-396 without the vkit geometry."""

    def __init__(self, config: AdaptiveScalingInferencingConfig):
        self.config = config
        self.graphs = GraphCache(enabled=config.use_hip_graphs)
        model = config.model_jit
        if isinstance(model, str):
            try:  # :85-90: a TorchScript file (the operator it calls is registered by importing this package)
                model = torch.jit.load(model, map_location=config.device)
            except RuntimeError:  # not a TorchScript archive: a state-dict / RestoreState file
                if config.model_config is None:
                    raise ValueError('model_config is required to rebuild the module from a state-dict file') from None
                sd = torch.load(model, map_location='cpu', weights_only=True)
                sd = sd.get('model_jit_state_dict', sd) if isinstance(sd, dict) else sd  # RestoreState schema, train.py:91-96
                module = AdaptiveScaling(config.model_config)
                module.load_state_dict(sd)
                model = module
        if isinstance(model, torch.jit.ScriptModule):
            # a scripted module carries its construction recipe as a string attribute (model/scripting.py); the storage type
            # in it is switched to config.compute_dtype, as set_compute_dtype does for an eager module below
            from ..model import scripting
            if not hasattr(model, '_script_spec'):
                raise TypeError('config.model_jit is a TorchScript module that this package did not script')
            model._script_spec = scripting.with_compute_dtype(model._script_spec, config.compute_dtype)
            self.model = model.to(config.device).eval()
            return
        if not isinstance(model, AdaptiveScaling):
            raise TypeError('config.model_jit must be a TorchScript file / module, an AdaptiveScaling module or a state-dict file')
        self.model = model.to(config.device).eval()
        self.model.set_compute_dtype(config.compute_dtype)

    # ---- shared pieces ------------------------------------------------------------------------------------------
    def _to_device(self, mats: Sequence[np.ndarray]) -> torch.Tensor:
        """(H, W, 3) uint8 arrays of one padded size -> (B, 3, H, W) fp32 on the device (:117-122)."""
        x = torch.from_numpy(np.stack([np.ascontiguousarray(m) for m in mats]))
        x = x.to(self.config.device, non_blocking=True)
        return x.permute(0, 3, 1, 2).float()

    @staticmethod
    def _valid(sizes: Sequence[Tuple[int, int]], fdf: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
        vh = torch.tensor([math.ceil(h / fdf) for h, _ in sizes], dtype=torch.int32, device=device)
        vw = torch.tensor([math.ceil(w / fdf) for _, w in sizes], dtype=torch.int32, device=device)
        return vh, vw

    # ---- rough pass ----------------------------------------------------------------------------------------------
    def _device_rough_page(self, src: torch.Tensor, h: int, w: int) -> torch.Tensor:
        """The (H, W, 3) uint8 device image resampled to h x w (the area-coverage shrink of the 720 rule; the identity when
        the sizes agree) inside a zero page padded to the backbone's factor: csrc/respack.hip with a single placement."""
        f = self.config.backbone_downsampling_factor
        H, W = int(src.shape[0]), int(src.shape[1])
        if max(H, W) > SIDE_MAX:
            raise ValueError(f'image {(H, W)}: the device resampler takes sides up to {SIDE_MAX}')
        table = np.array([[0, 0, H, W, 0, 0, h, w]], np.int32)
        return ops.resample_pack_u8(src, table, (-(-h // f) * f, -(-w // f) * f))

    def _rough_input(self, image, resize_fn):
        """-> the image as given, (h, w) after the 720 rule, the padded image (numpy) and the model input on the device.
        ``resize_fn``: None (an image that needs shrinking is rejected), a callable ``(mat, height, width)`` on the host, or
        'device': the shrink runs on the MI355X with this package's own integer area rule (inferencing/packing.py)."""
        c = self.config
        mat = _as_mat(image)
        h, w = rough_resized_shape(mat.shape[0], mat.shape[1], c.rough_downsample_short_side_legnth)
        if isinstance(resize_fn, str) and resize_fn != 'device':
            raise ValueError(f"resize_fn must be None, a callable or 'device', got {resize_fn!r}")
        if (h, w) != mat.shape[:2]:
            if resize_fn is None:
                raise ValueError(f'image {mat.shape[:2]} exceeds the short-side limit {c.rough_downsample_short_side_legnth}: '
                                 f"pass resize_fn (a callable, or 'device') or an image already resized to {(h, w)}")
            if isinstance(resize_fn, str):
                if mat.dtype != np.uint8:
                    raise ValueError(f"resize_fn='device' takes a uint8 image, got {mat.dtype}")
                src = torch.from_numpy(np.ascontiguousarray(mat)).to(c.device, non_blocking=True)
                page = self._device_rough_page(src, h, w)
                return mat, (h, w), page.cpu().numpy(), page[None].permute(0, 3, 1, 2).float()
            resized = np.asarray(resize_fn(mat, h, w))
            assert resized.shape[:2] == (h, w)
            padded = pad_mat_to_make_divisible(resized, c.backbone_downsampling_factor)
        else:
            padded = pad_mat_to_make_divisible(mat, c.backbone_downsampling_factor)
        return mat, (h, w), padded, self._to_device([padded])

    def _rough_maps(self, x, vh, vw, H: int, W: int):
        """The rough model call + the device post-processing (:129-172): mask (B,H,W) uint8 and height (B,H,W) fp32."""
        c = self.config
        mask_feat, height_feat = self.model.forward_rough(x)
        B = mask_feat.shape[0]
        assert tuple(mask_feat.shape) == (B, 1, H, W) and height_feat.shape == mask_feat.shape
        out_mask = torch.empty((B, H, W), dtype=torch.uint8, device=x.device)
        out_height = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
        check(lib.vkas_rough_postprocess(_ptr(mask_feat.contiguous()), _ptr(height_feat.contiguous()), B, H, W, _ptr(vh),
                                         _ptr(vw), float(c.rough_char_mask_positive_thr), float(c.rough_valid_char_height_min),
                                         _ptr(out_mask), _ptr(out_height), ops._stream()), 'rough_postprocess')
        return out_mask, out_height

    def rough_infer(self, image, resize_fn=None) -> AdaptiveScalingInferencingRoughInferResult:
        """:92-188.  ``resize_fn(mat, height, width)`` performs the area-interpolation shrink of the 720 rule (cv2 in the
        reference); ``resize_fn='device'`` shrinks on the device with this package's own area rule; without either an image
        that needs shrinking is rejected."""
        c = self.config
        _, (h, w), padded, x = self._rough_input(image, resize_fn)
        fdf = 4 // c.rough_head_upsampling_factor
        H, W = padded.shape[0] // fdf, padded.shape[1] // fdf
        vh, vw = self._valid([(h, w)], fdf, x.device)
        thr, hmin = float(c.rough_char_mask_positive_thr), float(c.rough_valid_char_height_min)

        def rough_pass(x, vh, vw):  # the model call + the device post-processing: one HIP graph per padded shape
            return self._rough_maps(x, vh, vw, H, W)

        with torch.no_grad():
            out_mask, out_height = self.graphs.run(('rough', thr, hmin), rough_pass, [x, vh, vw], param_stamp(self.model))
        return AdaptiveScalingInferencingRoughInferResult(
            resized_shape=(math.ceil(h / fdf), math.ceil(w / fdf)), padded_image=padded,
            rough_char_mask=out_mask[0].cpu().numpy(), rough_char_height_score_map=out_height[0].cpu().numpy())

    def _rough_regions_graph(self, x, sizes: Sequence[Tuple[int, int]], with_moments: bool = False):
        """The rough-plus-regions graph on a device input (B, 3, Hp, Wp) whose images are valid on ``sizes``: the device
        tensors ``ops.text_regions`` returns (static outputs of the graph: consume them before the next graph of this cache
        runs).  ``with_moments``: the graph - one of its own key - also takes the regions' moments (csrc/orient.hip)."""
        c = self.config
        fdf = 4 // c.rough_head_upsampling_factor
        H, W = x.shape[2] // fdf, x.shape[3] // fdf
        vh, vw = self._valid(sizes, fdf, x.device)
        thr, hmin = float(c.rough_char_mask_positive_thr), float(c.rough_valid_char_height_min)
        cap = int(c.rough_text_regions_max)

        def rough_regions_pass(x, vh, vw):  # model call, post-processing and region table: one HIP graph per padded shape
            return ops.text_regions(*self._rough_maps(x, vh, vw, H, W), cap)

        def rough_regions_moments_pass(x, vh, vw):
            out = rough_regions_pass(x, vh, vw)
            return out + (ops.region_moments(out[1], cap),)

        with torch.no_grad():
            if with_moments:
                return self.graphs.run(('rough_text_regions_moments', thr, hmin, cap), rough_regions_moments_pass, [x, vh, vw],
                                       param_stamp(self.model))
            return self.graphs.run(('rough_text_regions', thr, hmin, cap), rough_regions_pass, [x, vh, vw],
                                   param_stamp(self.model))

    def _rough_regions_result(self, image_shape, h: int, w: int, padded, num: int, labels, boxes, areas, valid, medians):
        """The region table of one image from its rows as read back, with the reference's scale rule on the host."""
        c = self.config
        fdf = 4 // c.rough_head_upsampling_factor
        resized_shape = (math.ceil(h / fdf), math.ceil(w / fdf))
        scales, resized_shapes, keep = region_scales(
            boxes, medians, image_shape, resized_shape, c.precise_flattened_text_region_resized_char_height_median,
            c.precise_flattened_text_region_resized_ratio_min)
        return AdaptiveScalingInferencingRoughTextRegions(
            resized_shape=resized_shape, padded_image=padded, num_regions=num, labels=labels, boxes=boxes, areas=areas,
            valid=valid, char_height_medians=medians, scales=scales, resized_shapes=resized_shapes, keep=keep)

    def _rough_text_regions(self, x, image_shape, h: int, w: int, padded, return_labels: bool, with_moments: bool = False):
        """The rough-plus-regions graph on a device input and the table rows read back: the result, and the device label
        map (a static output of the graph: consume it before the next graph of this cache runs).  ``with_moments``: the
        regions' moments come third."""
        out = self._rough_regions_graph(x, [(h, w)], with_moments)
        count, labels, boxes, areas, valid, medians = out[:6]
        num = int(count[0].item())
        n = min(num, int(self.config.rough_text_regions_max))
        moments = out[6][0, :n].cpu().numpy() if with_moments else None
        boxes, areas, valid, medians = (t[0, :n].cpu().numpy() for t in (boxes, areas, valid, medians))
        return self._rough_regions_result(image_shape, h, w, padded, num, labels[0].cpu().numpy() if return_labels else None,
                                          boxes, areas, valid, medians), labels[0], moments

    def rough_infer_text_regions(self, image, resize_fn=None,
                                 return_labels: bool = True) -> AdaptiveScalingInferencingRoughTextRegions:
        """The rough pass followed by the text regions of its mask, the exact median of the valid character heights of
        each (csrc/regions.hip, in the same HIP graph) and the reference's scale rule on the host (:190-279 restated on
        pixels, inferencing/regions.py): the region count, the table rows and - if ``return_labels`` - the int32 label map
        cross PCIe, the mask and the height map do not.  ``image`` and ``resize_fn`` as in ``rough_infer``, whose maps this
        labels: the result equals ``text_regions_host`` + ``region_scales`` on them."""
        mat, (h, w), padded, x = self._rough_input(image, resize_fn)
        return self._rough_text_regions(x, mat.shape[:2], h, w, padded, return_labels)[0]

    # ---- a batch of images: one arena, rough graphs per padded shape --------------------------------------------------
    def _image_arena(self, images: Sequence):
        """The uint8 images of a batch in ONE device byte arena: copied once into one pinned host buffer, every image start
        16-byte aligned, and uploaded in one transfer.  -> the mats, the arena, and its (S, 4) int64 source table (byte
        offset, Hs, Ws, 0) on the host and on the device."""
        mats = [_as_mat(im) for im in images]
        arena, table, d_table = ops.image_arena(mats, self.config.device)
        return mats, arena, table, d_table

    def _multi_tables(self, rows: np.ndarray, source_shapes, page_shape, num_pages: int):
        """A multi-row table checked on the host (so the launches need no copy back) and uploaded with its page_start."""
        rows = check_multi_rows(rows, source_shapes, page_shape, num_pages)
        start = np.searchsorted(rows[:, 1], np.arange(num_pages + 1)).astype(np.int32)
        device = self.config.device
        return torch.from_numpy(rows).to(device, non_blocking=True), torch.from_numpy(start).to(device, non_blocking=True)

    def _rough_text_regions_batch(self, mats, arena, sources, d_sources, return_padded: bool, return_labels: bool,
                                  keep_labels: bool):
        """The rough pass of a batch: images grouped by padded rough shape, a group split into chunks of at most
        ``config.rough_batch_max``; per chunk ONE launch shrinks (the 720 rule) and pads its images out of the arena into a
        (B, Hp, Wp, 3) batch - one multi row per image, source i -> page k - and one ``graphs.run`` of the rough-plus-regions
        pass follows.  -> the region tables in input order and, ``keep_labels``, the int32 device arena of the rough label
        maps with its (S, 8) int64 source table (word offset, Hl, Wl, valid_h, valid_w, Hs, Ws, 0): the label tensor of a graph
        is a static output that the next replay overwrites, so each chunk's labels are copied there, device to device."""
        c = self.config
        f, fdf, cap = c.backbone_downsampling_factor, 4 // c.rough_head_upsampling_factor, int(c.rough_text_regions_max)
        step = int(c.rough_batch_max)
        if step < 1:
            raise ValueError(f'rough_batch_max must be at least 1, got {c.rough_batch_max}')
        shapes = [(int(m.shape[0]), int(m.shape[1])) for m in mats]
        sizes = [rough_resized_shape(H, W, c.rough_downsample_short_side_legnth) for H, W in shapes]
        groups = {}
        for i, (h, w) in enumerate(sizes):
            groups.setdefault((-(-h // f) * f, -(-w // f) * f), []).append(i)
        chunks = [(shape, idxs[k:k + step]) for shape, idxs in groups.items() for k in range(0, len(idxs), step)]
        label_sources = np.zeros((len(mats), 8), np.int64)
        words = 0
        for (Hp, Wp), idxs in chunks:  # the maps of a chunk lie side by side: one copy per chunk
            for i in idxs:
                label_sources[i] = (words, Hp // fdf, Wp // fdf, math.ceil(sizes[i][0] / fdf), math.ceil(sizes[i][1] / fdf),
                                    shapes[i][0], shapes[i][1], 0)
                words += (Hp // fdf) * (Wp // fdf)
        label_arena = torch.empty((words,), dtype=torch.int32, device=arena.device) if keep_labels else None
        results = [None] * len(mats)
        for (Hp, Wp), idxs in chunks:
            B = len(idxs)
            rows = np.array([[i, k, 0, 0, shapes[i][0], shapes[i][1], 0, 0, sizes[i][0], sizes[i][1], 1, 1]
                             for k, i in enumerate(idxs)], np.int32)
            d_rows, d_start = self._multi_tables(rows, shapes, (Hp, Wp), B)
            pages = ops.resample_pack_u8_multi(arena, d_sources, d_rows, B, (Hp, Wp), page_start=d_start, validate=False)
            count, labels, boxes, areas, valid, medians = self._rough_regions_graph(
                pages.permute(0, 3, 1, 2).float(), [sizes[i] for i in idxs])
            if keep_labels:
                first = int(label_sources[idxs[0], 0])
                label_arena[first:first + labels.numel()].view(labels.shape).copy_(labels)
            nums = count.cpu().numpy()
            most = min(int(nums.max()), cap)
            boxes, areas, valid, medians = (t[:, :most].cpu().numpy() for t in (boxes, areas, valid, medians))
            labels = labels.cpu().numpy() if return_labels else None
            pages = pages.cpu().numpy() if return_padded else None
            for k, i in enumerate(idxs):
                n = min(int(nums[k]), cap)
                results[i] = self._rough_regions_result(
                    shapes[i], sizes[i][0], sizes[i][1], pages[k] if return_padded else None, int(nums[k]),
                    labels[k] if return_labels else None,
                    *(np.ascontiguousarray(t[k, :n]) for t in (boxes, areas, valid, medians)))
        return results, label_arena, label_sources

    def rough_infer_text_regions_batch(self, images: Sequence,
                                       return_labels: bool = True) -> Sequence[AdaptiveScalingInferencingRoughTextRegions]:
        """``rough_infer_text_regions(image, resize_fn='device')`` for a list of uint8 (H, W, 3) images, in input order: the
        images go up in one transfer, the 720 rule's shrink and the padding run on the device (one launch per chunk), and
        images of one padded rough shape share a model call, at most ``config.rough_batch_max`` at a time.  A chunk of one
        image runs the very graph ``infer`` and ``rough_infer_text_regions`` run: its result equals theirs bit for bit."""
        if not len(images):
            return []
        mats, arena, sources, d_sources = self._image_arena(images)
        return self._rough_text_regions_batch(mats, arena, sources, d_sources, True, return_labels, False)[0]

    # ---- precise pass --------------------------------------------------------------------------------------------
    def _precise_groups(self, images: Sequence):
        """Pads each page to x32 and groups the pages by padded size: [(padded shape, indices)], the mats, the padded mats."""
        c = self.config
        mats = [_as_mat(im) for im in images]
        padded = [pad_mat_to_make_divisible(m, c.backbone_downsampling_factor) for m in mats]
        groups = {}
        for i, p in enumerate(padded):
            groups.setdefault(p.shape[:2], []).append(i)
        return list(groups.items()), mats, padded

    def _precise_maps(self, x, vh, vw, H: int, W: int):
        """The precise model call + the device post-processing (:318-396): prob (B,H,W), offset (B,H,W,2), softmaxed angle
        (B,H,W,4) and distance (B,H,W,4), fp32."""
        prob, offset, angle, dist = self.model.forward_precise(x)
        B = prob.shape[0]
        assert tuple(prob.shape) == (B, 1, H, W)
        o_prob = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
        o_off = torch.empty((B, H, W, 2), dtype=torch.float32, device=x.device)
        o_ang = torch.empty((B, H, W, 4), dtype=torch.float32, device=x.device)
        o_dist = torch.empty((B, H, W, 4), dtype=torch.float32, device=x.device)
        check(lib.vkas_precise_postprocess(_ptr(prob.contiguous()), _ptr(offset.contiguous()), _ptr(angle.contiguous()),
                                           _ptr(dist.contiguous()), B, H, W, _ptr(vh), _ptr(vw), _ptr(o_prob),
                                           _ptr(o_off), _ptr(o_ang), _ptr(o_dist), ops._stream()), 'precise_postprocess')
        return o_prob, o_off, o_ang, o_dist

    def precise_infer_batch(self, images: Sequence) -> Sequence[AdaptiveScalingInferencingPresiceInferResult]:
        """:295-396 for a batch of stacked-region pages: each is padded to x32, pages of one padded size share a model
        call (the reference feeds one page at a time)."""
        fdf = 4 // self.config.precise_head_upsampling_factor
        groups, mats, padded = self._precise_groups(images)
        results = [None] * len(mats)
        for shape, idxs in groups:
            x = self._to_device([padded[i] for i in idxs])
            H, W = shape[0] // fdf, shape[1] // fdf
            vh, vw = self._valid([mats[i].shape[:2] for i in idxs], fdf, x.device)

            def precise_pass(x, vh, vw):
                return self._precise_maps(x, vh, vw, H, W)

            with torch.no_grad():
                o_prob, o_off, o_ang, o_dist = self.graphs.run('precise', precise_pass, [x, vh, vw], param_stamp(self.model))
            o_prob, o_off, o_ang, o_dist = (t.cpu().numpy() for t in (o_prob, o_off, o_ang, o_dist))
            for k, i in enumerate(idxs):
                results[i] = AdaptiveScalingInferencingPresiceInferResult(
                    padded_image=padded[i], precise_char_mask=None, precise_char_prob_score_map=o_prob[k],
                    precise_np_char_up_left_corner_offset=o_off[k], precise_np_char_corner_angle_distribution=o_ang[k],
                    precise_np_char_corner_distance=o_dist[k])
        return results

    def precise_infer(self, image) -> AdaptiveScalingInferencingPresiceInferResult:
        return self.precise_infer_batch([image])[0]

    # ---- characters from the precise maps ----------------------------------------------------------------------
    def precise_infer_char_polygons_batch(self, images: Sequence) -> Sequence[AdaptiveScalingInferencingPreciseCharPolygons]:
        """The precise pass followed by peak finding and one quadrilateral per peak (:399-465,481-491) on the device, in
        the same HIP graph (csrc/charpoly.hip): only the peak count and the peak rows cross PCIe, not the maps.  Pages are
        grouped by padded size as in ``precise_infer_batch``.  A map point (y, x) sits at (y * Hp / H, x * Wp / W) of the
        Hp x Wp padded image (vkit's ``Point.to_conducted_resized_point``, restated as proportional scaling)."""
        groups, mats, padded = self._precise_groups(images)
        results = [None] * len(mats)
        for shape, idxs in groups:
            x = self._to_device([padded[i] for i in idxs])
            points, probs, quads = self._char_polygons(x, [mats[i].shape[:2] for i in idxs])
            bounds = np.searchsorted(points[:, 0], np.arange(len(idxs) + 1))  # rows are sorted by page
            for k, i in enumerate(idxs):
                lo, hi = bounds[k], bounds[k + 1]
                results[i] = AdaptiveScalingInferencingPreciseCharPolygons(
                    padded_image=padded[i], points=np.ascontiguousarray(points[lo:hi, 1:]), probs=probs[lo:hi],
                    polygons=quads[lo:hi])
        return results

    def _char_polygons(self, x: torch.Tensor, sizes: Sequence[Tuple[int, int]], on_device: bool = False):
        """The precise-plus-char-polygons graph on a device input (B, 3, Hp, Wp) whose pages are valid on ``sizes``: the
        (n, 3) int32 (page, y, x) points, (n,) probs and (n, 4, 2) quadrilaterals, as numpy arrays - or, ``on_device``, as
        device tensors (views of the graph's static outputs)."""
        c = self.config
        fdf = 4 // c.precise_head_upsampling_factor
        thr, size = float(c.precise_build_polygons_positive_char_prob_thr), c.precise_build_polygons_maximum_filter_size
        shape = (int(x.shape[2]), int(x.shape[3]))
        H, W = shape[0] // fdf, shape[1] // fdf
        scale_y, scale_x = shape[0] / H, shape[1] / W
        vh, vw = self._valid(sizes, fdf, x.device)

        def char_polygons_pass(x, vh, vw):
            o_prob, o_off, o_ang, o_dist = self._precise_maps(x, vh, vw, H, W)
            return ops.char_polygons(o_prob, o_off, o_ang, o_dist, thr, size, scale_y, scale_x)

        with torch.no_grad():
            count, points, probs, quads = self.graphs.run(('precise_char_polygons', thr, size), char_polygons_pass,
                                                          [x, vh, vw], param_stamp(self.model))
        n = int(count.item())
        if on_device:
            return points[:n], probs[:n], quads[:n]
        return tuple(t[:n].cpu().numpy() for t in (points, probs, quads))

    def precise_infer_char_polygons(self, image) -> AdaptiveScalingInferencingPreciseCharPolygons:
        return self.precise_infer_char_polygons_batch([image])[0]

    def _line_strips(self, results, images_or_arena):
        """The line-strip step of ``infer`` / ``infer_batch`` (after ``group_results``): the results with ``line_strip_ids``
        and the one ``QuadStrips`` of all their lines - with ``config.precise_line_strip_curved`` also ``line_spines``, and
        the one ``SpineStrips``."""
        c = self.config
        step = spine_strips_for_results if c.precise_line_strip_curved else strips_for_results
        return step(results, images_or_arena, c.precise_line_strip_height, c.precise_line_strip_width_max,
                    c.precise_line_strip_width_step, c.precise_line_strip_margin, c.device)

    def _check_line_flags(self):
        c = self.config
        if c.precise_line_strips and not c.precise_char_lines:
            raise ValueError('precise_line_strips cuts the text lines: set precise_char_lines too')
        if c.precise_line_strip_curved and not c.precise_line_strips:
            raise ValueError('precise_line_strip_curved is a way to cut the line strips: set precise_line_strips too')

    def _finish(self, results, strip_source):
        """The tail of ``infer`` / ``infer_batch``, each step one call for all images and only with its switch: suppress
        duplicates, group into lines, cut the lines' strips out of ``strip_source`` (what ``_line_strips`` takes) ->
        ``(results, strips)``, ``strips`` None without ``config.precise_line_strips``."""
        c = self.config
        if c.precise_char_nms_iou_thr:
            results = suppress_results(results, c.precise_char_nms_iou_thr, c.device)
        if c.precise_char_lines:
            results = group_results(results, c.precise_char_line_gap, c.precise_char_line_cross,
                                    c.precise_char_line_height_ratio, c.device)
        strips = None
        if c.precise_line_strips:
            results, strips = self._line_strips(results, strip_source)
        return results, strips

    # ---- image in, characters out --------------------------------------------------------------------------------
    def infer(self, image, return_page: bool = False, return_labels: bool = False) -> AdaptiveScalingInferencingResult:
        """Both passes and the step between them (:92-525 on pixels): the uint8 image is uploaded once; the 720 rule's shrink
        (if any) and the padding run on the device; the rough-plus-regions graph gives the region table, whose rows come
        back; scales, crops and the shelf packing are host arithmetic on that table (inferencing/regions.py, packing.py);
        the placements go up, the regions are resampled into the stacked page and the label page is written on the device
        (csrc/respack.hip); the precise-plus-char-polygons graph runs on that device page; the characters are grouped by
        the label under their point and their quadrilaterals mapped back into the image.  The image, the maps and the page
        do not cross back over PCIe unless ``return_page`` / ``return_labels`` ask for them.  Equal, bit for bit, to
        ``rough_infer_text_regions`` -> ``resample_host`` -> ``precise_infer_char_polygons`` ->
        ``precise_group_char_polygons`` -> ``remap_polygons``.

        With ``config.precise_text_region_orient`` the rough graph (one of its own key) also takes the regions' moments;
        their directions go up and their extents come back - one extra small round trip -; the rule of
        inferencing/orient.py decides which regions are oriented; ``stack_regions`` runs on the mixed shapes;
        ``ops.warp_pack_u8`` / ``ops.warp_region_labels`` write the oriented regions into the page and the label page after
        the axis-aligned ones; their characters go back through ``remap_polygons_affine``."""
        c = self.config
        self._check_line_flags()
        mat = _as_mat(image)
        if mat.dtype != np.uint8:
            raise ValueError(f'infer takes a uint8 image, got {mat.dtype}')
        image_shape = (int(mat.shape[0]), int(mat.shape[1]))
        h, w = rough_resized_shape(image_shape[0], image_shape[1], c.rough_downsample_short_side_legnth)
        src = torch.from_numpy(np.ascontiguousarray(mat)).to(c.device, non_blocking=True)
        rough_page = self._device_rough_page(src, h, w)
        orient = bool(c.precise_text_region_orient)
        regions, d_labels, moments = self._rough_text_regions(
            rough_page[None].permute(0, 3, 1, 2).float(), image_shape, h, w, rough_page.cpu().numpy() if return_page else None,
            return_labels, with_moments=orient)
        n = len(regions.boxes)
        crops = region_crops(regions.boxes, image_shape, regions.resized_shape)
        source_fits = (crops[:, 2:] <= SIDE_MAX).all(axis=1)
        oriented = np.zeros((n,), bool)
        if orient and n:
            # the one extra round trip of the oriented path: directions up, extents back (both a few bytes per region)
            _, dirs = region_directions(moments)
            extents = ops.region_extents(d_labels[None], dirs[None])[0].cpu().numpy()
            oriented, rects, shapes, keep = orient_regions(
                dirs, extents, regions.scales, regions.resized_shapes, regions.keep, image_shape, regions.resized_shape,
                c.precise_text_region_flattener_typical_long_side_ratio_min,
                c.precise_flattened_text_region_resized_char_height_median, c.precise_flattened_text_region_resized_ratio_min)
            regions = attrs.evolve(regions, resized_shapes=shapes, keep=keep)
            source_fits = source_fits | oriented  # an oriented region has no crop: its warp row was checked by the rule
        page_shape, boxes, packed, too_large = stack_regions(
            regions.resized_shapes, c.precise_stack_flattened_text_regions_page_pad, c.precise_stack_flattened_text_regions_pad,
            c.precise_page_width_max, c.precise_page_height_step, keep=regions.keep & source_fits)
        too_large |= regions.keep & ~source_fits
        straight = packed & ~oriented
        ids = (np.flatnonzero(straight) + 1).astype(np.int32)
        placements = np.ascontiguousarray(np.concatenate([crops[straight], boxes[straight]], axis=1).astype(np.int32))
        warp_ids = (np.flatnonzero(packed & oriented) + 1).astype(np.int32)
        warps = np.zeros((len(warp_ids), 12), np.int64)
        for k, rid in enumerate(warp_ids.tolist()):
            warps[k] = warp_row(dirs[rid - 1], rects[rid - 1], image_shape, regions.resized_shape, boxes[rid - 1],
                                regions.scales[rid - 1])
        points, probs, polygons = _no_characters(n)
        page = region_labels = None
        if len(ids) or len(warp_ids):
            fdf = 4 // c.precise_head_upsampling_factor
            d_page = ops.resample_pack_u8(src, placements, page_shape)
            d_region_labels = ops.pack_region_labels(d_labels, regions.resized_shape, image_shape, placements, ids,
                                                     (page_shape[0] // fdf, page_shape[1] // fdf), fdf)
            if len(warp_ids):
                check_warps(warps, page_shape, placements)
                d_warps = torch.from_numpy(warps).to(c.device, non_blocking=True)
                ops.warp_pack_u8(src, d_warps, d_page, validate=False)
                ops.warp_region_labels(d_labels, regions.resized_shape, image_shape, d_warps, warp_ids, d_region_labels, fdf,
                                       validate=False)
            d_points, d_probs, d_quads = self._char_polygons(d_page[None].permute(0, 3, 1, 2).float(), [page_shape],
                                                             on_device=True)
            at = d_region_labels[d_points[:, 1].long(), d_points[:, 2].long()].cpu().numpy()
            all_points, all_probs, all_quads = (t.cpu().numpy() for t in (d_points[:, 1:], d_probs, d_quads))
            for table, table_ids, remap in ((placements, ids, remap_polygons), (warps, warp_ids, remap_polygons_affine)):
                for k, rid in enumerate(table_ids.tolist()):
                    sel = at == rid
                    points[rid - 1] = np.ascontiguousarray(all_points[sel])
                    probs[rid - 1] = all_probs[sel]
                    polygons[rid - 1] = remap(all_quads[sel], table[k])
            if return_page:
                page = d_page.cpu().numpy()
            if return_labels:
                region_labels = d_region_labels.cpu().numpy()
        result = AdaptiveScalingInferencingResult(
            image_shape=image_shape, regions=regions, packed=packed, too_large=too_large, placements=placements,
            placement_regions=ids, page_shape=page_shape, page=page, region_labels=region_labels, points=points, probs=probs,
            polygons=polygons)
        if orient:
            result.oriented, result.warps, result.warp_regions = oriented, warps, warp_ids
        # the image is on the device already: a one-entry source table
        (result,), strips = self._finish([result], (src.reshape(-1), np.array([[0, *image_shape, 0]], np.int64)))
        result.line_strips = strips
        return result

    def infer_batch(self, images: Sequence, return_pages: bool = False,
                    return_labels: bool = False) -> AdaptiveScalingInferencingBatchResult:
        """``infer`` for a list of uint8 (H, W, 3) images whose text regions share the pages of the precise pass: N small
        images cost a few full precise passes instead of N padded ones.  The images are copied into one pinned buffer and go
        up in one transfer (``_image_arena``); the rough pass runs per chunk of one padded rough shape
        (``_rough_text_regions_batch``); scales and crops are host arithmetic per image; ONE ``stack_regions_pages`` over the
        kept regions of all images, in input order, fills pages of at most ``precise_page_width_max`` x
        ``precise_page_height_max`` - a region's global id is 1 + its position in that concatenation -; the multi rows go
        up, one launch cuts every region out of the arena into the full-height pages and one writes their label pages
        (csrc/respack.hip), and once more for the last page if its height differs; the precise-plus-char-polygons graph
        runs on the page batch, and again on the last page; one label per character is gathered on the device; the
        characters are split by global id, then image, and mapped back through ``remap_polygons``.

        Host round trips per batch: three uploads (arena, image table, label table); per rough chunk two small uploads
        (rows, page_start) and five read-backs (counts, then four table slices); per page group - at most two - two small
        uploads and five read-backs (count, labels under the points, points, probabilities, quadrilaterals).  Images,
        maps and pages do not cross back over PCIe unless ``return_pages`` / ``return_labels`` ask for them.

        ``infer_batch([image]).results[0]`` equals ``infer(image)`` bit for bit whenever the regions fit one page of
        ``precise_page_height_max`` rows.  Oriented regions (``config.precise_text_region_orient``) on shared pages are not
        built yet: with the flag set this raises ValueError."""
        c = self.config
        if c.precise_text_region_orient:
            raise ValueError('infer_batch does not take oriented text regions yet: unset precise_text_region_orient or use infer')
        self._check_line_flags()
        if not len(images):
            return AdaptiveScalingInferencingBatchResult(results=[], page_shapes=[], rows=np.zeros((0, 12), np.int32),
                                                         pages=[] if return_pages else None,
                                                         region_labels=[] if return_labels else None)
        mats, arena, sources, d_sources = self._image_arena(images)
        all_regions, label_arena, label_sources = self._rough_text_regions_batch(mats, arena, sources, d_sources, return_pages,
                                                                                 return_labels, True)
        shapes = [(int(m.shape[0]), int(m.shape[1])) for m in mats]
        counts = np.array([len(r.boxes) for r in all_regions], np.int64)
        first = np.concatenate([[0], np.cumsum(counts)])
        image_of = np.repeat(np.arange(len(mats)), counts)
        crops = np.concatenate([region_crops(r.boxes, shape, r.resized_shape) for r, shape in zip(all_regions, shapes)])
        source_fits = (crops[:, 2:] <= SIDE_MAX).all(axis=1)
        keep = np.concatenate([r.keep for r in all_regions])
        page_shapes, boxes, page_of, packed, too_large = stack_regions_pages(
            np.concatenate([r.resized_shapes for r in all_regions]), c.precise_stack_flattened_text_regions_page_pad,
            c.precise_stack_flattened_text_regions_pad, c.precise_page_width_max, c.precise_page_height_step,
            c.precise_page_height_max, keep=keep & source_fits)
        too_large |= keep & ~source_fits
        g = np.flatnonzero(packed)  # global region id - 1, ascending: image after image, region after region
        by_region = np.concatenate([image_of[g, None], page_of[g, None], crops[g], boxes[g], (g - first[image_of[g]])[:, None] + 1,
                                    g[:, None] + 1], axis=1).astype(np.int32)
        rows = np.ascontiguousarray(by_region[np.argsort(by_region[:, 1], kind='stable')])
        Q = len(page_shapes)
        fdf = 4 // c.precise_head_upsampling_factor
        d_label_sources = torch.from_numpy(label_sources).to(c.device, non_blocking=True)
        # the pages of full height are one batch of the precise graph; the last page joins them only if it is as high
        if Q == 1 or page_shapes[-1] == page_shapes[0]:
            groups = [(0, Q)]
        else:
            groups = [(0, Q - 1), (Q - 1, Q)]
        at, all_points, all_probs, all_quads, pages, region_labels = [], [], [], [], [], []
        for q0, q1 in groups if len(rows) else []:
            shape = page_shapes[q0]
            sub = rows[(rows[:, 1] >= q0) & (rows[:, 1] < q1)] - np.array([0, q0] + [0] * 10, np.int32)
            d_rows, d_start = self._multi_tables(sub, shapes, shape, q1 - q0)
            d_pages = ops.resample_pack_u8_multi(arena, d_sources, d_rows, q1 - q0, shape, page_start=d_start, validate=False)
            d_region_labels = ops.pack_region_labels_multi(label_arena, d_label_sources, d_rows, q1 - q0,
                                                           (shape[0] // fdf, shape[1] // fdf), fdf, page_start=d_start,
                                                           validate=False)
            d_points, d_probs, d_quads = self._char_polygons(d_pages.permute(0, 3, 1, 2).float(), [shape] * (q1 - q0),
                                                             on_device=True)
            # static outputs of the graph: on the host before the graph of the last page runs
            at.append(d_region_labels[d_points[:, 0].long(), d_points[:, 1].long(), d_points[:, 2].long()].cpu().numpy())
            for store, t in ((all_points, d_points[:, 1:]), (all_probs, d_probs), (all_quads, d_quads)):
                store.append(t.cpu().numpy())
            if return_pages:
                pages.extend(d_pages.cpu().numpy())
            if return_labels:
                region_labels.extend(d_region_labels.cpu().numpy())
        if len(rows):
            at, all_points, all_probs, all_quads = (np.concatenate(t) for t in (at, all_points, all_probs, all_quads))
            order = np.argsort(at, kind='stable')  # the characters of a region stay in np.nonzero order
            lo = np.searchsorted(at[order], by_region[:, 11], side='left')
            hi = np.searchsorted(at[order], by_region[:, 11], side='right')
        results = []
        for i, regions in enumerate(all_regions):
            n = int(counts[i])
            mine = np.flatnonzero(by_region[:, 0] == i)
            points, probs, polygons = _no_characters(n)
            for k in mine.tolist():
                sel, r = order[lo[k]:hi[k]], int(by_region[k, 10]) - 1
                points[r] = np.ascontiguousarray(all_points[sel])
                probs[r] = all_probs[sel]
                polygons[r] = remap_polygons(all_quads[sel], by_region[k, 2:10])
            placement_pages = np.ascontiguousarray(by_region[mine, 1])
            page = int(placement_pages[0]) if len(mine) else 0
            results.append(AdaptiveScalingInferencingResult(
                image_shape=shapes[i], regions=regions, packed=packed[first[i]:first[i + 1]],
                too_large=too_large[first[i]:first[i + 1]], placements=np.ascontiguousarray(by_region[mine, 2:10]),
                placement_regions=np.ascontiguousarray(by_region[mine, 10]), page_shape=page_shapes[page],
                page=pages[page] if return_pages and len(mine) else None,
                region_labels=region_labels[page] if return_labels and len(mine) else None, points=points, probs=probs,
                polygons=polygons, placement_pages=placement_pages))
        results, strips = self._finish(results, (arena, sources, d_sources))  # the strips: one launch, out of the arena
        return AdaptiveScalingInferencingBatchResult(
            results=results, page_shapes=page_shapes, rows=rows, pages=pages if return_pages else None,
            region_labels=region_labels if return_labels else None, line_strips=strips)

    @staticmethod
    def precise_group_char_polygons(result: AdaptiveScalingInferencingPreciseCharPolygons,
                                    region_labels: np.ndarray) -> Sequence[AdaptiveScalingInferencingPreciseCharPolygons]:
        """The module-level ``precise_group_char_polygons`` (host only)."""
        return precise_group_char_polygons(result, region_labels)


def precise_group_char_polygons(result: AdaptiveScalingInferencingPreciseCharPolygons,
                                region_labels: np.ndarray) -> Sequence[AdaptiveScalingInferencingPreciseCharPolygons]:
    """The device-free half of ``precise_build_grouped_polygons`` (:467-525): ``region_labels`` is an (H, W) integer map at
    the precise map's resolution, 0 = no region; returns one result per label 1..max with the points that fall on it, in
    the order of ``result`` - np.nonzero's, which is the reference's per-region order, since it restricts the peaks to a
    region after the maximum filter.  Building the label map from the flattened text regions and their boxes stays with
    the caller."""
    labels = np.asarray(region_labels)
    if labels.ndim != 2 or not np.issubdtype(labels.dtype, np.integer):
        raise ValueError(f'region_labels must be a 2-D integer map, got {labels.dtype} {labels.shape}')
    Hp, Wp = result.padded_image.shape[:2]
    H, W = labels.shape
    if H < 1 or W < 1 or Hp % H or Wp % W or Hp // H != Wp // W:
        raise ValueError(f'region_labels {labels.shape} is not at the precise map resolution of a {(Hp, Wp)} page')
    at = labels[result.points[:, 0], result.points[:, 1]]
    groups = []
    for label in range(1, int(labels.max()) + 1):
        sel = at == label
        groups.append(AdaptiveScalingInferencingPreciseCharPolygons(
            padded_image=result.padded_image, points=result.points[sel], probs=result.probs[sel],
            polygons=result.polygons[sel]))
    return groups
