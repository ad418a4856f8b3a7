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

Out of scope: the CPU geometry around it - polygons of the rough regions, text-region flattening /
stacking, building the region label map from them and remapping polygons through the flattening (vkit, cv2; third-party
code that is absent here).  Images are plain (H, W, 3) uint8 arrays instead of ``vkit.element.Image``; results carry
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
    def rough_infer(self, image, resize_fn=None) -> AdaptiveScalingInferencingRoughInferResult:
        """:92-188.  ``resize_fn(mat, height, width)`` performs the area-interpolation shrink of the 720 rule (cv2 in the
        reference); without it an image that needs shrinking is rejected - resampling pixels is host-side image I/O."""
        c = self.config
        mat = _as_mat(image)
        h, w = rough_resized_shape(mat.shape[0], mat.shape[1], c.rough_downsample_short_side_legnth)
        if (h, w) != mat.shape[:2]:
            if resize_fn is None:
                raise ValueError(f'image {mat.shape[:2]} exceeds the short-side limit {c.rough_downsample_short_side_legnth}: '
                                 f'pass resize_fn or an image already resized to {(h, w)}')
            mat = np.asarray(resize_fn(mat, h, w))
            assert mat.shape[:2] == (h, w)
        padded = pad_mat_to_make_divisible(mat, c.backbone_downsampling_factor)
        fdf = 4 // c.rough_head_upsampling_factor
        x = self._to_device([padded])
        H, W = padded.shape[0] // fdf, padded.shape[1] // fdf
        vh, vw = self._valid([(h, w)], fdf, x.device)
        thr, hmin = float(c.rough_char_mask_positive_thr), float(c.rough_valid_char_height_min)

        def rough_pass(x, vh, vw):  # the model call + the device post-processing: one HIP graph per padded shape
            mask_feat, height_feat = self.model.forward_rough(x)
            B = mask_feat.shape[0]
            assert tuple(mask_feat.shape) == (B, 1, H, W) and height_feat.shape == mask_feat.shape
            out_mask = torch.empty((B, H, W), dtype=torch.uint8, device=x.device)
            out_height = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
            check(lib.vkas_rough_postprocess(_ptr(mask_feat.contiguous()), _ptr(height_feat.contiguous()), B, H, W, _ptr(vh),
                                             _ptr(vw), thr, hmin, _ptr(out_mask), _ptr(out_height), ops._stream()),
                  'rough_postprocess')
            return out_mask, out_height

        with torch.no_grad():
            out_mask, out_height = self.graphs.run(('rough', thr, hmin), rough_pass, [x, vh, vw], param_stamp(self.model))
        return AdaptiveScalingInferencingRoughInferResult(
            resized_shape=(math.ceil(h / fdf), math.ceil(w / fdf)), padded_image=padded,
            rough_char_mask=out_mask[0].cpu().numpy(), rough_char_height_score_map=out_height[0].cpu().numpy())

    def rough_infer_text_regions(self, image, resize_fn=None,
                                 return_labels: bool = True) -> AdaptiveScalingInferencingRoughTextRegions:
        """The rough pass followed by the text regions of its mask, the exact median of the valid character heights of
        each (csrc/regions.hip, in the same HIP graph) and the reference's scale rule on the host (:190-279 restated on
        pixels, inferencing/regions.py): the region count, the table rows and - if ``return_labels`` - the int32 label map
        cross PCIe, the mask and the height map do not.  ``image`` and ``resize_fn`` as in ``rough_infer``, whose maps this
        labels: the result equals ``text_regions_host`` + ``region_scales`` on them."""
        c = self.config
        mat = _as_mat(image)
        image_shape = mat.shape[:2]
        h, w = rough_resized_shape(mat.shape[0], mat.shape[1], c.rough_downsample_short_side_legnth)
        if (h, w) != mat.shape[:2]:
            if resize_fn is None:
                raise ValueError(f'image {mat.shape[:2]} exceeds the short-side limit {c.rough_downsample_short_side_legnth}: '
                                 f'pass resize_fn or an image already resized to {(h, w)}')
            mat = np.asarray(resize_fn(mat, h, w))
            assert mat.shape[:2] == (h, w)
        padded = pad_mat_to_make_divisible(mat, c.backbone_downsampling_factor)
        fdf = 4 // c.rough_head_upsampling_factor
        x = self._to_device([padded])
        H, W = padded.shape[0] // fdf, padded.shape[1] // fdf
        vh, vw = self._valid([(h, w)], fdf, x.device)
        thr, hmin = float(c.rough_char_mask_positive_thr), float(c.rough_valid_char_height_min)
        cap = int(c.rough_text_regions_max)

        def rough_regions_pass(x, vh, vw):  # model call, post-processing and region table: one HIP graph per padded shape
            mask_feat, height_feat = self.model.forward_rough(x)
            B = mask_feat.shape[0]
            assert tuple(mask_feat.shape) == (B, 1, H, W) and height_feat.shape == mask_feat.shape
            out_mask = torch.empty((B, H, W), dtype=torch.uint8, device=x.device)
            out_height = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
            check(lib.vkas_rough_postprocess(_ptr(mask_feat.contiguous()), _ptr(height_feat.contiguous()), B, H, W, _ptr(vh),
                                             _ptr(vw), thr, hmin, _ptr(out_mask), _ptr(out_height), ops._stream()),
                  'rough_postprocess')
            return ops.text_regions(out_mask, out_height, cap)

        with torch.no_grad():
            count, labels, boxes, areas, valid, medians = self.graphs.run(
                ('rough_text_regions', thr, hmin, cap), rough_regions_pass, [x, vh, vw], param_stamp(self.model))
        num = int(count[0].item())
        n = min(num, cap)
        boxes, areas, valid, medians = (t[0, :n].cpu().numpy() for t in (boxes, areas, valid, medians))
        resized_shape = (math.ceil(h / fdf), math.ceil(w / fdf))
        scales, resized_shapes, keep = region_scales(
            boxes, medians, image_shape, resized_shape, c.precise_flattened_text_region_resized_char_height_median,
            c.precise_flattened_text_region_resized_ratio_min)
        return AdaptiveScalingInferencingRoughTextRegions(
            resized_shape=resized_shape, padded_image=padded, num_regions=num,
            labels=labels[0].cpu().numpy() if return_labels else None, boxes=boxes, areas=areas, valid=valid,
            char_height_medians=medians, scales=scales, resized_shapes=resized_shapes, keep=keep)

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
        c = self.config
        fdf = 4 // c.precise_head_upsampling_factor
        thr, size = float(c.precise_build_polygons_positive_char_prob_thr), c.precise_build_polygons_maximum_filter_size
        groups, mats, padded = self._precise_groups(images)
        results = [None] * len(mats)
        for shape, idxs in groups:
            x = self._to_device([padded[i] for i in idxs])
            H, W = shape[0] // fdf, shape[1] // fdf
            scale_y, scale_x = shape[0] / H, shape[1] / W
            vh, vw = self._valid([mats[i].shape[:2] for i in idxs], fdf, x.device)

            def char_polygons_pass(x, vh, vw):
                o_prob, o_off, o_ang, o_dist = self._precise_maps(x, vh, vw, H, W)
                return ops.char_polygons(o_prob, o_off, o_ang, o_dist, thr, size, scale_y, scale_x)

            with torch.no_grad():
                count, points, probs, quads = self.graphs.run(('precise_char_polygons', thr, size), char_polygons_pass,
                                                              [x, vh, vw], param_stamp(self.model))
            n = int(count.item())
            points, probs, quads = (t[:n].cpu().numpy() for t in (points, probs, quads))
            bounds = np.searchsorted(points[:, 0], np.arange(len(idxs) + 1))  # rows are sorted by page
            for k, i in enumerate(idxs):
                lo, hi = bounds[k], bounds[k + 1]
                results[i] = AdaptiveScalingInferencingPreciseCharPolygons(
                    padded_image=padded[i], points=np.ascontiguousarray(points[lo:hi, 1:]), probs=probs[lo:hi],
                    polygons=quads[lo:hi])
        return results

    def precise_infer_char_polygons(self, image) -> AdaptiveScalingInferencingPreciseCharPolygons:
        return self.precise_infer_char_polygons_batch([image])[0]

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
