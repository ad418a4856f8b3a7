"""Text regions of the rough maps and the scale of each (inferencing/adaptive_scaling.py:190-279), host side, numpy only.

The reference takes the external contours of the rough character mask (vkit ``Mask.to_disconnected_polygons``, cv2), the
median of the valid character heights inside each (``extract_score_map``) and rescales the flattened region so that this
median becomes 35 px.  vkit and cv2 are absent here, so the step is restated on pixels:

* a region is an 8-connected component of ``mask != 0``.  External contours fill holes and drop a component nested inside a
  hole of another; pixel components do neither - a hole's pixels belong to no region, a nested component is a region of
  its own;
* regions are numbered 1..N by their first pixel in row-major order (smallest ``y * W + x``); label 0 is background;
* ``median`` is the float32 median of the region's heights that are > 0: the middle element of the sorted values, or
  ``(a + b) * 0.5`` in float32 of the two middle ones - ``np.median``'s bits -, 0 when there is none;
* the region's axis-aligned box stands in for vkit's flattened region in the scale rule.

``text_regions_host`` is the oracle of the device path (``ops.text_regions``, csrc/regions.hip): plain and obviously
correct rather than fast.  ``region_scales`` is the rule of :235-277 on the table and is what
``AdaptiveScalingInferencing.rough_infer_text_regions`` applies to the rows it reads back."""
from typing import Tuple

import numpy as np


def text_regions_host(mask: np.ndarray, height: np.ndarray):
    """One (H, W) mask and one (H, W) float32 height map -> ``(labels, boxes, areas, valid, medians)``: (H, W) int32,
    (N, 4) int32 inclusive (y0, x0, y1, x1), (N,) int32, (N,) int32, (N,) float32."""
    mask = np.asarray(mask)
    height = np.asarray(height)
    if mask.ndim != 2 or height.shape != mask.shape:
        raise ValueError(f'expected one (H, W) mask and a height map of its shape, got {mask.shape} and {height.shape}')
    if height.dtype != np.float32:
        raise ValueError(f'height must be float32, got {height.dtype}')
    H, W = mask.shape
    fg = np.zeros((H + 2, W + 2), bool)  # a background frame: no bounds checks in the fill
    fg[1:-1, 1:-1] = mask != 0
    lab = np.zeros((H + 2, W + 2), np.int32)
    n = 0
    for y, x in zip(*np.nonzero(fg)):  # row-major: a pixel without a label yet is the first pixel of its region
        if lab[y, x]:
            continue
        n += 1
        lab[y, x] = n
        stack = [(y, x)]
        while stack:
            cy, cx = stack.pop()
            for ny in (cy - 1, cy, cy + 1):
                for nx in (cx - 1, cx, cx + 1):
                    if fg[ny, nx] and not lab[ny, nx]:
                        lab[ny, nx] = n
                        stack.append((ny, nx))
    labels = np.ascontiguousarray(lab[1:-1, 1:-1])
    boxes = np.zeros((n, 4), np.int32)
    areas = np.zeros((n,), np.int32)
    valid = np.zeros((n,), np.int32)
    medians = np.zeros((n,), np.float32)
    ys, xs = np.nonzero(labels)
    of = labels[ys, xs]
    order = np.argsort(of, kind='stable')
    ys, xs, of = ys[order], xs[order], of[order]
    bounds = np.searchsorted(of, np.arange(1, n + 2))
    hs = height[ys, xs]
    for r in range(n):
        lo, hi = bounds[r], bounds[r + 1]
        boxes[r] = (ys[lo:hi].min(), xs[lo:hi].min(), ys[lo:hi].max(), xs[lo:hi].max())
        areas[r] = hi - lo
        v = np.sort(hs[lo:hi][hs[lo:hi] > 0])
        valid[r] = len(v)
        if len(v) % 2:
            medians[r] = v[len(v) // 2]
        elif len(v):
            medians[r] = (v[len(v) // 2 - 1] + v[len(v) // 2]) * np.float32(0.5)
    return labels, boxes, areas, valid, medians


def region_scales(boxes: np.ndarray, medians: np.ndarray, image_shape: Tuple[int, int], resized_shape: Tuple[int, int],
                  resized_char_height_median: float = 35, resized_ratio_min: float = 0.25):
    """The scale, skip and resized-shape rule of :235-277 on the region table.  ``image_shape`` is the (height, width) of
    the page as given, ``resized_shape`` the rough result's (the valid part of the rough maps, in map pixels), ``boxes`` /
    ``medians`` in map pixels as ``text_regions_host`` returns them.  Returns ``(scales, resized_shapes, keep)``:

    * ``scales`` (N,) float64 = ``resized_char_height_median / char_height_median`` with ``char_height_median = median *
      image_height / (resized_shape[0] * 2)`` (the reference's literal 2); 0 where the median is not positive;
    * ``resized_shapes`` (N, 2) int64 = ``(round(h * scale), round(w * scale))`` (Python's round: half to even), h and w the
      box's extent in page pixels, i.e. its rows and columns times ``image_height / resized_shape[0]`` and ``image_width /
      resized_shape[1]`` - the box in place of the reference's flattened region;
    * ``keep`` (N,) bool: False where the median is not positive, and where both sides fall below
      ``round(resized_char_height_median * resized_ratio_min)``."""
    boxes = np.asarray(boxes).reshape(-1, 4)
    medians = np.asarray(medians, dtype=np.float64).reshape(-1)
    if len(boxes) != len(medians):
        raise ValueError(f'{len(boxes)} boxes for {len(medians)} medians')
    image_height, image_width = image_shape
    inverse_resized_ratio = image_height / (resized_shape[0] * 2)
    side_min = round(resized_char_height_median * resized_ratio_min)
    n = len(boxes)
    scales = np.zeros((n,), np.float64)
    resized = np.zeros((n, 2), np.int64)
    keep = np.zeros((n,), bool)
    for r in range(n):
        char_height_median = float(medians[r]) * inverse_resized_ratio
        if not char_height_median > 0.0:
            continue
        scale = resized_char_height_median / char_height_median
        y0, x0, y1, x1 = (int(v) for v in boxes[r])
        h = (y1 - y0 + 1) * image_height / resized_shape[0]
        w = (x1 - x0 + 1) * image_width / resized_shape[1]
        big = int(np.iinfo(np.int64).max)  # a denormal median: the sides saturate instead of overflowing the table
        rh, rw = min(round(h * scale), big), min(round(w * scale), big)
        scales[r] = scale
        resized[r] = (rh, rw)
        keep[r] = not (rh < side_min and rw < side_min)
    return scales, resized, keep
