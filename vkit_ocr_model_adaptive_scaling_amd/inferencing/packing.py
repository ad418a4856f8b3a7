"""Cropping, rescaling and stacking the text regions into the page of the precise pass (inferencing/adaptive_scaling.py:
190-293), host side, numpy only: the resampling rule, the geometry around it and the oracles of the device path
(``ops.resample_pack_u8`` / ``ops.pack_region_labels``, csrc/respack.hip).

The reference flattens every text region (vkit, cv2), resizes it with cv2's interpolation and stacks the results with
``stack_flattened_text_regions``.  vkit and cv2 are absent here, so the step is restated on pixels:

* a region's axis-aligned box stands in for the flattened region (no rotation, no perspective);
* the interpolation rule is this project's own, defined in integers so that host and device agree bit for bit;
* stacking is a deterministic shelf packing.

A **placement** is a row ``(sy, sx, sh, sw, dy, dx, dh, dw)`` of int32: the source rectangle ``[sy, sy + sh) x [sx, sx + sw)``
of the image is resampled to the destination rectangle ``[dy, dy + dh) x [dx, dx + dw)`` of the page.  Destinations are
pairwise disjoint; every side is at least 1 and at most ``SIDE_MAX``.

The resampling rule, per axis, from ``S`` source samples to ``D`` destination samples (``axis_weights``):

* ``D < S`` (shrink): area coverage.  Destination sample ``i`` covers the source interval ``[i*S/D, (i+1)*S/D)``; in units of
  ``1/D`` source pixel the weight of source sample ``j`` is the integer overlap of ``[i*S, (i+1)*S)`` with ``[j*D, (j+1)*D)``.
  The weights of a destination sample sum to ``S`` (the axis denominator);
* ``D >= S`` (same size or enlarge): two-tap bilinear with half-pixel centres.  The source coordinate of destination sample
  ``i`` is ``((2i+1)*S - D) / (2D)``; its floor ``j`` is the first tap, the remainder ``f`` of the numerator over ``2D`` gives
  the weights ``(2D - f, f)`` of taps ``j`` and ``j + 1``, each clamped to ``[0, S - 1]``.  The axis denominator is ``2D``;
  ``D == S`` is the identity;
* a pixel channel is ``(sum_y sum_x wy * wx * p + den // 2) // den`` with ``den`` the product of the two axis denominators:
  one rounding, half up, no floating point.  With sides up to ``SIDE_MAX`` = 8192 a row's inner sum stays below 2^32 and the
  whole sum below 2^37.

The centre mapping of the label page (``pack_region_labels_host``): label pixel ``(v, u)`` of a page at ``1/fdf`` resolution
has its centre at page position ``(v*fdf + fdf/2, u*fdf + fdf/2)``; it belongs to the placement whose destination rectangle
(as a half-open interval of the continuous page axis) contains that centre.  With ``t2 = 2*v*fdf + fdf - 2*dy`` (the centre's
offset in the destination, in half pixels) the source position is ``sy + t2*sh / (2*dh)`` image pixels, and the rough map
row under it is ``min(valid_h - 1, ((2*dh*sy + t2*sh) * valid_h) // (2*dh*Hs))`` - image row ``Y`` lies on map row
``floor(Y * valid_h / Hs)``, the inverse of ``region_crops`` -; columns likewise.  All of it in integers."""
from typing import Optional, Sequence, Tuple

import numpy as np

SIDE_MAX = 8192  # of a placement's source and destination rectangles: keeps a row's inner sum within 32 bits


def axis_weights(S: int, D: int) -> Tuple[np.ndarray, int]:
    """The (D, S) int64 weight matrix of one axis and its denominator: the rule of the module docstring, sample by sample."""
    S, D = int(S), int(D)
    if not (1 <= S <= SIDE_MAX and 1 <= D <= SIDE_MAX):
        raise ValueError(f'resampling sides must be in [1, {SIDE_MAX}], got {S} -> {D}')
    w = np.zeros((D, S), np.int64)
    if D < S:
        for i in range(D):
            a, b = i * S, (i + 1) * S
            for j in range(a // D, (b - 1) // D + 1):
                w[i, j] = min((j + 1) * D, b) - max(j * D, a)
        return w, S
    for i in range(D):
        num = (2 * i + 1) * S - D
        j = num // (2 * D)  # floor, also below zero
        f = num - j * 2 * D
        w[i, min(max(j, 0), S - 1)] += 2 * D - f
        w[i, min(max(j + 1, 0), S - 1)] += f
    return w, 2 * D


def check_placements(placements, src_shape: Tuple[int, int], page_shape: Tuple[int, int]) -> np.ndarray:
    """Validates an (n, 8) table against an (Hs, Ws) source and an (Hp, Wp) page - integer rows, sides in [1, SIDE_MAX],
    rectangles inside, destinations pairwise disjoint - and returns it as contiguous int32.  Raises ValueError."""
    p = np.asarray(placements)
    if p.ndim != 2 or p.shape[1] != 8 or not np.issubdtype(p.dtype, np.integer):
        raise ValueError(f'placements must be an (n, 8) integer table, got {p.dtype} {p.shape}')
    (Hs, Ws), (Hp, Wp) = (int(v) for v in src_shape), (int(v) for v in page_shape)
    q = p.astype(np.int64)
    sy, sx, sh, sw, dy, dx, dh, dw = q.T
    sides = q[:, [2, 3, 6, 7]]
    if ((sides < 1) | (sides > SIDE_MAX)).any():
        raise ValueError(f'placements: every side must be in [1, {SIDE_MAX}]')
    if ((sy < 0) | (sx < 0) | (sy + sh > Hs) | (sx + sw > Ws)).any():
        raise ValueError(f'placements: a source rectangle leaves the {(Hs, Ws)} source')
    if ((dy < 0) | (dx < 0) | (dy + dh > Hp) | (dx + dw > Wp)).any():
        raise ValueError(f'placements: a destination rectangle leaves the {(Hp, Wp)} page')
    # disjointness by a sweep over the rows sorted by top edge: only rectangles whose row spans overlap are compared
    order = np.argsort(dy, kind='stable')
    live = []
    for r in order:
        live = [k for k in live if dy[k] + dh[k] > dy[r]]
        for k in live:
            if dx[k] < dx[r] + dw[r] and dx[r] < dx[k] + dw[k]:
                raise ValueError(f'placements: destinations {int(min(k, r))} and {int(max(k, r))} overlap')
        live.append(r)
    return np.ascontiguousarray(p.astype(np.int32))


def resample_host(src: np.ndarray, placements, page_shape: Tuple[int, int]) -> np.ndarray:
    """The definition: an (Hs, Ws, 3) uint8 image and an (n, 8) placement table -> the (Hp, Wp, 3) uint8 page, resampled
    pixels inside the placements and zero elsewhere.  Plain and slow."""
    src = np.asarray(src)
    if src.ndim != 3 or src.shape[2] != 3 or src.dtype != np.uint8:
        raise ValueError(f'src must be an (H, W, 3) uint8 image, got {src.dtype} {src.shape}')
    Hp, Wp = (int(v) for v in page_shape)
    table = check_placements(placements, src.shape[:2], (Hp, Wp))
    page = np.zeros((Hp, Wp, 3), np.uint8)
    for sy, sx, sh, sw, dy, dx, dh, dw in table.tolist():
        wy, den_y = axis_weights(sh, dh)
        wx, den_x = axis_weights(sw, dw)
        den = den_y * den_x
        # the sums are integers below 2^37: float64 products and sums of them are exact, and its matrix product is the fast one
        crop = np.ascontiguousarray(src[sy:sy + sh, sx:sx + sw].transpose(2, 0, 1)).astype(np.float64)
        fy, fx = wy.astype(np.float64), wx.T.astype(np.float64)
        for c in range(3):
            total = (fy @ crop[c] @ fx).astype(np.int64)
            page[dy:dy + dh, dx:dx + dw, c] = (total + den // 2) // den
    return page


def label_cells(d0: int, dlen: int, fdf: int) -> Tuple[int, int]:
    """The label pixels ``[lo, hi)`` of one axis whose centres ``v*fdf + fdf/2`` lie in the page interval ``[d0, d0 + dlen)``."""
    lo = max(0, -((fdf - 2 * d0) // (2 * fdf)))                # ceil((2*d0 - fdf) / (2*fdf))
    hi = max(0, -((fdf - 2 * (d0 + dlen)) // (2 * fdf)))
    return lo, hi


def pack_region_labels_host(labels: np.ndarray, valid_shape: Tuple[int, int], image_shape: Tuple[int, int], placements,
                            region_ids, out_shape: Tuple[int, int], fdf: int) -> np.ndarray:
    """The label page of the precise pass, (Hq, Wq) int32 at ``1/fdf`` of the page: a label pixel whose centre falls in
    placement k gets ``region_ids[k]`` - unless the rough label map (``labels``, of which ``valid_shape`` rows and columns
    cover the ``image_shape`` image the placements' sources refer to) holds the label of ANOTHER region at the pixel's
    source position (the centre mapping of the module docstring); then, and outside every placement, it gets 0.  This stands
    in for the reference's ``flattened_mask``: a character of a neighbouring region inside an overlapping box is not
    reported twice."""
    labels = np.asarray(labels)
    if labels.ndim != 2 or labels.dtype != np.int32:
        raise ValueError(f'labels must be an (H, W) int32 map, got {labels.dtype} {labels.shape}')
    vh, vw = (int(v) for v in valid_shape)
    Hs, Ws = (int(v) for v in image_shape)
    Hq, Wq = (int(v) for v in out_shape)
    fdf = int(fdf)
    if not (1 <= vh <= labels.shape[0] and 1 <= vw <= labels.shape[1]):
        raise ValueError(f'valid_shape {(vh, vw)} does not fit the {labels.shape} label map')
    if fdf < 1 or Hq < 1 or Wq < 1:
        raise ValueError(f'bad label page {(Hq, Wq)} at factor {fdf}')
    table = np.asarray(placements).reshape(-1, 8)
    ids = np.asarray(region_ids).reshape(-1)
    if len(ids) != len(table):
        raise ValueError(f'{len(ids)} region ids for {len(table)} placements')
    out = np.zeros((Hq, Wq), np.int32)
    for (sy, sx, sh, sw, dy, dx, dh, dw), rid in zip(table.tolist(), ids.tolist()):
        v0, v1 = label_cells(dy, dh, fdf)
        u0, u1 = label_cells(dx, dw, fdf)
        for v in range(v0, min(v1, Hq)):
            ty = 2 * v * fdf + fdf - 2 * dy
            my = min(vh - 1, ((2 * dh * sy + ty * sh) * vh) // (2 * dh * Hs))
            for u in range(u0, min(u1, Wq)):
                tx = 2 * u * fdf + fdf - 2 * dx
                mx = min(vw - 1, ((2 * dw * sx + tx * sw) * vw) // (2 * dw * Ws))
                other = int(labels[my, mx])
                out[v, u] = 0 if other not in (0, rid) else rid
    return out


def region_crops(boxes, image_shape: Tuple[int, int], resized_shape: Tuple[int, int]) -> np.ndarray:
    """Inclusive map-pixel boxes (N, 4) (y0, x0, y1, x1) -> (N, 4) int64 image rectangles (sy, sx, sh, sw): map row m covers
    the image rows ``[m*H/rs_h, (m+1)*H/rs_h)``, so ``Y0 = floor(y0*H/rs_h)`` and ``Y1 = min(H, ceil((y1+1)*H/rs_h))``;
    columns likewise.  Integer arithmetic."""
    boxes = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    H, W = (int(v) for v in image_shape)
    rs_h, rs_w = (int(v) for v in resized_shape)
    out = np.zeros((len(boxes), 4), np.int64)
    for r, (y0, x0, y1, x1) in enumerate(boxes.tolist()):
        Y0, X0 = y0 * H // rs_h, x0 * W // rs_w
        Y1, X1 = min(H, -((-(y1 + 1) * H) // rs_h)), min(W, -((-(x1 + 1) * W) // rs_w))
        out[r] = (Y0, X0, Y1 - Y0, X1 - X0)
    return out


def stack_regions(shapes, page_pad: int, pad: int, width_max: int, height_step: int,
                  keep: Optional[Sequence[bool]] = None, side_max: int = SIDE_MAX):
    """Deterministic shelf packing of (N, 2) rectangles (height, width) into one page.  The regions with ``keep`` (default:
    all) are taken in stable order of decreasing height and fill rows left to right, ``pad`` pixels between neighbours (and
    between rows), ``page_pad`` around the page.  Page width: the smallest multiple of 32 that holds the widest row plus its
    ``page_pad``s, at most ``width_max`` (a multiple of 32); page height: rounded up to a multiple of ``height_step`` (a
    multiple of 32, so the page needs no further padding and the graph cache sees few shapes).

    Returns ``(page_shape, boxes, packed, too_large)``: (Hp, Wp); (N, 4) int64 (dy, dx, dh, dw), zero for a region that is not
    packed; (N,) bool; (N,) bool - a kept region wider than ``width_max - 2*page_pad`` or with a side above ``side_max``: it is
    reported here and not packed, never clamped.  A kept region with an empty side is neither packed nor too large."""
    shapes = np.asarray(shapes, dtype=np.int64).reshape(-1, 2)
    n = len(shapes)
    keep = np.ones((n,), bool) if keep is None else np.asarray(keep, dtype=bool).reshape(-1)
    if len(keep) != n:
        raise ValueError(f'{len(keep)} keep flags for {n} shapes')
    page_pad, pad, width_max, height_step = int(page_pad), int(pad), int(width_max), int(height_step)
    if page_pad < 0 or pad < 0:
        raise ValueError(f'pads must not be negative, got page_pad {page_pad}, pad {pad}')
    if width_max < 32 or width_max % 32 or height_step < 32 or height_step % 32:
        raise ValueError(f'width_max and height_step must be positive multiples of 32, got {width_max} and {height_step}')
    if width_max - 2 * page_pad < 1:
        raise ValueError(f'width_max {width_max} leaves no room between two page_pads of {page_pad}')
    h, w = shapes[:, 0], shapes[:, 1]
    too_large = keep & ((w > width_max - 2 * page_pad) | (h > side_max) | (w > side_max))
    fits = keep & ~too_large & (h >= 1) & (w >= 1)
    order = [r for r in np.argsort(-h, kind='stable').tolist() if fits[r]]
    boxes = np.zeros((n, 4), np.int64)
    x, y, row_h, right = page_pad, page_pad, 0, page_pad
    for r in order:
        if x > page_pad and x + w[r] > width_max - page_pad:  # the row is full: the next one starts below its tallest
            y += row_h + pad
            x, row_h = page_pad, 0
        boxes[r] = (y, x, h[r], w[r])
        right = max(right, x + int(w[r]))
        row_h = max(row_h, int(h[r]))
        x += int(w[r]) + pad
    width = min(width_max, -(-(right + page_pad) // 32) * 32)
    height = -(-(y + row_h + page_pad) // height_step) * height_step
    return (int(height), int(width)), boxes, fits, too_large


def remap_polygons(polygons, placement) -> np.ndarray:
    """(..., 2) (y, x) page positions -> float64 positions in the image the placement's source refers to:
    ``Y = sy + (y - dy) * sh / dh``, ``X = sx + (x - dx) * sw / dw``."""
    sy, sx, sh, sw, dy, dx, dh, dw = (int(v) for v in np.asarray(placement).reshape(8))
    p = np.asarray(polygons, dtype=np.float64)
    out = np.empty(p.shape, np.float64)
    out[..., 0] = sy + (p[..., 0] - dy) * sh / dh
    out[..., 1] = sx + (p[..., 1] - dx) * sw / dw
    return out
