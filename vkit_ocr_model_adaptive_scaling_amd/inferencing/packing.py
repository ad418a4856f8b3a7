"""Cropping, rescaling and stacking the text regions into the page of the precise pass (inferencing/adaptive_scaling.py:
190-293), host side, numpy only: the resampling rule, the geometry around it and the oracles of the device path
(``ops.resample_pack_u8`` / ``ops.pack_region_labels``, csrc/respack.hip).

The reference flattens every text region (vkit, cv2), resizes it with cv2's interpolation and stacks the results with
``stack_flattened_text_regions``.  vkit and cv2 are absent here, so the step is restated on pixels:

* a region's axis-aligned box stands in for the flattened region (no rotation, no perspective) - or, for a region that
  inferencing/orient.py finds elongated and slanted, its oriented rectangle: an affine **warp** (the last part of this
  module; ``ops.warp_pack_u8`` / ``ops.warp_region_labels``);
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


# ---- several sources, several pages (infer_batch; the multi kernels of csrc/respack.hip) ---------------------------------
# A **multi row** is ``(src, page, sy, sx, sh, sw, dy, dx, dh, dw, local_id, global_id)`` of int32: the placement in columns
# 2..9 reads source image ``src`` and writes page ``page``; ``local_id`` is the region's label in that image's rough label
# map, ``global_id`` the label it gets on the label page.  Rows are sorted by page; destinations are disjoint per page.
def check_multi_rows(rows, source_shapes, page_shape: Tuple[int, int], num_pages: int) -> np.ndarray:
    """Validates an (n, 12) multi-row table against the (S, 2) source shapes (Hs, Ws) and ``num_pages`` pages of
    ``page_shape`` - integer rows sorted by page, ``src`` and ``page`` in range, ids at least 1, sides in [1, SIDE_MAX],
    rectangles inside their source / page, destinations pairwise disjoint per page - and returns it as contiguous int32.
    Raises ValueError."""
    r = np.asarray(rows)
    if r.ndim != 2 or r.shape[1] != 12 or not np.issubdtype(r.dtype, np.integer):
        raise ValueError(f'multi rows must be an (n, 12) integer table, got {r.dtype} {r.shape}')
    shapes = np.asarray(source_shapes, dtype=np.int64).reshape(-1, 2)
    S, Q = len(shapes), int(num_pages)
    Hp, Wp = (int(v) for v in page_shape)
    q = r.astype(np.int64)
    src, page, sy, sx, sh, sw, dy, dx, dh, dw = q[:, :10].T
    if ((src < 0) | (src >= S)).any():
        raise ValueError(f'multi rows: a source index is outside [0, {S})')
    if ((page < 0) | (page >= Q)).any():
        raise ValueError(f'multi rows: a page index is outside [0, {Q})')
    if (np.diff(page) < 0).any():
        raise ValueError('multi rows: the rows must be sorted by page')
    if (q[:, 10:] < 1).any():
        raise ValueError('multi rows: region ids start at 1 (0 is "no region")')
    sides = q[:, [4, 5, 8, 9]]
    if ((sides < 1) | (sides > SIDE_MAX)).any():
        raise ValueError(f'multi rows: every side must be in [1, {SIDE_MAX}]')
    if ((sy < 0) | (sx < 0) | (sy + sh > shapes[src, 0]) | (sx + sw > shapes[src, 1])).any():
        raise ValueError('multi rows: a source rectangle leaves its source')
    if ((dy < 0) | (dx < 0) | (dy + dh > Hp) | (dx + dw > Wp)).any():
        raise ValueError(f'multi rows: a destination rectangle leaves the {(Hp, Wp)} page')
    order = np.lexsort((dy, page))  # the sweep of check_placements, page after page
    live = []
    for k in order:
        live = [j for j in live if page[j] == page[k] and dy[j] + dh[j] > dy[k]]
        for j in live:
            if dx[j] < dx[k] + dw[k] and dx[k] < dx[j] + dw[j]:
                raise ValueError(f'multi rows: destinations {int(min(j, k))} and {int(max(j, k))} overlap on page {int(page[k])}')
        live.append(k)
    return np.ascontiguousarray(r.astype(np.int32))


def resample_pack_multi_host(sources: Sequence[np.ndarray], rows, page_shape: Tuple[int, int], num_pages: int) -> np.ndarray:
    """The definition of the multi pack: (Hs, Ws, 3) uint8 images and an (n, 12) multi-row table -> the (Q, Hp, Wp, 3) uint8
    pages; ``resample_host`` per (source, page).  Plain and slow."""
    table = check_multi_rows(rows, [np.asarray(s).shape[:2] for s in sources], page_shape, num_pages)
    Hp, Wp = (int(v) for v in page_shape)
    pages = np.zeros((int(num_pages), Hp, Wp, 3), np.uint8)
    for s, src in enumerate(sources):
        for page in range(int(num_pages)):
            sel = (table[:, 0] == s) & (table[:, 1] == page)
            if sel.any():  # destinations are disjoint and a page is zero outside them: the pages of the sources add up
                pages[page] += resample_host(src, table[sel][:, 2:10], (Hp, Wp))
    return pages


def pack_region_labels_multi_host(label_maps: Sequence[np.ndarray], valid_shapes, image_shapes, rows,
                                  out_shape: Tuple[int, int], fdf: int, num_pages: int) -> np.ndarray:
    """The label pages of the multi pack, (Q, Hq, Wq) int32: ``pack_region_labels_host`` per (source, page) with the
    rows' ``local_id`` - the ids of that image's rough label map ``label_maps[src]`` -, then every cell it kept gets the
    row's ``global_id``: the regions of two images may share a local id, never a global one."""
    Hq, Wq = (int(v) for v in out_shape)
    fdf, Q = int(fdf), int(num_pages)
    table = check_multi_rows(rows, np.asarray(image_shapes).reshape(-1, 2), (Hq * fdf, Wq * fdf), Q)
    out = np.zeros((Q, Hq, Wq), np.int32)
    for s, labels in enumerate(label_maps):
        for page in range(Q):
            for row in table[(table[:, 0] == s) & (table[:, 1] == page)]:  # a row at a time: local ids may repeat
                kept = pack_region_labels_host(labels, valid_shapes[s], image_shapes[s], row[None, 2:10], row[10:11],
                                               (Hq, Wq), fdf)
                out[page][kept != 0] = row[11]
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


def stack_regions_pages(shapes, page_pad: int, pad: int, width_max: int, height_step: int, height_max: int,
                        keep: Optional[Sequence[bool]] = None, side_max: int = SIDE_MAX):
    """``stack_regions`` onto pages of bounded height (``infer_batch``: the regions of many images share pages).  Same
    order and shelf rule; a new row that would end below ``height_max - page_pad`` (a multiple of ``height_step``) opens the
    next page at ``y = page_pad``.  All pages share one width - the smallest multiple of 32 that holds the widest row of
    any page, at most ``width_max`` -; pages ``0 .. Q-2`` are ``height_max`` high, the last one has its own height, rounded
    up to ``height_step``.

    Returns ``(page_shapes, boxes, pages, packed, too_large)``: a list of Q >= 1 (Hp, Wp); (N, 4) int64 (dy, dx, dh, dw)
    inside the region's page; (N,) int32 page index, -1 for a region that is not packed; (N,) bool; (N,) bool - as
    ``stack_regions``, and also a kept region taller than ``height_max - 2*page_pad``: reported, never clamped.  Whenever
    everything fits one page of ``height_max`` the result is ``stack_regions``' on the same arguments, with ``pages == 0``."""
    shapes = np.asarray(shapes, dtype=np.int64).reshape(-1, 2)
    n = len(shapes)
    keep = np.ones((n,), bool) if keep is None else np.asarray(keep, dtype=bool).reshape(-1)
    if len(keep) != n:
        raise ValueError(f'{len(keep)} keep flags for {n} shapes')
    page_pad, pad, width_max, height_step, height_max = (int(v) for v in (page_pad, pad, width_max, height_step, height_max))
    if page_pad < 0 or pad < 0:
        raise ValueError(f'pads must not be negative, got page_pad {page_pad}, pad {pad}')
    if width_max < 32 or width_max % 32 or height_step < 32 or height_step % 32:
        raise ValueError(f'width_max and height_step must be positive multiples of 32, got {width_max} and {height_step}')
    if height_max < height_step or height_max % height_step:
        raise ValueError(f'height_max must be a positive multiple of height_step {height_step}, got {height_max}')
    if width_max - 2 * page_pad < 1 or height_max - 2 * page_pad < 1:
        raise ValueError(f'a {height_max} x {width_max} page leaves no room between two page_pads of {page_pad}')
    h, w = shapes[:, 0], shapes[:, 1]
    too_large = keep & ((w > width_max - 2 * page_pad) | (h > height_max - 2 * page_pad) | (h > side_max) | (w > side_max))
    fits = keep & ~too_large & (h >= 1) & (w >= 1)
    order = [r for r in np.argsort(-h, kind='stable').tolist() if fits[r]]
    boxes = np.zeros((n, 4), np.int64)
    pages = np.full((n,), -1, np.int32)
    x, y, row_h, right, q = page_pad, page_pad, 0, page_pad, 0
    for r in order:
        if x > page_pad and x + w[r] > width_max - page_pad:  # the row is full: the next one starts below its tallest
            y += row_h + pad
            x, row_h = page_pad, 0
            if y + h[r] > height_max - page_pad:  # heights decrease: the first region of a row is its tallest
                q, y = q + 1, page_pad
        boxes[r] = (y, x, h[r], w[r])
        pages[r] = q
        right = max(right, x + int(w[r]))
        row_h = max(row_h, int(h[r]))
        x += int(w[r]) + pad
    width = min(width_max, -(-(right + page_pad) // 32) * 32)
    height = -(-(y + row_h + page_pad) // height_step) * height_step
    return [(height_max, int(width))] * q + [(int(height), int(width))], boxes, pages, fits, too_large


def remap_polygons(polygons, placement) -> np.ndarray:
    """(..., 2) (y, x) page positions -> float64 positions in the image the placement's source refers to:
    ``Y = sy + (y - dy) * sh / dh``, ``X = sx + (x - dx) * sw / dw``."""
    sy, sx, sh, sw, dy, dx, dh, dw = (int(v) for v in np.asarray(placement).reshape(8))
    p = np.asarray(polygons, dtype=np.float64)
    out = np.empty(p.shape, np.float64)
    out[..., 0] = sy + (p[..., 0] - dy) * sh / dh
    out[..., 1] = sx + (p[..., 1] - dx) * sw / dw
    return out


# ---- affine warps: a slanted region cut out along its own axis (inferencing/orient.py builds the rows) ------------------
# A **warp** is a row ``(dy, dx, dh, dw, ay, ax, myy, myx, mxy, mxx, log2n, 0)`` of int64: destination pixel ``(i, j)`` of the
# page rectangle ``[dy, dy + dh) x [dx, dx + dw)`` reads the source at the sample coordinates ``Y = ay + i*myy + j*myx``,
# ``X = ax + i*mxy + j*mxx`` in Q16; an integer coordinate is a pixel centre.  With ``n = 2^log2n`` a pixel is the mean of
# ``n x n`` sub-samples at ``Y + ((2a+1-n)*myy + (2b+1-n)*myx) >> (1 + log2n)`` (floor; ``X`` likewise), each two-tap
# bilinear per axis: ``k = Y >> 16``, ``f = Y & 65535``, weights ``(65536 - f, f)`` on ``k`` and ``k + 1``, a tap outside the
# source reading 0.  A channel is ``(sum + den/2) >> (32 + 2*log2n)``: one rounding, 64-bit sums (below 2^46), shifts only.
# ``n`` is the smallest power of two >= 1/scale, at most 8: a region shrunk by more than 8 aliases.
WARP_M_MAX = 1 << 22   # |myy|, |myx|, |mxy|, |mxx|: a destination step of at most 64 source pixels
WARP_A_MAX = 1 << 40   # |ay|, |ax| stay below


def check_warps(warps, page_shape: Tuple[int, int], placements=None) -> np.ndarray:
    """Validates a (K, 12) warp table against an (Hp, Wp) page - integer rows, sides in [1, SIDE_MAX], coefficients within
    their bounds, destinations inside the page, pairwise disjoint and disjoint from the destinations of the (n, 8)
    ``placements`` (if given) - and returns it as contiguous int64.  Raises ValueError."""
    w = np.asarray(warps)
    if w.ndim != 2 or w.shape[1] != 12 or not np.issubdtype(w.dtype, np.integer):
        raise ValueError(f'warps must be a (K, 12) integer table, got {w.dtype} {w.shape}')
    w = np.ascontiguousarray(w.astype(np.int64))
    Hp, Wp = (int(v) for v in page_shape)
    dy, dx, dh, dw = w[:, 0], w[:, 1], w[:, 2], w[:, 3]
    if ((w[:, 2:4] < 1) | (w[:, 2:4] > SIDE_MAX)).any():
        raise ValueError(f'warps: every side must be in [1, {SIDE_MAX}]')
    if ((dy < 0) | (dx < 0) | (dy + dh > Hp) | (dx + dw > Wp)).any():
        raise ValueError(f'warps: a destination rectangle leaves the {(Hp, Wp)} page')
    if (np.abs(w[:, 6:10]) > WARP_M_MAX).any() or (np.abs(w[:, 4:6]) >= WARP_A_MAX).any():
        raise ValueError(f'warps: a coefficient exceeds 2^22 or an anchor reaches 2^40')
    if ((w[:, 10] < 0) | (w[:, 10] > 3)).any():
        raise ValueError('warps: log2n must be in [0, 3]')
    rects = w[:, :4]
    if placements is not None:
        rects = np.concatenate([rects, np.asarray(placements, dtype=np.int64).reshape(-1, 8)[:, 4:]])
    ry, rx, rh, rw = rects.T
    order = np.argsort(ry, kind='stable')  # the sweep of check_placements, over warps and placements together
    live = []
    for r in order:
        live = [k for k in live if ry[k] + rh[k] > ry[r]]
        for k in live:
            if min(k, r) < len(w) and rx[k] < rx[r] + rw[r] and rx[r] < rx[k] + rw[k]:
                raise ValueError(f'warps: destination {int(min(k, r))} overlaps another destination')
        live.append(r)
    return w


def _warp_samples(src: np.ndarray, Y: np.ndarray, X: np.ndarray) -> np.ndarray:
    """One bilinear sub-sample per element of the int64 Q16 coordinate arrays (Y, X): (..., 3) int64 channel sums, the
    weights of a sample summing to 2^32 (so a sum stays below 2^40)."""
    Hs, Ws = src.shape[:2]
    ky, fy, kx, fx = Y >> 16, Y & 65535, X >> 16, X & 65535
    total = np.zeros(Y.shape + (3,), np.int64)
    for k, wy in ((ky, 65536 - fy), (ky + 1, fy)):
        for m, wx in ((kx, 65536 - fx), (kx + 1, fx)):
            inside = (k >= 0) & (k < Hs) & (m >= 0) & (m < Ws)
            pixels = src[np.clip(k, 0, Hs - 1), np.clip(m, 0, Ws - 1)].astype(np.int64)
            total += np.where(inside, wy * wx, 0)[..., None] * pixels
    return total


def warp_host(src: np.ndarray, warps, page: np.ndarray) -> np.ndarray:
    """The definition: writes the pixels of the (K, 12) warps into a copy of the (Hp, Wp, 3) uint8 ``page`` and leaves
    every other byte of it alone.  Plain: one int64 array expression per sub-sample and tap."""
    src, page = np.asarray(src), np.array(page)
    if src.ndim != 3 or src.shape[2] != 3 or src.dtype != np.uint8:
        raise ValueError(f'src must be an (H, W, 3) uint8 image, got {src.dtype} {src.shape}')
    if page.ndim != 3 or page.shape[2] != 3 or page.dtype != np.uint8:
        raise ValueError(f'page must be an (H, W, 3) uint8 image, got {page.dtype} {page.shape}')
    for dy, dx, dh, dw, ay, ax, myy, myx, mxy, mxx, log2n, _ in check_warps(warps, page.shape[:2]).tolist():
        n, shift = 1 << log2n, 32 + 2 * log2n
        i, j = np.arange(dh, dtype=np.int64)[:, None], np.arange(dw, dtype=np.int64)[None, :]
        Y, X = ay + i * myy + j * myx, ax + i * mxy + j * mxx
        total = np.zeros((dh, dw, 3), np.int64)
        for a in range(n):
            for b in range(n):
                ka, kb = 2 * a + 1 - n, 2 * b + 1 - n
                total += _warp_samples(src, Y + ((ka * myy + kb * myx) >> (1 + log2n)), X + ((ka * mxy + kb * mxx) >> (1 + log2n)))
        page[dy:dy + dh, dx:dx + dw] = (total + (1 << (shift - 1))) >> shift
    return page


def warp_region_labels_host(labels: np.ndarray, valid_shape: Tuple[int, int], image_shape: Tuple[int, int], warps,
                            region_ids, out: np.ndarray, fdf: int) -> np.ndarray:
    """The label cells of the warps, written into a copy of the (Hq, Wq) int32 label page ``out`` (every other cell stays):
    a cell ``(v, u)`` whose centre lies in the destination of warp k (``label_cells``) has ``i2 = 2*v*fdf + fdf - 2*dy - 1``
    (twice its row in the destination, pixel centres being integers), ``j2`` likewise, ``Y = ay + ((i2*myy + j2*myx) >> 1)``
    and the source pixel ``Yp = (Y + 32768) >> 16``.  Outside the image the cell gets 0; else ``region_ids[k]`` unless the
    rough map holds another region's label at row ``min(vh - 1, ((2*Yp + 1) * vh) // (2*Hs))``, column likewise."""
    labels, out = np.asarray(labels), np.array(out)
    if labels.ndim != 2 or labels.dtype != np.int32 or out.ndim != 2 or out.dtype != np.int32:
        raise ValueError('labels and out must be (H, W) int32 maps')
    vh, vw = (int(v) for v in valid_shape)
    Hs, Ws = (int(v) for v in image_shape)
    Hq, Wq = out.shape
    fdf = int(fdf)
    table = check_warps(warps, (Hq * fdf, Wq * fdf))
    ids = np.asarray(region_ids).reshape(-1)
    if len(ids) != len(table):
        raise ValueError(f'{len(ids)} region ids for {len(table)} warps')
    for (dy, dx, dh, dw, ay, ax, myy, myx, mxy, mxx, _, _), rid in zip(table.tolist(), ids.tolist()):
        v0, v1 = label_cells(dy, dh, fdf)
        u0, u1 = label_cells(dx, dw, fdf)
        for v in range(v0, min(v1, Hq)):
            i2 = 2 * v * fdf + fdf - 2 * dy - 1
            for u in range(u0, min(u1, Wq)):
                j2 = 2 * u * fdf + fdf - 2 * dx - 1
                Yp = (ay + ((i2 * myy + j2 * myx) >> 1) + 32768) >> 16
                Xp = (ax + ((i2 * mxy + j2 * mxx) >> 1) + 32768) >> 16
                if not (0 <= Yp < Hs and 0 <= Xp < Ws):
                    out[v, u] = 0
                    continue
                other = int(labels[min(vh - 1, ((2 * Yp + 1) * vh) // (2 * Hs)), min(vw - 1, ((2 * Xp + 1) * vw) // (2 * Ws))])
                out[v, u] = 0 if other not in (0, rid) else rid
    return out


def remap_polygons_affine(polygons, warp) -> np.ndarray:
    """(..., 2) (y, x) page positions -> float64 positions in the image the warp's source refers to: ``(i, j) = (y - dy -
    1/2, x - dx - 1/2)`` (destination pixel centres are integers), ``Y = (ay + i*myy + j*myx) / 65536 + 1/2``, ``X``
    likewise - positions as ``remap_polygons`` gives them, pixel k covering ``[k, k + 1)``."""
    dy, dx, _, _, ay, ax, myy, myx, mxy, mxx, _, _ = (int(v) for v in np.asarray(warp).reshape(12))
    p = np.asarray(polygons, dtype=np.float64)
    i, j = p[..., 0] - dy - 0.5, p[..., 1] - dx - 0.5
    out = np.empty(p.shape, np.float64)
    out[..., 0] = (ay + i * myy + j * myx) / 65536 + 0.5
    out[..., 1] = (ax + i * mxy + j * mxx) / 65536 + 0.5
    return out
