"""Oriented text regions (the reference's ``TextRegionFlattener`` / ``flattening_rotate_angle`` restated on pixels, deskewing
only), host side, numpy and float64: the one place where the geometry is computed.  Everything the device sees is an integer
table (csrc/orient.hip: ``ops.region_moments`` / ``ops.region_extents``; csrc/respack.hip: ``ops.warp_pack_u8`` /
``ops.warp_region_labels``), and this module also holds the host oracles of the two orientation kernels.

Coordinates.  A map pixel ``(y, x)`` is the unit square around its integer centre.  The image the map was made from covers
the ``resized_shape`` valid part of the map, so map position ``p`` (centre convention) lies at image sample coordinate
``(p + 1/2) * ratio - 1/2`` with ``ratio = image side / valid side`` per axis - the ratios of ``region_crops`` and
``region_scales`` -, an integer image coordinate being a pixel centre as well.

The rule, per region:

* moments ``n, Sy, Sx, Syy, Sxx, Sxy`` over its pixels give the central moments ``mu20 = Sxx - Sx^2/n`` (along x), ``mu02 = Syy
  - Sy^2/n``, ``mu11 = Sxy - Sx*Sy/n`` and the axis angle ``theta = atan2(2*mu11, mu20 - mu02) / 2`` (from the x axis towards y);
* ``|theta| > pi/4`` is folded by ``sign(theta) * pi/2``: a vertical line stays vertical, nothing turns by more than 45 degrees;
* the direction is quantised to Q14: ``c = round(cos(theta) * 2^14)``, ``s = round(sin(theta) * 2^14)``;
* extents ``min/max u, min/max v`` over its pixels, ``u = c*x + s*y``, ``v = -s*x + c*y`` (Q14 map pixels), widened by the
  half-pixel margin ``(|c| + |s|) / 2`` on each side - the reach of a pixel square's corner - give the oriented rectangle:
  every pixel square of the region lies inside it;
* its sides ``Lu``, ``Lv`` are carried to image pixels as the lengths of the side vectors under the per-axis ratios.

A region is **oriented** iff it is kept by ``region_scales``' rule, ``|s| >= S_MIN`` (1 degree), long side over short side is
at least ``long_side_ratio_min``, the oriented destination ``(round(Lv*scale), round(Lu*scale))`` has less area than the box's
``resized_shapes`` row, and its warp row stays inside the kernels' bounds (else it goes by its box).  ``scale`` is the median
rule's; ``keep`` is re-applied to the oriented shape."""
import math
from typing import Tuple

import numpy as np

Q = 14
ONE = 1 << Q
S_MIN = 286                 # round(sin(1 degree) * 2^14)
WARP_SIDE_MAX = 8192
WARP_M_MAX = 1 << 22        # a destination step of at most 64 source pixels
WARP_A_MAX = 1 << 40
EMPTY_EXTENT = (np.iinfo(np.int32).max, np.iinfo(np.int32).min, np.iinfo(np.int32).max, np.iinfo(np.int32).min)


def _label_batch(labels) -> np.ndarray:
    labels = np.asarray(labels)
    if labels.ndim == 2:
        labels = labels[None]
    if labels.ndim != 3 or labels.dtype != np.int32:
        raise ValueError(f'labels must be (B, H, W) int32, got {labels.dtype} {labels.shape}')
    return labels


def region_moments_host(labels, max_regions: int) -> np.ndarray:
    """The oracle of ``ops.region_moments``: (B, H, W) int32 labels -> (B, R, 6) int64 ``n, Sy, Sx, Syy, Sxx, Sxy`` of the
    regions 1..R; label 0 and labels above R are ignored.  Python integers, so exact whatever the size."""
    labels = _label_batch(labels)
    R = int(max_regions)
    out = np.zeros((labels.shape[0], R, 6), np.int64)
    for b, lab in enumerate(labels):
        ys, xs = np.nonzero((lab >= 1) & (lab <= R))
        for r, y, x in zip(lab[ys, xs].tolist(), ys.tolist(), xs.tolist()):
            out[b, r - 1] += (1, y, x, y * y, x * x, x * y)
    return out


def region_extents_host(labels, dirs) -> np.ndarray:
    """The oracle of ``ops.region_extents``: labels as above and (B, R, 2) int32 ``(c, s)`` -> (B, R, 4) int32 ``min u, max u,
    min v, max v`` with ``u = c*x + s*y``, ``v = -s*x + c*y``; ``EMPTY_EXTENT`` for a region without pixels."""
    labels = _label_batch(labels)
    dirs = np.asarray(dirs)
    if dirs.ndim == 2:
        dirs = dirs[None]
    if dirs.ndim != 3 or dirs.shape[0] != labels.shape[0] or dirs.shape[2] != 2:
        raise ValueError(f'dirs must be ({labels.shape[0]}, R, 2), got {dirs.shape}')
    R = dirs.shape[1]
    out = np.empty((labels.shape[0], R, 4), np.int64)
    out[:] = EMPTY_EXTENT
    for b, lab in enumerate(labels):
        ys, xs = np.nonzero((lab >= 1) & (lab <= R))
        for r, y, x in zip(lab[ys, xs].tolist(), ys.tolist(), xs.tolist()):
            c, s = int(dirs[b, r - 1, 0]), int(dirs[b, r - 1, 1])
            u, v = c * x + s * y, c * y - s * x
            o = out[b, r - 1]
            o[0], o[1], o[2], o[3] = min(o[0], u), max(o[1], u), min(o[2], v), max(o[3], v)
    return out.astype(np.int32)


def region_directions(moments) -> Tuple[np.ndarray, np.ndarray]:
    """(N, 6) moments -> the folded angles (N,) float64 and the Q14 directions (N, 2) int32 ``(c, s)``; a region without
    pixels (or without a preferred axis) gets angle 0, direction (2^14, 0)."""
    m = np.asarray(moments).reshape(-1, 6)
    theta = np.zeros((len(m),), np.float64)
    dirs = np.zeros((len(m), 2), np.int32)
    for r, (n, sy, sx, syy, sxx, sxy) in enumerate(m.tolist()):
        if n > 0:
            # exact integers (Python's) times n, so that the differences lose nothing before they become floats
            mu20, mu02, mu11 = n * sxx - sx * sx, n * syy - sy * sy, n * sxy - sx * sy
            t = 0.5 * math.atan2(2.0 * mu11, float(mu20 - mu02))
            if abs(t) > math.pi / 4:
                t -= math.copysign(math.pi / 2, t)
            theta[r] = t
        dirs[r] = (round(math.cos(theta[r]) * ONE), round(math.sin(theta[r]) * ONE))
    return theta, dirs


def oriented_rects(extents, dirs) -> np.ndarray:
    """(N, 4) extents and (N, 2) directions -> (N, 4) float64 ``(u0, v0, Lu, Lv)`` in map pixels: the oriented rectangle
    ``[u0, u0 + Lu] x [v0, v0 + Lv]`` in the region's own (u, v) frame, the extents widened by the half-pixel margin; zero
    for a region without pixels."""
    e = np.asarray(extents, dtype=np.int64).reshape(-1, 4)
    d = np.asarray(dirs, dtype=np.int64).reshape(-1, 2)
    out = np.zeros((len(e), 4), np.float64)
    for r in range(len(e)):
        if e[r, 0] > e[r, 1]:
            continue
        margin = abs(int(d[r, 0])) + abs(int(d[r, 1]))   # twice the half-pixel margin, Q14
        out[r] = ((2 * e[r, 0] - margin) / (2 * ONE), (2 * e[r, 2] - margin) / (2 * ONE),
                  (e[r, 1] - e[r, 0] + margin) / ONE, (e[r, 3] - e[r, 2] + margin) / ONE)
    return out


def _ratios(image_shape, resized_shape):
    return image_shape[0] / resized_shape[0], image_shape[1] / resized_shape[1]


def _frame(direction, image_shape, resized_shape):
    """The unit steps of u and v in image pixels, as (dY, dX) each, and their lengths."""
    ry, rx = _ratios(image_shape, resized_shape)
    cq, sq = int(direction[0]) / ONE, int(direction[1]) / ONE
    nn = cq * cq + sq * sq
    eu = (ry * sq / nn, rx * cq / nn)      # u = c*x + s*y inverted: x = (c*u - s*v) / (c^2 + s^2), y = (s*u + c*v) / (..)
    ev = (ry * cq / nn, -rx * sq / nn)
    return eu, ev, math.hypot(*eu), math.hypot(*ev)


def warp_log2n(scale: float) -> int:
    """Sub-samples per axis of the warp, as a power of two: the smallest one >= 1 / scale, at most 8 (a shrink beyond 8
    aliases)."""
    k = 0
    while k < 3 and (1 << k) * scale < 1.0:
        k += 1
    return k


def warp_row(direction, rect, image_shape: Tuple[int, int], resized_shape: Tuple[int, int], dest, scale: float) -> np.ndarray:
    """The 12 int64 of one warp (see inferencing/packing.py): destination ``dest = (dy, dx, dh, dw)`` of the page shows the
    oriented rectangle ``rect`` of a region with ``direction``; destination pixel (i, j) has its centre at ``((i + 1/2) / dh,
    (j + 1/2) / dw)`` of the rectangle.  The anchor is placed so that the rectangle's centre is exact and the rounding of the
    coefficients (2^-17 per step) is split between the two ends."""
    u0, v0, lu, lv = (float(v) for v in rect)
    dy, dx, dh, dw = (int(v) for v in dest)
    ry, rx = _ratios(image_shape, resized_shape)
    eu, ev, _, _ = _frame(direction, image_shape, resized_shape)
    myy, mxy = (round(65536 * ev[k] * lv / dh) for k in (0, 1))
    myx, mxx = (round(65536 * eu[k] * lu / dw) for k in (0, 1))
    uc, vc = u0 + lu / 2, v0 + lv / 2
    yc = uc * eu[0] + vc * ev[0] + ry / 2 - 0.5   # image sample coordinate of the centre: (map + 1/2) * ratio - 1/2
    xc = uc * eu[1] + vc * ev[1] + rx / 2 - 0.5
    # the centre of the destination is (i, j) = ((dh - 1) / 2, (dw - 1) / 2)
    ay = round(65536 * yc - ((dh - 1) * myy + (dw - 1) * myx) / 2)
    ax = round(65536 * xc - ((dh - 1) * mxy + (dw - 1) * mxx) / 2)
    return np.array([dy, dx, dh, dw, ay, ax, myy, myx, mxy, mxx, warp_log2n(scale), 0], np.int64)


def warp_row_in_bounds(row) -> bool:
    dy, dx, dh, dw, ay, ax, myy, myx, mxy, mxx, log2n, _ = (int(v) for v in row)
    return (1 <= dh <= WARP_SIDE_MAX and 1 <= dw <= WARP_SIDE_MAX and abs(ay) < WARP_A_MAX and abs(ax) < WARP_A_MAX
            and all(abs(m) <= WARP_M_MAX for m in (myy, myx, mxy, mxx)) and 0 <= log2n <= 3)


def orient_regions(dirs, extents, scales, resized_shapes, keep, image_shape: Tuple[int, int], resized_shape: Tuple[int, int],
                   long_side_ratio_min: float = 3.0, resized_char_height_median: float = 35,
                   resized_ratio_min: float = 0.25):
    """The rule of the module docstring on the tables of one page.  ``scales``, ``resized_shapes`` and ``keep`` are
    ``region_scales``' results (the box path).  Returns ``(oriented, rects, shapes, keep)``: (N,) bool; (N, 4) float64
    ``oriented_rects``; (N, 2) int64 destination shapes - the oriented one where ``oriented``, else the box's -; and the keep
    flags with the side rule re-applied to the oriented shapes."""
    dirs = np.asarray(dirs).reshape(-1, 2)
    n = len(dirs)
    scales = np.asarray(scales, dtype=np.float64).reshape(-1)
    shapes = np.array(resized_shapes, dtype=np.int64).reshape(-1, 2)
    keep = np.array(keep, dtype=bool).reshape(-1)
    if not (len(scales) == len(shapes) == len(keep) == n):
        raise ValueError('orient_regions: tables of different lengths')
    rects = oriented_rects(extents, dirs)
    oriented = np.zeros((n,), bool)
    side_min = round(resized_char_height_median * resized_ratio_min)
    for r in range(n):
        lu, lv = rects[r, 2], rects[r, 3]
        if not keep[r] or abs(int(dirs[r, 1])) < S_MIN or lu <= 0 or lv <= 0:
            continue
        _, _, nu, nv = _frame(dirs[r], image_shape, resized_shape)
        su, sv = lu * nu, lv * nv                       # the sides in image pixels
        if max(su, sv) < long_side_ratio_min * min(su, sv):
            continue
        dh, dw = round(sv * scales[r]), round(su * scales[r])
        if not dh * dw < int(shapes[r, 0]) * int(shapes[r, 1]):
            continue
        if dh < 1 or dw < 1 or not warp_row_in_bounds(warp_row(dirs[r], rects[r], image_shape, resized_shape,
                                                               (0, 0, dh, dw), scales[r])):
            continue
        oriented[r] = True
        shapes[r] = (dh, dw)
        keep[r] = not (dh < side_min and dw < side_min)
    return oriented, rects, shapes, keep


def warp_parallelogram(row) -> np.ndarray:
    """The corners (4, 2) float64 (Y, X), image sample coordinates, of the source parallelogram of a warp row: the images
    of the destination's corners (-1/2, -1/2), (-1/2, dw - 1/2), (dh - 1/2, dw - 1/2), (dh - 1/2, -1/2)."""
    _, _, dh, dw, ay, ax, myy, myx, mxy, mxx, _, _ = (int(v) for v in row)
    out = []
    for i, j in ((-0.5, -0.5), (-0.5, dw - 0.5), (dh - 0.5, dw - 0.5), (dh - 0.5, -0.5)):
        out.append(((ay + i * myy + j * myx) / 65536, (ax + i * mxy + j * mxx) / 65536))
    return np.array(out, np.float64)
