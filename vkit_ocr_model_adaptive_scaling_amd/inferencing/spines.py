"""Curved text lines cut into strips along their spines: the rule from the character quads of one line to a centre line
with down vectors (float64), the integer rule from those knots to one affine warp per strip column, the table layout and the
host oracle of the device route (``ops.spine_strips_u8``, csrc/spines.hip).  Host only: numpy and Python.  Slots, buckets
and ``bucket_views`` are those of strips.py.

**The spine of a line.**  The input is the quads of the line's members in reading order, (m, 4, 2) float64 ``(y, x)``
(``result_quads(result)[0][line_chars[l]]``).  Per member ``A``, ``D``, ``C``, ``la``, ``ld`` are those of ``strip_warp``.  All
of the rule is float64, evaluated in this order:

* ``H = max ld_m``; ``sgn = +1`` if ``sum_m (A_m.x * D_m.y - A_m.y * D_m.x) >= 0`` else ``-1`` (a mirrored line gives a
  mirrored strip);
* the points ``C_0 - A_0/2``, ``C_0 .. C_{m-1}``, ``C_{m-1} + A_{m-1}/2``: both ends are kept, an interior point is dropped
  when its distance to the previously kept point or to the last point is at most ``H/4``;
* **status 1** (no strip): a corner that is not finite, ``H < 1/16`` or a polyline shorter than ``1/16`` (tested before the
  ends are pushed, as ``strip_warp`` tests ``la``);
* the ends are pushed outwards by ``margin * H`` along the first and the last segment; ``arc_k`` is the length of the
  polyline up to point k, ``L = arc_K`` the whole;
* the tangent ``T_k = unit(p_{k+1} - p_{k-1})``, one-sided at the ends (and where the two neighbours coincide), the down
  vector ``V_k = sgn * (T_k.x, -T_k.y) * H * (1 + 2*margin)`` in ``(y, x)``: reading to the right points down;
* ``w_nat = floor(h * L / (H * (1 + 2*margin)) + 0.5)``, ``w`` and ``squeezed`` as in ``strip_warp``;
* the knot columns ``q_k = rint(w * arc_k / L)`` with ``q_0 = 0``, ``q_K = w``; an interior knot is dropped when its ``q``
  equals the previously kept knot's or ``w``;
* a **knot** is ``KNOT_WORDS = 6`` int64 words ``q, cy, cx, vy, vx, 0``: ``cy, cx = rint(65536 * (p - 1/2))`` (an integer
  coordinate is a pixel centre, as in packing.py), ``vy, vx = rint(65536 * V)``;
* **status 2** (no strip, ``knot_status``): ``|cy|`` or ``|cx| >= 2^39``, ``|vy|`` or ``|vx| > h * (2^22 - 1)``, or a segment
  of ``n`` columns with ``|dcy|`` or ``|dcx| > n * (2^22 - 1)`` - within these every column below is inside the warp bounds;
* ``log2n`` of the strip: the largest ``log2n_of(rdiv(vy, h), rdiv(dcy, n), rdiv(vx, h), rdiv(dcx, n))`` over the segments
  and both end knots of each.

**From knots to columns** (``spine_columns_host``; the same integers on the device).  ``fdiv`` is floor division, ``rdiv(x,
d) = fdiv(2x + d, 2d)``.  Column ``j`` finds its segment by THIS search: ``lo = 0, hi = knots``; while ``hi - lo > 1``: ``mid =
(lo + hi) >> 1``, ``lo = mid`` if ``q[mid] <= j`` else ``hi = mid``.  The column is valid iff ``lo + 1 < knots``, ``q[lo] <= j <
q[lo+1]``, ``n = q[lo+1] - q[lo] <= 8192``, both knots have ``|c| < 2^39`` and ``|v| <= 2^30``, and the record below is within
the bounds of a warp row (``|a| < 2^40``, ``|m| <= 2^22``).  With ``a = 2*(j - q[lo]) + 1``: ``Cy = cy_lo + fdiv(dcy * a, 2n)``
(``Cx, Vy, Vx`` likewise), ``myy = rdiv(Vy, h)``, ``mxy = rdiv(Vx, h)``, ``ay = Cy - fdiv((h - 1) * myy, 2)`` (``ax`` likewise),
``myx = rdiv(dcy, n)``, ``mxx = rdiv(dcx, n)`` (the last two only spread the sub-samples).  No intermediate leaves 64 bits:
``|dc| * a < 2^40 * 2^14``.  A column record is ``COLUMN_WORDS = 6`` int64 words ``ay, ax, myy, myx, mxy, mxx``; an invalid
column is six words of ``INT64_MIN`` and gives zero pixels.  Pixel ``(i, j)`` of the strip is the pixel ``(i, 0)`` of
``warp_host`` for the warp ``(0, 0, h, 1, ay, ax, myy, myx, mxy, mxx, log2n, 0)``.

**Limits.**  The height is one per line (the tallest member's).  Columns are even in arc length within a segment, and a
knot sits on the nearest whole column: the step along the line differs between neighbouring segments by up to one column per
segment.  A bend tighter than the line's height folds the down vectors over each other and is cut as it falls.  There is no
perspective, and a long line is squeezed, not split.

A **spine row** is 12 int64 words ``src, offset, slot_w, w, knot_start, knots, col_start, log2n, 0, 0, 0, 0``: the row's knots
are ``knots`` records from ``knot_start`` of the knot table, its column records ``w`` records from ``col_start`` of the
workspace (``col_start`` is the exclusive scan of ``w``).  The device reads ONE table (``spine_table``): the rows, then
``tile_start`` as in ``strip_table``, then the knot records."""
import math
from typing import Sequence

import attrs
import numpy as np

from .packing import SIDE_MAX, WARP_A_MAX, WARP_M_MAX, _warp_samples
from .strips import (ROW_WORDS, QuadStrips, StripLayout, bucket_views, check_slot_rows, int_rows, log2n_of, slot_layout,
                     strip_params, tile_starts)

KNOT_WORDS = 6
COLUMN_WORDS = 6
INT64_MIN = -(1 << 63)
KNOT_C_MAX = 1 << 39       # |cy|, |cx| stay below
KNOT_V_MAX = 1 << 30       # |vy|, |vx| of a knot the device reads: h * 2^22 at h = 256
STEP_MAX = (1 << 22) - 1   # per strip row / per column, in Q16: the host rule's bound


def rdiv(x: int, d: int) -> int:
    return (2 * x + d) // (2 * d)


def spine_points(quads, margin: float):
    """The float half of the rule up to the pushed points: ``(status, points (K, 2), H, sgn)``; without a spine (status 1 or
    2) the rest is None."""
    P = np.asarray(quads, dtype=np.float64).reshape(-1, 4, 2)
    none = (None, None, None)
    if len(P) == 0 or not np.isfinite(P).all():
        return (1,) + none
    with np.errstate(over='ignore', invalid='ignore'):
        A = ((P[:, 1] - P[:, 0]) + (P[:, 2] - P[:, 3])) / 2
        D = ((P[:, 3] - P[:, 0]) + (P[:, 2] - P[:, 1])) / 2
        C = (P[:, 0] + P[:, 1] + P[:, 2] + P[:, 3]) / 4
        H = float(np.hypot(D[:, 0], D[:, 1]).max())
        sgn = 1.0 if float((A[:, 1] * D[:, 0] - A[:, 0] * D[:, 1]).sum()) >= 0 else -1.0
        pts = [C[0] - A[0] / 2] + list(C) + [C[-1] + A[-1] / 2]
        if not (math.isfinite(H) and all(np.isfinite(p).all() for p in pts)):
            return (2,) + none  # corners so far apart that float64 overflows
        if H < 1 / 16:
            return (1,) + none
        kept = [pts[0]]
        for p in pts[1:-1]:
            if float(np.hypot(*(p - kept[-1]))) <= H / 4 or float(np.hypot(*(p - pts[-1]))) <= H / 4:
                continue
            kept.append(p)
        kept.append(pts[-1])
        p = np.array(kept)
        seg = np.hypot(*(p[1:] - p[:-1]).T)
        if not np.isfinite(seg).all():
            return (2,) + none
        if float(seg.sum()) < 1 / 16:
            return (1,) + none
        p[0] = p[0] - (p[1] - p[0]) / seg[0] * (margin * H)
        p[-1] = p[-1] + (p[-1] - p[-2]) / seg[-1] * (margin * H)
    return 0, p, H, sgn


def knot_status(knots, h: int) -> int:
    """0, or 2 for (K, 6) knots outside the host rule's bounds (module docstring, status 2), in Python integers."""
    k = [[int(v) for v in r] for r in np.asarray(knots).reshape(-1, KNOT_WORDS).tolist()]
    for q, cy, cx, vy, vx, _ in k:
        if max(abs(cy), abs(cx)) >= KNOT_C_MAX or max(abs(vy), abs(vx)) > h * STEP_MAX:
            return 2
    for a, b in zip(k[:-1], k[1:]):
        n = b[0] - a[0]
        if max(abs(b[1] - a[1]), abs(b[2] - a[2])) > n * STEP_MAX:
            return 2
    return 0


def knots_log2n(knots, h: int) -> int:
    k = [[int(v) for v in r] for r in np.asarray(knots).reshape(-1, KNOT_WORDS).tolist()]
    best = 0
    for a, b in zip(k[:-1], k[1:]):
        n = b[0] - a[0]
        myx, mxx = rdiv(b[1] - a[1], n), rdiv(b[2] - a[2], n)
        for e in (a, b):
            best = max(best, log2n_of(rdiv(e[3], h), myx, rdiv(e[4], h), mxx))
    return best


def spine_knots(quads, h: int, width_max: int, margin: float):
    """The quads of one line's members in reading order -> ``(status, squeezed, w, knots (K, 6) int64, log2n)``: the rule of
    the module docstring.  Without a strip (status 1 or 2) ``w`` is 0 and ``knots`` is None."""
    none = (False, 0, None, 0)
    status, p, H, sgn = spine_points(quads, margin)
    if status:
        return (status,) + none
    with np.errstate(over='ignore', invalid='ignore'):
        seg = np.hypot(*(p[1:] - p[:-1]).T)
        arc = np.concatenate([[0.0], np.cumsum(seg)])
        L = float(arc[-1])
        Hm = H * (1 + 2 * margin)
        ratio = h * L / Hm + 0.5
        if not (np.isfinite(p).all() and math.isfinite(ratio)):
            return (2,) + none
        w_nat = math.floor(ratio)
        w = min(max(w_nat, 1), width_max)
        T = np.empty_like(p)
        T[1:-1], T[0], T[-1] = p[2:] - p[:-2], p[1] - p[0], p[-1] - p[-2]
        for k in range(1, len(p) - 1):
            if not T[k].any():
                T[k] = p[k + 1] - p[k]
        T = T / np.hypot(T[:, 0], T[:, 1])[:, None]
        V = np.stack([sgn * T[:, 1], -sgn * T[:, 0]], axis=1) * Hm
        q = np.rint(w * arc / L)
        q[0], q[-1] = 0, w
        keep = [0]
        for k in range(1, len(p) - 1):
            if q[k] != q[keep[-1]] and q[k] != w:
                keep.append(k)
        keep.append(len(p) - 1)
        rec = np.concatenate([q[keep, None], np.rint(65536 * (p[keep] - 0.5)), np.rint(65536 * V[keep]),
                              np.zeros((len(keep), 1))], axis=1)
    if not np.isfinite(rec).all() or np.abs(rec).max() >= 2.0 ** 62:
        return (2,) + none
    knots = rec.astype(np.int64)
    if knot_status(knots, h):
        return (2,) + none
    return 0, w_nat > width_max, w, knots, knots_log2n(knots, h)


def spine_columns_host(knots, w: int, h: int) -> np.ndarray:
    """The (w, 6) int64 column records of (K, 6) ``knots`` for a strip of ``w`` columns and ``h`` rows: the integer rule of
    the module docstring in vectorised int64, whatever the knots hold."""
    k = np.ascontiguousarray(np.asarray(knots, dtype=np.int64).reshape(-1, KNOT_WORDS))
    K, w, h = len(k), int(w), int(h)
    out = np.full((w, COLUMN_WORDS), INT64_MIN, np.int64)
    if K < 2 or w < 1:
        return out
    j = np.arange(w, dtype=np.int64)
    q = k[:, 0]
    lo, hi = np.zeros((w,), np.int64), np.full((w,), K, np.int64)
    while (hi - lo > 1).any():
        go, mid = hi - lo > 1, (lo + hi) >> 1
        le = q[mid] <= j
        lo, hi = np.where(go & le, mid, lo), np.where(go & ~le, mid, hi)
    e0, e1 = k[lo], k[np.minimum(lo + 1, K - 1)]
    # n <= 8192 needs q[lo] > j - 8192 and q[lo+1] <= j + 8192: tested first, so that n itself cannot overflow
    ok = (lo + 1 < K) & (e0[:, 0] <= j) & (j < e1[:, 0]) & (e0[:, 0] > j - SIDE_MAX) & (e1[:, 0] <= j + SIDE_MAX)
    for e in (e0, e1):
        ok &= ((e[:, 1:3] > -KNOT_C_MAX) & (e[:, 1:3] < KNOT_C_MAX)).all(axis=1)
        ok &= ((e[:, 3:5] >= -KNOT_V_MAX) & (e[:, 3:5] <= KNOT_V_MAX)).all(axis=1)
    e0, e1 = np.where(ok[:, None], e0, 0), np.where(ok[:, None], e1, 0)
    n = np.where(ok, e1[:, 0] - e0[:, 0], 1)
    ok &= n <= SIDE_MAX
    n = np.where(ok, n, 1)
    a = np.where(ok, 2 * (j - e0[:, 0]) + 1, 1)
    d = e1[:, 1:5] - e0[:, 1:5]
    Cy, Cx, Vy, Vx = (e0[:, 1:5] + (d * a[:, None]) // (2 * n)[:, None]).T
    myy, mxy = (2 * Vy + h) // (2 * h), (2 * Vx + h) // (2 * h)
    myx, mxx = (2 * d[:, 0] + n) // (2 * n), (2 * d[:, 1] + n) // (2 * n)
    ay, ax = Cy - ((h - 1) * myy) // 2, Cx - ((h - 1) * mxy) // 2
    rec = np.stack([ay, ax, myy, myx, mxy, mxx], axis=1)
    ok &= (np.abs(rec[:, :2]) < WARP_A_MAX).all(axis=1) & (np.abs(rec[:, 2:]) <= WARP_M_MAX).all(axis=1)
    out[ok] = rec[ok]
    return out


def spine_pixels_host(src: np.ndarray, columns, h: int, log2n: int) -> np.ndarray:
    """The (h, w, 3) uint8 pixels of (w, 6) column records: per column ``warp_host`` of the one-pixel-wide warp ``(0, 0, h, 1,
    ay, ax, myy, myx, mxy, mxx, log2n, 0)``, all columns in one array expression per sub-sample; an invalid column is 0."""
    src = np.asarray(src)
    if src.ndim != 3 or src.shape[2] != 3 or src.dtype != np.uint8:
        raise ValueError(f'src must be an (H, W, 3) uint8 image, got {src.dtype} {src.shape}')
    c = np.asarray(columns, dtype=np.int64).reshape(-1, COLUMN_WORDS)
    h, log2n = int(h), int(log2n)
    valid = (c != INT64_MIN).all(axis=1)
    ay, ax, myy, myx, mxy, mxx = np.where(valid[:, None], c, 0).T[:, None, :]
    i = np.arange(h, dtype=np.int64)[:, None]
    Y, X = ay + i * myy, ax + i * mxy
    n, shift = 1 << log2n, 32 + 2 * log2n
    total = np.zeros((h, len(c), 3), np.int64)
    for a in range(n):
        for b in range(n):
            ka, kb = 2 * a + 1 - n, 2 * b + 1 - n
            total += _warp_samples(src, Y + ((ka * myy + kb * myx) >> (1 + log2n)), X + ((ka * mxy + kb * mxx) >> (1 + log2n)))
    out = ((total + (1 << (shift - 1))) >> shift).astype(np.uint8)
    out[:, ~valid] = 0
    return out


def spine_polygon(knots) -> np.ndarray:
    """The outline of a line from its (K, 6) knots: (2K, 2) float64 ``(y, x)`` image positions, ``C - V/2`` in knot order, then
    ``C + V/2`` in reverse order."""
    k = np.asarray(knots, dtype=np.float64).reshape(-1, KNOT_WORDS)
    C, V = k[:, 1:3] / 65536 + 0.5, k[:, 3:5] / 65536
    return np.concatenate([C - V / 2, (C + V / 2)[::-1]])


@attrs.define
class SpineLayout(StripLayout):
    """``spine_rows``: ``StripLayout`` with K spine rows in input order of the lines that have a strip, per line (N of them,
    image after image) what became of it, and the rows' knots."""
    knots: np.ndarray      # (knots_total, 6) int64
    columns: int           # the sum of w: the column records of the workspace


def spine_rows(lines_per_image: Sequence, h: int = 32, width_max: int = 2048, width_step: int = 64,
               margin: float = 0.125) -> SpineLayout:
    """The spine rows of the lines of several images - ``lines_per_image[s]`` is a list of (m, 4, 2) arrays, the members of
    each line of source s in reading order - with the slots of ``strip_rows``."""
    h, width_max, width_step, margin = strip_params(h, width_max, width_step, margin)
    lines = [[np.asarray(q, dtype=np.float64).reshape(-1, 4, 2) for q in ls] for ls in lines_per_image]
    image = np.repeat(np.arange(len(lines), dtype=np.int32), [len(ls) for ls in lines])
    N = len(image)
    status, squeezed, widths = np.zeros((N,), np.int32), np.zeros((N,), bool), np.zeros((N,), np.int32)
    knots, log2n = [None] * N, [0] * N
    for k, quads in enumerate(q for ls in lines for q in ls):
        status[k], squeezed[k], widths[k], knots[k], log2n[k] = spine_knots(quads, h, width_max, margin)
    have = status == 0
    slot_w, offset, bucket, index, shapes, total = slot_layout(have, widths, h, width_step)
    rows = np.zeros((int(have.sum()), ROW_WORDS), np.int64)
    knot_at = col_at = 0
    for r, k in enumerate(np.flatnonzero(have).tolist()):
        rows[r, :8] = (image[k], offset[k], slot_w[k], widths[k], knot_at, len(knots[k]), col_at, log2n[k])
        knot_at, col_at = knot_at + len(knots[k]), col_at + int(widths[k])
    table = np.concatenate([knots[k] for k in np.flatnonzero(have).tolist()] + [np.zeros((0, KNOT_WORDS), np.int64)])
    return SpineLayout(rows, image, status, squeezed, widths, bucket, index, shapes, total, np.ascontiguousarray(table), col_at)


def check_spine_rows(rows, knots, sources, h: int, out_bytes: int, columns: int) -> np.ndarray:
    """Validates a (K, 12) spine table against its (T, 6) knot table, the (S, 4) source table, the height, the output size and
    a workspace of ``columns`` records - ``strips.check_slot_rows``, an integer knot table, ``log2n`` in 0..3, ``knots >= 2``
    and ``knot_start + knots`` inside the knot table, every row's ``q`` strictly increasing from 0 to ``w``, its columns inside
    the workspace and disjoint from the other rows' - and returns the rows as contiguous int64.  Raises ValueError."""
    r, t = int_rows('spines', rows), np.asarray(knots)
    if t.ndim != 2 or t.shape[1] != KNOT_WORDS or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f'spines: knots must be a (T, {KNOT_WORDS}) integer table, got {t.dtype} {t.shape}')
    t, columns = t.astype(np.int64), int(columns)

    def own(r):
        if ((r[:, 7] < 0) | (r[:, 7] > 3)).any():
            raise ValueError('spines: log2n must be in [0, 3]')
        if ((r[:, 4] < 0) | (r[:, 5] < 2) | (r[:, 4] > len(t)) | (r[:, 5] > len(t) - r[:, 4])).any():
            raise ValueError(f'spines: a row needs at least 2 knots inside the knot table of {len(t)} records')
        for _, _, _, w, at, count, *_ in r.tolist():
            q = t[at:at + count, 0]
            if q[0] != 0 or q[-1] != w or (np.diff(q) <= 0).any():
                raise ValueError('spines: the knot columns of a row must rise strictly from 0 to w')
        first, last = r[:, 6], r[:, 6] + r[:, 3]
        if ((first < 0) | (last > columns)).any():
            raise ValueError(f'spines: a row\'s columns leave the workspace of {columns} records')
        order = np.argsort(first, kind='stable')
        if (last[order][:-1] > first[order][1:]).any():
            raise ValueError('spines: two rows share column records')
    return check_slot_rows('spines', r, sources, h, out_bytes, own)


def spine_table(rows, knots, h: int) -> np.ndarray:
    """What the device reads (csrc/spines.hip): the (K, 12) rows flattened, then ``strips.tile_starts``, then the (T, 6) knot
    records flattened."""
    r = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, ROW_WORDS))
    t = np.ascontiguousarray(np.asarray(knots, dtype=np.int64).reshape(-1, KNOT_WORDS))
    return np.concatenate([r.reshape(-1), tile_starts(r[:, 2], h), t.reshape(-1)])


@attrs.define
class SpineStrips(QuadStrips):
    """The strips of N lines (image after image, each image's lines in input order): ``QuadStrips`` with spine rows - status 1
    is a degenerate line, 2 knots out of range -, and the knot table.  ``buckets`` are views of one allocation: device tensors
    from ``inferencing.spine_strips``, numpy arrays from ``spine_strips_host``."""
    knots: np.ndarray      # (T, 6) int64: the knot table the rows point into
    _item = 'line'

    def _knots(self, k: int) -> np.ndarray:
        row = self._row(k)
        return self.knots[int(row[4]):int(row[4] + row[5])]

    def remap(self, k: int, points) -> np.ndarray:
        """(..., 2) (y, x) positions in line k's strip (pixel k covers ``[k, k + 1)``) -> float64 positions in its image,
        piecewise affine: the column ``floor(x)`` (within 0..w-1) at ``i = y - 1/2``, plus ``(x - floor(x) - 1/2) * (myx,
        mxx)``.  A position in an invalid column maps to NaN."""
        w = int(self._row(k)[3])
        cols = spine_columns_host(self._knots(k), w, self.height)
        p = np.asarray(points, dtype=np.float64)
        j = np.clip(np.floor(p[..., 1]), 0, w - 1).astype(np.int64)
        c = np.where((cols[j] != INT64_MIN).all(axis=-1, keepdims=True), cols[j].astype(np.float64), np.nan)
        i, f = p[..., 0] - 0.5, p[..., 1] - j - 0.5
        out = np.empty(p.shape, np.float64)
        out[..., 0] = (c[..., 0] + i * c[..., 2] + f * c[..., 3]) / 65536 + 0.5
        out[..., 1] = (c[..., 1] + i * c[..., 4] + f * c[..., 5]) / 65536 + 0.5
        return out

    def spine(self, k: int) -> np.ndarray:
        """(K, 2, 2) float64: per knot of line k its centre and its down vector, ``(y, x)`` in image pixels."""
        t = self._knots(k).astype(np.float64)
        return np.stack([t[:, 1:3] / 65536 + 0.5, t[:, 3:5] / 65536], axis=1)


def spine_bytes_host(images: Sequence[np.ndarray], rows, knots, h: int, out: np.ndarray) -> np.ndarray:
    """Writes the slots of valid spine rows into the 1-D uint8 ``out`` (in place): each slot its strip and zeros beyond w."""
    for src, offset, slot_w, w, at, count, _, log2n, *_ in np.asarray(rows, dtype=np.int64).reshape(-1, ROW_WORDS).tolist():
        slot = out[offset:offset + h * slot_w * 3].reshape(h, slot_w, 3)
        slot[:] = 0
        slot[:, :w] = spine_pixels_host(images[src], spine_columns_host(knots[at:at + count], w, h), h, log2n)
    return out


def spine_strips_host(images: Sequence[np.ndarray], lines_per_image: Sequence, height: int = 32, width_max: int = 2048,
                      width_step: int = 64, margin: float = 0.125) -> SpineStrips:
    """The oracle of ``inferencing.spine_strips``: ``spine_rows``, ``spine_columns_host``, then the pixel rule of ``warp_host``
    per column into zeroed slots.  The same object as the device route gives, with numpy buckets."""
    if len(images) != len(lines_per_image):
        raise ValueError(f'{len(lines_per_image)} line lists for {len(images)} images')
    layout = spine_rows(lines_per_image, height, width_max, width_step, margin)
    h = int(height)
    out = spine_bytes_host(images, layout.rows, layout.knots, h, np.zeros((layout.out_bytes,), np.uint8))
    return SpineStrips.of(layout, bucket_views(out, layout.bucket_shapes), h)
