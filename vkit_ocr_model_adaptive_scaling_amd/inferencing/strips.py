"""Text lines cut into upright strips of one height: the rule from a quadrilateral to a strip, the layout of the strips in
one output buffer and the host oracle of the device route (``ops.quad_strips_u8``, csrc/strips.hip).  Host only: numpy and
Python.

A **strip** is the upright cut of one quadrilateral ``quad``, a (4, 2) float64 array of ``(y, x)`` image positions (pixel k
covers ``[k, k + 1)``) with the corners up-left, up-right, down-right, down-left as ``line_quads`` and the character quads
give them, resampled to ``h`` rows and ``w`` columns.  All of the rule is float64, evaluated in this order:

* ``A = ((P1 - P0) + (P2 - P3)) / 2`` runs along the reading direction, ``D = ((P3 - P0) + (P2 - P1)) / 2`` down the
  character, ``C = (P0 + P1 + P2 + P3) / 4``; ``la = hypot(A)``, ``ld = hypot(D)``;
* **status 1** (no strip): a corner that is not finite, ``la < 1/16`` or ``ld < 1/16``;
* with ``margin`` in units of the quad's height: ``la' = la + 2*margin*ld``, ``ld' = ld * (1 + 2*margin)``;
* ``w_nat = floor(h * la' / ld' + 0.5)``, ``w = min(max(w_nat, 1), width_max)``, ``squeezed = w_nat > width_max`` (the line
  is squeezed along its length; long lines are not split);
* ``step_j = A/la * (la'/w)``, ``step_i = D/ld * (ld'/h)``: source pixels per strip pixel; the centre of strip pixel
  ``(i, j)`` is ``C + (j + 1/2 - w/2) * step_j + (i + 1/2 - h/2) * step_i``;
* the Q16 coefficients in the warp convention of packing.py (an integer coordinate is a pixel centre): ``myx, mxx =
  rint(65536 * step_j)``, ``myy, mxy = rint(65536 * step_i)``, ``ay = rint(65536 * (C.y - 1/2 + (1/2 - w/2) * step_j.y +
  (1/2 - h/2) * step_i.y))``, ``ax`` likewise;
* ``log2n`` from ``t = max(myy^2 + mxy^2, myx^2 + mxx^2)`` in Python integers: 0 for ``t <= 2^32``, 1 for ``t <= 2^34``, 2 for
  ``t <= 2^36``, else 3 - the smallest power of two at or above the longer source step, at most 8 (a line shrunk by more
  aliases, as regions do);
* **status 2** (no strip): a coefficient above ``WARP_M_MAX`` or an anchor that reaches ``WARP_A_MAX``.

A mirrored (counter-clockwise) quad gives a mirrored strip; a quad that is no rectangle is cut as the parallelogram ``(C, A,
D)``.  The pixels are exactly those of ``warp_host`` for the warp ``(0, 0, h, w, ay, ax, myy, myx, mxy, mxx, log2n, 0)``.

**Slots and buckets.**  Strip k gets a slot of ``h x slot_w x 3`` bytes, ``slot_w`` the smallest multiple of ``width_step``
at or above ``w``; the columns ``w .. slot_w - 1`` are 0.  The strips of one ``slot_w`` form a bucket, one ``(n_b, h, slot_w,
3)`` uint8 tensor in input order; the buckets lie one after another, in ascending ``slot_w``, in ONE allocation.

A **strip row** is 12 int64 words ``src, offset, slot_w, w, ay, ax, myy, myx, mxy, mxx, log2n, 0``: ``src`` the row of the
``(S, 4)`` int64 source table ``byte offset, Hs, Ws, 0`` (``ops.image_arena``), ``offset`` the slot's byte offset in the
output.  The device reads the rows followed by ``tile_start`` (``strip_table``)."""
import math
from typing import List, Sequence, Tuple

import attrs
import numpy as np

from .packing import SIDE_MAX, WARP_A_MAX, WARP_M_MAX, remap_polygons_affine, warp_host

ROW_WORDS = 12
HEIGHT_MAX = 256
TILE_H, TILE_W = 16, 64     # csrc/strip_tiles.h: the pixels of one workgroup's tile
SOURCE_SIDE_MAX = 32768


def strip_params(h, width_max, width_step, margin) -> Tuple[int, int, int, float]:
    """The parameters, checked: ``h`` in 1..256, ``width_max`` in 1..8192, ``width_step`` in 1..``width_max``, ``margin`` in
    [0, 1].  Raises ValueError."""
    for name, v, lo, hi in (('height', h, 1, HEIGHT_MAX), ('width_max', width_max, 1, SIDE_MAX)):
        if isinstance(v, bool) or v != int(v) or not lo <= int(v) <= hi:
            raise ValueError(f'strips: {name} must be an integer in [{lo}, {hi}], got {v!r}')
    if isinstance(width_step, bool) or width_step != int(width_step) or not 1 <= int(width_step) <= int(width_max):
        raise ValueError(f'strips: width_step must be an integer in [1, {int(width_max)}], got {width_step!r}')
    if not 0.0 <= float(margin) <= 1.0:  # also rejects NaN
        raise ValueError(f'strips: margin must be in [0, 1], got {margin!r}')
    return int(h), int(width_max), int(width_step), float(margin)


def log2n_of(myy: int, myx: int, mxy: int, mxx: int) -> int:
    t = max(int(myy) ** 2 + int(mxy) ** 2, int(myx) ** 2 + int(mxx) ** 2)
    return 0 if t <= 1 << 32 else 1 if t <= 1 << 34 else 2 if t <= 1 << 36 else 3


def strip_warp(quad, h: int, width_max: int, margin: float):
    """One quad -> ``(status, squeezed, w, (ay, ax, myy, myx, mxy, mxx, log2n))``: the rule of the module docstring.  Without a
    strip (status 1 or 2) ``w`` is 0 and the coefficients are None."""
    P = np.asarray(quad, dtype=np.float64).reshape(4, 2)
    none = (False, 0, None)
    if not np.isfinite(P).all():
        return (1,) + none
    with np.errstate(over='ignore', invalid='ignore'):
        A = ((P[1] - P[0]) + (P[2] - P[3])) / 2
        D = ((P[3] - P[0]) + (P[2] - P[1])) / 2
        C = (P[0] + P[1] + P[2] + P[3]) / 4
        la, ld = float(np.hypot(A[0], A[1])), float(np.hypot(D[0], D[1]))
        if la < 1 / 16 or ld < 1 / 16:
            return (1,) + none
        la2, ld2 = la + 2 * margin * ld, ld * (1 + 2 * margin)
        ratio = h * la2 / ld2 + 0.5
        if not (math.isfinite(la) and math.isfinite(ld) and math.isfinite(ratio) and np.isfinite(C).all()):
            return (2,) + none  # corners so far apart that float64 overflows: no coefficient is in range
        w_nat = math.floor(ratio)
        w = min(max(w_nat, 1), width_max)
        step_j, step_i = A / la * (la2 / w), D / ld * (ld2 / h)
        myx, mxx = np.rint(65536 * step_j)
        myy, mxy = np.rint(65536 * step_i)
        ay, ax = np.rint(65536 * (C - 0.5 + (0.5 - w / 2) * step_j + (0.5 - h / 2) * step_i))
    coef = (ay, ax, myy, myx, mxy, mxx)
    if not all(math.isfinite(v) for v in coef) or max(abs(v) for v in coef[2:]) > WARP_M_MAX or \
            max(abs(ay), abs(ax)) >= WARP_A_MAX:
        return (2,) + none
    coef = tuple(int(v) for v in coef)
    return 0, w_nat > width_max, w, coef + (log2n_of(*coef[2:]),)


@attrs.define
class StripLayout:
    """``strip_rows``: K strip rows in input order of the quads that have a strip, and per quad (N of them, image after
    image) what became of it."""
    rows: np.ndarray       # (K, 12) int64 strip rows
    image: np.ndarray      # (N,) int32: the image (source row) of each quad
    status: np.ndarray     # (N,) int32: 0, or 1 / 2 for a quad without a strip
    squeezed: np.ndarray   # (N,) bool
    widths: np.ndarray     # (N,) int32: w, 0 without a strip
    bucket: np.ndarray     # (N,) int32: the strip's bucket, -1 without a strip
    index: np.ndarray      # (N,) int32: its place in the bucket, -1 without a strip
    bucket_shapes: List[Tuple[int, int, int, int]]  # per bucket (n_b, h, slot_w, 3), ascending slot_w
    out_bytes: int


def slot_layout(have: np.ndarray, widths: np.ndarray, h: int, width_step: int):
    """The slots and buckets of the module docstring for N strips of which ``have`` exist, ``widths`` columns wide ->
    ``(slot_w (N,) int64, offset (N,) int64, bucket (N,) int32, index (N,) int32, bucket_shapes, out_bytes)``."""
    N = len(widths)
    slot_w = np.where(have, -(-widths.astype(np.int64) // width_step) * width_step, 0)
    sizes = sorted(set(slot_w[have].tolist()))
    bucket = np.full((N,), -1, np.int32)
    index = np.full((N,), -1, np.int32)
    offset = np.zeros((N,), np.int64)
    shapes, total = [], 0
    for b, sw in enumerate(sizes):
        mine = np.flatnonzero(have & (slot_w == sw))
        bucket[mine], index[mine] = b, np.arange(len(mine))
        offset[mine] = total + np.arange(len(mine), dtype=np.int64) * (h * sw * 3)
        shapes.append((len(mine), h, int(sw), 3))
        total += len(mine) * h * sw * 3
    return slot_w, offset, bucket, index, shapes, int(total)


def strip_rows(quads_per_image: Sequence, h: int = 32, width_max: int = 2048, width_step: int = 64,
               margin: float = 0.125) -> StripLayout:
    """The strip rows of the quads of several images - ``quads_per_image[s]`` is an (n_s, 4, 2) array of quads of source s -
    and their slots: buckets in ascending ``slot_w``, a bucket's strips in input order."""
    h, width_max, width_step, margin = strip_params(h, width_max, width_step, margin)
    quads = [np.asarray(q, dtype=np.float64).reshape(-1, 4, 2) for q in quads_per_image]
    image = np.repeat(np.arange(len(quads), dtype=np.int32), [len(q) for q in quads])
    N = len(image)
    status, squeezed, widths = np.zeros((N,), np.int32), np.zeros((N,), bool), np.zeros((N,), np.int32)
    coefs = [None] * N
    for k, quad in enumerate(q for qs in quads for q in qs):
        status[k], squeezed[k], widths[k], coefs[k] = strip_warp(quad, h, width_max, margin)
    have = status == 0
    slot_w, offset, bucket, index, shapes, total = slot_layout(have, widths, h, width_step)
    rows = np.zeros((int(have.sum()), ROW_WORDS), np.int64)
    for r, k in enumerate(np.flatnonzero(have).tolist()):
        rows[r] = (image[k], offset[k], slot_w[k], widths[k]) + coefs[k] + (0,)
    return StripLayout(rows, image, status, squeezed, widths, bucket, index, shapes, int(total))


def int_rows(who: str, rows) -> np.ndarray:
    """A (K, 12) integer row table as contiguous int64.  Raises ValueError."""
    r = np.asarray(rows)
    if r.ndim != 2 or r.shape[1] != ROW_WORDS or not np.issubdtype(r.dtype, np.integer):
        raise ValueError(f'{who}: rows must be a (K, {ROW_WORDS}) integer table, got {r.dtype} {r.shape}')
    return np.ascontiguousarray(r.astype(np.int64))


def check_slot_rows(who: str, r: np.ndarray, sources, h: int, out_bytes: int, own) -> np.ndarray:
    """What strip rows and spine rows (``r`` from ``int_rows``) are checked for alike, their words 0 .. 3 meaning the same: the
    (S, 4) integer source table with sides in 1..32768, the height, ``src`` in range, ``1 <= w <= slot_w <= 8192``; then
    ``own(r)``, the checks of the rows' other words; then every slot inside the output and the slots pairwise disjoint.
    ``who`` begins the messages.  Returns ``r``; raises ValueError."""
    s = np.asarray(sources)
    if s.ndim != 2 or s.shape[1] != 4 or not np.issubdtype(s.dtype, np.integer):
        raise ValueError(f'{who}: sources must be an (S, 4) integer table, got {s.dtype} {s.shape}')
    h, out_bytes = int(h), int(out_bytes)
    if not 1 <= h <= HEIGHT_MAX:
        raise ValueError(f'{who}: height must be in [1, {HEIGHT_MAX}], got {h}')
    if ((s[:, 1:3] < 1) | (s[:, 1:3] > SOURCE_SIDE_MAX)).any() or (s[:, 0] < 0).any():
        raise ValueError(f'{who}: source sides must be in [1, {SOURCE_SIDE_MAX}] and offsets at or above 0')
    if ((r[:, 0] < 0) | (r[:, 0] >= len(s))).any():
        raise ValueError(f'{who}: a row names a source outside 0..{len(s) - 1}')
    if ((r[:, 3] < 1) | (r[:, 3] > r[:, 2]) | (r[:, 2] > SIDE_MAX)).any():
        raise ValueError(f'{who}: every row needs 1 <= w <= slot_w <= {SIDE_MAX}')
    own(r)
    start, end = r[:, 1], r[:, 1] + 3 * h * r[:, 2]
    if ((start < 0) | (end > out_bytes)).any():
        raise ValueError(f'{who}: a slot leaves the output of {out_bytes} bytes')
    order = np.argsort(start, kind='stable')
    if (end[order][:-1] > start[order][1:]).any():
        raise ValueError(f'{who}: two slots overlap')
    return r


def check_strip_rows(rows, sources, h: int, out_bytes: int) -> np.ndarray:
    """Validates a (K, 12) strip table against the (S, 4) source table, the height and the output size - ``check_slot_rows``,
    the coefficients within the warp bounds and ``log2n`` in 0..3 - and returns it as contiguous int64.  Raises ValueError."""
    def own(r):
        if (np.abs(r[:, 6:10]) > WARP_M_MAX).any() or (np.abs(r[:, 4:6]) >= WARP_A_MAX).any():
            raise ValueError('strips: a coefficient exceeds 2^22 or an anchor reaches 2^40')
        if ((r[:, 10] < 0) | (r[:, 10] > 3)).any():
            raise ValueError('strips: log2n must be in [0, 3]')
    return check_slot_rows('strips', int_rows('strips', rows), sources, h, out_bytes, own)


def tile_starts(slot_w, h: int) -> np.ndarray:
    """``tile_start``, K + 1 int64 words for K slots: row r owns the tiles ``tile_start[r] .. tile_start[r + 1] - 1`` of 16 x 64
    pixels, ``ceil(h/16) * ceil(slot_w/64)`` of them (csrc/strip_tiles.h)."""
    tiles = -(-int(h) // TILE_H) * (-(-np.clip(np.asarray(slot_w, dtype=np.int64), 0, SIDE_MAX) // TILE_W))
    return np.concatenate([[0], np.cumsum(tiles)]).astype(np.int64)


def strip_table(rows, h: int) -> np.ndarray:
    """What the device reads (csrc/strips.hip): the (K, 12) rows flattened, followed by ``tile_starts``."""
    r = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, ROW_WORDS))
    return np.concatenate([r.reshape(-1), tile_starts(r[:, 2], h)])


@attrs.define
class QuadStrips:
    """The strips of N quads (image after image, each image's quads in input order).  ``buckets`` are views of one
    allocation: device tensors from ``inferencing.quad_strips``, numpy arrays from ``quad_strips_host``."""
    buckets: list          # per bucket (n_b, h, slot_w, 3) uint8, ascending slot_w: a recogniser's batches as they are
    image: np.ndarray      # (N,) int32
    status: np.ndarray     # (N,) int32: 0, 1 (degenerate quad) or 2 (coefficients out of range)
    squeezed: np.ndarray   # (N,) bool: the natural width exceeded width_max
    widths: np.ndarray     # (N,) int32: w; 0 without a strip
    bucket: np.ndarray     # (N,) int32; -1 without a strip
    index: np.ndarray      # (N,) int32; -1 without a strip
    rows: np.ndarray       # (K, 12) int64 strip rows of the quads with status 0, in input order
    height: int
    _item = 'quad'         # what a strip is cut from, for the messages

    @classmethod
    def of(cls, layout: StripLayout, buckets: list, h: int):
        """The strips of a layout with their buckets; the fields a subclass adds come from the layout by name."""
        more = {f.name: getattr(layout, f.name) for f in attrs.fields(cls)[len(attrs.fields(QuadStrips)):]}
        return cls(buckets, layout.image, layout.status, layout.squeezed, layout.widths, layout.bucket, layout.index,
                   layout.rows, h, **more)

    def _row(self, k: int) -> np.ndarray:
        if self.status[k] != 0:
            raise ValueError(f'{self._item} {k} has no strip (status {int(self.status[k])})')
        return self.rows[int(np.count_nonzero(self.status[:k] == 0))]

    def strip(self, k: int):
        """The (h, w, 3) view of strip k (without the slot's zero columns)."""
        self._row(k)
        return self.buckets[int(self.bucket[k])][int(self.index[k])][:, :int(self.widths[k])]

    def remap(self, k: int, points) -> np.ndarray:
        """(..., 2) (y, x) positions in quad k's strip -> float64 positions in its image."""
        return remap_strip_points(points, self._row(k))


def remap_strip_points(points, row) -> np.ndarray:
    """(..., 2) (y, x) strip positions (pixel k covers ``[k, k + 1)``) -> float64 positions in the image the strip row reads:
    ``remap_polygons_affine`` with the destination at (0, 0)."""
    row = np.asarray(row, dtype=np.int64).reshape(ROW_WORDS)
    return remap_polygons_affine(points, np.concatenate([np.zeros((4,), np.int64), row[4:]]))


def bucket_views(out, bucket_shapes) -> list:
    """The buckets as views of the 1-D uint8 output (numpy array or tensor)."""
    views, at = [], 0
    for shape in bucket_shapes:
        size = int(np.prod(shape))
        views.append(out[at:at + size].reshape(shape))
        at += size
    return views


def quad_strips_host(images: Sequence[np.ndarray], quads_per_image: Sequence, height: int = 32, width_max: int = 2048,
                     width_step: int = 64, margin: float = 0.125) -> QuadStrips:
    """The oracle of ``inferencing.quad_strips``: ``strip_rows``, then ``warp_host`` per strip into zeroed slots.  The same
    object as the device route gives, with numpy buckets."""
    if len(images) != len(quads_per_image):
        raise ValueError(f'{len(quads_per_image)} quad arrays for {len(images)} images')
    layout = strip_rows(quads_per_image, height, width_max, width_step, margin)
    h = int(height)
    out = np.zeros((layout.out_bytes,), np.uint8)
    for src, offset, slot_w, w, *coef in layout.rows.tolist():
        page = warp_host(images[src], [[0, 0, h, w] + coef], np.zeros((h, w, 3), np.uint8))
        out[offset:offset + h * slot_w * 3].reshape(h, slot_w, 3)[:, :w] = page
    return QuadStrips.of(layout, bucket_views(out, layout.bucket_shapes), h)
