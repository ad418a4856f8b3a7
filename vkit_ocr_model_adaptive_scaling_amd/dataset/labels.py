"""Training labels from character quadrilaterals: the rule, its host oracle, and the batch side.

The reference takes its label maps from vkit's synthetic pipeline (``page_char_mask``, ``page_char_height_score_map``,
``page_char_gaussian_score_map``, ``PageCharRegressionLabel``; dataset/adaptive_scaling.py:93-146).  vkit is absent here, so
the rule below is THIS PROJECT'S OWN, restated on pixels: it is neither vkit's polygon fill nor its perspective-warped
Gaussian.  It is defined in integers and in float32 without contraction, so the device kernel (csrc/labels.hip) and
``char_label_maps_host`` are held to each other exactly.

A quadrilateral is ``(4, 2)`` ``(y, x)`` in pixels of the model-input image, corners up-left, up-right, down-right, down-left
(clockwise with y down) - the order ``ops.char_polygons`` and ``infer`` emit.  With ``f`` image pixels per map pixel:

A quad row is 20 int32 (80 bytes, five 16-byte loads; float fields stored as their bits):
    0..7    the corners in map coordinates, Q4: ``rint(c * 16 / f)`` (half to even)
    8..11   the inclusive pixel box (y0, x0, y1, x1) of the Q4 corners (``>> 4``), clipped to the map; may be empty
    12, 13  float32 centre (cy, cx) in map pixels: the mean of the four Q4 corners
    14..17  float32 (m00, m01, m10, m11): the inverse of the frame [a b], a = ((ur + dr) - (ul + dl)) / 4 and
            b = ((dl + dr) - (ul + ur)) / 4 in map pixels (of the Q4 corners), so that (s, t) = M (p - c) is (+-1, 0) at the
            side mid-points of a parallelogram
    18      float32 height: the mean of |dl - ul| and |dr - ur| in IMAGE pixels (of the given corners)
    19      int32 valid
(the listed fields fill the 20 words exactly: there is no padding word)

A quad is valid iff its Q4 corners lie within +-2^19, are strictly convex and clockwise (all four int64 cross products
positive), its frame is invertible and its height finite and positive.  An invalid quad gets a zero row and is reported
through the ``valid`` array; nothing is clamped or repaired.

A pixel (y, x) is inside a quad iff its centre (16y + 8, 16x + 8) has all four int64 edge functions >= 0 (inclusive: a
centre on a shared edge is inside both quads).  Its owner is the valid inside-quad with the smallest float32
    a = k * (s*s + t*t),  s = m00*dy + m01*dx,  t = m10*dy + m11*dx,  dy = (float(y) + 0.5f) - cy,  dx likewise
(every product and sum rounded, no fma), ties to the lowest index; k = float32(1 / (2 sigma^2)), e^-2 at a side mid-point
for the default sigma 0.5.  mask = (owner != 0), height = the owner's height, score = exp(-a) of the owner."""
from typing import Any, Dict, Iterable, Optional, Sequence, Tuple

import attrs
import numpy as np
import torch

from ..loss_function import Box
from ..utils import portable_rng as prng

ROW_WORDS = 20
ROW_BOX, ROW_CENTRE, ROW_FRAME, ROW_HEIGHT, ROW_VALID = 8, 12, 14, 18, 19
COORD_MAX = 1 << 19
_INT_MAX = np.iinfo(np.int32).max
_TWO_PI = 2.0 * np.pi


def _box4(box) -> Tuple[int, int, int, int]:
    if isinstance(box, (tuple, list)):
        up, down, left, right = box
    else:
        up, down, left, right = box.up, box.down, box.left, box.right
    return int(up), int(down), int(left), int(right)


def quad_rows(quads, h: int, w: int, f: float) -> Tuple[np.ndarray, np.ndarray]:
    """``quads`` (n, 4, 2) -> ``(rows (n, 20) int32, valid (n,) bool)`` for an (h, w) map at ``f`` image pixels per map pixel."""
    q = np.asarray(quads, dtype=np.float64).reshape(-1, 4, 2)
    n = len(q)
    rows = np.zeros((n, ROW_WORDS), dtype=np.int32)
    if n == 0:
        return rows, np.zeros((0,), dtype=bool)
    with np.errstate(all='ignore'):
        c16 = np.rint(q * 16.0 / f)
        ok = (np.abs(c16) <= COORD_MAX).all(axis=(1, 2))  # NaN and inf compare false
        ci = np.where(ok[:, None, None], c16, 0.0).astype(np.int64)
        e = np.roll(ci, -1, axis=1) - ci                   # ul->ur, ur->dr, dr->dl, dl->ul as (dy, dx)
        en = np.roll(e, -1, axis=1)
        ok &= (e[..., 1] * en[..., 0] - e[..., 0] * en[..., 1] > 0).all(axis=1)
        A = (ci[:, 1] + ci[:, 2]) - (ci[:, 0] + ci[:, 3])  # 64 a
        Bv = (ci[:, 3] + ci[:, 2]) - (ci[:, 0] + ci[:, 1])  # 64 b
        det = A[:, 0] * Bv[:, 1] - Bv[:, 0] * A[:, 1]
        ok &= det != 0
        inv = 64.0 / np.where(det != 0, det, 1).astype(np.float64)
        frame = np.stack([Bv[:, 1] * inv, -Bv[:, 0] * inv, -A[:, 1] * inv, A[:, 0] * inv], axis=1).astype(np.float32)
        ok &= np.isfinite(frame).all(axis=1)
        height = (0.5 * (np.hypot(*(q[:, 3] - q[:, 0]).T) + np.hypot(*(q[:, 2] - q[:, 1]).T))).astype(np.float32)
        ok &= np.isfinite(height) & (height > 0)
    fl = rows.view(np.float32)
    rows[:, 0:8] = ci.reshape(n, 8)
    lo, hi = ci.min(axis=1) >> 4, ci.max(axis=1) >> 4
    rows[:, ROW_BOX + 0] = np.maximum(lo[:, 0], 0)
    rows[:, ROW_BOX + 1] = np.maximum(lo[:, 1], 0)
    rows[:, ROW_BOX + 2] = np.minimum(hi[:, 0], h - 1)
    rows[:, ROW_BOX + 3] = np.minimum(hi[:, 1], w - 1)
    fl[:, ROW_CENTRE:ROW_CENTRE + 2] = (ci.sum(axis=1) / 64.0).astype(np.float32)
    fl[:, ROW_FRAME:ROW_FRAME + 4] = frame
    fl[:, ROW_HEIGHT] = height
    rows[:, ROW_VALID] = 1
    rows[~ok] = 0
    return rows, ok


def char_label_maps_host(rows, count, h: int, w: int, box, sigma: float = 0.5):
    """The oracle of ``ops.char_label_maps``: ``rows`` (B, K, 20) int32, ``count`` (B,), the (h, w) map, the inclusive core
    box -> ``(owner int32, mask, height, score float32)``, each (B, CH, CW), cropped to the box.  As on the device, ``count``
    is clamped to [0, K], a row with ``valid == 0`` is skipped and a row's box is intersected with the crop, whatever it
    holds.  ``score`` is the float64 exp of the float32 ``a``, rounded once."""
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    if rows.ndim != 3 or rows.shape[2] != ROW_WORDS:
        raise ValueError(f'rows must be (B, K, {ROW_WORDS}), got {rows.shape}')
    B, K, _ = rows.shape
    count = np.asarray(count).reshape(-1)
    if len(count) != B:
        raise ValueError(f'count must be ({B},), got {count.shape}')
    up, down, left, right = _box4(box)
    if not (0 <= up <= down < h and 0 <= left <= right < w):
        raise ValueError(f'core box {(up, down, left, right)} outside the {(h, w)} map')
    CH, CW = down - up + 1, right - left + 1
    k = np.float32(1.0 / (2.0 * sigma * sigma))
    half = np.float32(0.5)
    fl = rows.view(np.float32)
    best = np.full((B, CH, CW), np.inf, dtype=np.float32)
    index = np.full((B, CH, CW), _INT_MAX, dtype=np.int64)
    hmap = np.zeros((B, CH, CW), dtype=np.float32)
    with np.errstate(all='ignore'):
        for b in range(B):
            for i in range(int(min(max(int(count[b]), 0), K))):
                r, rf = rows[b, i].astype(np.int64), fl[b, i]
                if r[ROW_VALID] == 0:
                    continue
                y0, x0 = max(r[ROW_BOX], up), max(r[ROW_BOX + 1], left)
                y1, x1 = min(r[ROW_BOX + 2], down), min(r[ROW_BOX + 3], right)
                if y0 > y1 or x0 > x1:
                    continue
                Y, X = np.arange(y0, y1 + 1)[:, None], np.arange(x0, x1 + 1)[None, :]
                py, px = 16 * Y + 8, 16 * X + 8
                inside = np.ones((y1 - y0 + 1, x1 - x0 + 1), dtype=bool)
                for j in range(4):
                    ay, ax, by, bx = r[2 * j], r[2 * j + 1], r[(2 * j + 2) % 8], r[(2 * j + 3) % 8]
                    inside &= (bx - ax) * (py - ay) - (by - ay) * (px - ax) >= 0
                dy = (Y.astype(np.float32) + half) - rf[ROW_CENTRE]
                dx = (X.astype(np.float32) + half) - rf[ROW_CENTRE + 1]
                s = rf[ROW_FRAME] * dy + rf[ROW_FRAME + 1] * dx
                t = rf[ROW_FRAME + 2] * dy + rf[ROW_FRAME + 3] * dx
                a = k * (s * s + t * t)
                win = (b, slice(y0 - up, y1 - up + 1), slice(x0 - left, x1 - left + 1))
                take = inside & ((a < best[win]) | ((a == best[win]) & (i < index[win])))
                best[win] = np.where(take, a, best[win])
                index[win] = np.where(take, i, index[win])
                hmap[win] = np.where(take, rf[ROW_HEIGHT], hmap[win])
        owned = index != _INT_MAX
        owner = np.where(owned, index + 1, 0).astype(np.int32)
        score = np.where(owned, np.exp(-best.astype(np.float64)), 0.0).astype(np.float32)
    return owner, owned.astype(np.float32), hmap, score


def _strictly_inside(quads: np.ndarray, py, px):
    """float64: all four edge functions of the (m, 4, 2) quads positive at their points (py, px) (m,)"""
    ok = np.ones(len(quads), dtype=bool)
    for j in range(4):
        a, b = quads[:, j], quads[:, (j + 1) % 4]
        ok &= (b[:, 1] - a[:, 1]) * (py - a[:, 0]) - (b[:, 0] - a[:, 0]) * (px - a[:, 1]) > 0
    return ok


def label_points(quads, valid, h: int, w: int, f: float, box, P: int, rng_seed: int, deviate: float = 0.5,
                 rng_stream: int = 0) -> Dict[str, np.ndarray]:
    """Exactly ``P`` label-point rows of one image (``P`` is the reference's ``num_page_char_regression_labels``), float64 on
    the host.  A map pixel (y, x) is a candidate for quad q iff it lies in the core box and its regression origin p = (y f,
    x f) - in image pixels, the one ``vkas_char_polygons`` uses - lies strictly inside q.  A quad's centroid point is the
    pixel floor(c); a quad whose centroid point is no candidate yields no points.  With u usable quads in a seeded
    permutation, row j uses quad perm[j mod u]: the first pass takes the centroid points, later passes floor(c + s a + t b)
    with seeded s, t in [-deviate, deviate], falling back to the centroid point when that pixel is no candidate.  ``u == 0``
    raises ValueError.  Returns ``downsampled_label_point_y / _x`` (P,) int64, ``up_left_offsets`` (P, 2) int64 = trunc(ul -
    p) toward zero, ``corner_distances`` (P, 3) = |ur - p|, |dr - p|, |dl - p|, ``corner_angles`` (P, 4) = the clockwise
    angles between successive corner rays (the first ray goes to the TRUNCATED up-left position), mod 2 pi, over 2 pi, and
    ``quad_index`` (P,).  Applied to a row, precise_build_polygon returns ur, dr, dl to rounding and ul to under a pixel."""
    q = np.asarray(quads, dtype=np.float64).reshape(-1, 4, 2)
    valid = np.asarray(valid, dtype=bool).reshape(-1)
    if len(valid) != len(q):
        raise ValueError(f'valid must be ({len(q)},), got {valid.shape}')
    if P < 1:
        raise ValueError(f'P must be >= 1, got {P}')
    up, down, left, right = _box4(box)

    def candidates(idx, yx):
        """quads idx (m,) at the pixels yx (m, 2)"""
        y, x = yx[:, 0], yx[:, 1]
        return ((y >= max(up, 0)) & (y <= min(down, h - 1)) & (x >= max(left, 0)) & (x <= min(right, w - 1))
                & _strictly_inside(q[idx], y * float(f), x * float(f)))

    with np.errstate(all='ignore'):
        m = np.where(valid[:, None, None], q, 0.0) / f
    centre = m.mean(axis=1)
    fa = ((m[:, 1] + m[:, 2]) - (m[:, 0] + m[:, 3])) / 4.0
    fb = ((m[:, 3] + m[:, 2]) - (m[:, 0] + m[:, 1])) / 4.0
    cpt = np.floor(centre).astype(np.int64)
    usable = np.nonzero(valid & candidates(np.arange(len(q)), cpt))[0]
    u = len(usable)
    if u == 0:
        raise ValueError('label_points: no quad has a centroid point inside the core box: a precise sample needs one')
    perm = usable[np.argsort(prng.raw_u64(rng_seed, rng_stream, u, 0), kind='stable')]
    dev = ((2.0 * prng.uniform(rng_seed, rng_stream, 2 * P, 1) - 1.0) * deviate).reshape(P, 2)
    qi = perm[np.arange(P) % u]
    moved = np.floor(centre[qi] + dev[:, :1] * fa[qi] + dev[:, 1:] * fb[qi]).astype(np.int64)
    take = (np.arange(P) >= u) & candidates(qi, moved)
    yx = np.where(take[:, None], moved, cpt[qi])
    ys, xs = yx[:, 0].copy(), yx[:, 1].copy()
    p = np.stack([ys, xs], axis=1).astype(np.float64) * f
    c = q[qi]                                              # (P, 4, 2)
    offsets = np.trunc(c[:, 0] - p).astype(np.int64)
    rays = np.concatenate([offsets[:, None, :].astype(np.float64), c[:, 1:] - p[:, None, :]], axis=1)
    theta = np.arctan2(rays[..., 0], rays[..., 1])         # atan2(0, 0) = 0, as in the kernel
    angles = np.mod(np.roll(theta, -1, axis=1) - theta, _TWO_PI) / _TWO_PI
    return {'downsampled_label_point_y': ys, 'downsampled_label_point_x': xs, 'up_left_offsets': offsets,
            'corner_angles': angles, 'corner_distances': np.hypot(rays[:, 1:, 0], rays[:, 1:, 1]), 'quad_index': qi}


@attrs.define
class QuadSample:
    """One annotated page of one pass: the model-input image and its character quadrilaterals in its pixels."""
    image: np.ndarray                       # (H, W, 3) uint8
    quads: np.ndarray                       # (n, 4, 2) (y, x): up-left, up-right, down-right, down-left
    index: int = 0                          # the sample's number in its source: the stream of its label-point draws
    rng_state: Optional[Any] = None


def collate_quad_pass(quads: Sequence, indices: Sequence[int], rng_states: Sequence, image_shape: Tuple[int, int],
                      precise: bool, P: int, f: int, margin: int, rng_seed: int) -> Dict[str, Any]:
    """One pass of a collated quad batch without its ``image``: the quad tables, for the precise pass the five label-point
    arrays, and the batch-wide shape / core box / rng states.  ``quads[b]`` are the quadrilaterals of sample b in the pixels
    of its (H, W) = ``image_shape`` model input, ``indices[b]`` the stream of its label-point draws.  Shared by
    ``adaptive_scaling_quads_collate_fn`` and dataset/crops_batch.py::adaptive_scaling_pages_collate_fn."""
    H, W = image_shape
    if H % f or W % f:
        raise ValueError(f'image sides {(H, W)} must be multiples of f = {f}')
    h, w = H // f, W // f
    if h <= 2 * margin + 1 or w <= 2 * margin + 1:
        raise ValueError('margin leaves no core box')
    box = Box(up=margin, down=h - margin - 1, left=margin, right=w - margin - 1)
    tables = [quad_rows(q, h, w, f) for q in quads]
    K = max(1, max(len(r) for r, _ in tables))
    rows = np.zeros((len(tables), K, ROW_WORDS), dtype=np.int32)
    for b, (r, _) in enumerate(tables):
        rows[b, :len(r)] = r
    out = {'char_quad_rows': torch.from_numpy(rows),
           'char_quad_count': torch.tensor([len(r) for r, _ in tables], dtype=torch.int32)}
    if precise:
        pts = [label_points(q, ok, h, w, f, box, P, rng_seed, rng_stream=index)
               for q, index, (_, ok) in zip(quads, indices, tables)]
        for key, dtype in (('downsampled_label_point_y', np.int64), ('downsampled_label_point_x', np.int64),
                           ('up_left_offsets', np.int64), ('corner_angles', np.float32),
                           ('corner_distances', np.float32)):
            out[key] = torch.from_numpy(np.stack([p[key].astype(dtype) for p in pts]))
    out['downsampled_shape'] = (h, w)
    out['downsampled_core_box'] = box
    out['rng_states'] = list(rng_states)
    return out


def adaptive_scaling_quads_collate_fn(batch: Iterable[Tuple[QuadSample, QuadSample]], P: int, f: int = 2,
                                      margin: int = 10, rng_seed: int = 13371) -> Dict[str, Dict[str, Any]]:
    """``(rough QuadSample, precise QuadSample)`` pairs -> the collated batch of ``adaptive_scaling_dataset_collate_fn``
    without the two dense maps, plus the quad tables ``char_quad_rows`` (B, K, 20) int32 / ``char_quad_count`` (B,) int32
    (K = the batch's largest n, at least 1) that ``CharLabelRasterizer`` turns into them on the device.  Host only, so it
    is safe in DataLoader workers.  All images of a pass share one size whose sides are multiples of ``f``; the core box is
    the map minus ``margin`` pixels per side.  A precise sample needs a usable quad (``label_points``); a rough sample
    without characters is legal.  An invalid quad gets a ``valid = 0`` row: it is not rasterised and yields no label point
    (``quad_rows`` reports which ones to a caller who wants to know)."""
    pairs = list(batch)
    if not pairs:
        raise ValueError('empty batch')

    def one_pass(samples: Sequence[QuadSample], precise: bool) -> Dict[str, Any]:
        H, W = samples[0].image.shape[:2]
        if H % f or W % f:
            raise ValueError(f'image sides {(H, W)} must be multiples of f = {f}')
        for s in samples:
            if s.image.shape != (H, W, 3) or s.image.dtype != np.uint8:
                raise ValueError(f'images of a batch must all be {(H, W, 3)} uint8, got {s.image.shape} {s.image.dtype}')
        rest = collate_quad_pass([s.quads for s in samples], [s.index for s in samples], [s.rng_state for s in samples],
                                 (H, W), precise, P, f, margin, rng_seed)
        return {'image': torch.from_numpy(np.stack([s.image.transpose(2, 0, 1) for s in samples]).astype(np.float32)), **rest}

    return {'rough': one_pass([r for r, _ in pairs], False), 'precise': one_pass([p for _, p in pairs], True)}


def _finish(part: Dict[str, Any], mask, score) -> Dict[str, Any]:
    out = {k: v for k, v in part.items() if k not in ('char_quad_rows', 'char_quad_count')}
    out['downsampled_mask'], out['downsampled_score_map'] = mask, score
    return out


class CharLabelRasterizer:
    """Called in the main process on a batch of ``adaptive_scaling_quads_collate_fn``: uploads the quad tables (once per
    pass), launches ``ops.char_label_maps`` and returns the batch with ``downsampled_mask`` / ``downsampled_score_map`` of
    both passes as device tensors - (mask, height) for the rough pass, (mask, score) for the precise pass - and without the
    table keys: exactly the schema ``batch_to_device`` and ``TwoPassStep`` take."""

    def __init__(self, device, sigma: float = 0.5):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError(f'CharLabelRasterizer runs on the GPU, got device {self.device} (host route: char_labels_host)')
        self.sigma = float(sigma)

    def __call__(self, batch: Dict[str, Dict[str, Any]]) -> Dict[str, Dict[str, Any]]:
        from .. import ops
        out = {}
        for name in ('rough', 'precise'):
            part = batch[name]
            rows = part['char_quad_rows'].to(self.device, non_blocking=True)
            count = part['char_quad_count'].to(self.device, non_blocking=True)
            h, w = part['downsampled_shape']
            rough = name == 'rough'
            _, mask, height, score = ops.char_label_maps(rows, count, h, w, part['downsampled_core_box'], self.sigma,
                                                         with_height=rough, with_score=not rough)
            out[name] = _finish(part, mask, height if rough else score)
        return out


def char_labels_host(batch: Dict[str, Dict[str, Any]], sigma: float = 0.5) -> Dict[str, Dict[str, Any]]:
    """What ``CharLabelRasterizer`` returns, through ``char_label_maps_host`` and with host tensors: the slow route, for
    checks and for timing against."""
    out = {}
    for name in ('rough', 'precise'):
        part = batch[name]
        h, w = part['downsampled_shape']
        _, mask, height, score = char_label_maps_host(part['char_quad_rows'].numpy(), part['char_quad_count'].numpy(), h, w,
                                                      part['downsampled_core_box'], sigma)
        out[name] = _finish(part, torch.from_numpy(mask), torch.from_numpy(height if name == 'rough' else score))
    return out
