"""Blur for the training crops of dataset/crops.py: the rule, its host oracle, the table builders and the draws (numpy only,
worker-safe).  Defocus, camera shake and soft scans are the degradation a text detector meets most on real pages; the
reference gets them from vkit's page synthesis, which is absent here.  A crop is blurred between its geometric value and its
photometric jitter, by one small table of integer weights per sample, so that the device kernels (csrc/crops.hip,
``ops.crop_warp_blur``) and ``crop_blur_host`` are held to each other bit for bit.  The geometry does not change: quads, label
points and the rasteriser never see the blur.

A **blur row** is 226 int32:
    0        the radius ``R`` in [0, 7]
    1..225   a 15 x 15 weight table, row-major, centred at (7, 7)
It is valid when every weight is in [0, 65536], every weight outside the central ``(2R + 1)^2`` square is 0 and the weights sum
to exactly 65536.  ``R = 0`` with the centre weight 65536 is "no blur".

The pixel rule (``crop_blur_host``).  ``v_c(i, j)`` is the geometric value of ``crop_host`` for channel c at crop cell
``(i, j)``, which may lie outside ``[0, H) x [0, W)``: the row's affine map simply continues there - the same integer rule, the
same ``log2n``, zero outside the PAGE; neither a clamp nor a zero border of the crop.  Then
``acc = sum over a, b in [-R, R] of w[7 + a][7 + b] * v_c(y + a, x + b)``, an integer of at most 255 * 65536 < 2^24, so that
``vb = float32(acc) * 2^-16`` is exact, and the photometric steps of ``crop_host`` run on ``vb`` instead of ``float(v)``, word
for word: ``t = gain * vb``, ``+ bias``, ``+ amp * r``, the same clamp, the same ``noise_unit`` index.  So with ``R = 0`` the
result is ``crop_host``'s bit for bit, a region whose ``v`` is constant over the window keeps that constant exactly, and a
single 255 pixel under the identity map reproduces the mirrored weight table as ``255 * w * 2^-16``.

The bounds of a crop row hold over the halo: ``check_crop_rows`` (as ``WarpRow::ok`` of csrc/warp_pixel.h) bounds ``|ay|, |ax| <
2^40`` and ``|m| <= 2^22`` for cells in [0, 8192); for ``i, j`` in [-7, 8192 + 7) the coordinate is ``|Y| < 2^40 + 2 * 8199 * 2^22
< 2^40 + 2^36 + 2^26``: no intermediate leaves 64 bits, and a tap outside the page still reads 0."""
import math
from typing import Any, Dict, Optional, Sequence, Tuple

import attrs
import numpy as np

from ..inferencing.packing import SIDE_MAX, _warp_samples
from ..utils import portable_rng as prng
from .crops import (KINDS, ROW_AMP, ROW_AY, ROW_BIAS, ROW_GAIN, ROW_KEY, ROW_LOG2N, ROW_MXX, ROW_SOURCE, ROW_WORDS, _LANE0,
                    _bits_f32, _row_in_bounds, check_crop_rows, noise_unit)

BLUR_WORDS = 226
BLUR_RADIUS_MAX = 7
BLUR_SIDE = 2 * BLUR_RADIUS_MAX + 1
BLUR_ONE = 65536
BLUR_KINDS = ('gaussian', 'defocus', 'motion')
MOTION_POINTS = 256
_OFFSETS = np.arange(BLUR_SIDE) - BLUR_RADIUS_MAX


@attrs.define
class BlurConfig:
    """How the blur of a crop is drawn; every length is in crop pixels, for both kinds of crop."""
    prob: float = 0.0                                   # the share of the crops that are blurred
    kind_weights: Tuple[float, float, float] = (1.0, 1.0, 1.0)   # gaussian, defocus, motion
    gaussian_sigma: Tuple[float, float] = (0.5, 2.3)    # ceil(3 * 2.3) = 7
    defocus_radius: Tuple[float, float] = (1.0, 6.5)
    motion_length: Tuple[float, float] = (3.0, 15.0)    # the angle is uniform in [0, pi)

    def check(self) -> 'BlurConfig':
        if not 0.0 <= self.prob <= 1.0:
            raise ValueError(f'BlurConfig: prob must be in [0, 1], got {self.prob}')
        w = tuple(float(v) for v in self.kind_weights)
        if len(w) != 3 or min(w) < 0 or not sum(w) > 0:
            raise ValueError(f'BlurConfig: kind_weights must be three weights at or above 0, one of them positive, got {w}')
        for name, (lo, hi), low, high in (('gaussian_sigma', self.gaussian_sigma, 0.1, 7.0 / 3),
                                          ('defocus_radius', self.defocus_radius, 0.125, 7.5),
                                          ('motion_length', self.motion_length, 1.0, 15.0)):
            if not low <= lo <= hi <= high:   # the ranges within which every builder stays inside radius 7
                raise ValueError(f'BlurConfig: {name} must be an ordered pair within [{low:g}, {high:g}], got {(lo, hi)}')
        return self


def _quantise(p: np.ndarray, radius: Optional[int] = None) -> np.ndarray:
    """The shared last step of the builders: (15, 15) float64 weights ``p >= 0`` -> a blur row.  ``floor(65536 * p / sum p)``,
    the remainder to the centre weight: the sum is exact, and cells whose ``p`` are equal get equal weights.  ``radius``: the
    smallest one that holds every non-zero cell of ``p`` unless given."""
    p = np.asarray(p, dtype=np.float64)
    if p.shape != (BLUR_SIDE, BLUR_SIDE) or not np.isfinite(p).all() or (p < 0).any() or not p.sum() > 0:
        raise ValueError('a blur table needs (15, 15) finite weights at or above 0 with a positive sum')
    if radius is None:
        a, b = np.nonzero(p)
        radius = int(max(np.abs(a - BLUR_RADIUS_MAX).max(), np.abs(b - BLUR_RADIUS_MAX).max()))
    w = np.floor(BLUR_ONE * (p / p.sum())).astype(np.int64)
    w[BLUR_RADIUS_MAX, BLUR_RADIUS_MAX] += BLUR_ONE - int(w.sum())
    row = np.empty((BLUR_WORDS,), np.int32)
    row[0], row[1:] = radius, w.reshape(-1)
    return check_blur_rows(row[None])[0]


def identity_blur_row() -> np.ndarray:
    row = np.zeros((BLUR_WORDS,), np.int32)
    row[1 + BLUR_RADIUS_MAX * BLUR_SIDE + BLUR_RADIUS_MAX] = BLUR_ONE
    return row


def gaussian_blur_row(sigma: float) -> np.ndarray:
    """``p = exp(-(a^2 + b^2) / (2 sigma^2))`` inside the radius ``min(7, ceil(3 sigma))``."""
    sigma = float(sigma)
    if not sigma > 0 or not math.isfinite(sigma):
        raise ValueError(f'gaussian_blur_row: sigma must be positive, got {sigma}')
    radius = min(BLUR_RADIUS_MAX, math.ceil(3 * sigma))
    d2 = (_OFFSETS[:, None] ** 2 + _OFFSETS[None, :] ** 2).astype(np.float64)
    inside = (np.abs(_OFFSETS)[:, None] <= radius) & (np.abs(_OFFSETS)[None, :] <= radius)
    return _quantise(np.where(inside, np.exp(-d2 / (2 * sigma * sigma)), 0.0), radius)


def defocus_blur_row(rho: float) -> np.ndarray:
    """A disc of radius ``rho`` (rounded to 1/16 px): ``p`` of a cell is the count of its 8 x 8 sub-cell centres inside the disc,
    counted in integers - in units of 1/16 px the centres of cell ``a`` are ``16 a - 7 + 2 k``, ``k`` in [0, 8)."""
    r16 = int(round(float(rho) * 16))
    if not 2 <= r16 <= 120:   # below, no sub-cell centre lies inside; above, the disc leaves radius 7
        raise ValueError(f'defocus_blur_row: rho must be in [0.125, 7.5], got {rho}')
    c = (16 * _OFFSETS[:, None] - 7 + 2 * np.arange(8)[None, :]).reshape(-1)      # 120 sub-cell centres per axis
    inside = c[:, None] ** 2 + c[None, :] ** 2 <= r16 * r16
    return _quantise(inside.reshape(BLUR_SIDE, 8, BLUR_SIDE, 8).sum(axis=(1, 3)))


def motion_blur_row(length: float, angle: float) -> np.ndarray:
    """A straight stroke that covers ``length`` pixels (at most 15) at ``angle`` (radians from the x axis towards y): 256
    equally spaced points on the centred segment between the centres of its end pixels - ``length - 1`` long, so that
    ``length = 1`` is no blur and ``length = 15`` reaches the table's edge -, each splatted bilinearly."""
    length, angle = float(length), float(angle)
    if not 1.0 <= length <= BLUR_SIDE or not math.isfinite(angle):
        raise ValueError(f'motion_blur_row: length must be in [1, {BLUR_SIDE}], got {length}')
    t = ((np.arange(MOTION_POINTS) + 0.5) / MOTION_POINTS - 0.5) * (length - 1.0)
    p = np.zeros((BLUR_SIDE + 1, BLUR_SIDE + 1), np.float64)    # a guard row and column take the zero-weight far taps
    y, x = BLUR_RADIUS_MAX + t * math.sin(angle), BLUR_RADIUS_MAX + t * math.cos(angle)
    ky, kx = np.floor(y).astype(np.int64), np.floor(x).astype(np.int64)
    fy, fx = y - ky, x - kx
    for dy, wy in ((0, 1.0 - fy), (1, fy)):
        for dx, wx in ((0, 1.0 - fx), (1, fx)):
            np.add.at(p, (ky + dy, kx + dx), wy * wx)
    return _quantise(p[:BLUR_SIDE, :BLUR_SIDE])


def _blur_rows_bad(table: np.ndarray) -> np.ndarray:
    """(B,) bool: what makes a blur row invalid, as the device states it"""
    r = table[:, 0].astype(np.int64)
    w = table[:, 1:].astype(np.int64).reshape(-1, BLUR_SIDE, BLUR_SIDE)
    far = np.maximum(np.abs(_OFFSETS)[:, None], np.abs(_OFFSETS)[None, :])[None] > r[:, None, None]
    return ((r < 0) | (r > BLUR_RADIUS_MAX) | ((w < 0) | (w > BLUR_ONE)).any(axis=(1, 2)) | (far & (w != 0)).any(axis=(1, 2)) |
            (w.sum(axis=(1, 2)) != BLUR_ONE))


def check_blur_rows(blur_rows) -> np.ndarray:
    """Validates a (B, 226) blur-row table - integer words that fit int32, the radius in [0, 7], every weight in [0, 65536],
    zero outside the radius' square, the sum exactly 65536 - and returns it as contiguous int32.  Raises ValueError."""
    t = np.asarray(blur_rows)
    if t.ndim != 2 or t.shape[1] != BLUR_WORDS or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f'blur rows must be a (B, {BLUR_WORDS}) integer table, got {t.dtype} {t.shape}')
    if t.size and (t.min() < -(1 << 31) or t.max() >= 1 << 31):
        raise ValueError('blur rows: a word does not fit int32')
    t = np.ascontiguousarray(t.astype(np.int32))
    bad = np.nonzero(_blur_rows_bad(t))[0]
    if len(bad):
        raise ValueError(f'blur rows: row {int(bad[0])} is invalid (radius in [0, {BLUR_RADIUS_MAX}], weights in [0, {BLUR_ONE}], '
                         f'zero outside the radius, sum {BLUR_ONE})')
    return t


def _geometric(src: np.ndarray, row, i0: int, i1: int, j0: int, j1: int) -> np.ndarray:
    """``warp_host``'s uint8 for the crop cells [i0, i1) x [j0, j1) of a crop row, which may lie outside the crop: (rows,
    columns, 3) int64"""
    ay, ax, myy, myx, mxy, mxx = (int(v) for v in row[ROW_AY:ROW_MXX + 1])
    log2n = min(max(int(row[ROW_LOG2N]), 0), 3)
    n, shift = 1 << log2n, 32 + 2 * log2n
    i, j = np.arange(i0, i1, dtype=np.int64)[:, None], np.arange(j0, j1, dtype=np.int64)[None, :]
    Y, X = ay + i * myy + j * myx, ax + i * mxy + j * mxx
    total = np.zeros((i1 - i0, j1 - j0, 3), np.int64)
    for a in range(n):
        for b in range(n):
            ka, kb = 2 * a + 1 - n, 2 * b + 1 - n
            total += _warp_samples(src, Y + ((ka * myy + kb * myx) >> (1 + log2n)), X + ((ka * mxy + kb * mxx) >> (1 + log2n)))
    return (total + (1 << (shift - 1))) >> shift


def crop_blur_host(sources: Sequence[np.ndarray], rows, blur_rows, size: Tuple[int, int], strict: bool = True) -> np.ndarray:
    """The definition: (Hs, Ws, 3) uint8 pages, a (B, 16) crop-row table and a (B, 226) blur-row table -> (B, 3, H, W) float32,
    the pixel rule of the module docstring.  Plain and slow.  ``strict`` checks both tables; without it they are taken as the
    device takes unchecked ones: an image whose crop row cannot be trusted (``crop_host``) or whose blur row is invalid - the
    radius out of range, a weight out of range, a non-zero weight outside the square, a wrong sum - is zero."""
    H, W = (int(v) for v in size)
    if not (1 <= H <= SIDE_MAX and 1 <= W <= SIDE_MAX):
        raise ValueError(f'crop_blur_host: size sides must be in [1, {SIDE_MAX}], got {(H, W)}')
    mats = [np.asarray(s) for s in sources]
    for m in mats:
        if m.ndim != 3 or m.shape[2] != 3 or m.dtype != np.uint8:
            raise ValueError(f'crop_blur_host: a source must be (H, W, 3) uint8, got {m.dtype} {m.shape}')
    if strict:
        table = check_crop_rows(rows, [m.shape[:2] for m in mats])
        blur = check_blur_rows(blur_rows)
    else:
        table = np.ascontiguousarray(np.asarray(rows).astype(np.int64)).reshape(-1, ROW_WORDS)
        blur = np.ascontiguousarray(np.asarray(blur_rows).astype(np.int32)).reshape(-1, BLUR_WORDS)
    if len(blur) != len(table):
        raise ValueError(f'crop_blur_host: {len(table)} crop rows and {len(blur)} blur rows')
    bad = _blur_rows_bad(blur)
    out = np.zeros((len(table), 3, H, W), np.float32)
    for b, row in enumerate(table):
        s = int(row[ROW_SOURCE])
        if bad[b] or not (0 <= s < len(mats) and _row_in_bounds(row)):
            continue
        R = int(blur[b, 0])
        w = blur[b, 1:].astype(np.int64).reshape(BLUR_SIDE, BLUR_SIDE)
        v = _geometric(mats[s], row, -R, H + R, -R, W + R)
        acc = np.zeros((H, W, 3), np.int64)
        for a in range(-R, R + 1):
            for c in range(-R, R + 1):
                acc += w[BLUR_RADIUS_MAX + a, BLUR_RADIUS_MAX + c] * v[R + a:R + a + H, R + c:R + c + W]
        vb = acc.transpose(2, 0, 1).astype(np.float32) * np.float32(2.0 ** -16)
        gain, bias = _bits_f32(row[ROW_GAIN:ROW_GAIN + 3]), _bits_f32(row[ROW_BIAS:ROW_BIAS + 3])
        amp = _bits_f32(row[ROW_AMP:ROW_AMP + 1])[0]
        with np.errstate(all='ignore'):
            t = gain[:, None, None] * vb
            t = t + bias[:, None, None]
            t = t + amp * noise_unit(int(row[ROW_KEY]), (3, H, W))
            out[b] = np.where(t > 0, np.minimum(t, np.float32(255.0)), np.float32(0.0))
    return out


def blur_draw(kind: str, page, config, rng_seed: int, draw: int = 0) -> Dict[str, Any]:
    """The drawn blur of one crop (``config``: the crop's ``CropConfig``): ``blur`` (drawn or not), ``kind`` (of
    ``BLUR_KINDS``), ``size`` (sigma, disc radius or stroke length, crop pixels) and ``angle`` (radians, in [0, pi)).  The
    values are indices 13..17 of the very stream ``crop_draw`` reads - 13 decides blur or not, 14 the kind, 15 the size, 16 the
    angle, 17 is kept free -: the generator is counter based, so the first 13 values, and with them every crop row, do not
    move when blur is switched on."""
    if kind not in KINDS:
        raise ValueError(f'kind must be one of {KINDS}, got {kind!r}')
    if draw < 0 or page.index < 0:
        raise ValueError('draw and page.index must not be negative')
    cfg = config.blur
    if cfg is None:
        return {'blur': False, 'kind': None, 'size': 0.0, 'angle': 0.0}
    cfg.check()
    lane = _LANE0 + 2 * int(draw) + KINDS.index(kind)
    u = prng.uniform(rng_seed, page.index, 18, lane)[13:]
    weights = np.cumsum([float(v) for v in cfg.kind_weights])
    which = min(int(np.searchsorted(weights, float(u[1]) * weights[-1], side='right')), 2)
    lo, hi = (cfg.gaussian_sigma, cfg.defocus_radius, cfg.motion_length)[which]
    return {'blur': bool(float(u[0]) < cfg.prob), 'kind': BLUR_KINDS[which], 'size': lo + float(u[2]) * (hi - lo),
            'angle': float(u[3]) * math.pi}


def blur_row(kind: str, page, config, rng_seed: int, draw: int = 0) -> np.ndarray:
    """The blur row of ``blur_draw``'s parameters; the identity row when blur is off or not drawn."""
    d = blur_draw(kind, page, config, rng_seed, draw)
    if not d['blur']:
        return identity_blur_row()
    if d['kind'] == 'gaussian':
        return gaussian_blur_row(d['size'])
    if d['kind'] == 'defocus':
        return defocus_blur_row(d['size'])
    return motion_blur_row(d['size'], d['angle'])
