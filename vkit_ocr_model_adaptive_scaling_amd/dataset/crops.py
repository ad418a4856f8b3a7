"""Training crops from annotated pages: the rule, its host oracle and the row builder (numpy only, worker-safe).

The reference cuts its samples out of synthetic pages with vkit's ``page_cropping`` and ``page_text_region_cropping``
(dataset/adaptive_scaling.py:84-146): a rough sample is a crop at page scale, a precise sample a crop in which the characters
have been rescaled to about 35 px.  vkit and cv2 are absent here, so the step is restated as ONE affine map per sample - a
similarity: scale, a small rotation, a translation - sampled by the integer rule of inferencing/packing.py::warp_host, then a
photometric jitter in float32 without contraction, so that the device kernel (csrc/crops.hip, ``ops.crop_warp``) and
``crop_host`` are held to each other bit for bit.  No perspective, JPEG or page synthesis (blur: dataset/blur.py); outside the
page a crop is zero padded, and bias and noise still apply there.

A **crop row** is 16 int64:
    0       source: the index of the page in the batch's source list
    1, 2    ay, ax      Q16: destination pixel (i, j) of the (H, W) crop reads the page at the sample coordinates
    3..6    myy, myx, mxy, mxx   ``Y = ay + i*myy + j*myx``, ``X = ax + i*mxy + j*mxx`` - ``warp_host``'s row for a destination at
            (0, 0) of the crop's size; an integer coordinate is a pixel centre
    7       log2n: ``2^log2n`` sub-samples per axis (``inferencing.orient.warp_log2n`` of the scale)
    8..10   float32 bits (low 32, the high 32 are zero) of the gains of the channels
    11..13  float32 bits of their biases
    14      float32 bits of the noise amplitude
    15      noise_key, a 64-bit integer

The pixel rule (``crop_host``).  The geometric value ``v`` of a pixel and channel is exactly ``warp_host``'s uint8: ``n x n``
bilinear sub-samples, zero weight outside the page, one rounding.  Then in float32, every product and sum rounded once, no
fma: ``t = gain_c * float(v)``; ``t = t + bias_c``; ``t = t + amp * r``; the result is ``min(t, 255)`` where ``t > 0`` and ``+0``
elsewhere (``min(max(t, 0), 255)`` with the sign of a zero and a NaN settled).  ``r = float(u >> 40) * 2^-23 - 1`` (exact, in
``[-1, 1)``) with ``u = mix((idx + 1) * GOLD + noise_key)`` in 64-bit wrapping arithmetic, ``idx = (c*H + y)*W + x`` and ``mix``
the splitmix64 finaliser of ``utils/portable_rng``."""
import math
from typing import Any, Dict, Iterable, Optional, Sequence, Tuple

import attrs
import numpy as np

from ..inferencing.orient import warp_log2n
from ..inferencing.packing import SIDE_MAX, WARP_A_MAX, WARP_M_MAX, warp_host
from ..utils import portable_rng as prng
from .labels import quad_rows

ROW_WORDS = 16
ROW_SOURCE, ROW_AY, ROW_AX, ROW_MYY, ROW_MYX, ROW_MXY, ROW_MXX, ROW_LOG2N = range(8)
ROW_GAIN, ROW_BIAS, ROW_AMP, ROW_KEY = 8, 11, 14, 15
KINDS = ('rough', 'precise')
_LANE0 = 2   # label_points draws from lanes 0 and 1 of stream ``index``: the crops take lanes 2 + 2*draw + kind
_GOLD = np.uint64(0x9E3779B97F4A7C15)


@attrs.define
class AnnotatedPage:
    """One annotated page: an image of any size up to 8192 per side and its character quadrilaterals in its pixels."""
    image: np.ndarray                       # (H, W, 3) uint8
    quads: np.ndarray                       # (n, 4, 2) (y, x): up-left, up-right, down-right, down-left
    index: int = 0                          # the page's number in its source: the stream of its draws


@attrs.define
class CropConfig:
    size: Tuple[int, int] = (1024, 1024)    # of the crop = the model input; sides multiples of 32
    rough_short_side: int = 720             # a rough crop shows the page shrunk to this short side (never enlarged)
    precise_char_height: float = 35.0       # a precise crop shows its anchor character at this height
    scale_jitter: Tuple[float, float] = (0.8, 1.25)   # log-uniform factor on the scale
    rotate_max_deg: float = 5.0
    scale_min: float = 1.0 / 8
    scale_max: float = 8.0
    core_margin: int = 20                   # image pixels per side that the core box leaves out: the collate's f * margin
    gain: Tuple[float, float] = (0.8, 1.2)
    channel_gain: float = 0.05              # +- relative, per channel
    bias: float = 20.0                      # +-, one draw for the three channels
    noise_amp: Tuple[float, float] = (0.0, 8.0)
    photometric: bool = True
    blur: Optional[Any] = None              # a dataset/blur.py::BlurConfig; None: every crop is as sharp as its page

    def check(self) -> 'CropConfig':
        H, W = (int(v) for v in self.size)
        if H < 32 or W < 32 or H % 32 or W % 32 or max(H, W) > SIDE_MAX:
            raise ValueError(f'CropConfig: size sides must be multiples of 32 in [32, {SIDE_MAX}], got {self.size}')
        if not 0 < self.scale_min <= self.scale_max or 65536.0 / self.scale_min > WARP_M_MAX:
            raise ValueError(f'CropConfig: bad scale range [{self.scale_min}, {self.scale_max}] (a step of at most 64 pixels)')
        if not 0 < self.scale_jitter[0] <= self.scale_jitter[1]:
            raise ValueError(f'CropConfig: bad scale_jitter {self.scale_jitter}')
        if not 0 <= self.rotate_max_deg <= 45 or self.precise_char_height <= 0 or self.rough_short_side < 1:
            raise ValueError('CropConfig: rotate_max_deg in [0, 45], precise_char_height and rough_short_side positive')
        if self.core_margin < 0 or 2 * self.core_margin + 2 >= min(H, W):
            raise ValueError(f'CropConfig: core_margin {self.core_margin} leaves no core box in {(H, W)}')
        if self.blur is not None:
            self.blur.check()
        return self


def _f32_bits(x) -> int:
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def _bits_f32(words) -> np.ndarray:
    return (np.asarray(words, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


def _page_mat(page: AnnotatedPage) -> np.ndarray:
    m = np.asarray(page.image)
    if m.ndim != 3 or m.shape[2] != 3 or m.dtype != np.uint8:
        raise ValueError(f'a page image must be (H, W, 3) uint8, got {m.dtype} {m.shape}')
    if min(m.shape[:2]) < 1 or max(m.shape[:2]) > SIDE_MAX:
        raise ValueError(f'page {m.shape[:2]}: sides from 1 to {SIDE_MAX}')
    return m


def crop_draw(kind: str, page: AnnotatedPage, config: CropConfig, rng_seed: int, draw: int = 0) -> Dict[str, Any]:
    """The drawn parameters of one crop, float64: ``scale`` (after the clamp), ``clamped``, ``theta`` (radians), ``centre`` (y,
    x) in page positions (pixel k covers [k, k + 1)), ``anchor`` (the index of the anchor quad, -1 for a rough crop), and the
    photometric ``gain`` (3), ``bias`` (3), ``noise_amp``, ``noise_key``.  All randomness is ``utils/portable_rng`` keyed by
    ``(rng_seed, page.index, draw, kind)``; exp, log, sin and cos are the host's, whose last-bit differences the rounding of
    the row to Q16 absorbs."""
    if kind not in KINDS:
        raise ValueError(f'kind must be one of {KINDS}, got {kind!r}')
    config.check()
    if draw < 0 or page.index < 0:
        raise ValueError('draw and page.index must not be negative')
    H, W = (int(v) for v in config.size)
    Hp, Wp = _page_mat(page).shape[:2]
    lane = _LANE0 + 2 * int(draw) + KINDS.index(kind)
    u = prng.uniform(rng_seed, page.index, 13, lane)
    lo, hi = (math.log(v) for v in config.scale_jitter)
    jitter = math.exp(lo + float(u[0]) * (hi - lo))
    theta = math.radians((2.0 * float(u[1]) - 1.0) * config.rotate_max_deg)
    anchor = -1
    if kind == 'rough':
        scale = min(1.0, config.rough_short_side / min(Hp, Wp)) * jitter
    else:
        quads = np.asarray(page.quads, dtype=np.float64).reshape(-1, 4, 2)
        rows, ok = quad_rows(quads, Hp, Wp, 1.0)
        usable = np.nonzero(ok)[0]
        if len(usable) == 0:
            raise ValueError('crop_row: a precise crop needs a page with a valid quad')
        anchor = int(usable[min(int(float(u[4]) * len(usable)), len(usable) - 1)])
        height = float(rows[anchor:anchor + 1].view(np.float32)[0, 18])
        scale = config.precise_char_height * jitter / height
    clamped = not config.scale_min <= scale <= config.scale_max
    scale = min(max(scale, config.scale_min), config.scale_max)
    if kind == 'rough':
        centre = (float(u[2]) * Hp, float(u[3]) * Wp)
    else:
        # where the anchor's centroid lands in the crop: uniform over the core box, a pixel inside its edge
        m = config.core_margin + 1
        ty, tx = m + float(u[2]) * (H - 2 * m), m + float(u[3]) * (W - 2 * m)
        c = quads[anchor].mean(axis=0)
        oy, ox = (H / 2 - ty) / scale, (W / 2 - tx) / scale      # the crop centre's offset from it, turned into the page
        centre = (c[0] + math.cos(theta) * oy - math.sin(theta) * ox, c[1] + math.sin(theta) * oy + math.cos(theta) * ox)
    out = {'kind': kind, 'scale': scale, 'clamped': clamped, 'theta': theta, 'centre': centre, 'anchor': anchor}
    if config.photometric:
        g = config.gain[0] + float(u[5]) * (config.gain[1] - config.gain[0])
        out['gain'] = [g * (1.0 + (2.0 * float(u[6 + c]) - 1.0) * config.channel_gain) for c in range(3)]
        out['bias'] = [(2.0 * float(u[9]) - 1.0) * config.bias] * 3
        out['noise_amp'] = config.noise_amp[0] + float(u[10]) * (config.noise_amp[1] - config.noise_amp[0])
    else:
        out['gain'], out['bias'], out['noise_amp'] = [1.0] * 3, [0.0] * 3, 0.0
    out['noise_key'] = int(prng.raw_u64(rng_seed, page.index, 12, lane)[11].view(np.int64))
    return out


def affine_row(size: Tuple[int, int], scale: float, theta: float, centre: Tuple[float, float], source: int = 0,
               gain: Sequence[float] = (1.0, 1.0, 1.0), bias: Sequence[float] = (0.0, 0.0, 0.0), noise_amp: float = 0.0,
               noise_key: int = 0, log2n: Optional[int] = None) -> np.ndarray:
    """The 16 int64 of one crop: the (H, W) crop shows the page scaled by ``scale`` and turned by ``theta`` about ``centre`` (a
    page position).  The linear part is ``R(theta) / scale`` rounded to Q16; the anchor is placed as ``warp_row`` places it,
    so that the crop's centre is exact and the rounding of the coefficients is split between the two ends."""
    H, W = (int(v) for v in size)
    c, s = math.cos(theta) / scale, math.sin(theta) / scale
    myy, myx, mxy, mxx = round(65536 * c), round(-65536 * s), round(65536 * s), round(65536 * c)
    ay = round(65536 * (centre[0] - 0.5) - ((H - 1) * myy + (W - 1) * myx) / 2)
    ax = round(65536 * (centre[1] - 0.5) - ((H - 1) * mxy + (W - 1) * mxx) / 2)
    row = np.zeros((ROW_WORDS,), np.int64)
    row[:8] = (source, ay, ax, myy, myx, mxy, mxx, warp_log2n(scale) if log2n is None else log2n)
    row[ROW_GAIN:ROW_GAIN + 3] = [_f32_bits(g) for g in gain]
    row[ROW_BIAS:ROW_BIAS + 3] = [_f32_bits(b) for b in bias]
    row[ROW_AMP] = _f32_bits(noise_amp)
    row[ROW_KEY] = np.array([int(noise_key) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64).view(np.int64)[0]
    return row


def crop_row(kind: str, page: AnnotatedPage, config: CropConfig, rng_seed: int, draw: int = 0, source: int = 0) -> np.ndarray:
    """The crop row of ``crop_draw``'s parameters.  *rough*: the page shrunk to ``rough_short_side`` (never enlarged) times
    the jitter, centred uniformly over the page.  *precise*: an anchor drawn among the page's valid quads (``quad_rows``'
    validity and height) shown at ``precise_char_height`` times the jitter, its centroid uniform over the crop's core box.
    The scale is clamped to ``[scale_min, scale_max]``, the angle uniform in ``+-rotate_max_deg``.  The same arguments give
    the same row; a page without a valid quad raises ValueError for a precise crop."""
    d = crop_draw(kind, page, config, rng_seed, draw)
    return affine_row(config.size, d['scale'], d['theta'], d['centre'], source, d['gain'], d['bias'], d['noise_amp'],
                      d['noise_key'])


def check_crop_rows(rows, source_shapes) -> np.ndarray:
    """Validates a (B, 16) crop-row table against the (S, 2) source shapes (Hs, Ws) - integer rows, ``source`` in range,
    source sides in [1, SIDE_MAX], coefficients within ``WARP_M_MAX`` / ``WARP_A_MAX``, ``log2n`` in [0, 3], float words
    that hold 32 bits and finite gains, biases and amplitude - and returns it as contiguous int64.  Raises ValueError."""
    r = np.asarray(rows)
    if r.ndim != 2 or r.shape[1] != ROW_WORDS or not np.issubdtype(r.dtype, np.integer):
        raise ValueError(f'crop rows must be a (B, {ROW_WORDS}) integer table, got {r.dtype} {r.shape}')
    r = np.ascontiguousarray(r.astype(np.int64))
    shapes = np.asarray(source_shapes, dtype=np.int64).reshape(-1, 2)
    if ((shapes < 1) | (shapes > SIDE_MAX)).any():
        raise ValueError(f'crop rows: source sides must be in [1, {SIDE_MAX}]')
    if ((r[:, ROW_SOURCE] < 0) | (r[:, ROW_SOURCE] >= len(shapes))).any():
        raise ValueError(f'crop rows: a source index is outside [0, {len(shapes)})')
    if (np.abs(r[:, ROW_MYY:ROW_MXX + 1]) > WARP_M_MAX).any() or (np.abs(r[:, ROW_AY:ROW_AX + 1]) >= WARP_A_MAX).any():
        raise ValueError('crop rows: a coefficient exceeds 2^22 or an anchor reaches 2^40')
    if ((r[:, ROW_LOG2N] < 0) | (r[:, ROW_LOG2N] > 3)).any():
        raise ValueError('crop rows: log2n must be in [0, 3]')
    words = r[:, ROW_GAIN:ROW_AMP + 1]
    if ((words < 0) | (words > 0xFFFFFFFF)).any():
        raise ValueError('crop rows: a gain, bias or amplitude word does not hold float32 bits in its low 32')
    if not np.isfinite(_bits_f32(words)).all():
        raise ValueError('crop rows: a gain, bias or amplitude is not finite')
    return r


def _row_in_bounds(row) -> bool:
    """what csrc/crops.hip asks of a row's geometry before it samples (its source entry aside)"""
    return bool((np.abs(row[ROW_MYY:ROW_MXX + 1]) <= WARP_M_MAX).all() and (np.abs(row[ROW_AY:ROW_AX + 1]) < WARP_A_MAX).all())


def crop_quads(quads, row) -> np.ndarray:
    """(..., 2) (y, x) page positions -> float64 positions in the crop: the exact inverse of the row's integer map under
    the conventions of ``remap_polygons_affine`` (pixel k covers [k, k + 1), sample coordinate = position - 1/2).  Nothing is
    clipped or dropped: ``quad_rows`` clips boxes to the map and ``label_points`` restricts itself to the core box."""
    _, ay, ax, myy, myx, mxy, mxx = (int(v) for v in np.asarray(row).reshape(ROW_WORDS)[:7])
    det = myy * mxx - myx * mxy
    if det == 0:
        raise ValueError('crop_quads: the row is not invertible')
    p = np.asarray(quads, dtype=np.float64)
    ry, rx = 65536.0 * (p[..., 0] - 0.5) - ay, 65536.0 * (p[..., 1] - 0.5) - ax
    out = np.empty(p.shape, np.float64)
    out[..., 0] = (mxx * ry - myx * rx) / det + 0.5
    out[..., 1] = (myy * rx - mxy * ry) / det + 0.5
    return out


def page_positions(points, row) -> np.ndarray:
    """The forward map of a row, as ``remap_polygons_affine`` states it: (..., 2) crop positions -> page positions."""
    _, ay, ax, myy, myx, mxy, mxx = (int(v) for v in np.asarray(row).reshape(ROW_WORDS)[:7])
    p = np.asarray(points, dtype=np.float64)
    i, j = p[..., 0] - 0.5, p[..., 1] - 0.5
    out = np.empty(p.shape, np.float64)
    out[..., 0] = (ay + i * myy + j * myx) / 65536 + 0.5
    out[..., 1] = (ax + i * mxy + j * mxx) / 65536 + 0.5
    return out


def noise_unit(noise_key: int, shape: Tuple[int, int, int]) -> np.ndarray:
    """``r`` of the module docstring for a (3, H, W) image: float32 in [-1, 1), a multiple of 2^-23."""
    C, H, W = (int(v) for v in shape)
    key = np.array([int(noise_key) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)[0]
    with np.errstate(over='ignore'):
        idx = np.arange(C * H * W, dtype=np.uint64).reshape(C, H, W)
        u = prng._mix((idx + np.uint64(1)) * _GOLD + key)
    return (u >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)


def crop_host(sources: Sequence[np.ndarray], rows, size: Tuple[int, int], strict: bool = True) -> np.ndarray:
    """The definition: (Hs, Ws, 3) uint8 pages and a (B, 16) crop-row table -> (B, 3, H, W) float32, the pixel rule of the
    module docstring.  Plain and slow.  ``strict`` checks the table (``check_crop_rows``); without it the table is taken as
    the device takes an unchecked one: an image whose row has a source index outside the list or a coefficient out of
    bounds is zero, ``log2n`` is clamped to [0, 3] and only the low 32 bits of a float word count."""
    H, W = (int(v) for v in size)
    if not (1 <= H <= SIDE_MAX and 1 <= W <= SIDE_MAX):
        raise ValueError(f'crop_host: size sides must be in [1, {SIDE_MAX}], got {(H, W)}')
    mats = [np.asarray(s) for s in sources]
    for m in mats:
        if m.ndim != 3 or m.shape[2] != 3 or m.dtype != np.uint8:
            raise ValueError(f'crop_host: a source must be (H, W, 3) uint8, got {m.dtype} {m.shape}')
    if strict:
        table = check_crop_rows(rows, [m.shape[:2] for m in mats])
    else:
        table = np.ascontiguousarray(np.asarray(rows).astype(np.int64)).reshape(-1, ROW_WORDS)
    out = np.zeros((len(table), 3, H, W), np.float32)
    zero_page = np.zeros((H, W, 3), np.uint8)
    for b, row in enumerate(table):
        s = int(row[ROW_SOURCE])
        if not (0 <= s < len(mats) and _row_in_bounds(row)):
            continue
        warp = np.array([[0, 0, H, W, *row[ROW_AY:ROW_MXX + 1].tolist(), min(max(int(row[ROW_LOG2N]), 0), 3), 0]], np.int64)
        v = warp_host(mats[s], warp, zero_page).transpose(2, 0, 1).astype(np.float32)
        gain, bias = _bits_f32(row[ROW_GAIN:ROW_GAIN + 3]), _bits_f32(row[ROW_BIAS:ROW_BIAS + 3])
        amp = _bits_f32(row[ROW_AMP:ROW_AMP + 1])[0]
        with np.errstate(all='ignore'):
            t = gain[:, None, None] * v
            t = t + bias[:, None, None]
            t = t + amp * noise_unit(int(row[ROW_KEY]), (3, H, W))
            out[b] = np.where(t > 0, np.minimum(t, np.float32(255.0)), np.float32(0.0))
    return out
