"""Quad scenes shared by tests/test_cpu_char_labels.py and tests/test_gpu_char_labels*.py: the smallest maps that reach every
branch of csrc/labels.hip (one tile, ragged tiles with scalar stores, a crop with 16-byte stores, a batch with an empty
image, two table chunks) and the quad cases of dataset/labels.py's rule (exact ties, pixel centres on an edge and on a
corner, a quad thinner than a pixel, quads partly and wholly outside the map and the crop, rotations).  Quads are given in
map pixels and scaled by ``f``; the oracle results are computed once per case and must not be modified."""
import functools
import math

import numpy as np

from vkit_ocr_model_adaptive_scaling_amd.dataset.labels import quad_rows, char_label_maps_host


def rect(y0, x0, y1, x1):
    """up-left, up-right, down-right, down-left of an axis-aligned box, (y, x)"""
    return [(y0, x0), (y0, x1), (y1, x1), (y1, x0)]


def rot(cy, cx, hw, hh, deg):
    """a rectangle of half width hw and half height hh turned clockwise (y down) by deg about (cy, cx)"""
    t = math.radians(deg)
    right, down = np.array([math.sin(t), math.cos(t)]), np.array([math.cos(t), -math.sin(t)])
    c = np.array([cy, cx], dtype=np.float64)
    return [tuple(c - hw * right - hh * down), tuple(c + hw * right - hh * down), tuple(c + hw * right + hh * down),
            tuple(c - hw * right + hh * down)]


def table(quad_lists, h, w, f=1, K=None):
    """per-image lists of quads in MAP pixels -> (rows (B, K, 20) int32, count (B,) int32); every quad must be valid"""
    tabs = []
    for quads in quad_lists:
        r, ok = quad_rows(np.asarray(quads, dtype=np.float64).reshape(-1, 4, 2) * f, h, w, f)
        assert ok.all(), 'a scene quad is invalid'
        tabs.append(r)
    K = max(1, max(len(r) for r in tabs)) if K is None else K
    rows = np.zeros((len(tabs), K, 20), dtype=np.int32)
    for b, r in enumerate(tabs):
        rows[b, :len(r)] = r
    return rows, np.array([len(r) for r in tabs], dtype=np.int32)


# the quad cases, placed on a map of at least 16 x 64
TIES = [rect(2, 2, 8, 11), rect(2, 2, 8, 11),          # identical: the lower index owns every pixel
        rect(9, 2, 15, 11), rect(9, 6, 15, 15)]        # mirrored about x = 8.5: pixel column 8 is equidistant
ON_CENTRES = [rect(2.5, 20.5, 6.5, 27.5)]              # corners at 16k + 8: pixel centres on every edge and corner
THIN = [rect(10.6, 20, 10.9, 30), rect(8, 30.55, 14, 30.95)]  # contain no pixel centre
OUTSIDE = [rect(-5, 36, 4, 47), rect(12, 58, 22, 70), rect(-20, -20, -10, -5), rect(5, 70, 9, 80), rect(30, 3, 40, 9)]
TURNED = [rot(8, 40, 7, 3.5, 30), rot(8, 54, 6, 2.5, 80)]
SCENE = TIES + ON_CENTRES + THIN + OUTSIDE + TURNED


def _shift(quads, dy, dx):
    return [[(y + dy, x + dx) for y, x in q] for q in quads]


def two_chunk_quads():
    """300 overlapping boxes on 48 x 192; quad 280 (second table chunk) lies over quad 0 and is nearer to pixel (5, 7)"""
    quads = [rect((i // 30) * 4.6, (i % 30) * 6.3, (i // 30) * 4.6 + 6, (i % 30) * 6.3 + 8) for i in range(300)]
    quads[280] = rect(2, 3, 8, 11)
    return quads


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(rows, count, h, w, box, f, ref=(owner, mask, height, score))"""
    f = 1
    if name == 'one_tile':
        h, w, box, lists = 16, 64, (0, 15, 0, 63), [SCENE]
    elif name == 'ragged_17x65':
        h, w, box, lists = 17, 65, (0, 16, 0, 64), [SCENE + [rect(14.2, 60.3, 16.9, 64.8)]]
    elif name == 'ragged_33x130':
        h, w, box = 33, 130, (0, 32, 0, 129)
        lists = [SCENE + _shift(SCENE, 17, 64) + [rot(24, 30, 12, 5, -30), rect(30.1, 120.2, 32.7, 129.6)]]
    elif name == 'crop_3_5':  # CH = 32, CW = 64: 16-byte stores at a shifted origin; f = 2
        h, w, box, f = 40, 80, (3, 34, 5, 68), 2
        lists = [SCENE + _shift(SCENE, 18, 6) + [rect(0, 0, 2.9, 4.9), rect(35, 69, 39, 79), rect(1, 1, 6, 9)]]
    elif name == 'batch3':    # counts (5, 0, K)
        h, w, box = 24, 72, (2, 21, 4, 67)
        lists = [SCENE[:5], [], SCENE]
    elif name == 'two_chunks':
        h, w, box, lists = 48, 192, (0, 47, 0, 191), [two_chunk_quads()]
    else:
        raise KeyError(name)
    rows, count = table(lists, h, w, f)
    for a in (rows, count):
        a.setflags(write=False)
    ref = char_label_maps_host(rows, count, h, w, box)
    for a in ref:
        a.setflags(write=False)
    return dict(rows=rows, count=count, h=h, w=w, box=box, f=f, ref=ref)


CASES = ('one_tile', 'ragged_17x65', 'ragged_33x130', 'crop_3_5', 'batch3', 'two_chunks')

# labels meet inference: quads at least 8 map pixels on a side and at least 6 apart, centres on pixel centres (so the
# centroid pixel holds score 1 and every other pixel less); map 48 x 96, f = 2
MEET = dict(h=48, w=96, f=2, box=(4, 43, 6, 89),
            quads=[rect(6, 10, 17, 23), rot(12.5, 40.5, 7, 4, 20), rot(13.5, 66.5, 6, 5, -35), rect(24, 8, 35, 27),
                   rot(33.5, 44.5, 8, 4, 75), rect(28, 62, 41, 73), rect(28, 80, 39, 89)])


def ulp_distance(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """distance in float32 steps between non-negative float32 arrays"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
