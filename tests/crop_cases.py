"""Crop scenes shared by tests/test_cpu_crops.py and tests/test_gpu_crops*.py: the smallest outputs that reach every branch of
csrc/crops.hip (one tile, ragged tiles with plain stores, an unaligned plane, several sources in one arena) and the cases of
dataset/crops.py's rule (every log2n, rotations, crops partly and wholly outside the page, sub-pixel offsets with fy == 0 and
fx == 0, the photometric clamps, noise).  The oracle results are computed once per case and must not be modified."""
import functools
import math

import numpy as np

from vkit_ocr_model_adaptive_scaling_amd.dataset.crops import AnnotatedPage, affine_row, crop_host


def image(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def parallelogram(cy, cx, half_w, half_h, deg, shear=0.0):
    """up-left, up-right, down-right, down-left of a parallelogram about (cy, cx): a rectangle sheared along x, then turned
    clockwise (y down) by deg"""
    t = math.radians(deg)
    right, down = np.array([math.sin(t), math.cos(t)]), np.array([math.cos(t), -math.sin(t)])
    c = np.array([cy, cx], dtype=np.float64)
    top, bottom = c - half_h * down + shear * half_h * right, c + half_h * down - shear * half_h * right
    return np.array([top - half_w * right, top + half_w * right, bottom + half_w * right, bottom - half_w * right])


def inside(quad, py, px, grow=0.0):
    """float64: the points lie inside the convex clockwise quad moved outwards by ``grow`` pixels (inwards when negative)"""
    ok = np.ones(np.broadcast(py, px).shape, dtype=bool)
    for j in range(4):
        a, b = quad[j], quad[(j + 1) % 4]
        e = b - a
        ok &= (e[1] * (py - a[0]) - e[0] * (px - a[1])) / math.hypot(*e) >= -grow
    return ok


def painted_page(h, w, quads, seed=0):
    """a white page (light noise, 225..255) with the quads filled dark (0..30): every pixel whose centre lies inside"""
    rng = np.random.default_rng(seed)
    page = rng.integers(225, 256, (h, w, 3), dtype=np.uint8)
    py, px = np.mgrid[0:h, 0:w] + 0.5
    for q in quads:
        m = inside(np.asarray(q, dtype=np.float64), py, px)
        page[m] = rng.integers(0, 31, (int(m.sum()), 3), dtype=np.uint8)
    return page


def synthetic_page(seed, h, w, char_h, index):
    """an annotated page of ``h x w`` with rows of dark parallelogram characters about ``char_h`` px high"""
    rng = np.random.default_rng(seed)
    quads, half_h, half_w = [], char_h / 2, char_h * 0.35
    y = char_h
    while y + char_h < h:
        x = char_h
        while x + char_h < w:
            quads.append(parallelogram(y + rng.uniform(-1, 1), x, half_w, half_h, rng.uniform(-8, 8), rng.uniform(-0.2, 0.2)))
            x += 2 * half_w + 0.45 * char_h
        y += 1.6 * char_h
    quads = np.array(quads)
    return AnnotatedPage(painted_page(h, w, quads, seed), quads, index)


PHOTO = {'off': {},
         'gain0': dict(gain=(0.0, 0.0, 0.0), bias=(40.0, -3.0, 250.0), noise_amp=8.0, noise_key=0x1234567890ABCDEF),
         'clamps': dict(gain=(4.0, 1.0, 0.25), bias=(100.0, -300.0, 0.0), noise_amp=0.0, noise_key=5),
         'noise': dict(gain=(1.1, 0.95, 1.0), bias=(-12.5, 3.25, 0.0), noise_amp=6.5, noise_key=-987654321)}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(sources, rows (B, 16) int64, size, ref (B, 3, H, W) float32)"""
    rad = math.radians
    if name == 'one_tile':     # every log2n, the rotations, every photometric variant
        size, sources = (16, 64), [image(1, 60, 90)]
        rows = [affine_row(size, 1.0, 0.0, (30.0, 45.0), **PHOTO['off']),
                affine_row(size, 0.5, rad(5), (30.0, 45.0), **PHOTO['noise']),
                affine_row(size, 0.25, rad(-5), (28.3, 47.7), **PHOTO['clamps']),
                affine_row(size, 0.125, rad(90), (30.0, 45.0), **PHOTO['gain0']),
                affine_row(size, 2.0, rad(180), (31.25, 44.5), **PHOTO['off'])]
    elif name == 'ragged_37x70':  # plain stores; outside the page; taps with fy == 0 / fx == 0
        size, sources = (37, 70), [image(2, 50, 64)]
        rows = [affine_row(size, 1.0, 0.0, (18.5, 35.25), **PHOTO['off']),       # integer rows, quarter columns: fy == 0
                affine_row(size, 1.0, 0.0, (18.75, 35.0), **PHOTO['noise']),     # fx == 0
                affine_row(size, 1.0, rad(180), (0.0, 0.0), **PHOTO['off']),     # three quarters outside
                affine_row(size, 0.7, rad(5), (-400.0, 900.0), **PHOTO['noise']),  # wholly outside: bias and noise only
                affine_row(size, 3.0, rad(90), (49.0, 63.0), **PHOTO['clamps']),
                affine_row(size, 0.3, rad(-90), (25.0, 32.0), log2n=2, **PHOTO['off'])]
    elif name == 'unaligned_32x128':
        size, sources = (32, 128), [image(3, 40, 150)]
        rows = [affine_row(size, 1.0, rad(-5), (20.0, 75.0), **PHOTO['noise']),
                affine_row(size, 0.6, rad(5), (20.0, 75.0), **PHOTO['clamps'])]
    elif name == 'batch3':     # three sources of different sizes in one arena, two rows sharing one
        size, sources = (32, 64), [image(4, 1, 1), image(5, 5, 8192), image(6, 300, 200)]
        rows = [affine_row(size, 1.0, rad(5), (150.0, 100.0), source=2, **PHOTO['noise']),
                affine_row(size, 8.0, 0.0, (0.5, 0.5), source=0, **PHOTO['off']),
                affine_row(size, 0.125, rad(-5), (2.5, 8000.0), source=1, **PHOTO['off']),
                affine_row(size, 0.5, rad(180), (290.0, 10.0), source=2, **PHOTO['gain0'])]
    else:
        raise KeyError(name)
    rows = np.stack(rows)
    rows.setflags(write=False)
    ref = crop_host(sources, rows, size)
    ref.setflags(write=False)
    return dict(sources=sources, rows=rows, size=size, ref=ref)


CASES = ('one_tile', 'ragged_37x70', 'unaligned_32x128', 'batch3')
