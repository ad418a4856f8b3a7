"""Blurred crop scenes shared by tests/test_cpu_blur.py and tests/test_gpu_crop_blur*.py: the smallest outputs that reach every
branch of the blur kernels of csrc/crops.hip (one tile, a halo of 7 that crosses tile borders on every side, ragged tiles with
plain stores, an unaligned plane, several sources and radii in one batch) and the cases of dataset/blur.py's rule (every log2n,
rotations, crops partly and wholly outside the page, the three kinds of table, the photometric clamps, noise).  The oracle
results are computed once per case and must not be modified."""
import functools
import math

import numpy as np

from tests.crop_cases import PHOTO, image
from vkit_ocr_model_adaptive_scaling_amd.dataset import (affine_row, crop_blur_host, defocus_blur_row, gaussian_blur_row,
                                                         identity_blur_row, motion_blur_row)


def radius_row(radius, seed):
    """a valid row of exactly this radius with uneven weights: no symmetry hides a transposed or mirrored table"""
    side = 2 * radius + 1
    p = np.zeros((15, 15))
    p[7 - radius:8 + radius, 7 - radius:8 + radius] = np.random.default_rng(seed).uniform(0.05, 1.0, (side, side))
    w = np.floor(65536 * p / p.sum()).astype(np.int64)
    w[7, 7] += 65536 - w.sum()
    return np.concatenate([[radius], w.reshape(-1)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(sources, rows (B, 16) int64, blur (B, 226) int32, size, ref (B, 3, H, W) float32)"""
    rad = math.radians
    if name == 'one_tile':       # every log2n (3 only here, for the oracle's time), the rotations, the three kinds
        size, sources = (16, 64), [image(1, 60, 90)]
        rows = [affine_row(size, 1.0, 0.0, (30.0, 45.0), **PHOTO['off']),
                affine_row(size, 0.5, rad(5), (30.0, 45.0), **PHOTO['noise']),
                affine_row(size, 0.25, rad(-5), (28.3, 47.7), **PHOTO['clamps']),
                affine_row(size, 0.125, rad(90), (30.0, 45.0), **PHOTO['gain0']),
                affine_row(size, 2.0, rad(180), (31.25, 44.5), **PHOTO['off'])]
        blur = [gaussian_blur_row(0.8), defocus_blur_row(2.0), motion_blur_row(7.0, 0.6), radius_row(2, 1), identity_blur_row()]
    elif name == 'halo_48x192':  # 3 x 3 tiles at R = 7: the window of the middle tile reaches into all eight neighbours
        size, sources = (48, 192), [image(2, 70, 230)]
        rows = [affine_row(size, 1.0, 0.0, (35.0, 115.0), **PHOTO['off']),
                affine_row(size, 0.7, rad(5), (30.0, 100.0), **PHOTO['noise']),
                affine_row(size, 1.5, rad(-5), (40.0, 120.0), **PHOTO['clamps'])]
        blur = [radius_row(7, 2), gaussian_blur_row(2.3), defocus_blur_row(6.5)]
    elif name == 'ragged_37x70':  # plain stores; crops partly and wholly outside the page
        size, sources = (37, 70), [image(3, 50, 64)]
        rows = [affine_row(size, 1.0, 0.0, (18.5, 35.25), **PHOTO['off']),
                affine_row(size, 1.0, rad(180), (0.0, 0.0), **PHOTO['off']),       # three quarters outside
                affine_row(size, 0.7, rad(5), (-400.0, 900.0), **PHOTO['noise']),  # wholly outside: bias and noise only
                affine_row(size, 3.0, rad(90), (49.0, 63.0), **PHOTO['clamps']),
                affine_row(size, 0.3, rad(-90), (25.0, 32.0), log2n=2, **PHOTO['off'])]
        blur = [radius_row(5, 3), motion_blur_row(15.0, 2.2), gaussian_blur_row(1.0), defocus_blur_row(3.3), radius_row(6, 4)]
    elif name == 'unaligned_32x128':
        size, sources = (32, 128), [image(4, 40, 150)]
        rows = [affine_row(size, 1.0, rad(-5), (20.0, 75.0), **PHOTO['noise']),
                affine_row(size, 0.6, rad(5), (20.0, 75.0), **PHOTO['clamps'])]
        blur = [radius_row(4, 5), motion_blur_row(9.0, 1.0)]
    elif name == 'batch4':       # radii 0, 1, 3, 7, the kinds mixed, three sources of different sizes, two rows sharing one
        size, sources = (32, 64), [image(5, 1, 1), image(6, 23, 37), image(7, 300, 200)]
        rows = [affine_row(size, 1.0, rad(5), (150.0, 100.0), source=2, **PHOTO['noise']),
                affine_row(size, 8.0, 0.0, (0.5, 0.5), source=0, **PHOTO['off']),
                affine_row(size, 1.0, rad(-5), (11.0, 18.0), source=1, **PHOTO['clamps']),
                affine_row(size, 0.5, rad(180), (290.0, 10.0), source=2, **PHOTO['gain0'])]
        blur = [identity_blur_row(), motion_blur_row(3.0, 0.0), gaussian_blur_row(1.0), defocus_blur_row(7.0)]
    else:
        raise KeyError(name)
    rows, blur = np.stack(rows), np.stack(blur)
    ref = crop_blur_host(sources, rows, blur, size)
    for a in (rows, blur, ref):
        a.setflags(write=False)
    return dict(sources=sources, rows=rows, blur=blur, size=size, ref=ref)


CASES = ('one_tile', 'halo_48x192', 'ragged_37x70', 'unaligned_32x128', 'batch4')
