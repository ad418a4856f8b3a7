"""Quadrilaterals for the strip tests (tests/test_cpu_strips.py, tests/test_gpu_strips.py): corners as ``(y, x)`` rows in the
order up-left, up-right, down-right, down-left."""
import numpy as np


def picture(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, tuple(shape) + (3,), dtype=np.uint8)


def box(y0, x0, height, width):
    """The axis-aligned rectangle of ``height`` x ``width`` pixels at (y0, x0), read left to right."""
    return np.array([[y0, x0], [y0, x0 + width], [y0 + height, x0 + width], [y0 + height, x0]], np.float64)


def rect(cy, cx, length, height, angle):
    """A ``length`` x ``height`` rectangle about (cy, cx) whose reading direction is turned by ``angle`` (y pointing down)."""
    A = np.array([np.sin(angle), np.cos(angle)]) * length / 2
    D = np.array([np.cos(angle), -np.sin(angle)]) * height / 2
    C = np.array([cy, cx], np.float64)
    return np.stack([C - A - D, C + A - D, C + A + D, C - A + D])


def turned(quad, k):
    """The same rectangle with its corner list started k corners later: the text turned by k quarter turns."""
    return np.roll(np.asarray(quad, np.float64), -k, axis=0)


def block_mean(crop, n):
    """(n x n block sum + n*n/2) // (n*n) of an (H, W, 3) uint8 crop whose sides are multiples of n."""
    H, W = crop.shape[:2]
    s = crop.astype(np.int64).reshape(H // n, n, W // n, n, 3).sum(axis=(1, 3))
    return ((s + n * n // 2) // (n * n)).astype(np.uint8)
