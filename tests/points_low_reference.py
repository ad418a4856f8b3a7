"""Host restatement of vkas_points_scatter3x3_low (csrc/points.hip) with obvious loops, and the point sets its tests share.

D[i][t] is the input-gradient contribution of owner point i to the upsampled pixel q = pixel(i) + (ky-1, kx-1); the upsampled
map is U x with U the x2 bilinear upsample (align_corners=False, source coordinates clamped at the border), so the gradient of
x receives U[q, s] * D[i][t] at each of the (at most four) source pixels s that q reads.  Sums in fp64.
tests/test_cpu_points_low_reference.py holds this to autograd of F.interpolate; tests/test_gpu_points_low.py the kernel to this."""
import math

import numpy as np
import torch

from tests import points_reference as R


def sources(d, n):
    """[(source index, weight)] x 2 of destination d of a x2 bilinear upsample of n samples, as F.interpolate computes it"""
    c = max((d + 0.5) / 2.0 - 0.5, 0.0)
    i0 = int(math.floor(c))
    i1 = min(i0 + 1, n - 1)
    lam = c - i0
    return [(i0, 1.0 - lam), (i1, lam)]


def scatter3x3_low(D, pix, pmap, dx0):
    """D (Mp, 9, C); pix / pmap of the upsampled (2h x 2w) map; dx0 (B, h, w, C) -> fp64 (B, h, w, C)"""
    B, h, w, C = dx0.shape
    H, W = 2 * h, 2 * w
    out = dx0.double().clone()
    for i in range(len(pix)):
        q = int(pix[i])
        if q < 0:
            continue
        assert int(pmap[q]) == i
        b, y, xx = q // (H * W), (q // W) % H, q % W
        for t in range(9):
            ty, tx = y + t // 3 - 1, xx + t % 3 - 1
            if not (0 <= ty < H and 0 <= tx < W):
                continue
            for sy, wy in sources(ty, h):
                for sx, wx in sources(tx, w):
                    out[b, sy, sx] += (wy * wx) * D[i, t].double()
    return out


def point_sets(h, w):
    """{name: (py, px, Mp)} on the upsampled 2h x 2w map, B = 2: py, px (2, P) int64; Mp = B*P rounded up to 64"""
    H, W = 2 * h, 2 * w
    g = np.random.RandomState(1000 * h + w)
    sets = {}
    # the four corners, the middle of the four edges, one of them twice: the clamped weights; 18 points -> 46 padding rows
    ys = [0, 0, H - 1, H - 1, 0, H - 1, H // 2, H // 2, 0]
    xs = [0, W - 1, 0, W - 1, W // 2, W // 2, 0, W - 1, 0]
    sets['borders'] = (np.array([ys, ys[::-1]]), np.array([xs, xs[::-1]]))
    # all P points of an image on one pixel: a corner / the middle
    sets['one_pixel'] = (np.array([[0] * 5, [H // 2] * 5]), np.array([[0] * 5, [W // 2 - 1] * 5]))
    # a 6 x 6 block (cut at the map) in which every upsampled pixel is a point: the most contributors a source pixel can have
    y0, x0 = max(0, min(H - 6, 2 * (h // 2) - 2)), max(0, min(W - 6, 2 * (w // 2) - 2))
    by, bx = np.meshgrid(np.arange(y0, min(y0 + 6, H)), np.arange(x0, min(x0 + 6, W)), indexing='ij')
    by, bx = np.resize(by.reshape(-1), 36), np.resize(bx.reshape(-1), 36)  # a smaller map: the block again (duplicates)
    sets['block6'] = (np.array([by, by[::-1]]), np.array([bx, bx[::-1]]))
    # random with duplicates; 74 points -> Mp = 128
    ry, rx = g.randint(0, H, (2, 37)), g.randint(0, W, (2, 37))
    ry[:, 1], rx[:, 1] = ry[:, 0], rx[:, 0]
    sets['random'] = (ry, rx)
    out = {}
    for name, (py, px) in sets.items():
        py, px = py.astype(np.int64), px.astype(np.int64)
        n = py.size
        out[name] = (py, px, -(-n // 64) * 64)
    return out


def prepared(py, px, h, w, Mp):
    """(pmap, pix) of the upsampled map, as vkas_points_prepare writes them"""
    return R.prepare(py, px, 2, py.shape[1], 2 * h, 2 * w, Mp)
