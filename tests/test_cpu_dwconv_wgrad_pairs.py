"""The index algebra of dwconv7x7_wgrad_mfma_kernel (csrc/dwconv.hip), restated in NumPy fp64 where no GPU is needed.

The kernel walks the 22 staged input rows of a 16 x 32 tile as 11 pairs m = 0 .. 10 and issues one 16 x 16 x 32 matrix product
per channel and pair: D += A . B with
    A[i][k]     = dy tile row 2m - 6 + i, column k        (i < 8; the zero row outside the tile; rows i >= 8 are zero),
    B[k][j]     = staged x row 2m,     element k + j      (j < 7),        B[k][7]  = 1,
    B[k][8 + j] = staged x row 2m + 1, element k + j      (j < 7),        B[k][15] = 1 (ignored),
and reads the taps back as gw[ky][kx] = D[6 - ky][kx] + D[7 - ky][8 + kx], the bias gradient as D[3][7] + D[4][7].  This file
states exactly that, tile by tile, and compares it with autograd of F.conv2d(padding=3) for one channel.  Both sides are
fp64, so the bound of 1e-12 only absorbs the summation order (measured: below 1e-15 relative for the weights).  The bias sum is
set against sum |dy|, the scale of its rounding error: dy.sum() itself can cancel to nothing.
"""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

MTY, MTX = 16, 32          # tile
MIY = MTY + 6              # staged input rows
SHAPES = [(1, 1), (2, 1), (3, 70), (7, 7), (15, 31), (16, 32), (17, 33), (18, 9), (31, 64), (33, 65), (37, 53)]
BOUND = 1e-12


def paired_wgrad(x, dy):
    """x, dy: (H, W) fp64 -> (gw (7, 7), gb) by the paired formulation; one accumulator D for all tiles, as in a walker."""
    H, W = x.shape
    D = np.zeros((16, 16))
    for y0 in range(0, H, MTY):
        for x0 in range(0, W, MTX):
            xs = np.zeros((MIY, MTX + 8))       # staged x: row rr = image row y0 - 3 + rr, element e = image column x0 - 3 + e
            for rr in range(MIY):
                for e in range(MTX + 6):
                    gy, gx = y0 - 3 + rr, x0 - 3 + e
                    if 0 <= gy < H and 0 <= gx < W:
                        xs[rr, e] = x[gy, gx]
            dt = np.zeros((MTY, MTX))           # staged dy tile
            dt[:min(MTY, H - y0), :min(MTX, W - x0)] = dy[y0:y0 + MTY, x0:x0 + MTX]
            for m in range(MIY // 2):
                A = np.zeros((16, MTX))
                for i in range(8):
                    p = 2 * m - 6 + i
                    if 0 <= p < MTY:
                        A[i] = dt[p]
                Bm = np.zeros((MTX, 16))
                for k in range(MTX):
                    for j in range(7):
                        Bm[k, j] = xs[2 * m, k + j]
                        Bm[k, 8 + j] = xs[2 * m + 1, k + j]
                Bm[:, 7] = 1.0
                Bm[:, 15] = 1.0
                D += A @ Bm
    gw = np.zeros((7, 7))
    for ky in range(7):
        for kx in range(7):
            gw[ky, kx] = D[6 - ky, kx] + D[7 - ky, 8 + kx]
    return gw, D[3, 7] + D[4, 7]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_paired_formulation_matches_autograd(shape):
    H, W = shape
    g = torch.Generator().manual_seed(100 * H + W)
    x = torch.randn((1, 1, H, W), generator=g, dtype=torch.float64)
    dy = torch.randn((1, 1, H, W), generator=g, dtype=torch.float64)
    w = torch.zeros((1, 1, 7, 7), dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, None, padding=3).backward(dy)
    ref = w.grad[0, 0].numpy()
    gw, gb = paired_wgrad(x[0, 0].numpy(), dy[0, 0].numpy())
    scale = max(float(np.abs(ref).max()), 1e-300)
    rel = float(np.abs(gw - ref).max()) / scale
    bref = float(dy.sum())
    brel = abs(gb - bref) / max(float(dy.abs().sum()), 1e-300)
    print('paired wgrad %dx%d: weights rel %.2e, bias rel (of sum |dy|) %.2e' % (H, W, rel, brel))
    assert rel <= BOUND, (shape, rel)
    assert brel <= BOUND, (shape, gb, bref)

