"""The algebra behind the heads' backward at the neck's resolution (csrc/upconv_adj.hip, ops.UpHeadsFused), pinned in fp64 on
the host: for z = conv3x3(U x), U the x2 bilinear upsample (align_corners=False), the nine maps

    E_k[s, n] = sum_q U[q, s] * dz[q + (k - 1), n]          (zero where q + (k - 1) leaves the map)

give dx = sum_k E_k . Bt_k with Bt the dgrad weight image (taps rotated by 180 degrees: Bt_k = W[:, :, 8 - k]) and
dW[:, :, 8 - k] = E_k^T x - the autograd gradients of F.interpolate + F.conv2d, borders and odd sizes included."""
import pytest
import torch
from torch.nn import functional as F


def upsample_adjoint(g, h, w):
    """U^T g for g (B, N, 2h, 2w): the gradient of the x2 bilinear upsample with respect to its (B, N, h, w) input."""
    a = torch.zeros(g.shape[0], g.shape[1], h, w, dtype=g.dtype, requires_grad=True)
    up = F.interpolate(a, scale_factor=2, mode='bilinear', align_corners=False)
    return torch.autograd.grad(up, a, g)[0]


def moved(dz, ky, kx):
    """out[q] = dz[q + (ky - 1, kx - 1)], zero where that leaves the map.  dz (B, N, H, W)."""
    H, W = dz.shape[2], dz.shape[3]
    ty, tx = ky - 1, kx - 1
    out = torch.zeros_like(dz)
    ys, yd = slice(max(ty, 0), H + min(ty, 0)), slice(max(-ty, 0), H + min(-ty, 0))
    xs, xd = slice(max(tx, 0), W + min(tx, 0)), slice(max(-tx, 0), W + min(-tx, 0))
    out[:, :, yd, xd] = dz[:, :, ys, xs]
    return out


def e_maps(dz, h, w):
    """(B, 9, N, h, w): E_k for k = ky * 3 + kx, the column order of vkas_upconv_adj."""
    return torch.stack([upsample_adjoint(moved(dz, k // 3, k % 3), h, w) for k in range(9)], 1)


@pytest.mark.parametrize('shape', [(2, 5, 3, 7, 6), (1, 3, 4, 1, 5), (1, 2, 2, 2, 2), (3, 4, 6, 9, 11)])
def test_lowres_identity_matches_autograd_fp64(shape):
    B, C, N, h, w = shape
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, C, h, w, dtype=torch.float64, generator=g, requires_grad=True)
    W = torch.randn(N, C, 3, 3, dtype=torch.float64, generator=g, requires_grad=True)
    z = F.conv2d(F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False), W, padding=1)
    dz = torch.randn(z.shape, dtype=torch.float64, generator=g)
    z.backward(dz)
    E = e_maps(dz, h, w)
    Wt = W.detach().reshape(N, C, 9)
    dx = torch.einsum('bknyx,nck->bcyx', E, Wt.flip(2))             # Bt_k = W[:, :, 8 - k]
    dW = torch.einsum('bknyx,bcyx->nck', E, x.detach()).flip(2).reshape(N, C, 3, 3)
    assert float((dx - x.grad).abs().max()) < 1e-12 * max(1.0, float(x.grad.abs().max()))
    assert float((dW - W.grad).abs().max()) < 1e-12 * max(1.0, float(W.grad.abs().max()))
    # the centre tap's column sums are the bias gradient (U's rows sum to one); the other taps' are not (zero padding)
    assert float((E[:, 4].sum((0, 2, 3)) - dz.sum((0, 2, 3))).abs().max()) < 1e-11
