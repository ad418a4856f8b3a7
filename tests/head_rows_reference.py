"""Host restatement of the heads' forward at the neck's height (ops.UpHeadsFused, csrc/head.hip head_rows_fwd_kernel):

    X1 = Ux x                                                    (B, h, 2w, C)    upsampled along x only
    T[b, i, X, ky, n] = sum_{kx, c} W[n][c][ky][kx] X1[b, i, X + kx - 1, c]       zero where X + kx - 1 leaves [0, 2w)
    z[b, r, X, n] = bias[n] + sum_{ky : 0 <= r + ky - 1 < 2h} (Uy T_ky)[b, r + ky - 1, X, n]

U = Uy (x) Ux is the x2 bilinear upsample (align_corners=False, clamped at the border); a tap row outside the upsampled map is
the convolution's zero padding, not a clamped row.  Everything here runs in the dtype of its inputs (fp64 in the tests)."""
import torch


def up2_index(o: int, n: int):
    """(first source, second source, weight of the second) of output o of a x2 bilinear axis with n sources: the generic
    index function of F.interpolate(align_corners=False) at scale 2"""
    i = o >> 1
    if o & 1:
        return i, min(i + 1, n - 1), 0.25
    if i == 0:
        return 0, min(1, n - 1), 0.0
    return i - 1, i, 0.75


def up2_axis(t: torch.Tensor, dim: int) -> torch.Tensor:
    """x2 bilinear upsample of t along dim: out[o] = (1 - w) t[a] + w t[b]"""
    n = t.shape[dim]
    idx = [up2_index(o, n) for o in range(2 * n)]
    a = torch.tensor([i[0] for i in idx], device=t.device)
    b = torch.tensor([i[1] for i in idx], device=t.device)
    shape = [1] * t.dim()
    shape[dim] = 2 * n
    w = torch.tensor([i[2] for i in idx], dtype=t.dtype, device=t.device).view(shape)
    return t.index_select(dim, a) * (1 - w) + t.index_select(dim, b) * w


def row_conv(x1: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """T (B, h, W2, 3, N) from X1 (B, h, W2, C) and weight (N, C, 3, 3): per kernel row ky a 1x3 convolution along x"""
    B, h, W2, C = x1.shape
    pad = torch.zeros((B, h, 1, C), dtype=x1.dtype, device=x1.device)
    xp = torch.cat([pad, x1, pad], dim=2)
    return torch.stack([sum(xp[:, :, kx:kx + W2, :] @ weight[:, :, ky, kx].T for kx in range(3)) for ky in range(3)], dim=3)


def rows_to_z(T: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """z (B, 2h, W2, N) from T (B, h, W2, 3, N): the y half of the upsample per kernel row, then the sum over ky"""
    B, h, W2, _, N = T.shape
    up = up2_axis(T, 1)  # (B, 2h, W2, 3, N)
    zero = torch.zeros((B, 1, W2, N), dtype=T.dtype, device=T.device)
    rows = torch.cat([zero, up[:, :-1, :, 0, :]], dim=1) + up[:, :, :, 1, :] + torch.cat([up[:, 1:, :, 2, :], zero], dim=1)
    return bias.to(T.dtype).view(1, 1, 1, N) + rows


def head_conv_rows(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """z (B, 2h, 2w, N) = bias + conv3x3(U x) for x (B, h, w, C), by the three formulas above"""
    return rows_to_z(row_conv(up2_axis(x, 2), weight), bias)


def head_tail(z: torch.Tensor, c: int, gamma, beta, wproj, bproj):
    """LayerNorm over the first c channels (eps 1e-6, biased variance) -> exact GELU -> Linear: (maps, mean, rstd)"""
    v = z[..., :c]
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-6)
    u = (v - mean) * rstd * gamma + beta
    a = 0.5 * u * (1.0 + torch.erf(u / 2.0 ** 0.5))
    return a @ wproj.T + bproj, mean[..., 0], rstd[..., 0]
