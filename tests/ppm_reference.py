"""fp64 restatement of the fused pyramid-pooling branches (csrc/ppm.hip, ops.PpmBranchesCat) in their factored form: pooling
and the bilinear resize as per-axis matrices, the forward as three steps and the backward as the four steps the kernels take.
tests/test_cpu_ppm_fused.py checks it against autograd of the stock torch functions; tests/test_gpu_ppm_fused.py measures the
kernels against it.  Activations are NHWC (B, H, W, C); params is [W_k (Cb, C), b_k, gamma_k, beta_k] per scale."""
import math

import torch

EPS = 1e-6
F64 = torch.float64


def pool_matrix(n: int, s: int) -> torch.Tensor:
    """(s, n): row i averages bin i = [floor(i n / s), ceil((i + 1) n / s)) of nn.AdaptiveAvgPool (bins may overlap, n < s legal)."""
    m = torch.zeros((s, n), dtype=F64)
    for i in range(s):
        lo, hi = (i * n) // s, -((-(i + 1) * n) // s)
        m[i, lo:hi] = 1.0 / (hi - lo)
    return m


def resize_matrix(n_in: int, n_out: int) -> torch.Tensor:
    """(n_out, n_in): F.interpolate(bilinear, align_corners=False) along one axis; src = max((dst + 0.5) n_in / n_out - 0.5, 0),
    the upper neighbour clamped to the border."""
    m = torch.zeros((n_out, n_in), dtype=F64)
    for d in range(n_out):
        src = max((d + 0.5) * n_in / n_out - 0.5, 0.0)
        i0 = min(int(src), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        w1 = src - i0
        m[d, i0] += 1.0 - w1
        m[d, i1] += w1
    return m


def gelu(u):
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def dgelu(u):
    return 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def forward(x, params, scales):
    """-> cat (B, H, W, C + nb Cb) and what the backward needs per branch."""
    x = x.to(F64)
    B, H, W, C = x.shape
    parts, saved = [x], []
    for k, s in enumerate(scales):
        Wk, bk, gk, btk = [p.to(F64) for p in params[4 * k:4 * k + 4]]
        Py, Px = pool_matrix(H, s), pool_matrix(W, s)
        P = torch.einsum('iy,byxc,jx->bijc', Py, x, Px)                 # 1: pooled cells
        Z = P @ Wk.t() + bk                                             # 2: Linear, LayerNorm, GELU on the pooled rows
        mean = Z.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((Z - mean) ** 2).mean(-1, keepdim=True) + EPS)
        A = gelu((Z - mean) * rstd * gk + btk)
        Uy, Ux = resize_matrix(s, H), resize_matrix(s, W)
        parts.append(torch.einsum('yi,bijc,xj->byxc', Uy, A, Ux))       # 3: resize into the channel slice
        saved.append((P, Z, mean, rstd))
    return torch.cat(parts, dim=3), saved


def backward(dcat, params, scales, saved, C):
    """-> dx and [dW_k, db_k, dgamma_k, dbeta_k] per scale, in the kernels' four steps."""
    dcat = dcat.to(F64)
    B, H, W, _ = dcat.shape
    Cb = params[0].shape[0]
    dx = dcat[..., :C].clone()                                          # 4 starts from the x slice of dcat
    grads = []
    for k, s in enumerate(scales):
        Wk, bk, gk, btk = [p.to(F64) for p in params[4 * k:4 * k + 4]]
        P, Z, mean, rstd = saved[k]
        Uy, Ux = resize_matrix(s, H), resize_matrix(s, W)
        dk = dcat[..., C + k * Cb:C + (k + 1) * Cb]
        dA = torch.einsum('yi,byxc,xj->bijc', Uy, dk, Ux)               # 1: U^T, x half then y half
        h = (Z - mean) * rstd                                           # 2: LN + GELU backward, dP = dZ W
        gg = dA * dgelu(h * gk + btk)
        dxh = gg * gk
        s1 = dxh.mean(-1, keepdim=True)
        s2 = (dxh * h).mean(-1, keepdim=True)
        dZ = rstd * (dxh - s1 - h * s2)
        dP = dZ @ Wk
        dW = torch.einsum('bijn,bijc->nc', dZ, P)                       # 3: parameter gradients
        grads.extend([dW, dZ.sum((0, 1, 2)), (gg * h).sum((0, 1, 2)), gg.sum((0, 1, 2))])
        Py, Px = pool_matrix(H, s), pool_matrix(W, s)
        dx = dx + torch.einsum('iy,bijc,jx->byxc', Py, dP, Px)          # 4: one sum over all branches
    return dx, grads


def stock(x, params, scales):
    """The same block from the stock torch functions (NCHW inside), for autograd."""
    import torch.nn.functional as F
    xn = x.permute(0, 3, 1, 2)
    H, W = xn.shape[2:]
    parts = [xn]
    for k, s in enumerate(scales):
        Wk, bk, gk, btk = params[4 * k:4 * k + 4]
        f = F.adaptive_avg_pool2d(xn, s).permute(0, 2, 3, 1)
        f = F.gelu(F.layer_norm(F.linear(f, Wk, bk), (Wk.shape[0],), gk, btk, EPS)).permute(0, 3, 1, 2)
        parts.append(F.interpolate(f, size=(H, W), mode='bilinear', align_corners=False))
    return torch.cat(parts, dim=1).permute(0, 2, 3, 1)


def make_case(seed: int, B: int, H: int, W: int, C: int, Cb: int, scales):
    """x, params and dcat in fp64 from a seeded host generator (parameters away from their initial 1 / 0 values)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, H, W, C), generator=g, dtype=F64)
    params = []
    for _ in scales:
        params.append(torch.randn((Cb, C), generator=g, dtype=F64) * (1.0 / math.sqrt(C)))
        params.append(torch.randn((Cb,), generator=g, dtype=F64) * 0.2)
        params.append(1.0 + 0.3 * torch.randn((Cb,), generator=g, dtype=F64))
        params.append(0.3 * torch.randn((Cb,), generator=g, dtype=F64))
    dcat = torch.randn((B, H, W, C + len(scales) * Cb), generator=g, dtype=F64)
    return x, params, dcat
