"""The factored form of the fused pyramid-pooling branches (tests/ppm_reference.py: what csrc/ppm.hip computes, in fp64)
against autograd of the stock torch functions, and the eligibility function of ops.PpmBranchesCat.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import ppm_reference as R

MAPS = [(7, 9), (5, 4), (1, 1), (32, 32)]
SCALES = [(1, 2, 3, 6), (1,), (2, 5)]
TOL = 1e-11  # fp64 sums of at most ~1e3 terms of order one


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize('n,s', [(7, 2), (7, 3), (9, 6), (4, 6), (5, 6), (1, 3), (32, 6), (32, 3), (6, 6)])
def test_pool_matrix_and_adjoint(n, s):
    """Bins overlap when s does not divide n and repeat pixels when n < s: forward = AdaptiveAvgPool, adjoint = its autograd."""
    g = torch.Generator().manual_seed(n * 31 + s)
    x = torch.randn((2, 3, n, n), generator=g, dtype=R.F64, requires_grad=True)
    y = F.adaptive_avg_pool2d(x, s)
    P = R.pool_matrix(n, s)
    assert (P.sum(1) - 1).abs().max() < 1e-15
    if n % s != 0:
        assert (P > 0).sum(0).max() >= 2  # some pixel lies in two bins
    assert _rel(torch.einsum('iy,bcyx,jx->bcij', P, x.detach(), P), y.detach()) < TOL
    dy = torch.randn(y.shape, generator=g, dtype=R.F64)
    y.backward(dy)
    assert _rel(torch.einsum('iy,bcij,jx->bcyx', P, dy, P), x.grad) < TOL


@pytest.mark.parametrize('n_in,n_out', [(1, 7), (2, 7), (3, 9), (6, 5), (6, 4), (5, 1), (6, 32), (3, 32), (2, 32)])
def test_resize_matrix_and_adjoint(n_in, n_out):
    """U^T at the clamped borders: the first and last source rows collect the destinations whose neighbour was clamped."""
    g = torch.Generator().manual_seed(n_in * 37 + n_out)
    a = torch.randn((2, 3, n_in, n_in), generator=g, dtype=R.F64, requires_grad=True)
    y = F.interpolate(a, size=(n_out, n_out), mode='bilinear', align_corners=False)
    U = R.resize_matrix(n_in, n_out)
    assert (U.sum(1) - 1).abs().max() < 1e-15
    assert _rel(torch.einsum('yi,bcij,xj->bcyx', U, a.detach(), U), y.detach()) < TOL
    dy = torch.randn(y.shape, generator=g, dtype=R.F64)
    y.backward(dy)
    assert _rel(torch.einsum('yi,bcyx,xj->bcij', U, dy, U), a.grad) < TOL
    if n_out > 2 * n_in:  # upsampling: the border rows weigh more than the inner ones
        assert U[:, 0].sum() > U.sum() / n_in - 1e-12 or n_in == 1


@pytest.mark.parametrize('scales', SCALES)
@pytest.mark.parametrize('hw', MAPS)
def test_factored_block_matches_autograd(hw, scales):
    H, W = hw
    C, Cb = (8, 8) if hw == (32, 32) else (16, 24)
    x, params, dcat = R.make_case(H * 100 + W + len(scales), 2, H, W, C, Cb, scales)
    xs = x.clone().requires_grad_(True)
    ps = [p.clone().requires_grad_(True) for p in params]
    cat_ref = R.stock(xs, ps, scales)
    cat_ref.backward(dcat)
    cat, saved = R.forward(x, params, scales)
    assert cat.shape == (2, H, W, C + len(scales) * Cb)
    assert torch.equal(cat[..., :C], x)
    assert _rel(cat, cat_ref.detach()) < TOL
    dx, grads = R.backward(dcat, params, scales, saved, C)
    # the single dx sum: the x slice of dcat plus every branch's pooled gradient, as autograd adds x's two consumers
    assert _rel(dx, xs.grad) < 1e-10
    for g, p in zip(grads, ps):
        assert g.shape == p.shape
        assert _rel(g, p.grad) < 1e-10


def test_no_branch_gradient_leaves_dcat_slice():
    """dcat zero on the branch slices: dx is dcat's x slice exactly and every parameter gradient vanishes."""
    scales = (2, 5)
    x, params, dcat = R.make_case(5, 1, 7, 9, 8, 8, scales)
    dcat[..., 8:] = 0
    _, saved = R.forward(x, params, scales)
    dx, grads = R.backward(dcat, params, scales, saved, 8)
    assert torch.equal(dx, dcat[..., :8])
    assert all(float(g.abs().max()) == 0.0 for g in grads)


def test_eligibility():
    from vkit_ocr_model_adaptive_scaling_amd import ops
    ok = ops.ppm_fused_eligible
    bf, hf, f32 = torch.bfloat16, torch.float16, torch.float32
    assert ok(bf, 768, 96, (1, 2, 3, 6)) and ok(hf, 1024, 128, (1, 2, 3, 6))
    assert ok(bf, 8, 8, (1,)) and ok(hf, 72, 24, (2, 5)) and ok(bf, 128, 16, (1, 2, 3, 6))
    assert not ok(f32, 768, 96, (1, 2, 3, 6))                 # fp32 keeps the exact path
    assert not ok(bf, 72, 20, (1, 2, 3, 6))                   # Cb not its own padded width (the existing PpmBlock tests)
    assert not ok(bf, 76, 24, (1, 2, 3, 6))                   # C not a multiple of 8
    assert not ok(bf, 768, 96, ())                            # no branch
    assert not ok(bf, 768, 96, (1, 2, 3, 6, 7))               # more branches than the kernels take
    assert not ok(bf, 768, 96, (0, 2)) and not ok(bf, 768, 96, (ops.PPM_MAX_SCALE + 1,))
    assert ok(bf, 768, 96, (ops.PPM_MAX_SCALE,))              # 256 cells: the limit itself
    assert not ok(bf, 768, 96, (ops.PPM_MAX_SCALE, 1))        # 257 cells
    assert ok(bf, ops.PPM_MAX_C, ops.PPM_MAX_CB, (1, 2, 3, 6))
    assert not ok(bf, ops.PPM_MAX_C + 8, 96, (1, 2, 3, 6)) and not ok(bf, 768, ops.PPM_MAX_CB + 8, (1, 2, 3, 6))
    # the limits stated in Python are the ones the library checks
    assert (ops.PPM_MAX_BRANCHES, ops.PPM_MAX_SCALE, ops.PPM_MAX_CELLS) == (4, 16, 256)
