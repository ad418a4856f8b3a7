"""tests/points_low_reference.py against autograd: the label-point input gradient taken through U^T is the gradient that
F.interpolate(scale_factor=2, mode='bilinear', align_corners=False) sends back for the dense scatter of the same D."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

from tests import points_low_reference as L
from tests import points_reference as R

SIZES = [(2, 2), (5, 7), (16, 31), (1, 1), (1, 4), (3, 1)]


@pytest.mark.parametrize('hw', SIZES, ids=lambda s: '%dx%d' % s)
def test_low_scatter_is_the_adjoint_of_interpolate_applied_to_the_dense_scatter(hw):
    h, w = hw
    C = 3
    for name, (py, px, Mp) in L.point_sets(h, w).items():
        pmap, pix = L.prepared(py, px, h, w, Mp)
        g = torch.Generator().manual_seed(h * 100 + w)
        D = torch.randn((Mp, 9, C), generator=g, dtype=torch.float64)
        dx0 = torch.randn((2, h, w, C), generator=g, dtype=torch.float64)
        dense = R.scatter3x3(D, pix, pmap, torch.zeros((2, 2 * h, 2 * w, C), dtype=torch.float64))
        x = torch.zeros((2, C, h, w), dtype=torch.float64, requires_grad=True)
        up = F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)
        (up * dense.permute(0, 3, 1, 2)).sum().backward()
        ref = dx0 + x.grad.permute(0, 2, 3, 1)
        got = L.scatter3x3_low(D, pix, pmap, dx0)
        assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12), (name, float((got - ref).abs().max()))


def test_sources_are_the_weights_of_the_kernels():
    """0.25 / 0.75 inside, 1 at the clamped border: what ut_weights of csrc/upconv_adj.hip says from the source's side"""
    n = 5
    got = np.zeros((2 * n, n))
    for d in range(2 * n):
        for s, wt in L.sources(d, n):
            got[d, s] += wt
    for i in range(n):
        col = {2 * i - 1: 0.25, 2 * i: 0.75, 2 * i + 1: 0.75, 2 * i + 2: 0.25}
        if i == 0:
            col = {0: 1.0, 1: 0.75, 2: 0.25}
        if i == n - 1:
            col = {2 * i - 1: 0.25, 2 * i: 0.75, 2 * i + 1: 1.0}
        exp = np.zeros(2 * n)
        for d, wt in col.items():
            exp[d] = wt
        assert np.array_equal(got[:, i], exp), i


def test_point_sets_hold_the_cases():
    for h, w in SIZES[:3]:
        S = L.point_sets(h, w)
        H, W = 2 * h, 2 * w
        py, px, Mp = S['borders']
        assert {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)} <= set(zip(py[0].tolist(), px[0].tolist()))
        assert all(Mp % 64 == 0 and Mp > py.size for py, px, Mp in S.values())  # padding rows everywhere
        for name in ('borders', 'one_pixel', 'random'):
            py, px, Mp = S[name]
            assert (L.prepared(py, px, h, w, Mp)[1][:py.size] < 0).any(), name  # duplicates
        py, px, Mp = S['block6']
        assert len(set(zip(py[0].tolist(), px[0].tolist()))) == min(6, H) * min(6, W)
