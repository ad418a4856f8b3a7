"""The identity behind the heads' forward at the neck's height, on the host in fp64: the three formulas of
tests/head_rows_reference.py against F.interpolate(x2 bilinear, align_corners=False) followed by F.conv2d(padding=1).  The
1-pixel maps and the first and last rows are where a clamped row and the convolution's zero padding part."""
import pytest
import torch
import torch.nn.functional as F

from tests import head_rows_reference as R

SIZES = (1, 2, 3, 5)


@pytest.mark.parametrize('w', SIZES)
@pytest.mark.parametrize('h', SIZES)
def test_rows_form_equals_upsample_then_conv3x3(h, w):
    B, C, N = 2, 5, 3
    g = torch.Generator().manual_seed(1000 * h + w)
    x = torch.randn((B, h, w, C), generator=g, dtype=torch.float64)
    weight = torch.randn((N, C, 3, 3), generator=g, dtype=torch.float64)
    bias = torch.randn((N,), generator=g, dtype=torch.float64)
    up = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode='bilinear', align_corners=False)
    ref = F.conv2d(up, weight, bias, padding=1).permute(0, 2, 3, 1)
    got = R.head_conv_rows(x, weight, bias)
    assert got.shape == ref.shape == (B, 2 * h, 2 * w, N)
    # fp64 rounding: sums of 9 C products of O(1) values, evaluated in another order
    assert float((got - ref).abs().max()) <= 64 * 2.0 ** -52 * float(ref.abs().max() + 9 * C)


@pytest.mark.parametrize('n', SIZES)
def test_up2_axis_is_the_bilinear_upsample(n):
    t = torch.arange(2 * n * 3, dtype=torch.float64).view(2, n, 3) ** 1.5
    ref = F.interpolate(t.permute(0, 2, 1), scale_factor=2, mode='linear', align_corners=False).permute(0, 2, 1)
    assert torch.allclose(R.up2_axis(t, 1), ref, rtol=1e-14, atol=0)
