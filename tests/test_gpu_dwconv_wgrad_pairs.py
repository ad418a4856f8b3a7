"""dwconv7x7_wgrad_mfma_kernel puts two input rows into one matrix product (csrc/dwconv.hip): these cases sit where that pairing
can go wrong, not at workload size.  Through vkas_dwconv7x7_wgrad with the helpers of test_gpu_dwconv (padded pixel strides for
x and dy, NaN-filled workspace with a guard block, pad channels exactly zero).

H in {1, 2, 15, 16, 17, 18, 33}: a last tile with an odd number of valid dy rows, a pair whose second row lies outside the image,
one row and two rows past a tile edge.  W in {1, 31, 33}; C in {8, 24, 40}: half a slice, a slice and a half, pad-free and padded;
B = 2.  One case with several tiles per walker, (3, 768, 40, 70).

Two kinds of check: random operands against fp64 autograd within the single-op table TOL of test_gpu_ops (the operands are
rounded to the storage type first, so what is left is fp32 accumulation order), and impulses of dy over integer x, where every
tap is one element of x and the comparison is ==.
"""
import pytest
import torch
from torch.nn import functional as F

from tests.test_gpu_dwconv import IDS, mfma_geometry, run_wgrad, unpack
from tests.test_gpu_ops import close, q, rnd

pytestmark = pytest.mark.gpu

HALF = [torch.bfloat16, torch.float16]
SMALL = [(2, C, H, W) for H in (1, 2, 15, 16, 17, 18, 33) for W in (1, 31, 33) for C in (8, 24, 40)]
MANY_TILES = (3, 768, 40, 70)
CASES = SMALL + [MANY_TILES]


def case_id(c):
    return 'x'.join(map(str, c))


def test_many_tiles_case_has_several_tiles_per_walker():
    assert mfma_geometry(*MANY_TILES)[2] == 4


@pytest.mark.parametrize('dtype', HALF, ids=[IDS[d] for d in HALF])
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_random_against_fp64(case, dtype):
    B, C, H, W = case
    x, dy = q(rnd(case, 71), dtype), q(rnd(case, 72), dtype)
    w = torch.zeros((C, 1, 7, 7), dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, None, padding=3, groups=C).backward(dy)
    ref_w, ref_b = w.grad.reshape(C, 49), dy.sum((0, 2, 3))
    for mode in ('fused', 'parts'):
        gw, gb = run_wgrad(x, dy, dtype, mode)
        close(unpack(gw, C), ref_w, dtype, 'paired weight gradient, %s %s' % (mode, case))
        close(gb[:C], ref_b, dtype, 'paired bias gradient, %s %s' % (mode, case))


def impulse_rows(H):
    """Row 0, row H - 1, an even and an odd row, and the rows on both sides of the first tile edge."""
    even = (H - 1) // 2 * 2
    return sorted({r for r in (0, H - 1, even, even - 1, 1, 15, 16, 17) if 0 <= r < H})


@pytest.mark.parametrize('dtype', HALF, ids=[IDS[d] for d in HALF])
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_impulse_exact(case, dtype):
    """dy = one impulse (channel c: 1 + c % 3) at (b, py, px): tap (ky, kx) of channel c must be exactly
    (1 + c % 3) * x[b, c, py + ky - 3, px + kx - 3], zero outside the image, and the bias gradient exactly dy.sum().  Integer
    |x| <= 40 keeps every product and sum exact in bf16, fp16 and fp32."""
    B, C, H, W = case
    g = torch.Generator().manual_seed(73)
    x = torch.randint(-40, 41, case, generator=g).double()
    xpad = F.pad(x, (3, 3, 3, 3))
    amp = (1 + torch.arange(C) % 3).double()
    rows = impulse_rows(H) if case != MANY_TILES else [0, 16, 31, 39]
    for n, py in enumerate(rows):
        b, px = n % B, (n * 13 + W // 2) % W
        dy = torch.zeros(case, dtype=torch.float64)
        dy[b, :, py, px] = amp
        ref = (xpad[b, :, py:py + 7, px:px + 7] * amp[:, None, None]).reshape(C, 49)
        gw, gb = run_wgrad(x, dy, dtype, 'fused')
        got = unpack(gw, C).double().cpu()
        bad = (got != ref).nonzero().tolist()
        assert not bad, 'impulse at row %d, column %d: (channel, tap) that differ: %s' % (py, px, bad[:20])
        assert torch.equal(gb[:C].double().cpu(), dy.sum((0, 2, 3))), 'bias gradient, impulse at row %d' % py
