"""vkas_points_scatter3x3_low (csrc/points.hip) on the MI355X, through the C ABI, against its host restatement
tests/points_low_reference.py (held to autograd of F.interpolate in tests/test_cpu_points_low_reference.py).

Integer operands: D holds small integers times 16, so every product with a weight in {1, 3, 4, 9, 12, 16} / 16 and every fp32
sum is an exact integer below 2^24; the kernel's result is then the restatement rounded once to the storage type, bit for bit.
Rows of duplicates and padding hold a sentinel no result may show.  Random operands: against the route the entry replaces
(vkas_points_scatter3x3 into zeros at 2h x 2w, then vkas_resize_bwd onto dx) within the single-op tolerance of
tests/test_gpu_ops.py, and two launches bit-identical.  Point sets (points_low_reference.point_sets): corners and edges,
duplicates, all points on one pixel, a full 6 x 6 block, P no multiple of 64."""
import pytest
import torch

from tests import points_low_reference as L
from tests.test_gpu_ops import close
from tests.test_gpu_points import CODE, _bits, _lib, guard_ok, guarded, p, st

pytestmark = pytest.mark.gpu

SIZES = [(2, 2), (5, 7), (16, 31)]
CPS = (8, 40, 384)
DTYPES = [torch.bfloat16, torch.float16]
B = 2


def _low(lib, check, D, d_pix, d_map, Mp, h, w, Cp, dx0, lddx, dtype):
    dx, gd = guarded((B, h, w, lddx), 0.0, dtype)
    gd.fill_(-3.0)
    dx.copy_(dx0)
    check(lib.vkas_points_scatter3x3_low(p(D), p(d_pix), p(d_map), Mp, B, h, w, Cp, p(dx), lddx, CODE[dtype], st()),
          'points_scatter3x3_low')
    torch.cuda.synchronize()
    assert guard_ok(gd, -3.0), 'guard words overwritten'
    return dx.cpu()


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'f16'])
@pytest.mark.parametrize('Cp', CPS)
@pytest.mark.parametrize('hw', SIZES, ids=lambda s: '%dx%d' % s)
def test_low_scatter_integer_operands_bit_for_bit(hw, Cp, dtype):
    lib, check = _lib()
    h, w = hw
    for name, (py, px, Mp) in L.point_sets(h, w).items():
        pmap, pix = L.prepared(py, px, h, w, Mp)
        d_map, d_pix = torch.from_numpy(pmap.copy()).cuda(), torch.from_numpy(pix.copy()).cuda()
        g = torch.Generator().manual_seed(Cp + h)
        lddx = Cp + 8
        D = (torch.randint(-4, 5, (Mp, 9, Cp), generator=g) * 16).float()
        D[torch.from_numpy(pix < 0)] = 1e30  # rows of duplicates and padding: only owners' rows may be read
        dx0 = torch.full((B, h, w, lddx), 123.0, dtype=dtype)  # canaries in the slack columns
        dx0[..., :Cp] = torch.randint(-8, 9, (B, h, w, Cp), generator=g).to(dtype)
        ref = L.scatter3x3_low(D, pix, pmap, dx0[..., :Cp])
        assert float(ref.abs().max()) < 2 ** 24 and torch.equal(ref, ref.round())  # every fp32 sum is exact
        got = _low(lib, check, D.cuda(), d_pix, d_map, Mp, h, w, Cp, dx0.cuda(), lddx, dtype)
        assert torch.equal(got[..., :Cp], ref.to(dtype)), (name, float((got[..., :Cp].double() - ref).abs().max()))
        assert torch.equal(_bits(got[..., Cp:]), _bits(dx0[..., Cp:])), (name, 'slack columns touched')
        untouched = L.scatter3x3_low(torch.ones((Mp, 9, 1), dtype=torch.float64), pix, pmap,
                                     torch.zeros((B, h, w, 1), dtype=torch.float64))[..., 0] == 0
        assert torch.equal(_bits(got[untouched]), _bits(dx0[untouched])), (name, 'a pixel no point reaches changed')


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'f16'])
@pytest.mark.parametrize('Cp', CPS)
@pytest.mark.parametrize('hw', SIZES, ids=lambda s: '%dx%d' % s)
def test_low_scatter_random_operands_match_the_route_it_replaces(hw, Cp, dtype):
    lib, check = _lib()
    h, w = hw
    H, W = 2 * h, 2 * w
    for name, (py, px, Mp) in L.point_sets(h, w).items():
        pmap, pix = L.prepared(py, px, h, w, Mp)
        d_map, d_pix = torch.from_numpy(pmap.copy()).cuda(), torch.from_numpy(pix.copy()).cuda()
        g = torch.Generator().manual_seed(3 * Cp + w)
        D = torch.randn((Mp, 9, Cp), generator=g).cuda()
        dx0 = torch.randn((B, h, w, Cp), generator=g).to(dtype).cuda()
        got = _low(lib, check, D, d_pix, d_map, Mp, h, w, Cp, dx0, Cp, dtype)
        again = _low(lib, check, D, d_pix, d_map, Mp, h, w, Cp, dx0, Cp, dtype)
        assert torch.equal(_bits(again), _bits(got)), (name, 'two launches differ')
        up = torch.zeros((B, H, W, Cp), dtype=dtype, device='cuda')
        check(lib.vkas_points_scatter3x3(p(D), p(d_pix), p(d_map), Mp, B, H, W, Cp, p(up), Cp, CODE[dtype], st()),
              'points_scatter3x3')
        old = dx0.clone()
        check(lib.vkas_resize_bwd(p(up), Cp, p(old), Cp, B, h, w, H, W, Cp, 0, 1, CODE[dtype], st()), 'resize_bwd')
        torch.cuda.synchronize()
        close(got, old, dtype, name)
        # and the restatement itself, which rounds once where the old route rounds twice
        close(got, L.scatter3x3_low(D.cpu(), pix, pmap, dx0.cpu()), dtype, name + ' vs restatement')
