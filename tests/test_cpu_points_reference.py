"""The host restatement of the label-point kernels (tests/points_reference.py) against independent torch / numpy formulations,
on every point set tests/test_gpu_points.py uses: gather_patches against F.unfold, scatter3x3 against F.fold (the adjoint of
F.unfold) and against the autograd backward of F.unfold, prepare's ownership against np.unique, the rest against indexing."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

from tests import points_reference as R

SETS = list(R.POINT_SETS)


def _pixels(c):
    """clamped flat pixel index of every point, in point order"""
    B, P, H, W = c['B'], c['P'], c['H'], c['W']
    y, x = np.clip(c['py'], 0, H - 1), np.clip(c['px'], 0, W - 1)
    return (np.arange(B)[:, None] * H * W + y * W + x).reshape(-1)


def test_point_sets_cover_the_configurations_the_kernels_can_get_wrong():
    S = R.POINT_SETS
    assert all(c['B'] <= 3 and c['H'] <= 12 and c['W'] <= 12 and c['Mp'] >= c['B'] * c['P'] for c in S.values())
    assert S['n300_Mp320']['B'] * S['n300_Mp320']['P'] == 300 and S['n300_Mp320']['Mp'] == 320
    assert S['random_12x10']['P'] == 12 * 10 // 3 and S['random_12x10']['B'] == 3
    assert (S['H1']['H'], S['W1']['W'], S['map1x1']['H'], S['map1x1']['W']) == (1, 1, 1, 1)
    o = S['outside']
    assert (o['py'] < 0).any() and (o['px'] < 0).any() and (o['py'] >= o['H']).any() and (o['px'] >= o['W']).any()
    assert len(np.unique(_pixels(S['every_pixel_5x4']))) == 20
    for name in ('one_pixel_x3', 'map1x1', 'outside', 'random_12x10', 'n300_Mp320'):  # sets with duplicates
        assert (R.prepared(name)[1][:S[name]['B'] * S[name]['P']] < 0).any(), name
    c = S['last_col_first_col']
    assert c['px'][0, 0] == c['W'] - 1 and c['px'][0, 1] == 0 and c['py'][0, 1] == c['py'][0, 0] + 1
    c = S['last_row_first_row']
    assert c['py'][0, 0] == c['H'] - 1 and c['py'][1, 0] == 0 and c['px'][0, 0] == c['px'][1, 0]


@pytest.mark.parametrize('name', SETS)
def test_prepare_ownership_matches_np_unique(name):
    c = R.POINT_SETS[name]
    n, M = c['B'] * c['P'], c['B'] * c['H'] * c['W']
    for Mp in sorted({c['Mp'], n, n + 3}):
        pmap, pix = R.prepare(c['py'], c['px'], c['B'], c['P'], c['H'], c['W'], Mp)
        assert pmap.dtype == pix.dtype == np.int32 and pmap.shape == (M,) and pix.shape == (Mp,)
        q = _pixels(c)
        uq, first = np.unique(q, return_index=True)  # first: the lowest point index of every occupied pixel
        exp_map = np.full((M,), 0x7f7f7f7f, np.int64)
        exp_map[uq] = first
        assert np.array_equal(pmap, exp_map)
        owner = np.zeros((n,), bool)
        owner[first] = True
        assert np.array_equal(pix[:n], np.where(owner, q, -1 - q))
        assert (pix[n:] == np.iinfo(np.int32).min).all()


@pytest.mark.parametrize('name', SETS)
def test_gather_patches_matches_unfold(name):
    c = R.POINT_SETS[name]
    B, H, W, C = c['B'], c['H'], c['W'], 5
    pmap, pix = R.prepared(name)
    x = torch.randn((B, H, W, C), dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    got = R.gather_patches(x, pix)
    cols = F.unfold(x.permute(0, 3, 1, 2), 3, padding=1).view(B, C, 9, H * W)  # [b, c, t, pixel]
    exp = torch.zeros_like(got)
    for i, q in enumerate(pix):
        if q >= 0:
            exp[i] = cols[q // (H * W), :, :, q % (H * W)].t()
    assert torch.equal(got, exp)
    assert (pix >= 0).sum() == len(np.unique(_pixels(c)))


@pytest.mark.parametrize('name', SETS)
def test_scatter3x3_matches_fold_and_unfold_backward(name):
    c = R.POINT_SETS[name]
    B, H, W, C = c['B'], c['H'], c['W'], 3
    pmap, pix = R.prepared(name)
    g = torch.Generator().manual_seed(2)
    D = torch.randint(-8, 9, (len(pix), 9, C), generator=g).double()  # integers: every order of summation is exact
    dx0 = torch.randint(-8, 9, (B, H, W, C), generator=g).double()
    Dbad = D.clone()
    Dbad[torch.from_numpy(pix < 0)] = 1e30  # rows of duplicates and padding are never read
    got = R.scatter3x3(Dbad, pix, pmap, dx0)
    cols = torch.zeros((B, C, 9, H * W), dtype=torch.float64)  # the dense tensor that holds the owners' rows
    for i, q in enumerate(pix):
        if q >= 0:
            cols[q // (H * W), :, :, q % (H * W)] = D[i].t()
    exp = dx0 + F.fold(cols.view(B, C * 9, H * W), (H, W), 3, padding=1).permute(0, 2, 3, 1)
    assert torch.equal(got, exp)
    xr = torch.zeros((B, C, H, W), dtype=torch.float64, requires_grad=True)
    F.unfold(xr, 3, padding=1).backward(cols.view(B, C * 9, H * W))
    assert torch.equal(got, dx0 + xr.grad.permute(0, 2, 3, 1))
    # the touched pixels are the dilation of the occupied ones, image by image
    occ = torch.from_numpy(np.asarray(pmap) != R.EMPTY).view(B, 1, H, W).double()
    assert torch.equal(R.touched(pix, B, H, W), F.max_pool2d(occ, 3, 1, 1)[:, 0] > 0)


@pytest.mark.parametrize('name', SETS)
def test_row_and_vec8_copies_match_indexing(name):
    c = R.POINT_SETS[name]
    n, M = c['B'] * c['P'], c['B'] * c['H'] * c['W']
    pmap, pix = R.prepared(name)
    g = torch.Generator().manual_seed(3)
    q = torch.from_numpy(_pixels(c))
    own = torch.from_numpy(pix[:n] >= 0)
    z, stats = torch.randn((M, 40), generator=g).bfloat16(), torch.randn((3, M, 2), generator=g)
    dprojs = [torch.randn((M, 8), generator=g) for _ in range(3)]
    zs, stats_s, dproj_s = R.gather_rows(z, 8, 24, stats, dprojs, pix)
    assert zs.dtype == z.dtype and torch.equal(zs[:n], z[q, 8:32]) and not zs[n:].any()
    assert torch.equal(stats_s[:, :n], stats[:, q]) and not stats_s[:, n:].any()
    assert torch.equal(dproj_s[:, :n], torch.stack(dprojs)[:, q] * own[None, :, None]) and not dproj_s[:, n:].any()
    src = torch.randn((M, 8), generator=g)
    rows = R.gather_vec8(src, pix)
    assert torch.equal(rows[:n], src[q] * own[:, None]) and not rows[n:].any()
    dst = torch.randn((M, 8), generator=g)
    back = R.scatter_vec8(rows, pix, dst)
    occ = torch.from_numpy(np.asarray(pmap) != R.EMPTY)
    assert torch.equal(back[occ], src[occ]) and torch.equal(back[~occ], dst[~occ])


def test_margin_matches_numpy():
    g = np.random.default_rng(4)
    H, W = 50, 70
    py, px = g.integers(0, H, 300), g.integers(0, W, 300)
    exp = lambda: int(np.minimum(np.minimum(py, H - 1 - py), np.minimum(px, W - 1 - px)).min())
    assert R.margin(py, px, H, W) == exp() >= 0
    py[299] = H + 2
    assert R.margin(py, px, H, W) == exp() == -3
    px[0] = -7
    assert R.margin(py, px, H, W) == exp() == -7
