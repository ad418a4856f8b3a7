"""Host restatement of the label-point kernels (csrc/points.hip, vkas_points_margin in csrc/loss.hip) with obvious loops, and
the point sets the tests share.  tests/test_cpu_points_reference.py holds it to independent torch formulations (F.unfold,
F.fold, np.unique); tests/test_gpu_points.py holds the kernels to it, exactly.

Tensors are torch CPU tensors: copies keep the dtype they are given, sums are taken in fp64.  pix and map are int32 numpy
arrays as vkas_points_prepare writes them."""
import numpy as np
import torch

EMPTY = 0x7f7f7f7f   # map value of a pixel without a label point
PAD = -2 ** 31       # pix value of the padding rows behind the last point (INT_MIN)


def _clamp(v, n):
    return min(max(int(v), 0), n - 1)


def prepare(py, px, B, P, H, W, Mp):
    """(map (B*H*W,), pix (Mp,)): coordinates clamped into the map; the owner of a pixel is its lowest point index; pix[i] is the
    pixel q for an owner, -1 - q for another point of that pixel, PAD for the rows behind B*P; map[q] is the owner or EMPTY."""
    py, px = np.asarray(py).reshape(-1), np.asarray(px).reshape(-1)
    n = B * P
    assert py.size == px.size == n and Mp >= n
    pmap = np.full((B * H * W,), EMPTY, np.int32)
    pix = np.full((Mp,), PAD, np.int32)
    for i in range(n):  # ascending: the first point to reach a pixel is its lowest index
        q = (i // P) * H * W + _clamp(py[i], H) * W + _clamp(px[i], W)
        if pmap[q] == EMPTY:
            pmap[q] = i
            pix[i] = q
        else:
            pix[i] = -1 - q
    return pmap, pix


def gather_rows(z, c0, Ns, stats, dprojs, pix):
    """z (M, ldz); stats (n_heads, M, 2); dprojs: n_heads tensors (M, 8).  Returns zs (Mp, Ns), stats_s (n_heads, Mp, 2),
    dproj_s (n_heads, Mp, 8): owners get everything, duplicates z and stats but zero d(proj), padding rows zeros."""
    Mp, nh = len(pix), len(dprojs)
    zs = torch.zeros((Mp, Ns), dtype=z.dtype)
    stats_s = torch.zeros((nh, Mp, 2), dtype=stats.dtype)
    dproj_s = torch.zeros((nh, Mp, 8), dtype=dprojs[0].dtype)
    for i in range(Mp):
        p = int(pix[i])
        if p == PAD:
            continue
        q = p if p >= 0 else -1 - p
        zs[i] = z[q, c0:c0 + Ns]
        for h in range(nh):
            stats_s[h, i] = stats[h, q]
            if p >= 0:
                dproj_s[h, i] = dprojs[h][q]
    return zs, stats_s, dproj_s


def gather_patches(x, pix):
    """x (B, H, W, C) -> (Mp, 9, C): tap t = ky*3 + kx of row i is x at pixel(i) + (ky-1, kx-1) inside the same image, zero
    where that leaves the map; duplicate and padding rows are zero."""
    B, H, W, C = x.shape
    out = torch.zeros((len(pix), 9, C), dtype=x.dtype)
    for i in range(len(pix)):
        q = int(pix[i])
        if q < 0:
            continue
        b, y, xx = q // (H * W), (q // W) % H, q % W
        for t in range(9):
            ty, tx = y + t // 3 - 1, xx + t % 3 - 1
            if 0 <= ty < H and 0 <= tx < W:
                out[i, t] = x[b, ty, tx]
    return out


def scatter3x3(D, pix, pmap, dx0):
    """D (Mp, 9, C), dx0 (B, H, W, C) -> fp64 (B, H, W, C): for every owner point i and tap t whose target
    pixel(i) + (ky-1, kx-1) lies inside the same image, D[i, t] added onto that pixel.  Only owners' rows of D are read."""
    B, H, W, C = dx0.shape
    out = dx0.double().clone()
    for i in range(len(pix)):
        q = int(pix[i])
        if q < 0:
            continue
        assert int(pmap[q]) == i
        b, y, xx = q // (H * W), (q // W) % H, q % W
        for t in range(9):
            ty, tx = y + t // 3 - 1, xx + t % 3 - 1
            if 0 <= ty < H and 0 <= tx < W:
                out[b, ty, tx] += D[i, t].double()
    return out


def touched(pix, B, H, W):
    """(B, H, W) bool: the union of the 3x3 neighbourhoods of the owners' pixels, cut at the borders of their image."""
    ones = torch.ones((len(pix), 9, 1), dtype=torch.float64)
    pmap = np.full((B * H * W,), EMPTY, np.int32)
    for i, q in enumerate(pix):
        if q >= 0:
            pmap[q] = i
    return scatter3x3(ones, pix, pmap, torch.zeros((B, H, W, 1), dtype=torch.float64))[..., 0] > 0


def scatter_vec8(src, pix, dst):
    """src (Mp, 8), dst (M, 8) -> dst with the owners' rows written to their pixels; everything else as it was."""
    out = dst.clone()
    for i in range(len(pix)):
        if pix[i] >= 0:
            out[int(pix[i])] = src[i]
    return out


def gather_vec8(src, pix):
    """src (M, 8) -> (Mp, 8): the owners' pixels; duplicate and padding rows are zero."""
    out = torch.zeros((len(pix), 8), dtype=src.dtype)
    for i in range(len(pix)):
        if pix[i] >= 0:
            out[i] = src[int(pix[i])]
    return out


def margin(py, px, H, W):
    """smallest distance of any point to the border of the (H, W) map; negative when a point lies outside"""
    return min(min(int(y), H - 1 - int(y), int(x), W - 1 - int(x)) for y, x in zip(np.asarray(py).reshape(-1), np.asarray(px).reshape(-1)))


# ------------------------------------------------------------------------------------------------------------ point sets
def _set(H, W, images, Mp=None):
    """images: per image its list of (y, x); every image holds the same number of points"""
    B, P = len(images), len(images[0])
    assert all(len(im) == P for im in images)
    py = np.array([[p[0] for p in im] for im in images], np.int64)
    px = np.array([[p[1] for p in im] for im in images], np.int64)
    return dict(B=B, P=P, H=H, W=W, Mp=Mp if Mp is not None else -(-(B * P) // 64) * 64, py=py, px=px)


def _random_images(B, P, H, W, seed):
    g = np.random.default_rng(seed)
    return [list(zip(g.integers(0, H, P).tolist(), g.integers(0, W, P).tolist())) for _ in range(B)]


def _make_sets():
    s = {}
    s['single'] = _set(7, 9, [[(3, 4)]])
    s['corners_edges'] = _set(7, 9, [[(0, 0), (0, 8), (6, 0), (6, 8), (0, 4), (6, 4), (3, 0), (3, 8)]])
    s['one_pixel_x3'] = _set(6, 5, [[(2, 2), (2, 2), (2, 2)]], Mp=8)
    s['same_in_two_images'] = _set(6, 7, [[(1, 2), (4, 5)], [(1, 2), (4, 5)]])
    s['block2x2'] = _set(6, 6, [[(2, 2), (2, 3), (3, 2), (3, 3)]])
    s['block3x3'] = _set(7, 7, [[(y, x) for y in (4, 3, 2) for x in (4, 3, 2)]], Mp=9)  # owners against raster order
    for d in (1, 2, 3):
        s['pair_h%d' % d] = _set(8, 9, [[(3, 2), (3, 2 + d)]])
        s['pair_v%d' % d] = _set(8, 9, [[(2 + d, 4), (2, 4)]])  # the lower point first
    s['last_col_first_col'] = _set(6, 7, [[(2, 6), (3, 0)]])
    s['last_row_first_row'] = _set(5, 6, [[(4, 3)], [(0, 3)], [(4, 3)]])
    g = np.random.default_rng(5)
    s['every_pixel_5x4'] = _set(5, 4, [[(int(q) // 4, int(q) % 4) for q in g.permutation(20)]], Mp=20)
    s['H1'] = _set(1, 9, [[(0, 0), (0, 4), (0, 5)], [(0, 8), (0, 8), (0, 2)]])
    s['W1'] = _set(8, 1, [[(0, 0), (4, 0), (5, 0)], [(7, 0), (7, 0), (2, 0)]])
    s['map1x1'] = _set(1, 1, [[(0, 0), (0, 0)], [(0, 0), (0, 0)], [(0, 0), (0, 0)]])
    s['outside'] = _set(6, 7, [[(-1, -1), (-5, 3), (6, 7), (2, -3), (3, 99), (100, 100)]])  # the last clamps onto the third
    s['random_12x10'] = _set(12, 10, _random_images(3, 40, 12, 10, 11))
    s['n300_Mp320'] = _set(12, 10, _random_images(3, 100, 12, 10, 12), Mp=320)  # more than one 256-thread workgroup
    return s


POINT_SETS = _make_sets()
_PREPARED = {}


def prepared(name, Mp=None):
    """(map, pix) of a point set from prepare(), computed once per (set, Mp) and left unchanged"""
    c = POINT_SETS[name]
    Mp = c['Mp'] if Mp is None else Mp
    if (name, Mp) not in _PREPARED:
        pmap, pix = prepare(c['py'], c['px'], c['B'], c['P'], c['H'], c['W'], Mp)
        pmap.setflags(write=False)
        pix.setflags(write=False)
        _PREPARED[(name, Mp)] = (pmap, pix)
    return _PREPARED[(name, Mp)]
