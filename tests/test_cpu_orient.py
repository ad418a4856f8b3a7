"""Oriented text regions, host side (inferencing/orient.py and the warp definitions of inferencing/packing.py): the angle
rule on rasterised bars, the oriented / not oriented decision, the geometry of the warp row built from a region (every pixel
square of the region inside its source parallelogram), and ``warp_host`` / ``remap_polygons_affine`` on rows whose result is
known without the rule.  No GPU."""
import math

import numpy as np
import pytest

MAP = (64, 96)


def bar(angle_deg, length=60, width=6, shape=MAP):
    """The pixels whose centres lie in a length x width rectangle centred in the map, its long side at ``angle_deg`` from
    the x axis towards y."""
    a = math.radians(angle_deg)
    ys, xs = np.mgrid[0:shape[0], 0:shape[1]]
    y, x = ys - (shape[0] - 1) / 2, xs - (shape[1] - 1) / 2
    u, v = math.cos(a) * x + math.sin(a) * y, -math.sin(a) * x + math.cos(a) * y
    return ((np.abs(u) <= length / 2) & (np.abs(v) <= width / 2)).astype(np.int32)


def orient(labels, ratio_min=3.0, image_shape=MAP):
    """One region, median height 70 map pixels' worth so that the scale is exactly 1 on an image of the map's size."""
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import orient as O
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import region_scales
    moments = O.region_moments_host(labels, 1)[0]
    theta, dirs = O.region_directions(moments)
    extents = O.region_extents_host(labels, dirs[None])[0]
    ys, xs = np.nonzero(labels)
    boxes = np.array([[ys.min(), xs.min(), ys.max(), xs.max()]], np.int32)
    scales, shapes, keep = region_scales(boxes, np.array([70.0], np.float32), image_shape, labels.shape)
    oriented, rects, new_shapes, new_keep = O.orient_regions(dirs, extents, scales, shapes, keep, image_shape, labels.shape,
                                                             long_side_ratio_min=ratio_min)
    return dict(theta=theta[0], dir=dirs[0], extents=extents[0], scale=scales[0], box_shape=shapes[0], oriented=oriented[0],
                rect=rects[0], shape=new_shapes[0], keep=new_keep[0])


def test_host_oracles_on_a_hand_case():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import orient as O
    lab = np.array([[[1, 1, 0, 2], [0, 1, 0, 2], [3, 0, 0, 9]]], np.int32)
    m = O.region_moments_host(lab, 3)
    assert m.shape == (1, 3, 6) and m.dtype == np.int64
    assert m[0, 0].tolist() == [3, 1, 2, 1, 2, 1]      # pixels (0,0), (0,1), (1,1)
    assert m[0, 1].tolist() == [2, 1, 6, 1, 18, 3]     # pixels (0,3), (1,3)
    assert m[0, 2].tolist() == [1, 2, 0, 4, 0, 0]
    assert O.region_moments_host(lab, 2).tolist() == m[:, :2].tolist()  # labels above R are ignored
    dirs = np.array([[[16384, 0], [0, 16384], [-3, 5], [7, 7]]], np.int32)
    e = O.region_extents_host(lab, dirs)
    assert e.dtype == np.int32 and e[0, 0].tolist() == [0, 16384, 0, 16384]
    assert e[0, 1].tolist() == [0, 16384, -3 * 16384, -3 * 16384]      # u = s*y, v = -s*x
    assert e[0, 2].tolist() == [10, 10, -6, -6]
    assert tuple(e[0, 3].tolist()) == O.EMPTY_EXTENT                    # region 4 has no pixel (9 is above R)


@pytest.mark.parametrize('angle', [3, 10, 20, 40, -20])
def test_slanted_bar_is_oriented(angle):
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import orient as O
    lab = bar(angle)
    r = orient(lab)
    assert abs(math.degrees(r['theta']) - angle) < 1.0, math.degrees(r['theta'])
    assert abs(int(r['dir'][0]) - math.cos(r['theta']) * 16384) <= 0.5 and abs(int(r['dir'][1]) - math.sin(r['theta']) * 16384) <= 0.5
    assert r['oriented'] and r['keep']
    lu, lv = r['rect'][2], r['rect'][3]
    assert abs(lu - 61) <= 2 and abs(lv - 7) <= 2, (lu, lv)
    assert tuple(r['shape']) == (round(lv), round(lu)) and r['shape'][0] * r['shape'][1] < r['box_shape'][0] * r['box_shape'][1]
    # every pixel square of the region lies inside the source parallelogram of the warp row: invert the row's matrix and
    # look at the corners in destination coordinates.  eps: the coefficients are rounded to 2^-17 per step, the anchor
    # splits that between the two ends (at most 31 steps from the centre), and the anchor itself to 2^-17: below 2^-11.
    row = O.warp_row(r['dir'], r['rect'], MAP, MAP, (5, 9) + tuple(int(v) for v in r['shape']), r['scale'])
    assert O.warp_row_in_bounds(row) and row[10] == 0 and row[11] == 0
    dy, dx, dh, dw, ay, ax, myy, myx, mxy, mxx = (int(v) for v in row[:10])
    inv = np.linalg.inv(np.array([[myy, myx], [mxy, mxx]], np.float64))
    ys, xs = np.nonzero(lab)
    eps = 2.0 ** -11
    for cy, cx in ((-0.5, -0.5), (-0.5, 0.5), (0.5, -0.5), (0.5, 0.5)):
        ij = inv @ np.stack([(ys + cy) * 65536 - ay, (xs + cx) * 65536 - ax])
        assert (ij[0] >= -0.5 - eps).all() and (ij[0] <= dh - 0.5 + eps).all(), (ij[0].min(), ij[0].max(), dh)
        assert (ij[1] >= -0.5 - eps).all() and (ij[1] <= dw - 0.5 + eps).all(), (ij[1].min(), ij[1].max(), dw)
    # and the parallelogram is the oriented rectangle: its sides have the rectangle's lengths
    quad = O.warp_parallelogram(row)
    assert abs(np.hypot(*(quad[1] - quad[0])) - lu) < 0.01 and abs(np.hypot(*(quad[3] - quad[0])) - lv) < 0.01


def test_level_bar_is_not_oriented():
    r = orient(bar(0))
    assert int(r['dir'][1]) == 0 and int(r['dir'][0]) == 16384 and not r['oriented']
    assert tuple(r['shape']) == tuple(r['box_shape']) and r['keep']


def test_steep_bar_folds_and_stays_vertical():
    r = orient(bar(70))
    assert abs(math.degrees(r['theta']) + 20) < 1.0, math.degrees(r['theta'])
    assert r['oriented'] and r['rect'][3] > 3 * r['rect'][2], 'the long side is v: the line stays vertical'
    assert r['shape'][0] > 3 * r['shape'][1]


def test_blob_is_not_oriented():
    lab = np.zeros(MAP, np.int32)
    lab[20:40, 30:50] = 1
    lab[20, 30:40] = 0  # not symmetric: the angle is something, the ratio decides
    r = orient(lab)
    assert not r['oriented'] and tuple(r['shape']) == tuple(r['box_shape'])


def test_ratio_and_anisotropic_image():
    # the same bar on an image twice as wide as high per map pixel: the sides are carried by the per-axis ratios
    r = orient(bar(20), image_shape=(128, 384))
    assert r['oriented']
    assert not orient(bar(20), ratio_min=20.0)['oriented']


def test_warp_log2n():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing.orient import warp_log2n
    assert [warp_log2n(s) for s in (4.0, 1.0, 0.99, 0.5, 0.49, 0.25, 0.2, 0.125, 0.01)] == [0, 0, 1, 1, 2, 2, 3, 3, 3]


def image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def identity_row(sy, sx, dy, dx, dh, dw, log2n=0):
    return [dy, dx, dh, dw, sy * 65536, sx * 65536, 65536, 0, 0, 65536, log2n, 0]


def quarter_turn_row(sy, sx, sh, sw, dy, dx):
    """Destination (i, j) reads source (sy + j, sx + sw - 1 - i): the crop transposed and flipped, shape (sw, sh)."""
    return [dy, dx, sw, sh, sy * 65536, (sx + sw - 1) * 65536, 0, 65536, -65536, 0, 0, 0]


def test_warp_host_identity_quarter_turn_and_outside():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import warp_host
    src = image(23, 31, 1)
    page = np.full((40, 72, 3), 0xAB, np.uint8)
    rows = np.array([identity_row(3, 4, 2, 5, 11, 13), quarter_turn_row(6, 2, 9, 17, 20, 30),
                     identity_row(-2, 27, 14, 50, 6, 8)], np.int64)
    out = warp_host(src, rows, page)
    assert (page == 0xAB).all(), 'the page given is not written'
    want = page.copy()
    want[2:13, 5:18] = src[3:14, 4:17]
    want[20:37, 30:39] = src[6:15, 2:19].transpose(1, 0, 2)[::-1]
    want[14:20, 50:58] = 0
    want[16:20, 50:54] = src[0:4, 27:31]   # rows -2, -1 and columns 31.. are outside: zeros
    assert np.array_equal(out, want)
    # sub-samples of an identity row at log2n = 1 sit at +-1/4 pixel: the mean of four bilinear samples
    one = warp_host(src, np.array([identity_row(5, 5, 0, 0, 1, 1, log2n=1)], np.int64), np.zeros((1, 1, 3), np.uint8))
    acc = np.zeros(3)
    for oy, wy in ((4, 1), (5, 6), (6, 1)):
        for ox, wx in ((4, 1), (5, 6), (6, 1)):
            acc += wy * wx * src[oy, ox].astype(np.float64)
    assert np.array_equal(one[0, 0], np.floor(acc / 64 + 0.5).astype(np.uint8))


def test_check_warps():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import check_warps
    good = np.array([identity_row(0, 0, 0, 0, 4, 4), identity_row(0, 0, 0, 4, 4, 4)], np.int64)
    assert check_warps(good, (8, 8)).dtype == np.int64
    placements = np.array([[0, 0, 2, 2, 4, 0, 2, 2], [0, 0, 2, 2, 4, 1, 2, 2]], np.int32)  # these may overlap each other here
    check_warps(good, (8, 8), placements)
    for bad in (np.array([identity_row(0, 0, 0, 0, 4, 4), identity_row(0, 0, 3, 3, 4, 4)]),   # overlap
                np.array([identity_row(0, 0, 5, 0, 4, 4)]),                                    # leaves the page
                np.array([identity_row(0, 0, 0, 0, 0, 4)]),                                    # empty side
                np.array([identity_row(0, 0, 0, 0, 4, 4, log2n=4)]),
                np.array([[0, 0, 4, 4, 1 << 40, 0, 65536, 0, 0, 65536, 0, 0]]),
                np.array([[0, 0, 4, 4, 0, 0, (1 << 22) + 1, 0, 0, 65536, 0, 0]]),
                np.zeros((1, 8), np.int64), good.astype(np.float64)):
        with pytest.raises(ValueError):
            check_warps(bad, (8, 8))
    with pytest.raises(ValueError):
        check_warps(good, (8, 8), np.array([[0, 0, 2, 2, 3, 3, 2, 2]], np.int32))  # a placement under a warp


def test_remap_polygons_affine_inverts_the_centre_mapping():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import remap_polygons_affine
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import orient as O
    r = orient(bar(20))
    row = O.warp_row(r['dir'], r['rect'], MAP, MAP, (5, 9) + tuple(int(v) for v in r['shape']), r['scale'])
    dy, dx, dh, dw, ay, ax, myy, myx, mxy, mxx = (int(v) for v in row[:10])
    i, j = np.mgrid[0:dh, 0:dw]
    centres = np.stack([dy + i + 0.5, dx + j + 0.5], axis=-1)         # page positions of the destination pixel centres
    got = remap_polygons_affine(centres, row)
    want = np.stack([(ay + i * myy + j * myx) / 65536 + 0.5, (ax + i * mxy + j * mxx) / 65536 + 0.5], axis=-1)
    assert got.shape == want.shape and np.array_equal(got, want)
    # the centre of the destination is the centre of the bar (position convention: pixel k covers [k, k + 1))
    mid = remap_polygons_affine(np.array([dy + dh / 2, dx + dw / 2]), row)
    assert np.abs(mid - np.array([32.0, 48.0])).max() < 0.75, mid
    quarter = quarter_turn_row(6, 2, 9, 17, 20, 30)
    assert remap_polygons_affine(np.array([20.5, 30.5]), quarter).tolist() == [6.5, 18.5]
