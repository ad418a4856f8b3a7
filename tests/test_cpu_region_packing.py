"""Cropping, rescaling and stacking text regions (inferencing/packing.py), host side: the integer resampling rule against the
round-half-up block mean and its other invariants, the shelf packing, the crop and remap arithmetic, the label-page oracle on
a hand-made case, the new config defaults, and the argument checks of the C ABI and of ops.resample_pack_u8 /
ops.pack_region_labels, which run before anything touches the device.  The table builders are shared with the GPU tests."""
import ctypes

import numpy as np
import pytest
import torch


def image(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def one(src, sy, sx, sh, sw, dh, dw):
    """The (dh, dw, 3) resampling of one source rectangle."""
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import resample_host
    return resample_host(src, np.array([[sy, sx, sh, sw, 0, 0, dh, dw]], np.int32), (dh, dw))


@pytest.mark.parametrize('ky,kx', [(1, 2), (2, 1), (3, 3), (4, 5), (7, 2), (16, 1)])
def test_integer_shrink_is_the_round_half_up_block_mean(ky, kx):
    dh, dw = 6, 5
    src = image(dh * ky + 3, dw * kx + 2, ky * 10 + kx)
    got = one(src, 2, 1, dh * ky, dw * kx, dh, dw)
    crop = src[2:2 + dh * ky, 1:1 + dw * kx].astype(np.int64)
    sums = crop.reshape(dh, ky, dw, kx, 3).sum(axis=(1, 3))
    assert np.array_equal(got, (sums + ky * kx // 2) // (ky * kx))


def test_identity_and_constant_images():
    src = image(23, 31, 1)
    assert np.array_equal(one(src, 3, 4, 17, 9, 17, 9), src[3:20, 4:13])
    assert np.array_equal(one(src, 0, 0, 23, 31, 23, 31), src)
    for value in (0, 1, 127, 255):
        flat = np.full((13, 11, 3), value, np.uint8)
        for dh, dw in ((1, 1), (13, 11), (5, 3), (40, 7), (12, 29), (14, 10), (12, 12), (64, 65)):
            assert (one(flat, 0, 0, 13, 11, dh, dw) == value).all(), (value, dh, dw)


@pytest.mark.parametrize('S,D', [(1, 1), (1, 4), (3, 8), (5, 5), (7, 3), (64, 1), (65, 64), (64, 65), (300, 7), (8192, 3)])
def test_axis_weights(S, D):
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import axis_weights
    w, den = axis_weights(S, D)
    assert w.shape == (D, S) and w.dtype == np.int64 and (w >= 0).all()
    assert den == (S if D < S else 2 * D) and (w.sum(axis=1) == den).all()
    if D < S:
        assert (w.sum(axis=0) == D).all(), 'area coverage uses every source sample equally'
        taps = (w > 0).sum(axis=1)
        assert taps.max() <= -(-S // D) + 1
    else:
        assert ((w > 0).sum(axis=1) <= 2).all()
        if D == S:
            assert np.array_equal(w, 2 * D * np.eye(S, dtype=np.int64))
    # a monotone ramp stays monotone, and within the source's range
    ramp = np.arange(S, dtype=np.int64) * 3
    out = (w @ ramp + den // 2) // den
    assert (np.diff(out) >= 0).all() and out.min() >= ramp.min() and out.max() <= ramp.max()


def test_monotone_ramps_stay_monotone_in_two_dimensions():
    y, x = np.mgrid[0:37, 0:53]
    src = np.stack([y * 4 + x, x * 3, y * 6], axis=-1).astype(np.uint8)  # no wrap: 36*4+52 = 196, 156, 216
    for dh, dw in ((9, 100), (80, 11), (37, 53), (5, 5), (111, 97)):
        out = one(src, 0, 0, 37, 53, dh, dw).astype(np.int64)
        assert (np.diff(out[:, :, 0], axis=0) >= 0).all() and (np.diff(out[:, :, 0], axis=1) >= 0).all()
        assert (np.diff(out[:, :, 1], axis=1) >= 0).all() and (np.diff(out[:, :, 2], axis=0) >= 0).all()


def test_resample_host_rejects_bad_tables():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import resample_host, SIDE_MAX
    src = image(20, 30, 2)
    row = lambda *v: np.array([v], np.int32)
    assert SIDE_MAX == 8192
    assert not resample_host(src, np.zeros((0, 8), np.int32), (8, 8)).any()
    for bad, what in ((row(0, 0, 21, 5, 0, 0, 4, 4), 'source'), (row(0, 26, 5, 5, 0, 0, 4, 4), 'source'),
                      (row(-1, 0, 5, 5, 0, 0, 4, 4), 'source'), (row(0, 0, 5, 5, 5, 0, 4, 4), 'destination'),
                      (row(0, 0, 5, 5, 0, -1, 4, 4), 'destination'), (row(0, 0, 0, 5, 0, 0, 4, 4), 'side'),
                      (row(0, 0, 5, 5, 0, 0, 4, 0), 'side')):
        with pytest.raises(ValueError, match=what):
            resample_host(src, bad, (8, 8))
    with pytest.raises(ValueError, match='side'):
        resample_host(src, row(0, 0, 5, 5, 0, 0, 4, 8193), (8, 8200))
    with pytest.raises(ValueError, match='overlap'):
        resample_host(src, np.concatenate([row(0, 0, 5, 5, 0, 0, 4, 4), row(0, 0, 5, 5, 3, 3, 4, 4)]), (8, 8))
    resample_host(src, np.concatenate([row(0, 0, 5, 5, 0, 0, 4, 4), row(0, 0, 5, 5, 4, 0, 4, 4), row(0, 0, 5, 5, 0, 4, 8, 4)]),
                  (8, 8))  # touching is not overlapping
    with pytest.raises(ValueError, match='uint8'):
        resample_host(src.astype(np.int32), np.zeros((0, 8), np.int32), (8, 8))
    with pytest.raises(ValueError, match=r'\(n, 8\)'):
        resample_host(src, np.zeros((2, 7), np.int32), (8, 8))


def random_shapes(seed, n, hmax=60, wmax=120):
    g = np.random.default_rng(seed)
    return np.stack([g.integers(1, hmax + 1, n), g.integers(1, wmax + 1, n)], axis=1)


@pytest.mark.parametrize('seed,n,page_pad,pad,width_max,step', [(1, 40, 10, 2, 512, 64), (2, 7, 0, 0, 128, 32),
                                                                (3, 200, 3, 1, 320, 32), (4, 1, 10, 2, 2048, 256)])
def test_stack_regions(seed, n, page_pad, pad, width_max, step):
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import stack_regions
    shapes = random_shapes(seed, n)
    keep = np.random.default_rng(seed).random(n) < 0.8
    keep[0] = True
    (Hp, Wp), boxes, packed, too_large = stack_regions(shapes, page_pad, pad, width_max, step, keep=keep)
    again = stack_regions(shapes.copy(), page_pad, pad, width_max, step, keep=keep.copy())
    assert again[0] == (Hp, Wp) and all(np.array_equal(a, b) for a, b in zip(again[1:], (boxes, packed, too_large)))
    assert Wp % 32 == 0 and 32 <= Wp <= width_max and Hp % step == 0 and Hp >= step
    assert np.array_equal(packed, keep) and not too_large.any()
    assert not boxes[~packed].any() and np.array_equal(boxes[packed][:, 2:], shapes[packed])
    dy, dx, dh, dw = boxes[packed].T
    assert (dy >= page_pad).all() and (dx >= page_pad).all()
    assert (dy + dh <= Hp - page_pad).all() and (dx + dw <= Wp - page_pad).all()
    assert Wp - 32 < (dx + dw).max() + page_pad and Hp - step < (dy + dh).max() + page_pad, 'the smallest such page'
    # pairwise: the rectangles grown by pad on the right and below are still disjoint
    idx = np.flatnonzero(packed)
    for a in range(len(idx)):
        for b in range(a + 1, len(idx)):
            apart_x = dx[a] + dw[a] + pad <= dx[b] or dx[b] + dw[b] + pad <= dx[a]
            apart_y = dy[a] + dh[a] + pad <= dy[b] or dy[b] + dh[b] + pad <= dy[a]
            assert apart_x or apart_y, (idx[a], idx[b])
    # shelves: stable order of decreasing height, row-major
    order = [r for r in np.argsort(-shapes[:, 0], kind='stable') if packed[r]]
    keys = [(boxes[r, 0], boxes[r, 1]) for r in order]
    assert keys == sorted(keys)


def test_stack_regions_too_large_empty_and_errors():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import stack_regions
    shapes = np.array([(10, 20), (5, 109), (9000, 4), (0, 7), (30, 108), (12, 8193)])
    keep = np.array([True, True, True, True, True, False])
    (Hp, Wp), boxes, packed, too_large = stack_regions(shapes, 10, 2, 128, 32, keep=keep)
    assert too_large.tolist() == [False, True, True, False, False, False]  # 109 > 128 - 20; a side above 8192
    assert packed.tolist() == [True, False, False, False, True, False]    # the empty one is neither
    assert boxes.tolist() == [[42, 10, 10, 20], [0] * 4, [0] * 4, [0] * 4, [10, 10, 30, 108], [0] * 4]
    assert (Hp, Wp) == (64, 128)
    page, boxes, packed, too_large = stack_regions(np.zeros((0, 2), np.int64), 10, 2, 2048, 256)
    assert page == (256, 32) and boxes.shape == (0, 4) and packed.shape == (0,) and too_large.shape == (0,)
    page, _, packed, _ = stack_regions(shapes, 10, 2, 128, 32, keep=np.zeros(6, bool))
    assert page == (32, 32) and not packed.any()
    for bad in (dict(width_max=100), dict(height_step=48), dict(page_pad=-1), dict(pad=-1), dict(width_max=32, page_pad=16)):
        args = dict(page_pad=10, pad=2, width_max=128, height_step=32)
        args.update(bad)
        with pytest.raises(ValueError):
            stack_regions(shapes, **args)
    with pytest.raises(ValueError):
        stack_regions(shapes, 10, 2, 128, 32, keep=keep[:3])


def test_region_crops():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import region_crops
    # a 100 x 150 image on 50 x 75 maps: a map pixel is 2 x 2 image pixels
    got = region_crops(np.array([(0, 0, 49, 74), (3, 4, 3, 4), (49, 74, 49, 74)], np.int32), (100, 150), (50, 75))
    assert got.dtype == np.int64 and got.tolist() == [[0, 0, 100, 150], [6, 8, 2, 2], [98, 148, 2, 2]]
    # a 10 x 10 image on 7 x 7 maps (10/7 per map pixel): floor below, ceil above, clipped at the edge
    got = region_crops(np.array([(0, 0, 2, 2), (6, 6, 6, 6), (1, 3, 4, 5)], np.int32), (10, 10), (7, 7))
    assert got.tolist() == [[0, 0, 5, 5], [8, 8, 2, 2], [1, 4, 7, 5]]  # floor(10/7)=1 .. ceil(50/7)=8; floor(30/7)=4 .. ceil(60/7)=9
    # an 800 x 1000 image whose rough maps are valid on 360 x 450 (shrunk to 720 x 900)
    got = region_crops(np.array([(359, 449, 359, 449), (7, 7, 8, 8)], np.int32), (800, 1000), (360, 450))
    assert got.tolist() == [[797, 997, 3, 3], [15, 15, 5, 5]]
    assert region_crops(np.zeros((0, 4), np.int32), (10, 10), (5, 5)).shape == (0, 4)


def test_remap_polygons_inverts_the_placement():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import remap_polygons
    placement = np.array([30, 40, 17, 9, 100, 200, 51, 4], np.int32)
    corners = np.array([[(100, 200), (100, 204), (151, 204), (151, 200)]], np.float32)
    got = remap_polygons(corners, placement)
    assert got.dtype == np.float64 and got.shape == (1, 4, 2)
    assert got.tolist() == [[[30, 40], [30, 49], [47, 49], [47, 40]]]
    mid = remap_polygons(np.array([125.5, 202.0]), placement)  # the centre of the destination is the centre of the source
    assert mid.tolist() == [38.5, 44.5]
    assert remap_polygons(np.zeros((0, 4, 2), np.float32), placement).shape == (0, 4, 2)


def labels_case():
    """An 8 x 12 rough label map (valid 7 x 11) over a 28 x 44 image (4 x 4 image pixels per map pixel): regions 1 and 2
    interlock, so the box of each covers pixels of the other; region 3 is apart.  Placements: the boxes of 1, 2 and 3, the
    first enlarged x2, the second shrunk, the third kept, on a 70 x 100 page (label page 35 x 50 at factor 2)."""
    lab = np.zeros((8, 12), np.int32)
    lab[1:5, 1] = 1; lab[1, 1:6] = 1          # a corner shape: box rows 1..4, columns 1..5
    lab[3:5, 3:7] = 2                         # inside the box of 1; box rows 3..4, columns 3..6
    lab[6, 9:11] = 3
    placements = np.array([(4, 4, 16, 20, 2, 3, 32, 40),     # region 1, x2
                           (12, 12, 8, 16, 40, 1, 5, 9),     # region 2, shrunk
                           (24, 36, 4, 8, 51, 60, 4, 8)],    # region 3, same size
                          np.int32)
    return lab, (7, 11), (28, 44), placements, np.array([1, 2, 3], np.int32), (35, 50), 2


def test_pack_region_labels_host_on_a_hand_made_case():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import pack_region_labels_host
    lab, valid, shape, placements, ids, out_shape, fdf = labels_case()
    out = pack_region_labels_host(lab, valid, shape, placements, ids, out_shape, fdf)
    assert out.shape == (35, 50) and out.dtype == np.int32
    # placement 0 covers page rows 2..33 and columns 3..42: the label centres (2v+1, 2u+1) inside are v = 1..16, u = 1..20.
    # The centre sits (2v-1)/2 page rows = (2v-1)/4 image rows into the crop: image row 3.5 + v, map row (7 + 2v) // 8;
    # likewise image column 3 + u, map column (3 + u) // 4
    want = np.zeros((35, 50), np.int32)
    for v in range(1, 17):
        for u in range(1, 21):
            want[v, u] = 0 if lab[(7 + 2 * v) // 8, (3 + u) // 4] == 2 else 1
    assert (want[1:17, 1:21] == 0).any() and (want == 1).any(), 'region 2 inside the box of region 1 is excluded'
    want[20:22, 0:5] = 2    # placement 1: page rows 40..44, columns 1..9: centres 41, 43 and 1..9; region 2 fills its own box
    want[25:27, 30:34] = 3  # placement 2: page rows 51..54, columns 60..67
    assert np.array_equal(out, want)
    # region ids are values, not positions
    again = pack_region_labels_host(lab, valid, shape, placements[::-1], ids[::-1], out_shape, fdf)
    assert np.array_equal(again, out)
    # a ragged label page: fewer rows than the page holds
    short = pack_region_labels_host(lab, valid, shape, placements, ids, (21, 50), fdf)
    assert np.array_equal(short, out[:21])
    with pytest.raises(ValueError):
        pack_region_labels_host(lab.astype(np.int64), valid, shape, placements, ids, out_shape, fdf)
    with pytest.raises(ValueError):
        pack_region_labels_host(lab, (9, 11), shape, placements, ids, out_shape, fdf)
    with pytest.raises(ValueError):
        pack_region_labels_host(lab, valid, shape, placements, ids[:2], out_shape, fdf)


def test_config_defaults():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import AdaptiveScalingInferencingConfig
    c = AdaptiveScalingInferencingConfig()
    assert c.precise_stack_flattened_text_regions_page_pad == 10 and c.precise_stack_flattened_text_regions_pad == 2
    assert c.precise_page_width_max % 32 == 0 and c.precise_page_height_step % 32 == 0
    assert c.precise_page_width_max >= 2048 - 0 and c.precise_page_height_step <= 1536


def test_c_entry_points_validate_before_launch():
    from vkit_ocr_model_adaptive_scaling_amd import _lib
    L, P = _lib.lib, ctypes.c_void_p
    a = lambda: P(256)  # any aligned non-null address: the checks run before anything is dereferenced or launched

    def pack(*, src=a(), Hs=8, Ws=8, table=a(), n=1, page=a(), Hp=8, Wp=8):
        return L.vkas_resample_pack_u8(src, Hs, Ws, table, n, page, Hp, Wp, None)

    assert pack(src=None) == -1 and b'null pointer' in L.vkas_last_error()
    assert pack(page=None) == -1 and b'null pointer' in L.vkas_last_error()
    assert pack(table=None) == -1 and b'bad table' in L.vkas_last_error()
    assert pack(n=-1) == -1 and b'bad table' in L.vkas_last_error()
    for dims in (dict(Hs=0), dict(Ws=-1), dict(Hp=0), dict(Wp=0)):
        assert pack(**dims) == -1 and b'bad dims' in L.vkas_last_error()
    assert pack(Hs=32769) == -1 and b'32768' in L.vkas_last_error()
    assert pack(Wp=40000) == -1 and b'32768' in L.vkas_last_error()
    assert pack(table=P(264)) == -1 and b'aligned' in L.vkas_last_error()

    def lab(*, labels=a(), Hl=8, Wl=8, vh=8, vw=8, Hs=16, Ws=16, table=a(), ids=a(), n=1, fdf=2, out=a(), Hq=8, Wq=8):
        return L.vkas_pack_region_labels(labels, Hl, Wl, vh, vw, Hs, Ws, table, ids, n, fdf, out, Hq, Wq, None)

    assert lab(labels=None) == -1 and b'null pointer' in L.vkas_last_error()
    assert lab(out=None) == -1 and b'null pointer' in L.vkas_last_error()
    assert lab(ids=None) == -1 and b'bad table' in L.vkas_last_error()
    assert lab(table=None) == -1 and b'bad table' in L.vkas_last_error()
    assert lab(Hq=0) == -1 and b'bad dims' in L.vkas_last_error()
    assert lab(vh=9) == -1 and b'does not fit' in L.vkas_last_error()
    assert lab(vw=0) == -1 and b'does not fit' in L.vkas_last_error()
    assert lab(fdf=0) == -1 and b'bad factor' in L.vkas_last_error()
    assert lab(Hq=20000) == -1 and b'32768' in L.vkas_last_error()
    assert lab(table=P(264)) == -1 and b'aligned' in L.vkas_last_error()


def test_ops_wrappers_validate_before_launch():
    from vkit_ocr_model_adaptive_scaling_amd import ops
    src = torch.zeros(20, 30, 3, dtype=torch.uint8)
    row = lambda *v: np.array([v], np.int32)
    good = row(0, 0, 5, 5, 0, 0, 4, 4)
    with pytest.raises(ValueError, match=r'src must be \(H, W, 3\)'):
        ops.resample_pack_u8(src[:, :, :2], good, (8, 8))
    with pytest.raises(ValueError, match='uint8'):
        ops.resample_pack_u8(src.float(), good, (8, 8))
    with pytest.raises(ValueError, match='page_shape'):
        ops.resample_pack_u8(src, good, 8)
    with pytest.raises(ValueError, match='empty'):
        ops.resample_pack_u8(src, good, (0, 8))
    with pytest.raises(ValueError, match='32768'):
        ops.resample_pack_u8(src, good, (8, 40000))
    with pytest.raises(ValueError, match=r'\(n, 8\)'):
        ops.resample_pack_u8(src, np.zeros((2, 7), np.int32), (8, 8))
    with pytest.raises(ValueError, match='int32'):
        ops.resample_pack_u8(src, good.astype(np.int64), (8, 8))
    with pytest.raises(ValueError, match='int32'):
        ops.resample_pack_u8(src, torch.from_numpy(good).long(), (8, 8))
    with pytest.raises(ValueError, match='source'):
        ops.resample_pack_u8(src, row(0, 0, 21, 5, 0, 0, 4, 4), (8, 8))
    with pytest.raises(ValueError, match='destination'):
        ops.resample_pack_u8(src, row(0, 0, 5, 5, 5, 5, 4, 4), (8, 8))
    with pytest.raises(ValueError, match='side'):
        ops.resample_pack_u8(torch.zeros(2, 9000, 3, dtype=torch.uint8), row(0, 0, 1, 8193, 0, 0, 4, 4), (8, 8))
    with pytest.raises(ValueError, match='overlap'):
        ops.resample_pack_u8(src, np.concatenate([good, row(1, 1, 5, 5, 3, 3, 4, 4)]), (8, 8))
    with pytest.raises(ValueError, match='out must be'):
        ops.resample_pack_u8(src, good, (8, 8), out=torch.zeros(8, 8, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.resample_pack_u8(src, good, (8, 8))  # valid arguments: no CPU fallback
    lab = torch.zeros(10, 15, dtype=torch.int32)
    ids = np.array([1], np.int32)
    call = lambda **kw: ops.pack_region_labels(**{**dict(labels=lab, valid_shape=(10, 15), image_shape=(20, 30), placements=good,
                                                         region_ids=ids, out_shape=(4, 4), fdf=2), **kw})
    with pytest.raises(ValueError, match=r'labels must be \(H, W\)'):
        call(labels=lab[None])
    with pytest.raises(ValueError, match='int32'):
        call(labels=lab.long())
    with pytest.raises(ValueError, match='valid_shape'):
        call(valid_shape=(11, 15))
    with pytest.raises(ValueError, match='fdf'):
        call(fdf=0)
    with pytest.raises(ValueError, match='fdf'):
        call(fdf=1.5)
    with pytest.raises(ValueError, match='empty'):
        call(out_shape=(0, 4))
    with pytest.raises(ValueError, match='destination'):
        call(out_shape=(1, 4))  # the page is out_shape * fdf: 2 x 8 does not hold a 4 x 4 destination
    with pytest.raises(ValueError, match='region_ids must be'):
        call(region_ids=np.array([1, 2], np.int32))
    with pytest.raises(ValueError, match='int32'):
        call(region_ids=np.array([1], np.int64))
    with pytest.raises(ValueError, match='start at 1'):
        call(region_ids=np.array([0], np.int32))
    with pytest.raises(RuntimeError, match='MI355X'):
        call()
