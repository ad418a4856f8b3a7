"""Crop / rescale / pack on the MI355X (csrc/respack.hip, ops.resample_pack_u8, ops.pack_region_labels, infer) against the
host oracles of inferencing/packing.py (checked on their own in test_cpu_region_packing.py): every comparison is exact
equality.  The kernels work on 16 x 64 output tiles, four adjacent outputs per thread, and gather the source directly (no
source window), so the seams are: tile edges in both directions, quads that straddle a placement's edge, page widths that
are and are not multiples of 4 (dword / byte stores), the shrink / enlarge switch per axis, clamped taps at every image
corner, and the 64-row chunks of the per-block table search.  Then determinism, replay from a captured graph with the
source and the table overwritten in place, and the inference API end to end, eager and replayed."""
import numpy as np
import pytest
import torch

from tests import test_cpu_region_packing as C
from tests.test_gpu_inferencing import build

pytestmark = pytest.mark.gpu

# per-axis (S, D); the last pair is a ratio far above anything a tile could hold in a window (the kernel has none)
PAIRS = [(1, 1), (1, 4), (3, 8), (5, 5), (7, 3), (64, 1), (65, 64), (64, 65), (300, 2)]
SRC = C.image(310, 317, 11)


def device_pack(src, table, page_shape, prefill=0xFF):
    from vkit_ocr_model_adaptive_scaling_amd import ops
    out = torch.full(tuple(page_shape) + (3,), prefill, dtype=torch.uint8, device='cuda')
    page = ops.resample_pack_u8(torch.from_numpy(src).cuda(), table, page_shape, out=out)
    assert page.data_ptr() == out.data_ptr()
    return page.cpu().numpy()


def assert_pack_equals_host(src, table, page_shape):
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import resample_host
    want = resample_host(src, table, page_shape)
    got = device_pack(src, table, page_shape)
    outside = np.ones(page_shape, bool)
    for _, _, _, _, dy, dx, dh, dw in np.asarray(table).reshape(-1, 8).tolist():
        outside[dy:dy + dh, dx:dx + dw] = False
    assert not got[outside].any(), 'the 0xFF prefill shows outside the placements'
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, (len(bad), bad[:5].tolist())


@pytest.mark.parametrize('shift', [0, 3, 5])
@pytest.mark.parametrize('iy', range(len(PAIRS)))
def test_single_placements(iy, shift):
    (Sy, Dy), (Sx, Dx) = PAIRS[iy], PAIRS[(iy + shift) % len(PAIRS)]
    Hs, Ws = SRC.shape[:2]
    sources = [(0, 0), (0, Ws - Sx), (Hs - Sy, 0), (Hs - Sy, Ws - Sx), ((Hs - Sy) // 2 + 1, (Ws - Sx) // 3 + 1)]
    for k, (sy, sx) in enumerate(sources):
        Hp, Wp = Dy + 37, Dx + 131 + (k % 2)
        if k >= 3:
            Wp = -(-Wp // 4) * 4  # the dword-store path
        offsets = [(0, 0), (13, 61), (15, 63), (5, 2), (Hp - Dy, Wp - Dx)]  # off the quad grid; across the tile edges; last cell
        dy, dx = offsets[k]
        assert_pack_equals_host(SRC, np.array([[sy, sx, Sy, Sx, dy, dx, Dy, Dx]], np.int32), (Hp, Wp))


def grid_table(seed, page_shape, cell, max_src):
    """One placement of random size (up to the cell) and random source rectangle in every cell x cell square of the page."""
    g = np.random.default_rng(seed)
    Hs, Ws = SRC.shape[:2]
    rows = []
    for y in range(0, page_shape[0] - cell + 1, cell):
        for x in range(0, page_shape[1] - cell + 1, cell):
            dh, dw = (int(v) for v in g.integers(1, cell + 1, 2))
            sh, sw = (int(v) for v in g.integers(1, max_src + 1, 2))
            rows.append((int(g.integers(0, Hs - sh + 1)), int(g.integers(0, Ws - sw + 1)), sh, sw,
                         y + int(g.integers(0, cell - dh + 1)), x + int(g.integers(0, cell - dw + 1)), dh, dw))
    return np.array(rows, np.int32)


def test_no_placements_gives_a_zero_page():
    for shape in ((1, 1), (16, 64), (17, 65), (50, 130)):
        assert_pack_equals_host(SRC, np.zeros((0, 8), np.int32), shape)


def test_one_pixel_destinations_and_touching_placements():
    # a 1-pixel destination on every other pixel of 32 x 96: 768 placements, up to 512 of them in one tile's lists
    ys, xs = np.mgrid[0:32:2, 0:96:2]
    g = np.random.default_rng(3)
    n = ys.size
    sh, sw = g.integers(1, 9, n), g.integers(1, 9, n)
    table = np.stack([g.integers(0, 300, n), g.integers(0, 300, n), sh, sw, ys.ravel(), xs.ravel(), np.ones(n), np.ones(n)],
                     axis=1).astype(np.int32)
    assert_pack_equals_host(SRC, table, (32, 96))
    # every pixel of 16 x 64 (one tile) its own placement: 1024 rows, the lists' capacity
    ys, xs = np.mgrid[0:16, 0:64]
    n = ys.size
    table = np.stack([g.integers(0, 300, n), g.integers(0, 300, n), g.integers(1, 5, n), g.integers(1, 5, n), ys.ravel(),
                      xs.ravel(), np.ones(n), np.ones(n)], axis=1).astype(np.int32)
    assert_pack_equals_host(SRC, table, (16, 64))
    # rectangles that touch along tile edges and off them, covering the page completely
    cuts_y, cuts_x = [0, 7, 16, 33, 48, 50], [0, 5, 64, 66, 127, 128, 200]
    rows = []
    for y0, y1 in zip(cuts_y, cuts_y[1:]):
        for x0, x1 in zip(cuts_x, cuts_x[1:]):
            sh, sw = int(g.integers(1, 90)), int(g.integers(1, 90))
            rows.append((int(g.integers(0, 200)), int(g.integers(0, 200)), sh, sw, y0, x0, y1 - y0, x1 - x0))
    assert_pack_equals_host(SRC, np.array(rows, np.int32), (50, 200))


def test_a_few_hundred_small_placements():
    table = grid_table(5, (256, 320), 16, 40)
    assert len(table) == 320
    assert_pack_equals_host(SRC, table, (256, 320))
    assert_pack_equals_host(SRC, grid_table(6, (250, 318), 23, 70), (250, 318))


def stacked_table(seed, n, width_max=320, step=32):
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import stack_regions
    g = np.random.default_rng(seed)
    shapes = C.random_shapes(seed, n, 50, 100)
    page, boxes, packed, _ = stack_regions(shapes, 10, 2, width_max, step)
    assert packed.all()
    Hs, Ws = SRC.shape[:2]
    sh, sw = g.integers(1, 120, n), g.integers(1, 120, n)
    table = np.stack([g.integers(0, Hs - sh + 1), g.integers(0, Ws - sw + 1), sh, sw], axis=1)
    return np.concatenate([table, boxes], axis=1).astype(np.int32), page


@pytest.mark.parametrize('seed,n', [(1, 1), (2, 30), (3, 90)])
def test_random_tables_from_stack_regions(seed, n):
    table, page = stacked_table(seed, n)
    assert_pack_equals_host(SRC, table, page)


def device_labels(case):
    from vkit_ocr_model_adaptive_scaling_amd import ops
    lab, valid, shape, placements, ids, out_shape, fdf = case
    return ops.pack_region_labels(torch.from_numpy(lab).cuda(), valid, shape, placements, ids, out_shape, fdf).cpu().numpy()


def random_labels_case(seed, fdf):
    """Blocky random label maps (regions 0..6, so that source boxes overlap other regions) under a stacked table; the label
    page is ragged: ceil(page / fdf), not a multiple of the tile."""
    g = np.random.default_rng(seed)
    lab = np.repeat(np.repeat(g.integers(0, 7, (9, 11)), 5, axis=0), 5, axis=1).astype(np.int32)[:43, :52]
    valid, shape = (41, 50), (123, 171)
    table, page = stacked_table(seed, 25, width_max=288)
    table[:, 0] = g.integers(0, shape[0] - table[:, 2] + 1)
    table[:, 1] = g.integers(0, shape[1] - table[:, 3] + 1)
    ids = g.integers(1, 7, len(table)).astype(np.int32)
    out_shape = (-(-page[0] // fdf), -(-page[1] // fdf))
    return lab, valid, shape, table, ids, out_shape, fdf


@pytest.mark.parametrize('case', ['hand', 'random1', 'random2', 'random3', 'random4', 'empty'])
def test_label_page_matches_host(case):
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import pack_region_labels_host
    if case == 'hand':
        args = C.labels_case()
    elif case == 'empty':
        args = C.labels_case()
        args = args[:3] + (np.zeros((0, 8), np.int32), np.zeros((0,), np.int32)) + args[5:]
    else:
        fdf = int(case[-1])
        args = random_labels_case(40 + fdf, fdf)
    want = pack_region_labels_host(*args)
    got = device_labels(args)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    if case.startswith('random'):
        ids = args[4]
        inside = np.zeros(want.shape, bool)
        from vkit_ocr_model_adaptive_scaling_amd.inferencing.packing import label_cells
        for _, _, _, _, dy, dx, dh, dw in args[3].tolist():
            (v0, v1), (u0, u1) = label_cells(dy, dh, args[6]), label_cells(dx, dw, args[6])
            inside[v0:v1, u0:u1] = True
        assert (want[inside] == 0).any() and (want[inside] != 0).any(), 'the exclusion rule must show both ways'
        assert not want[~inside].any() and set(np.unique(want).tolist()) <= {0, *ids.tolist()}


@pytest.mark.parametrize('Wp', [128, 130])  # dword / 16-byte stores, and byte / scalar stores
def test_rows_that_must_be_skipped(Wp):
    # a trusted device table (validate=False) whose bad rows the kernels must treat as absent; they point at page area that
    # no good row reaches, and neither the source (every byte >= 1) nor the label rule (zero map: the row's id) would leave
    # that area zero if one of them were taken
    from vkit_ocr_model_adaptive_scaling_amd import ops
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import pack_region_labels_host, resample_host
    src = np.maximum(C.image(40, 50, 13), 1)
    lab = np.zeros((20, 25), np.int32)
    lab[4:9, 3:12] = 2  # another region's label under part of the first good row
    good = [(0, 0, 40, 50, 0, 0, 16, 20), (5, 7, 10, 12, 3, 60, 20, 30), (30, 40, 10, 10, 17, 100, 15, 28)]
    bad = [(0, 0, 0, 4, 0, 24, 4, 4),         # an empty source side ...
           (0, 0, 4, 4, 0, 30, 4, 0),         # ... and an empty destination side
           (0, 0, 4, 4, 0, 36, 8193, 4),      # a side above 8192
           (37, 0, 4, 4, 24, 40, 4, 4),       # a source rectangle one pixel past the source, below ...
           (0, 47, 4, 4, 24, 46, 4, 4),       # ... and to the right
           (0, 0, 4, 4, -2, 52, 4, 4)]        # a negative dy
    rows = np.array(good[:1] + bad[:3] + good[1:2] + bad[3:] + good[2:], np.int32)
    ids = np.arange(1, len(rows) + 1, dtype=np.int32)
    is_good = np.array([tuple(r) in good for r in rows.tolist()])
    want_page = resample_host(src, rows[is_good], (32, Wp))
    d_rows, d_ids = torch.from_numpy(rows).cuda(), torch.from_numpy(ids).cuda()
    got_page = ops.resample_pack_u8(torch.from_numpy(src).cuda(), d_rows, (32, Wp), validate=False).cpu().numpy()
    assert not want_page[0:8, 24:56].any() and not want_page[24:28, 40:50].any(), 'the bad rows point at free page area'
    assert np.array_equal(got_page, want_page)
    for fdf in (1, 2):
        out_shape = (32 // fdf, Wp // fdf)
        want = pack_region_labels_host(lab, (20, 25), (40, 50), rows[is_good], ids[is_good], out_shape, fdf)
        got = ops.pack_region_labels(torch.from_numpy(lab).cuda(), (20, 25), (40, 50), d_rows, d_ids, out_shape, fdf,
                                     validate=False).cpu().numpy()
        assert set(np.unique(want).tolist()) == {0, *ids[is_good].tolist()} and (want[:16 // fdf, :20 // fdf] == 0).any()
        assert np.array_equal(got, want), fdf


def test_same_call_twice_is_bit_equal():
    table, page = stacked_table(7, 60)
    a, b = device_pack(SRC, table, page), device_pack(SRC, table, page, prefill=0x55)
    assert a.tobytes() == b.tobytes()
    case = random_labels_case(42, 2)
    assert device_labels(case).tobytes() == device_labels(case).tobytes()


def test_captured_graph_replays_with_source_and_table_overwritten_in_place():
    from vkit_ocr_model_adaptive_scaling_amd import ops
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import resample_host, pack_region_labels_host, stack_regions
    n, page = 40, (384, 320)
    g = np.random.default_rng(9)
    cases = []
    for k in range(4):
        shapes = C.random_shapes(20 + k, n, 40, 90)
        shape, boxes, packed, _ = stack_regions(shapes, 10, 2, 320, 384)
        assert shape == page and packed.all()
        sh, sw = g.integers(1, 100, n), g.integers(1, 100, n)
        table = np.concatenate([np.stack([g.integers(0, 310 - sh + 1), g.integers(0, 317 - sw + 1), sh, sw], axis=1), boxes],
                               axis=1).astype(np.int32)
        lab = np.repeat(np.repeat(g.integers(0, 5, (8, 8)), 20, axis=0), 20, axis=1).astype(np.int32)
        cases.append((C.image(310, 317, 30 + k), table, lab, g.integers(1, 5, n).astype(np.int32)))
    d_src = torch.from_numpy(cases[0][0]).cuda()
    d_table = torch.from_numpy(cases[0][1]).cuda()
    d_lab = torch.from_numpy(cases[0][2]).cuda()
    d_ids = torch.from_numpy(cases[0][3]).cuda()
    run = lambda: (ops.resample_pack_u8(d_src, d_table, page, validate=False),
                   ops.pack_region_labels(d_lab, (155, 158), (310, 317), d_table, d_ids, (192, 160), 2, validate=False))
    run()  # eager first
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_page, out_labels = run()
    for src, table, lab, ids in cases + cases[:1]:
        d_src.copy_(torch.from_numpy(src))
        d_table.copy_(torch.from_numpy(table))
        d_lab.copy_(torch.from_numpy(lab))
        d_ids.copy_(torch.from_numpy(ids))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out_page.cpu().numpy(), resample_host(src, table, page))
        assert np.array_equal(out_labels.cpu().numpy(),
                              pack_region_labels_host(lab, (155, 158), (310, 317), table, ids, (192, 160), 2))


def compose(inf, img, resize_fn):
    """infer() restated with the public pieces and the host oracles."""
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import (pack_region_labels_host, precise_group_char_polygons,
                                                                 region_crops, remap_polygons, resample_host, stack_regions)
    c = inf.config
    r = inf.rough_infer_text_regions(img, resize_fn=resize_fn)
    crops = region_crops(r.boxes, img.shape[:2], r.resized_shape)
    page_shape, boxes, packed, too_large = stack_regions(
        r.resized_shapes, c.precise_stack_flattened_text_regions_page_pad, c.precise_stack_flattened_text_regions_pad,
        c.precise_page_width_max, c.precise_page_height_step, keep=r.keep)
    placements = np.concatenate([crops[packed], boxes[packed]], axis=1).astype(np.int32)
    ids = (np.flatnonzero(packed) + 1).astype(np.int32)
    page = resample_host(img, placements, page_shape)
    chars = inf.precise_infer_char_polygons(page)
    assert chars.padded_image.shape[:2] == page_shape
    labels = pack_region_labels_host(r.labels, r.resized_shape, img.shape[:2], placements, ids,
                                     (page_shape[0] // 2, page_shape[1] // 2), 2)
    groups = precise_group_char_polygons(chars, labels)
    n = len(r.boxes)
    points = [np.zeros((0, 2), np.int32)] * n
    probs = [np.zeros((0,), np.float32)] * n
    polygons = [np.zeros((0, 4, 2), np.float64)] * n
    for k, rid in enumerate(ids.tolist()):
        if rid <= len(groups):
            points[rid - 1], probs[rid - 1] = groups[rid - 1].points, groups[rid - 1].probs
            polygons[rid - 1] = remap_polygons(groups[rid - 1].polygons, placements[k])
    return r, packed, too_large, placements, ids, page, labels, points, probs, polygons


@pytest.mark.parametrize('shape,resize_fn', [((100, 150), None), ((800, 1000), 'device')], ids=['100x150', '800x1000'])
def test_infer_equals_the_composition_of_public_pieces(shape, resize_fn):
    inf, _ = build(torch.float16)
    # this untrained model predicts heights near 0.9 and probabilities near 0.5: a height floor that leaves some regions
    # without a valid height (dropped), a target height that keeps the stacked page small, a peak threshold that leaves peaks
    inf.config.rough_valid_char_height_min = 0.85
    inf.config.precise_flattened_text_region_resized_char_height_median = 4
    inf.config.precise_build_polygons_positive_char_prob_thr = 0.5
    img = np.random.default_rng(5).integers(0, 256, shape + (3,), dtype=np.uint8)
    if resize_fn is None:
        with pytest.raises(ValueError):
            inf.rough_infer_text_regions(np.zeros((800, 1000, 3), np.uint8))  # the default still refuses to shrink
        with pytest.raises(ValueError):
            inf.rough_infer(img, resize_fn='host')
    first = inf.infer(img, return_page=True, return_labels=True)  # every graph signature's first call: eager
    replays = inf.graphs.replays
    r, packed, too_large, placements, ids, page, labels, points, probs, polygons = compose(inf, img, resize_fn)
    print(f'{shape}: {r.num_regions} regions, {int(r.keep.sum())} kept, {int(packed.sum())} packed, page {page.shape}, '
          f'{sum(len(p) for p in points)} characters, {int((labels == 0).sum())} label pixels off')
    assert r.keep.sum() >= 2 and (~r.keep).any() and packed.sum() >= 2, 'the page must hold kept and dropped regions'
    assert sum(len(p) for p in points) > 0 and sum(len(p) > 0 for p in points) >= 2, 'characters in at least two regions'
    later = [inf.infer(img, return_page=True, return_labels=True), inf.infer(img)]
    assert inf.graphs.replays >= replays + 6, 'the later calls replay both graphs'
    for k, res in enumerate([first] + later):
        assert res.image_shape == shape and res.page_shape == page.shape[:2] and res.regions.num_regions == r.num_regions
        assert np.array_equal(res.regions.boxes, r.boxes) and np.array_equal(res.regions.keep, r.keep)
        assert res.regions.char_height_medians.tobytes() == r.char_height_medians.tobytes()
        assert np.array_equal(res.regions.resized_shapes, r.resized_shapes)
        assert np.array_equal(res.packed, packed) and np.array_equal(res.too_large, too_large)
        assert np.array_equal(res.placements, placements) and np.array_equal(res.placement_regions, ids)
        if k < 2:
            assert np.array_equal(res.page, page) and np.array_equal(res.region_labels, labels)
            assert np.array_equal(res.regions.labels, r.labels) and np.array_equal(res.regions.padded_image, r.padded_image)
        else:
            assert res.page is None and res.region_labels is None and res.regions.labels is None
        assert len(res.points) == len(res.probs) == len(res.polygons) == len(r.boxes)
        for a, b, name in ((res.points, points, 'points'), (res.probs, probs, 'probs'), (res.polygons, polygons, 'polygons')):
            for u, v in zip(a, b):
                assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), (k, name)
    if resize_fn == 'device':
        from vkit_ocr_model_adaptive_scaling_amd.inferencing import resample_host
        assert r.padded_image.shape == (736, 928, 3)
        want = resample_host(img, np.array([[0, 0, 800, 1000, 0, 0, 720, 900]], np.int32), (736, 928))
        assert np.array_equal(r.padded_image, want), 'the 720 rule shrinks by the area rule, the padding is zero'
        maps = inf.rough_infer(img, resize_fn='device')
        assert np.array_equal(maps.padded_image, want) and maps.rough_char_mask.shape == (368, 464)
