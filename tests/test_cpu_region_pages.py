"""Pages of bounded height for the regions of a batch (inferencing/packing.py::stack_regions_pages), host side: equal to
``stack_regions`` whenever one page suffices, the spill rule, and the host oracles of the multi-source, multi-page pack
(csrc/respack.hip's multi kernels) against the single-image definitions they are built from; then the argument checks of the
two C entry points and of ops.resample_pack_u8_multi / ops.pack_region_labels_multi, which run before anything touches the
device.  The shape lists restate those of tests/test_cpu_region_packing.py."""
import ctypes

import numpy as np
import pytest
import torch


def image(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def random_shapes(seed, n, hmax=60, wmax=120):
    g = np.random.default_rng(seed)
    return np.stack([g.integers(1, hmax + 1, n), g.integers(1, wmax + 1, n)], axis=1)


def assert_equals_stack_regions(shapes, page_pad, pad, width_max, step, keep, height_max):
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import stack_regions, stack_regions_pages
    page, boxes, packed, too_large = stack_regions(shapes, page_pad, pad, width_max, step, keep=keep)
    assert page[0] <= height_max, 'the case must fit one page'
    page_shapes, boxes_p, pages, packed_p, too_large_p = stack_regions_pages(shapes, page_pad, pad, width_max, step, height_max,
                                                                             keep=keep)
    assert page_shapes == [page] and boxes_p.dtype == np.int64 and np.array_equal(boxes_p, boxes)
    assert np.array_equal(packed_p, packed) and np.array_equal(too_large_p, too_large)
    assert pages.dtype == np.int32 and np.array_equal(pages, np.where(packed, 0, -1))


@pytest.mark.parametrize('seed,n,page_pad,pad,width_max,step', [(1, 40, 10, 2, 512, 64), (2, 7, 0, 0, 128, 32),
                                                                (3, 200, 3, 1, 320, 32), (4, 1, 10, 2, 2048, 256)])
def test_one_page_equals_stack_regions_on_the_packing_cases(seed, n, page_pad, pad, width_max, step):
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import stack_regions
    shapes = random_shapes(seed, n)
    keep = np.random.default_rng(seed).random(n) < 0.8
    keep[0] = True
    height = stack_regions(shapes, page_pad, pad, width_max, step, keep=keep)[0][0]
    for height_max in (height, height + step, 64 * step):  # the tightest page that holds it, and looser ones
        assert_equals_stack_regions(shapes, page_pad, pad, width_max, step, keep, height_max)
    assert_equals_stack_regions(shapes, page_pad, pad, width_max, step, None, 64 * step)


def test_one_page_equals_stack_regions_with_too_large_empty_and_dropped_regions():
    shapes = np.array([(10, 20), (5, 109), (9000, 4), (0, 7), (30, 108), (12, 8193)])
    keep = np.array([True, True, True, True, True, False])
    assert_equals_stack_regions(shapes, 10, 2, 128, 32, keep, 64)
    assert_equals_stack_regions(np.zeros((0, 2), np.int64), 10, 2, 2048, 256, None, 1536)
    assert_equals_stack_regions(shapes, 10, 2, 128, 32, np.zeros(6, bool), 32)


def test_one_page_equals_stack_regions_on_200_random_lists():
    g = np.random.default_rng(2024)
    for seed in range(200):
        n = int(g.integers(0, 60))
        shapes = random_shapes(1000 + seed, n, int(g.integers(1, 80)), int(g.integers(1, 200)))
        keep = g.random(n) < 0.85
        page_pad, pad = int(g.integers(0, 12)), int(g.integers(0, 4))
        width_max, step = 32 * int(g.integers(3, 12)), 32 * int(g.integers(1, 5))
        from vkit_ocr_model_adaptive_scaling_amd.inferencing import stack_regions
        height = stack_regions(shapes, page_pad, pad, width_max, step, keep=keep)[0][0]
        height_max = height + step * int(g.integers(0, 3))
        if height_max - 2 * page_pad < 1:
            continue
        assert_equals_stack_regions(shapes, page_pad, pad, width_max, step, keep, height_max)


@pytest.mark.parametrize('seed,n,page_pad,pad,width_max,step,height_max', [
    (1, 60, 10, 2, 256, 64, 192), (2, 120, 0, 0, 128, 32, 96), (3, 200, 3, 1, 320, 32, 128), (5, 80, 10, 2, 512, 256, 256)])
def test_spill_onto_further_pages(seed, n, page_pad, pad, width_max, step, height_max):
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import stack_regions, stack_regions_pages
    shapes = random_shapes(seed, n)
    keep = np.random.default_rng(seed).random(n) < 0.8
    page_shapes, boxes, pages, packed, too_large = stack_regions_pages(shapes, page_pad, pad, width_max, step, height_max,
                                                                       keep=keep)
    Q = len(page_shapes)
    assert Q >= 2, 'the case must spill'
    assert np.array_equal(packed, keep) and not too_large.any() and (pages[~packed] == -1).all() and not boxes[~packed].any()
    assert sorted(set(pages[packed].tolist())) == list(range(Q)), 'no page is empty'
    # all pages share one width; only the last page is shorter
    Wp = page_shapes[0][1]
    assert all(shape == (height_max, Wp) for shape in page_shapes[:-1]) and page_shapes[-1][1] == Wp
    assert Wp % 32 == 0 and Wp <= width_max and page_shapes[-1][0] % step == 0 and step <= page_shapes[-1][0] <= height_max
    assert np.array_equal(boxes[packed][:, 2:], shapes[packed])
    assert Wp - 32 < (boxes[packed][:, 1] + boxes[packed][:, 3]).max() + page_pad, 'the smallest common width'
    order = [r for r in np.argsort(-shapes[:, 0], kind='stable') if packed[r]]
    keys = [(pages[r], boxes[r, 0], boxes[r, 1]) for r in order]
    assert keys == sorted(keys), 'shelves: stable order of decreasing height, page after page, row-major'
    for q, (Hp, _) in enumerate(page_shapes):
        idx = np.flatnonzero(pages == q)
        dy, dx, dh, dw = boxes[idx].T
        assert dy.min() == page_pad and dx.min() == page_pad, 'a page starts at (page_pad, page_pad)'
        assert (dy >= page_pad).all() and (dx >= page_pad).all()
        assert (dy + dh <= Hp - page_pad).all() and (dx + dw <= Wp - page_pad).all()
        if q == Q - 1:
            assert Hp - step < (dy + dh).max() + page_pad, 'the last page is the smallest that holds its rows'
        for a in range(len(idx)):
            for b in range(a + 1, len(idx)):
                apart_x = dx[a] + dw[a] + pad <= dx[b] or dx[b] + dw[b] + pad <= dx[a]
                apart_y = dy[a] + dh[a] + pad <= dy[b] or dy[b] + dh[b] + pad <= dy[a]
                assert apart_x or apart_y, (q, idx[a], idx[b])
        # the first row of the next page would have crossed height_max - page_pad on this one
        if q < Q - 1:
            nxt = [r for r in order if pages[r] == q + 1][0]
            last_row_y = dy.max()
            below = last_row_y + dh[dy == last_row_y].max() + pad
            assert below + shapes[nxt, 0] > height_max - page_pad
    # each page on its own is what stack_regions makes of its regions
    for q in range(Q):
        _, alone, alone_packed, _ = stack_regions(shapes, page_pad, pad, width_max, step, keep=pages == q)
        assert np.array_equal(alone_packed, pages == q) and np.array_equal(alone[pages == q], boxes[pages == q])


def test_spill_by_hand_too_tall_and_errors():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import stack_regions_pages
    # width 128, pads 10 / 2: a row holds 108 pixels.  height_max 96: rows may end at 86
    shapes = np.array([(40, 100), (30, 100), (30, 60), (77, 5), (20, 50), (0, 7), (10, 10)])
    keep = np.array([True, True, True, True, True, True, False])
    page_shapes, boxes, pages, packed, too_large = stack_regions_pages(shapes, 10, 2, 128, 32, 96, keep=keep)
    assert too_large.tolist() == [False, False, False, True, False, False, False]  # 77 > 96 - 20: reported, never clamped
    assert packed.tolist() == [True, True, True, False, True, False, False]       # the empty and the dropped are neither
    # page 0: 40 at y 10, 30 at y 52 (ends 82); the next 30 would end at 114 > 86: page 1 at y 10, the 20 beside it (62 + 50 > 118)
    assert pages.tolist() == [0, 0, 1, -1, 1, -1, -1]
    assert boxes.tolist() == [[10, 10, 40, 100], [52, 10, 30, 100], [10, 10, 30, 60], [0] * 4, [42, 10, 20, 50], [0] * 4, [0] * 4]
    assert page_shapes == [(96, 128), (96, 128)]
    page_shapes, _, pages, _, _ = stack_regions_pages(shapes[[0, 1, 2, 6]], 10, 2, 128, 32, 96)
    assert page_shapes == [(96, 128), (64, 128)] and pages.tolist() == [0, 0, 1, 1]  # a shorter last page
    for bad in (dict(height_max=100), dict(height_max=0), dict(height_step=48), dict(width_max=100), dict(page_pad=-1),
                dict(pad=-1), dict(height_max=32, page_pad=16)):
        args = dict(page_pad=10, pad=2, width_max=128, height_step=32, height_max=96)
        args.update(bad)
        with pytest.raises(ValueError):
            stack_regions_pages(shapes, **args)
    with pytest.raises(ValueError):
        stack_regions_pages(shapes, 10, 2, 128, 32, 96, keep=keep[:3])


def test_config_defaults():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import AdaptiveScalingInferencingConfig
    c = AdaptiveScalingInferencingConfig()
    assert c.precise_page_height_max == 1536 and c.precise_page_height_max % c.precise_page_height_step == 0
    assert c.rough_batch_max == 8


def labels_case():
    """tests/test_cpu_region_packing.py::labels_case: an 8 x 12 rough label map (valid 7 x 11) over a 28 x 44 image; regions
    1 and 2 interlock, region 3 is apart; three placements on a 70 x 100 page (label page 35 x 50 at factor 2)."""
    lab = np.zeros((8, 12), np.int32)
    lab[1:5, 1] = 1; lab[1, 1:6] = 1
    lab[3:5, 3:7] = 2
    lab[6, 9:11] = 3
    placements = np.array([(4, 4, 16, 20, 2, 3, 32, 40), (12, 12, 8, 16, 40, 1, 5, 9), (24, 36, 4, 8, 51, 60, 4, 8)], np.int32)
    return lab, (7, 11), (28, 44), placements, np.array([1, 2, 3], np.int32), (35, 50), 2


def multi(placements, src=0, page=0, local=None, glob=None):
    """(n, 8) placements -> (n, 12) multi rows of one source and page; ids default to 1..n."""
    placements = np.asarray(placements, np.int32).reshape(-1, 8)
    n = len(placements)
    col = lambda v, default: np.broadcast_to(np.asarray(default if v is None else v, np.int32), (n,))[:, None]
    ids = np.arange(1, n + 1)
    return np.concatenate([col(src, 0), col(page, 0), placements, col(local, ids), col(glob, ids)], axis=1).astype(np.int32)


def test_multi_pack_oracle_with_one_source_and_page_is_resample_host():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import resample_host, resample_pack_multi_host
    src = image(40, 50, 3)
    table = np.array([(0, 0, 40, 50, 1, 2, 12, 15), (5, 6, 7, 8, 20, 3, 19, 21), (30, 40, 10, 10, 0, 30, 10, 10)], np.int32)
    got = resample_pack_multi_host([src], multi(table), (48, 64), 1)
    assert got.shape == (1, 48, 64, 3) and got.dtype == np.uint8 and np.array_equal(got[0], resample_host(src, table, (48, 64)))
    # two sources, three pages, the middle one empty: each page is the sum of what its sources put there
    other = image(9, 200, 4)
    rows = np.concatenate([multi(table[:2], src=0, page=0), multi([(0, 0, 9, 200, 40, 0, 3, 64)], src=1, page=0),
                           multi([(2, 100, 7, 100, 12, 5, 30, 30)], src=1, page=2), multi(table[2:], src=0, page=2)])
    got = resample_pack_multi_host([src, other], rows, (48, 64), 3)
    want0 = resample_host(src, table[:2], (48, 64)) + resample_host(other, np.array([(0, 0, 9, 200, 40, 0, 3, 64)], np.int32), (48, 64))
    want2 = resample_host(other, np.array([(2, 100, 7, 100, 12, 5, 30, 30)], np.int32), (48, 64)) + resample_host(src, table[2:], (48, 64))
    assert np.array_equal(got[0], want0) and not got[1].any() and np.array_equal(got[2], want2)


def test_multi_label_oracle_with_one_source_and_page_is_pack_region_labels_host():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import pack_region_labels_host, pack_region_labels_multi_host
    lab, valid, shape, placements, ids, out_shape, fdf = labels_case()
    want = pack_region_labels_host(lab, valid, shape, placements, ids, out_shape, fdf)
    got = pack_region_labels_multi_host([lab], [valid], [shape], multi(placements, local=ids, glob=ids), out_shape, fdf, 1)
    assert got.shape == (1, 35, 50) and got.dtype == np.int32 and np.array_equal(got[0], want)
    # the same image twice: local ids coincide, global ids do not, and the exclusion rule follows the local ones
    rows = np.concatenate([multi(placements, src=0, page=0, local=ids, glob=ids),
                           multi(placements, src=1, page=1, local=ids, glob=ids + 3)])
    got = pack_region_labels_multi_host([lab, lab], [valid] * 2, [shape] * 2, rows, out_shape, fdf, 2)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], np.where(want > 0, want + 3, 0))


def test_check_multi_rows():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import check_multi_rows
    shapes = [(20, 30), (10, 40)]
    good = np.concatenate([multi([(0, 0, 20, 30, 0, 0, 4, 4), (1, 1, 5, 5, 4, 0, 4, 4)], src=0, page=0),
                           multi([(0, 0, 10, 40, 0, 0, 4, 4)], src=1, page=1)])  # the same destination on two pages
    out = check_multi_rows(good.astype(np.int64), shapes, (8, 8), 2)
    assert out.dtype == np.int32 and out.flags.c_contiguous and np.array_equal(out, good)
    assert check_multi_rows(np.zeros((0, 12), np.int32), shapes, (8, 8), 2).shape == (0, 12)

    def bad(match, **change):
        rows = good.copy()
        for (r, c), v in change.get('cells', {}).items():
            rows[r, c] = v
        with pytest.raises(ValueError, match=match):
            check_multi_rows(rows, shapes, change.get('page_shape', (8, 8)), change.get('pages', 2))

    bad('source index', cells={(0, 0): 2})
    bad('source index', cells={(0, 0): -1})
    bad('page index', cells={(2, 1): 2})
    bad('page index', cells={(0, 1): -1})
    bad('sorted by page', cells={(0, 1): 1})
    bad('leaves its source', cells={(2, 2): 1})          # 1 + 10 > 10 rows of source 1 ...
    bad('leaves its source', cells={(2, 0): 0})          # ... and its 40 columns do not fit source 0
    bad('destination rectangle leaves', cells={(1, 6): 5})
    bad('side', cells={(1, 9): 0})
    bad('overlap on page 0', cells={(1, 6): 3})
    bad('start at 1', cells={(1, 10): 0})
    with pytest.raises(ValueError, match=r'\(n, 12\)'):
        check_multi_rows(good[:, :8], shapes, (8, 8), 2)
    with pytest.raises(ValueError, match=r'\(n, 12\)'):
        check_multi_rows(good.astype(np.float32), shapes, (8, 8), 2)


def test_c_entry_points_validate_before_launch():
    from vkit_ocr_model_adaptive_scaling_amd import _lib
    L, P = _lib.lib, ctypes.c_void_p
    a = lambda: P(256)  # any aligned non-null address: the checks run before anything is dereferenced or launched

    def pack(*, arena=a(), size=64, sources=a(), S=1, rows=a(), n=1, start=a(), pages=a(), Q=1, Hp=8, Wp=8):
        return L.vkas_resample_pack_u8_multi(arena, size, sources, S, rows, n, start, pages, Q, Hp, Wp, None)

    def lab(*, arena=a(), size=64, sources=a(), S=1, rows=a(), n=1, start=a(), fdf=2, out=a(), Q=1, Hq=8, Wq=8):
        return L.vkas_pack_region_labels_multi(arena, size, sources, S, rows, n, start, fdf, out, Q, Hq, Wq, None)

    for call, out in ((pack, 'pages'), (lab, 'out')):
        for name in ('arena', 'sources', 'start', out):
            assert call(**{name: None}) == -1 and b'null pointer' in L.vkas_last_error()
        assert call(rows=None) == -1 and b'bad table' in L.vkas_last_error()
        assert call(n=-1) == -1 and b'bad table' in L.vkas_last_error()
        assert call(size=0) == -1 and b'empty arena' in L.vkas_last_error()
        assert call(S=0) == -1 and b'empty arena' in L.vkas_last_error()
        assert call(Q=0) == -1 and b'65535' in L.vkas_last_error()
        assert call(Q=65536) == -1 and b'65535' in L.vkas_last_error()
        assert call(rows=P(264)) == -1 and b'aligned' in L.vkas_last_error()
        assert call(sources=P(260)) == -1 and b'aligned' in L.vkas_last_error()
        assert call(start=P(258)) == -1 and b'aligned' in L.vkas_last_error()
    assert pack(Hp=0) == -1 and pack(Wp=40000) == -1 and b'32768' in L.vkas_last_error()
    assert lab(Hq=0) == -1 and lab(Hq=20000) == -1 and b'32768' in L.vkas_last_error()
    assert lab(fdf=0) == -1 and b'bad factor' in L.vkas_last_error()
    assert lab(arena=P(258)) == -1 and b'aligned' in L.vkas_last_error()


def test_ops_wrappers_validate_before_launch():
    from vkit_ocr_model_adaptive_scaling_amd import ops
    arena = torch.zeros(20 * 30 * 3 + 16, dtype=torch.uint8)
    sources = np.array([[16, 20, 30, 0]], np.int64)
    good = multi([(0, 0, 5, 5, 0, 0, 4, 4)])
    call = lambda **kw: ops.resample_pack_u8_multi(**{**dict(arena=arena, sources=sources, rows=good, num_pages=1,
                                                             page_shape=(8, 8)), **kw})
    with pytest.raises(ValueError, match='1-D uint8'):
        call(arena=arena.view(-1, 4))
    with pytest.raises(ValueError, match='1-D uint8'):
        call(arena=arena.int())
    with pytest.raises(ValueError, match='page_shape'):
        call(page_shape=8)
    with pytest.raises(ValueError, match='32768'):
        call(page_shape=(8, 40000))
    with pytest.raises(ValueError, match='num_pages'):
        call(num_pages=0)
    with pytest.raises(ValueError, match=r'sources must be \(None, 4\)'):
        call(sources=np.zeros((1, 8), np.int64))
    with pytest.raises(ValueError, match='int64'):
        call(sources=sources.astype(np.int32))
    with pytest.raises(ValueError, match='leaves the arena'):
        call(sources=np.array([[17, 20, 30, 0]], np.int64))
    with pytest.raises(ValueError, match='leaves the arena'):
        call(sources=np.array([[-16, 20, 30, 0]], np.int64))
    with pytest.raises(ValueError, match='sides'):
        call(sources=np.array([[0, 0, 30, 0]], np.int64))
    with pytest.raises(ValueError, match=r'rows must be \(None, 12\)'):
        call(rows=good[:, :8])
    with pytest.raises(ValueError, match='int32'):
        call(rows=good.astype(np.int64))
    with pytest.raises(ValueError, match='source index'):
        call(rows=multi([(0, 0, 5, 5, 0, 0, 4, 4)], src=1))
    with pytest.raises(ValueError, match='page index'):
        call(rows=multi([(0, 0, 5, 5, 0, 0, 4, 4)], page=1))
    with pytest.raises(ValueError, match='leaves its source'):
        call(rows=multi([(0, 0, 21, 5, 0, 0, 4, 4)]))
    with pytest.raises(ValueError, match='overlap'):
        call(rows=multi([(0, 0, 5, 5, 0, 0, 4, 4), (0, 0, 5, 5, 3, 3, 4, 4)]))
    with pytest.raises(ValueError, match='page_start'):
        call(page_start=np.array([0, 0], np.int32))
    with pytest.raises(ValueError, match='page_start must be'):
        call(page_start=np.array([0, 1, 1], np.int32))
    with pytest.raises(ValueError, match='out must be'):
        call(out=torch.zeros(1, 8, 8, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='MI355X'):
        call()  # valid arguments: no CPU fallback
    labels = torch.zeros(10 * 15 + 4, dtype=torch.int32)
    label_sources = np.array([[4, 10, 15, 10, 15, 20, 30, 0]], np.int64)
    call = lambda **kw: ops.pack_region_labels_multi(**{**dict(label_arena=labels, label_sources=label_sources, rows=good,
                                                               num_pages=1, out_shape=(4, 4), fdf=2), **kw})
    with pytest.raises(ValueError, match='1-D int32'):
        call(label_arena=labels.long())
    with pytest.raises(ValueError, match='fdf'):
        call(fdf=0)
    with pytest.raises(ValueError, match='fdf'):
        call(fdf=1.5)
    with pytest.raises(ValueError, match=r'sources must be \(None, 8\)'):
        call(label_sources=sources)
    with pytest.raises(ValueError, match='valid part'):
        call(label_sources=np.array([[4, 10, 15, 11, 15, 20, 30, 0]], np.int64))
    with pytest.raises(ValueError, match='leaves the arena'):
        call(label_sources=np.array([[5, 10, 15, 10, 15, 20, 30, 0]], np.int64))
    with pytest.raises(ValueError, match='destination rectangle leaves'):
        call(out_shape=(1, 4))  # the page is out_shape * fdf: 2 x 8 does not hold a 4 x 4 destination
    with pytest.raises(ValueError, match='out must be'):
        call(out=torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='MI355X'):
        call()
