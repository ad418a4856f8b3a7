"""The multi-source, multi-page pack on the MI355X (csrc/respack.hip's multi kernels, ops.resample_pack_u8_multi,
ops.pack_region_labels_multi) against the host oracles of inferencing/packing.py (checked on their own in
test_cpu_region_pages.py): every comparison is exact equality, eager and once captured in a graph and replayed with the
tables changed in place.  Three sources of different sizes share one arena; rows shrink and enlarge, cross the 16-row and
64-column tile seams and touch the page's last column; pages are 128 wide (dword / vector stores) and 130 wide (byte stores,
a label page of 65 columns); one page has no rows; one has more than 64, so the per-block search takes a second batch.  Rows
the kernels must skip are sent with ``validate=False``: a failure shows as a wrong byte - every output is prefilled with 0xFF -
and never as an out-of-bounds access, because every address is checked against the arena's size before use."""
import numpy as np
import pytest
import torch

from tests import test_cpu_region_pages as C

pytestmark = pytest.mark.gpu

SHAPES = [(37, 53), (64, 40), (9, 200)]
SOURCES = [C.image(h, w, 11 + k) for k, (h, w) in enumerate(SHAPES)]
FDF = 2


def blocky(seed, H, W, ids=3):
    g = np.random.default_rng(seed)
    return np.repeat(np.repeat(g.integers(0, ids + 1, (-(-H // 4), -(-W // 4))), 4, axis=0), 4, axis=1).astype(np.int32)[:H, :W]


# rough label maps with local ids 1..3: (map shape, valid part) per source; the first and the last are padded
LABEL_SHAPES = [((20, 28), (19, 27)), ((32, 20), (32, 20)), ((6, 100), (5, 100))]
LABEL_MAPS = [blocky(21 + k, *shape) for k, (shape, _) in enumerate(LABEL_SHAPES)]


def image_arena(sources, pad_byte=0xA5):
    """(flat uint8 arena with every image start 16-byte aligned, (S, 4) int64 table)"""
    table, total = [], 16  # the first image does not start the arena
    for s in sources:
        table.append((total, s.shape[0], s.shape[1], 0))
        total += -(-s.size // 16) * 16
    flat = np.full((total,), pad_byte, np.uint8)
    for s, (off, _, _, _) in zip(sources, table):
        flat[off:off + s.size] = s.reshape(-1)
    return flat, np.array(table, np.int64)


def label_arena(maps, valids, shapes):
    table, total = [], 3
    for m, (vh, vw), (Hs, Ws) in zip(maps, valids, shapes):
        table.append((total, m.shape[0], m.shape[1], vh, vw, Hs, Ws, 0))
        total += m.size + 5
    flat = np.full((total,), 7, np.int32)  # 7: no region's id; a read outside a map shows
    for m, row in zip(maps, table):
        flat[row[0]:row[0] + m.size] = m.reshape(-1)
    return flat, np.array(table, np.int64)


ARENA, TABLE = image_arena(SOURCES)
LABELS, LABEL_TABLE = label_arena(LABEL_MAPS, [v for _, v in LABEL_SHAPES], SHAPES)


def build(entries):
    """[(slice page, src, page, placement, local id, global id)] -> (n, 12) int32 rows sorted by slice, Q-free page_start
    builder: ``start(Q)``.  The slice is the page whose blocks search the row; it differs from ``page`` only in a bad row."""
    entries = sorted(entries, key=lambda e: e[0])
    rows = np.array([(src, page) + tuple(p) + (local, glob) for _, src, page, p, local, glob in entries], np.int32).reshape(-1, 12)
    slices = np.array([e[0] for e in entries], np.int64)
    return rows, lambda Q: np.searchsorted(slices, np.arange(Q + 1)).astype(np.int32)


def base_entries(Wp, pages=(0, 1)):
    a, b = pages
    return [
        (a, 0, a, (0, 0, 37, 53, 1, 2, 11, 16), 1, 11),           # the whole image at ratio 0.3
        (a, 1, a, (0, 0, 64, 40, 10, 50, 27, 30), 2, 12),         # across tile rows 16 and 32 and tile column 64
        (a, 2, a, (0, 100, 9, 64, 38, 101, 9, 1), 1, 13),         # 64 columns -> 1, under a label cell's centre
        (a, 0, a, (3, 3, 8, 8, 40, Wp - 9, 8, 9), 3, 14),         # up to the page's last column and row
        (b, 2, b, (2, 10, 5, 20, 20, 60, 14, 54), 2, 15),         # x2.7 across tile column 64 and tile row 32
        (b, 0, b, (5, 5, 30, 40, 0, 0, 30, 40), 3, 16),           # the identity across tile row 16
        (b, 1, b, (10, 3, 50, 30, 33, 2, 15, 50), 1, 17),         # shrunk in y, enlarged in x
    ]


def oracles(rows, Q, page_shape):
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import pack_region_labels_multi_host, resample_pack_multi_host
    out_shape = (-(-page_shape[0] // FDF), -(-page_shape[1] // FDF))
    return (resample_pack_multi_host(SOURCES, rows, page_shape, Q),
            pack_region_labels_multi_host(LABEL_MAPS, [v for _, v in LABEL_SHAPES], SHAPES, rows, out_shape, FDF, Q), out_shape)


def device(rows, start, Q, page_shape, out_shape, validate=True, table=TABLE, label_table=LABEL_TABLE):
    from vkit_ocr_model_adaptive_scaling_amd import ops
    up = (lambda a: torch.from_numpy(a).cuda()) if not validate else (lambda a: a)
    out = torch.full((Q,) + tuple(page_shape) + (3,), 0xFF, dtype=torch.uint8, device='cuda')
    pages = ops.resample_pack_u8_multi(torch.from_numpy(ARENA).cuda(), up(table), up(rows), Q, page_shape, page_start=up(start),
                                       validate=validate, out=out)
    assert pages.data_ptr() == out.data_ptr()
    out = torch.full((Q,) + tuple(out_shape), -1, dtype=torch.int32, device='cuda')
    labels = ops.pack_region_labels_multi(torch.from_numpy(LABELS).cuda(), up(label_table), up(rows), Q, out_shape, FDF,
                                          page_start=up(start), validate=validate, out=out)
    assert labels.data_ptr() == out.data_ptr()
    return pages.cpu().numpy(), labels.cpu().numpy()


def assert_equal(got, want):
    for g, w, name in zip(got, want, ('pages', 'labels')):
        assert g.dtype == w.dtype and g.shape == w.shape
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (name, len(bad), bad[:5].tolist())


@pytest.mark.parametrize('Wp', [128, 130])
def test_three_sources_two_pages(Wp):
    rows, start = build(base_entries(Wp))
    want_pages, want_labels, out_shape = oracles(rows, 2, (48, Wp))
    assert_equal(device(rows, start(2), 2, (48, Wp), out_shape), (want_pages, want_labels))
    assert_equal(device(rows, None, 2, (48, Wp), out_shape), (want_pages, want_labels))  # page_start from the host rows
    assert out_shape[1] % 4 == (0 if Wp == 128 else 1)
    from vkit_ocr_model_adaptive_scaling_amd.inferencing.packing import label_cells
    inside = np.zeros(want_labels.shape, bool)
    for _, page, _, _, _, _, dy, dx, dh, dw, _, _ in rows.tolist():
        (v0, v1), (u0, u1) = label_cells(dy, dh, FDF), label_cells(dx, dw, FDF)
        inside[page, v0:v1, u0:u1] = True
    # a neighbour's local id under a cell gives 0, the region's own and background give the global id
    assert (want_labels[inside] == 0).any() and not want_labels[~inside].any()
    assert set(np.unique(want_labels).tolist()) == {0, *rows[:, 11].tolist()}, 'every row shows, under its global id'
    assert want_pages.any(axis=(1, 2, 3)).all()


@pytest.mark.parametrize('Wp', [128, 130])
def test_empty_pages(Wp):
    # an empty middle page: Q = 3, page_start (0, 4, 4, 7)
    rows, start = build(base_entries(Wp, pages=(0, 2)))
    assert start(3).tolist() == [0, 4, 4, 7]
    want_pages, want_labels, out_shape = oracles(rows, 3, (48, Wp))
    got = device(rows, start(3), 3, (48, Wp), out_shape)
    assert_equal(got, (want_pages, want_labels))
    assert not got[0][1].any() and not got[1][1].any() and got[0][0].any() and got[0][2].any()
    # no rows at all
    none = np.zeros((0, 12), np.int32)
    got = device(none, np.zeros((3,), np.int32), 2, (17, Wp), (9, Wp // 2))
    assert got[0].shape == (2, 17, Wp, 3) and not got[0].any() and not got[1].any()


def test_more_than_64_rows_on_one_page():
    g = np.random.default_rng(5)
    entries = []
    for i in range(70):
        src = i % 3
        sh, sw = (int(v) for v in g.integers(1, 7, 2))
        sy, sx = int(g.integers(0, SHAPES[src][0] - sh + 1)), int(g.integers(0, SHAPES[src][1] - sw + 1))
        entries.append((0, src, 0, (sy, sx, sh, sw, 2 + (i % 5) * 9, 3 + 7 * i, 3, 3), 1 + i % 3, 100 + i))
    rows, start = build(entries)
    want_pages, want_labels, out_shape = oracles(rows, 1, (48, 512))
    assert_equal(device(rows, start(1), 1, (48, 512), out_shape), (want_pages, want_labels))
    assert all(want_pages[0, 2 + (i % 5) * 9:, 3 + 7 * i:][:3, :3].any() for i in range(70)), 'every placement shows'


@pytest.mark.parametrize('Wp', [128, 130])
def test_rows_that_must_be_skipped(Wp):
    good = base_entries(Wp)
    S = len(SOURCES)
    # a fourth and a fifth source entry that leave their arenas: by their size, and by a negative offset
    table = np.concatenate([TABLE, [[len(ARENA) - 3 * 8 * 8 + 1, 8, 8, 0], [-16, 8, 8, 0]]]).astype(np.int64)
    label_table = np.concatenate([LABEL_TABLE, [[len(LABELS) - 4 * 4 + 1, 4, 4, 4, 4, 8, 8, 0],
                                                [-1, 4, 4, 4, 4, 8, 8, 0]]]).astype(np.int64)
    free = lambda k: (13 + 5 * (k // 4), 84 + 5 * (k % 4), 4, 4)  # 4 x 4 destinations no good row reaches, on page 0
    bad = [
        (0, S + 2, 0, (0, 0, 4, 4) + free(0), 1, 90),   # src = S (of this table)
        (0, -1, 0, (0, 0, 4, 4) + free(1), 1, 91),      # src = -1
        (0, 0, 1, (0, 0, 4, 4) + free(2), 1, 92),       # page 1 in the slice of page 0
        (0, 0, 0, (34, 0, 4, 4) + free(3), 1, 93),      # a source rectangle one pixel past its image, below ...
        (0, 0, 0, (0, 50, 4, 4) + free(4), 1, 94),      # ... and to the right
        (0, S, 0, (0, 0, 4, 4) + free(5), 1, 95),       # a source entry whose offset + size exceeds the arena
        (0, S + 1, 0, (0, 0, 4, 4) + free(6), 1, 96),   # a source entry with a negative offset
        (0, 0, 0, (0, 0, 0, 4) + free(7), 1, 97),       # an empty side
        (1, 0, 0, (0, 0, 4, 4) + (40, 60, 4, 4), 1, 98),  # page 0 in the slice of page 1
    ]
    rows, start = build(good + bad)
    good_rows, _ = build(good)
    want_pages, want_labels, out_shape = oracles(good_rows, 2, (48, Wp))
    for k in range(8):
        dy, dx, dh, dw = free(k)
        assert not want_pages[0, dy:dy + dh, dx:dx + dw].any(), 'the bad rows point at free page area'
    assert not want_pages[1, 40:44, 60:64].any()
    got = device(rows, start(2), 2, (48, Wp), out_shape, validate=False, table=table, label_table=label_table)
    assert_equal(got, (want_pages, want_labels))
    # a page_start that leaves the table is clamped
    wild = np.array([-5, 4, 1000], np.int32)
    assert_equal(device(good_rows, wild, 2, (48, Wp), out_shape, validate=False), (want_pages, want_labels))


def test_coinciding_local_ids_get_different_global_ids():
    # test_cpu_region_pages.labels_case twice: both images have regions 1, 2, 3; the second image's become 4, 5, 6
    from vkit_ocr_model_adaptive_scaling_amd import ops
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import pack_region_labels_host, pack_region_labels_multi_host
    lab, valid, shape, placements, ids, out_shape, fdf = C.labels_case()
    flat, table = label_arena([lab, lab], [valid] * 2, [shape] * 2)
    rows = np.concatenate([C.multi(placements, src=0, page=0, local=ids, glob=ids),
                           C.multi(placements, src=1, page=1, local=ids, glob=ids + 3)])
    want = pack_region_labels_multi_host([lab, lab], [valid] * 2, [shape] * 2, rows, out_shape, fdf, 2)
    got = ops.pack_region_labels_multi(torch.from_numpy(flat).cuda(), table, rows, 2, out_shape, fdf).cpu().numpy()
    assert np.array_equal(got, want)
    single = pack_region_labels_host(lab, valid, shape, placements, ids, out_shape, fdf)
    assert np.array_equal(got[0], single) and np.array_equal(got[1], np.where(single > 0, single + 3, 0))
    assert (single == 0).any() and set(np.unique(got[1]).tolist()) == {0, 4, 5, 6}


def test_one_source_one_page_equals_the_single_image_kernels():
    from vkit_ocr_model_adaptive_scaling_amd import ops
    src = SOURCES[0]
    table = np.array([(0, 0, 37, 53, 1, 2, 11, 16), (3, 3, 30, 8, 10, 50, 27, 30), (5, 5, 30, 40, 14, 88, 30, 40),
                      (1, 1, 5, 20, 45, 3, 14, 54)], np.int32)
    ids = np.array([2, 1, 3, 2], np.int32)
    flat, sources = image_arena([src])
    lab_flat, lab_sources = label_arena(LABEL_MAPS[:1], [LABEL_SHAPES[0][1]], SHAPES[:1])
    rows = C.multi(table, local=ids, glob=ids)
    for page_shape in ((64, 128), (61, 130)):
        out_shape = (-(-page_shape[0] // FDF), -(-page_shape[1] // FDF))
        single = ops.resample_pack_u8(torch.from_numpy(src).cuda(), table, page_shape)
        pages = ops.resample_pack_u8_multi(torch.from_numpy(flat).cuda(), sources, rows, 1, page_shape)
        assert pages.shape == (1,) + page_shape + (3,) and torch.equal(pages[0], single) and bool(single.any())
        single = ops.pack_region_labels(torch.from_numpy(LABEL_MAPS[0]).cuda(), LABEL_SHAPES[0][1], SHAPES[0], table, ids,
                                        out_shape, FDF)
        labels = ops.pack_region_labels_multi(torch.from_numpy(lab_flat).cuda(), lab_sources, rows, 1, out_shape, FDF)
        assert torch.equal(labels[0], single) and bool(single.any())


def test_captured_graph_replays_with_the_tables_changed_in_place():
    from vkit_ocr_model_adaptive_scaling_amd import ops
    Wp, Q = 128, 3
    cases = []
    for pages, shift in (((0, 1), 0), ((0, 2), 1), ((1, 2), 2), ((0, 1), 0)):  # other pages, other ids, the first again
        entries = [(a, src, page, p, 1 + (local + shift) % 3, glob + 10 * shift)
                   for a, src, page, p, local, glob in base_entries(Wp, pages)]
        rows, start = build(entries)
        cases.append((rows, start(Q)) + oracles(rows, Q, (48, Wp))[:2])
    out_shape = (24, Wp // 2)
    d_arena, d_table = torch.from_numpy(ARENA).cuda(), torch.from_numpy(TABLE).cuda()
    d_labels, d_label_table = torch.from_numpy(LABELS).cuda(), torch.from_numpy(LABEL_TABLE).cuda()
    d_rows, d_start = torch.from_numpy(cases[0][0]).cuda(), torch.from_numpy(cases[0][1]).cuda()
    run = lambda: (ops.resample_pack_u8_multi(d_arena, d_table, d_rows, Q, (48, Wp), page_start=d_start, validate=False),
                   ops.pack_region_labels_multi(d_labels, d_label_table, d_rows, Q, out_shape, FDF, page_start=d_start,
                                                validate=False))
    run()  # eager first
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_pages, out_labels = run()
    for rows, start, want_pages, want_labels in cases:
        d_rows.copy_(torch.from_numpy(rows))
        d_start.copy_(torch.from_numpy(start))
        graph.replay()
        torch.cuda.synchronize()
        assert_equal((out_pages.cpu().numpy(), out_labels.cpu().numpy()), (want_pages, want_labels))
