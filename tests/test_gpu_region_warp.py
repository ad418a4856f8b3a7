"""Affine warps into the page on the MI355X (csrc/respack.hip, ops.warp_pack_u8 / ops.warp_region_labels) against the host
definitions of inferencing/packing.py (checked on their own in test_cpu_orient.py): exact equality, and every byte / cell
outside the destinations keeps its prefill.  The kernels share the 16 x 64 tiles and the per-block table search of the
axis-aligned kernels, so the seams are: tile corners, quads that straddle a destination's edge, page widths that are no
multiple of 4, more rows than one pass of the search takes, rows the kernel must skip; and of the sampling: every sub-sample
count, coefficients of both signs, taps outside the source on all four sides."""
import numpy as np
import pytest
import torch

from tests.test_cpu_orient import identity_row, image, quarter_turn_row

pytestmark = pytest.mark.gpu

SRC = image(23, 31, 3)
FILL = 0xAB


def device_warp(src, warps, page_shape, validate=True):
    from vkit_ocr_model_adaptive_scaling_amd import ops
    page = torch.full(tuple(page_shape) + (3,), FILL, dtype=torch.uint8, device='cuda')
    table = torch.from_numpy(np.asarray(warps)).cuda() if not validate else warps
    out = ops.warp_pack_u8(torch.from_numpy(src).cuda(), table, page, validate=validate)
    assert out.data_ptr() == page.data_ptr()
    return out.cpu().numpy()


def assert_warp_equals_host(src, warps, page_shape):
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import warp_host
    warps = np.asarray(warps, dtype=np.int64).reshape(-1, 12)
    want = warp_host(src, warps, np.full(tuple(page_shape) + (3,), FILL, np.uint8))
    got = device_warp(src, warps, page_shape)
    outside = np.ones(page_shape, bool)
    for dy, dx, dh, dw in warps[:, :4].tolist():
        outside[dy:dy + dh, dx:dx + dw] = False
    assert (got[outside] == FILL).all(), 'a byte outside the destinations was written'
    assert (want[outside] == FILL).all()
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, (len(bad), bad[:5].tolist())
    return want


def random_row(g, dy, dx, dh, dw, log2n, reach=1.0):
    """A warp whose source parallelogram is centred somewhere in (or, ``reach`` > 1, around) SRC: rotation by any angle,
    per-axis steps between 1/3 and 3 source pixels, so coefficients of both signs."""
    Hs, Ws = SRC.shape[:2]
    t = g.uniform(-np.pi, np.pi)
    sy, sx = g.uniform(1 / 3, 3, 2)
    myy, myx = round(65536 * np.cos(t) * sy), round(65536 * np.sin(t) * sx)
    mxy, mxx = round(-65536 * np.sin(t) * sy), round(65536 * np.cos(t) * sx)
    yc, xc = g.uniform(-(reach - 1) * Hs, reach * Hs), g.uniform(-(reach - 1) * Ws, reach * Ws)
    ay = round(65536 * yc - ((dh - 1) * myy + (dw - 1) * myx) / 2)
    ax = round(65536 * xc - ((dh - 1) * mxy + (dw - 1) * mxx) / 2)
    return [dy, dx, dh, dw, ay, ax, myy, myx, mxy, mxx, log2n, 0]


def grid_rows(seed, page_shape, cell, log2n=None, reach=1.0):
    """One random warp of random size (up to the cell) in every cell x cell square of the page."""
    g = np.random.default_rng(seed)
    rows = []
    for y in range(0, page_shape[0] - cell + 1, cell):
        for x in range(0, page_shape[1] - cell + 1, cell):
            dh, dw = (int(v) for v in g.integers(1, cell + 1, 2))
            rows.append(random_row(g, y + int(g.integers(0, cell - dh + 1)), x + int(g.integers(0, cell - dw + 1)), dh, dw,
                                   int(g.integers(0, 4)) if log2n is None else log2n, reach))
    return np.array(rows, np.int64)


def test_identity_and_quarter_turn():
    rows = [identity_row(3, 4, 2, 5, 11, 13), quarter_turn_row(6, 2, 9, 17, 20, 30)]
    want = assert_warp_equals_host(SRC, rows, (40, 72))
    assert np.array_equal(want[2:13, 5:18], SRC[3:14, 4:17])
    assert np.array_equal(want[20:37, 30:39], SRC[6:15, 2:19].transpose(1, 0, 2)[::-1])


@pytest.mark.parametrize('log2n', [0, 1, 2, 3])
def test_random_rows_every_subsample_count(log2n):
    rows = grid_rows(10 + log2n, (40, 72), 13, log2n=log2n)
    assert (rows[:, 6:10] < 0).any() and (rows[:, 6:10] > 0).any()
    assert_warp_equals_host(SRC, rows, (40, 72))


def test_page_width_no_multiple_of_four_and_mixed_subsamples():
    assert_warp_equals_host(SRC, grid_rows(20, (41, 71), 10), (41, 71))


def test_destination_across_a_tile_corner():
    g = np.random.default_rng(21)
    rows = [random_row(g, 9, 57, 14, 15, 1), random_row(g, 30, 120, 5, 17, 2), identity_row(0, 0, 31, 63, 2, 2)]
    assert_warp_equals_host(SRC, rows, (40, 140))


def test_taps_outside_the_source_on_all_four_sides():
    rows = [identity_row(-3, -4, 0, 0, 30, 40),                              # the whole source with a margin all round
            [0, 40, 8, 8, -65536 // 2, -65536 // 2, 65536, 0, 0, 65536, 1, 0],  # half-pixel taps across the top-left corner
            [8, 40, 8, 8, 65536 * 19 + 30000, 65536 * 27 + 30000, 65536, 0, 0, 65536, 0, 0],  # across the bottom-right corner
            identity_row(100, 100, 16, 40, 4, 4)]                            # entirely outside: zeros
    want = assert_warp_equals_host(SRC, rows, (40, 72))
    assert np.array_equal(want[3:26, 4:35], SRC) and not want[0:3, 0:40].any() and not want[26:30, 0:40].any()
    assert not want[0:30, 0:4].any() and not want[0:30, 35:40].any() and not want[16:20, 40:44].any()
    more = grid_rows(22, (40, 72), 12, reach=1.6)
    assert_warp_equals_host(SRC, more, (40, 72))


def test_one_pixel_destinations_and_300_rows():
    g = np.random.default_rng(23)
    ys, xs = np.mgrid[1:31:2, 1:41:2]  # 15 x 20 = 300 one-pixel destinations: more than one 256-row pass of the search
    rows = np.array([random_row(g, int(y), int(x), 1, 1, int(g.integers(0, 4))) for y, x in zip(ys.ravel(), xs.ravel())], np.int64)
    assert len(rows) == 300
    assert_warp_equals_host(SRC, rows, (40, 72))


def test_no_rows_leaves_the_page_alone():
    got = device_warp(SRC, np.zeros((0, 12), np.int64), (17, 65))
    assert (got == FILL).all()


def test_out_of_bounds_rows_are_skipped():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import warp_host
    good = grid_rows(24, (40, 72), 20, log2n=1)
    bad = [identity_row(0, 0, 0, 0, 40, 72, log2n=4), [0, 0, 40, 72, 1 << 40, 0, 65536, 0, 0, 65536, 0, 0],
           [0, 0, 40, 72, 0, 0, (1 << 22) + 1, 0, 0, 65536, 0, 0], [0, 0, 0, 72, 0, 0, 65536, 0, 0, 65536, 0, 0],
           [0, 0, 8193, 72, 0, 0, 65536, 0, 0, 65536, 0, 0], [-1, 0, 40, 72, 0, 0, 65536, 0, 0, 65536, 0, 0],
           [0, 0, 40, 72, 0, 0, 65536, 0, 0, -(1 << 22) - 1, 0, 0]]
    table = np.concatenate([np.array(bad[:3], np.int64), good[:2], np.array(bad[3:], np.int64), good[2:]])
    got = device_warp(SRC, table, (40, 72), validate=False)  # a device table, trusted: the kernel itself skips the bad rows
    want = warp_host(SRC, good, np.full((40, 72, 3), FILL, np.uint8))
    assert np.array_equal(got, want)


def labels_case(seed, fdf, page_shape=(40, 72)):
    """The warps of a random table over a blocky rough label map (regions 0..5, so that a destination's source runs over a
    neighbour's label) whose valid part covers an image of SRC's size."""
    g = np.random.default_rng(seed)
    lab = np.repeat(np.repeat(g.integers(0, 6, (5, 6)), 3, axis=0), 3, axis=1).astype(np.int32)[:14, :17]
    valid, shape = (12, 16), SRC.shape[:2]
    rows = grid_rows(seed, page_shape, 13, reach=1.3)
    ids = g.integers(1, 6, len(rows)).astype(np.int32)
    out_shape = (-(-page_shape[0] // fdf), -(-page_shape[1] // fdf))
    return lab, valid, shape, rows, ids, out_shape, fdf


@pytest.mark.parametrize('fdf', [1, 2])
@pytest.mark.parametrize('seed', [31, 32])
def test_label_cells_match_host(seed, fdf):
    from vkit_ocr_model_adaptive_scaling_amd import ops
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import warp_region_labels_host
    from vkit_ocr_model_adaptive_scaling_amd.inferencing.packing import label_cells
    lab, valid, shape, rows, ids, out_shape, fdf = labels_case(seed, fdf)
    prefill = np.full(out_shape, -7, np.int32)
    want = warp_region_labels_host(lab, valid, shape, rows, ids, prefill, fdf)
    got = ops.warp_region_labels(torch.from_numpy(lab).cuda(), valid, shape, rows, ids, torch.from_numpy(prefill).cuda(), fdf)
    got = got.cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want)
    inside = np.zeros(out_shape, bool)
    for dy, dx, dh, dw in rows[:, :4].tolist():
        (v0, v1), (u0, u1) = label_cells(dy, dh, fdf), label_cells(dx, dw, fdf)
        inside[v0:v1, u0:u1] = True
    assert (want[~inside] == -7).all() and (want[inside] != -7).all(), 'exactly the cells inside the destinations are written'
    assert (want[inside] == 0).any() and (want[inside] > 0).any(), 'a neighbour under part of a destination, and the region itself'


def test_label_cells_identity_row_by_hand():
    from vkit_ocr_model_adaptive_scaling_amd import ops
    lab = np.zeros((12, 16), np.int32)
    lab[:, 8:] = 2   # the right half of the rough map belongs to region 2
    rows = np.array([identity_row(0, 0, 4, 6, 23, 31)], np.int64)   # the whole image at page (4, 6), as region 1
    out = ops.warp_region_labels(torch.from_numpy(lab).cuda(), (12, 16), (23, 31), rows, np.array([1], np.int32),
                                 torch.zeros((40, 72), dtype=torch.int32, device='cuda'), 1).cpu().numpy()
    xs = np.arange(31)
    right = np.minimum(15, ((2 * xs + 1) * 16) // (2 * 31)) >= 8
    want = np.zeros((40, 72), np.int32)
    want[4:27, 6:37] = np.where(right, 0, 1)[None, :]
    assert np.array_equal(out, want)


def test_same_call_twice_is_bit_equal():
    rows = grid_rows(25, (40, 72), 13)
    assert device_warp(SRC, rows, (40, 72)).tobytes() == device_warp(SRC, rows, (40, 72)).tobytes()


def test_captured_graph_replays_with_source_and_table_overwritten_in_place():
    from vkit_ocr_model_adaptive_scaling_amd import ops
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import warp_host, warp_region_labels_host
    page_shape, fdf = (40, 72), 2
    cases = []
    for k in range(3):
        lab, valid, shape, rows, ids, out_shape, _ = labels_case(40 + k, fdf)
        cases.append((image(23, 31, 50 + k), rows, lab, ids))
    assert len({len(c[1]) for c in cases}) == 1
    d_src, d_rows, d_lab, d_ids = (torch.from_numpy(a).cuda() for a in cases[0])
    d_page = torch.full(page_shape + (3,), FILL, dtype=torch.uint8, device='cuda')
    d_out = torch.full(out_shape, -7, dtype=torch.int32, device='cuda')

    def run():
        d_page.fill_(FILL)
        d_out.fill_(-7)
        ops.warp_pack_u8(d_src, d_rows, d_page, validate=False)
        ops.warp_region_labels(d_lab, valid, shape, d_rows, d_ids, d_out, fdf, validate=False)

    run()  # eager first
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for src, rows, lab, ids in cases + cases[:1]:
        d_src.copy_(torch.from_numpy(src))
        d_rows.copy_(torch.from_numpy(rows))
        d_lab.copy_(torch.from_numpy(lab))
        d_ids.copy_(torch.from_numpy(ids))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(d_page.cpu().numpy(), warp_host(src, rows, np.full(page_shape + (3,), FILL, np.uint8)))
        assert np.array_equal(d_out.cpu().numpy(),
                              warp_region_labels_host(lab, valid, shape, rows, ids, np.full(out_shape, -7, np.int32), fdf))


def test_argument_checks():
    from vkit_ocr_model_adaptive_scaling_amd import ops
    src, page = torch.from_numpy(SRC), torch.zeros((40, 72, 3), dtype=torch.uint8)
    rows = np.array([identity_row(0, 0, 0, 0, 4, 4)], np.int64)
    with pytest.raises(RuntimeError):
        ops.warp_pack_u8(src, rows, page)
    lab, out, ids = torch.zeros((12, 16), dtype=torch.int32), torch.zeros((20, 36), dtype=torch.int32), np.array([1], np.int32)
    with pytest.raises(RuntimeError):
        ops.warp_region_labels(lab, (12, 16), (23, 31), rows, ids, out, 2)
    d_src, d_page, d_lab, d_out = src.cuda(), page.cuda(), lab.cuda(), out.cuda()
    overlap = np.array([identity_row(0, 0, 0, 0, 4, 4), identity_row(0, 0, 2, 2, 4, 4)], np.int64)
    for bad in (lambda: ops.warp_pack_u8(d_src, rows.astype(np.int32), d_page), lambda: ops.warp_pack_u8(d_src, rows[:, :8], d_page),
                lambda: ops.warp_pack_u8(d_src, overlap, d_page), lambda: ops.warp_pack_u8(d_src.float(), rows, d_page),
                lambda: ops.warp_pack_u8(d_src, torch.from_numpy(overlap).cuda(), d_page),
                lambda: ops.warp_pack_u8(d_src, rows, d_page[:, ::2]),
                lambda: ops.warp_region_labels(d_lab, (13, 16), (23, 31), rows, ids, d_out, 2),
                lambda: ops.warp_region_labels(d_lab, (12, 16), (23, 31), rows, ids[:0], d_out, 2),
                lambda: ops.warp_region_labels(d_lab, (12, 16), (23, 31), rows, np.array([0], np.int32), d_out, 2),
                lambda: ops.warp_region_labels(d_lab, (12, 16), (23, 31), rows, ids, d_out, 0)):
        with pytest.raises(ValueError):
            bad()
