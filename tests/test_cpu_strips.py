"""The rule from a quadrilateral to a strip and the layout of the strips (inferencing/strips.py), on the host: exact cuts
against numpy slicing, the geometry of slanted quads, the statuses, the ``log2n`` thresholds, slots, buckets, the table
checker and the parameter ranges."""
import numpy as np
import pytest

from tests import strip_cases as C
from vkit_ocr_model_adaptive_scaling_amd.inferencing import strips as S
from vkit_ocr_model_adaptive_scaling_amd.inferencing.packing import WARP_A_MAX, WARP_M_MAX, warp_host

IMG = C.picture((40, 60), 11)


def cut(quad, h=8, margin=0.0, width_max=2048, width_step=1, image=IMG):
    out = S.quad_strips_host([image], [np.asarray(quad)[None]], h, width_max, width_step, margin)
    assert out.status.tolist() == [0]
    return out, out.strip(0)


def test_exact_cuts_are_numpy_slices():
    crop = IMG[5:13, 7:27]
    q = C.box(5, 7, 8, 20)
    out, strip = cut(q)
    assert out.widths.tolist() == [20] and out.rows[0, 10] == 0 and strip.shape == (8, 20, 3)
    assert out.rows[0].tolist() == [0, 0, 20, 20, 5 << 16, 7 << 16, 65536, 0, 0, 65536, 0, 0]
    assert np.array_equal(strip, crop)
    assert np.array_equal(cut(C.turned(q, 2))[1], crop[::-1, ::-1]), 'text upside down'
    assert np.array_equal(cut(q[[1, 0, 3, 2]])[1], crop[:, ::-1]), 'a mirrored quad gives a mirrored strip'
    tall = IMG[10:30, 20:28]  # 20 tall, 8 wide
    down = np.array([[10, 28], [30, 28], [30, 20], [10, 20]], np.float64)  # top-right, bottom-right, bottom-left, top-left
    assert np.array_equal(cut(down)[1], np.rot90(tall, 1)), 'read downwards'
    assert np.array_equal(cut(C.turned(down, 2))[1], np.rot90(tall, -1)), 'read upwards'
    out, strip = cut(C.box(3, 9, 16, 40))
    assert out.rows[0, 10] == 1 and out.widths.tolist() == [20]
    assert np.array_equal(strip, C.block_mean(IMG[3:19, 9:49], 2))


@pytest.mark.parametrize('angle', [0.35, 1.57, 3.0])
def test_a_slanted_quad_maps_back_onto_its_corners(angle):
    q = C.rect(20.0, 30.0, 30.0, 9.0, angle)
    out, strip = cut(q, h=32)
    h, w = 32, 107
    assert out.widths.tolist() == [w] and out.rows[0, 10] == 0 and strip.shape == (h, w, 3) and not out.squeezed[0]
    back = out.remap(0, np.array([[0, 0], [0, w], [h, w], [h, 0]], np.float64))
    err = float(np.abs(back - q).max())
    bound = (w + h) * 2.0 ** -17 + 2.0 ** -16  # the coefficients' rounding over w + h steps plus the anchor's
    print(f'angle {angle}: corner error {err:.5f} px, bound {bound:.5f}')
    assert err <= bound
    assert np.array_equal(back, S.remap_strip_points([[0, 0], [0, w], [h, w], [h, 0]], out.rows[0]))
    # the strip is warp_host's for its row
    want = warp_host(IMG, [[0, 0, h, w] + out.rows[0, 4:].tolist()], np.zeros((h, w, 3), np.uint8))
    assert np.array_equal(strip, want)


def test_margin_reads_zero_outside_the_image():
    out, strip = cut(C.box(0, 0, 8, 16), margin=0.25)
    assert out.widths.tolist() == [13] and out.rows[0, 10] == 1
    assert not strip[0].any() and not strip[:, 0].any() and strip[1:, 1:].any()
    # step 1.5 px: strip pixel (i, j) is centred at (4 + (i - 3.5) * 1.5, 8 + (j - 6.5) * 20/13)
    assert out.rows[0, 6] == 98304 and out.rows[0, 9] == int(np.rint(65536 * 20 / 13))
    centre = out.remap(0, [[4.0, 6.5]])
    assert np.abs(centre - [[4.0, 8.0]]).max() < 1e-3


def test_width_max_squeezes():
    for length, w, squeezed in ((20, 20, False), (21, 20, True), (400, 20, True)):
        out, strip = cut(C.box(2, 3, 8, length), width_max=20)
        assert (out.widths.tolist(), out.squeezed.tolist()) == ([w], [squeezed]), length
        assert strip.shape == (8, 20, 3)
    out, _ = cut(C.box(2, 3, 8, 0.2))  # w_nat = 0: one column
    assert out.widths.tolist() == [1] and not out.squeezed[0]


def test_statuses():
    ok = C.box(5, 7, 8, 20)
    bad = ok.copy()
    bad[2, 1] = np.nan
    inf = ok.copy()
    inf[0, 0] = np.inf
    cases = [(ok, 0), (bad, 1), (inf, 1), (C.box(5, 7, 8, 0.05), 1), (C.box(5, 7, 0.05, 8), 1), (C.box(5, 7, 8, 1 / 16), 0),
             (C.box(5, 7, 1 / 16, 1 / 16), 0), (np.zeros((4, 2)), 1)]
    for quad, status in cases:
        assert S.strip_warp(quad, 8, 2048, 0.0)[0] == status
    # a coefficient above 2^22: a strip row more than 64 source pixels high
    assert S.strip_warp(C.box(0, 0, 64, 64), 1, 2048, 0.0)[0] == 0
    assert S.strip_warp(C.box(0, 0, 64, 64), 1, 2048, 0.0)[3][2] == WARP_M_MAX
    assert S.strip_warp(C.box(0, 0, 64.01, 64), 1, 2048, 0.0)[0] == 2
    # an anchor that reaches 2^40: the first pixel centre at 2^24 pixels
    far = float(1 << 24)
    assert S.strip_warp(C.box(far - 1, 0, 1, 4), 1, 2048, 0.0)[3][0] == WARP_A_MAX - 65536
    assert S.strip_warp(C.box(far, 0, 1, 4), 1, 2048, 0.0)[0] == 2
    assert S.strip_warp(C.box(0, -far - 1, 1, 4), 1, 2048, 0.0)[0] == 2
    assert S.strip_warp(C.box(1e300, 0, 1e300, 1e300), 8, 2048, 0.0)[0] == 2
    layout = S.strip_rows([np.stack([ok, bad]), np.stack([C.box(0, 0, 64.01, 64), ok])], 1, 2048, 1, 0.0)
    assert layout.status.tolist() == [0, 1, 2, 0] and layout.image.tolist() == [0, 0, 1, 1]
    assert layout.bucket.tolist() == [0, -1, -1, 0] and layout.index.tolist() == [0, -1, -1, 1]
    assert layout.widths.tolist() == [3, 0, 0, 3] and layout.rows[:, 0].tolist() == [0, 1] and len(layout.rows) == 2
    strips = S.quad_strips_host([IMG, IMG], [np.stack([ok, bad]), np.stack([C.box(0, 0, 64.01, 64), ok])], 1, 2048, 1, 0.0)
    assert np.array_equal(strips.strip(3), strips.strip(0))
    with pytest.raises(ValueError):
        strips.strip(1)
    with pytest.raises(ValueError):
        strips.remap(2, [[0, 0]])


def test_log2n_thresholds_at_equality():
    one = 65536
    for m, want in ((one, 0), (one + 1, 1), (2 * one, 1), (2 * one + 1, 2), (4 * one, 2), (4 * one + 1, 3), (64 * one, 3)):
        assert S.log2n_of(m, 0, 0, 0) == want and S.log2n_of(0, 0, 0, m) == want and S.log2n_of(0, m, 0, 0) == want
    assert S.log2n_of(46341, 0, 46341, 0) == 1 and S.log2n_of(46340, 0, 46340, 0) == 0  # the step's length, not a component
    for height, want in ((8, 0), (16, 1), (32, 2), (33, 3), (100, 3)):
        assert S.strip_warp(C.box(1, 2, height, 3 * height), 8, 2048, 0.0)[3][6] == want, height


def test_slots_and_buckets():
    lengths = [9, 4, 8, 12, 3, 13]
    quads = np.stack([C.box(1, 2, 8, n) for n in lengths])
    layout = S.strip_rows([quads], 8, 2048, 4, 0.0)
    assert layout.widths.tolist() == lengths
    assert layout.rows[:, 2].tolist() == [12, 4, 8, 12, 4, 16], 'slot widths at k * step and one beyond'
    assert layout.bucket_shapes == [(2, 8, 4, 3), (1, 8, 8, 3), (2, 8, 12, 3), (1, 8, 16, 3)]
    assert layout.bucket.tolist() == [2, 0, 1, 2, 0, 3] and layout.index.tolist() == [0, 0, 0, 1, 1, 0]
    slot = lambda sw: 8 * sw * 3
    starts = [0, 2 * slot(4), 2 * slot(4) + slot(8), 2 * slot(4) + slot(8) + 2 * slot(12)]
    assert layout.rows[:, 1].tolist() == [starts[2], starts[0], starts[1], starts[2] + slot(12), starts[0] + slot(4), starts[3]]
    assert layout.out_bytes == starts[3] + slot(16)
    S.check_strip_rows(layout.rows, [[0, 40, 60, 0]], 8, layout.out_bytes)
    strips = S.quad_strips_host([IMG], [quads], 8, 2048, 4, 0.0)
    assert [b.shape for b in strips.buckets] == layout.bucket_shapes and strips.height == 8
    for k, n in enumerate(lengths):
        assert np.array_equal(strips.strip(k), IMG[1:9, 2:2 + n])
        assert not strips.buckets[strips.bucket[k]][strips.index[k]][:, n:].any(), 'the columns beyond w are zero'
    assert strips.buckets[0].base is strips.buckets[3].base is not None, 'one allocation'
    table = S.strip_table(layout.rows, 8)
    assert table[:-7].reshape(-1, 12).tolist() == layout.rows.tolist() and table[-7:].tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert S.strip_table(np.array([[0, 0, 65, 1] + [0] * 8, [0, 0, 64, 1] + [0] * 8]), 37)[-3:].tolist() == [0, 6, 9]
    empty = S.strip_rows([np.zeros((0, 4, 2))], 8, 2048, 4, 0.0)
    assert empty.rows.shape == (0, 12) and empty.out_bytes == 0 and empty.bucket_shapes == []


def test_check_strip_rows_rejects():
    layout = S.strip_rows([np.stack([C.box(1, 2, 8, 9), C.box(1, 2, 8, 12)])], 8, 2048, 4, 0.0)
    sources, rows, size = [[0, 40, 60, 0]], layout.rows, layout.out_bytes
    assert np.array_equal(S.check_strip_rows(rows, sources, 8, size), rows)

    def bad(col, value, row=0, **kw):
        r = rows.copy()
        r[row, col] = value
        with pytest.raises(ValueError):
            S.check_strip_rows(r, kw.get('sources', sources), kw.get('h', 8), kw.get('size', size))

    bad(1, rows[1, 1])            # overlap: two rows on one slot
    bad(1, rows[1, 1] - 1)        # overlap by a byte
    bad(3, 13)                    # w > slot_w
    bad(3, 0)
    bad(2, 8196)
    bad(1, rows[1, 1] + 1, row=1)  # a slot past the end
    bad(1, -1)
    bad(0, 1)
    bad(0, -1)
    bad(6, WARP_M_MAX + 1)
    bad(5, WARP_A_MAX)
    bad(10, 4)
    bad(10, -1)
    with pytest.raises(ValueError):
        S.check_strip_rows(rows, sources, 8, size - 1)
    with pytest.raises(ValueError):
        S.check_strip_rows(rows, sources, 9, size)
    with pytest.raises(ValueError):
        S.check_strip_rows(rows, [[0, 40, 32769, 0]], 8, size)
    with pytest.raises(ValueError):
        S.check_strip_rows(rows.astype(np.float64), sources, 8, size)
    with pytest.raises(ValueError):
        S.check_strip_rows(rows[:, :11], sources, 8, size)


def test_parameter_ranges():
    q = [C.box(1, 2, 8, 9)[None]]
    for kw in (dict(h=0), dict(h=257), dict(h=8.5), dict(width_max=0), dict(width_max=8193), dict(width_step=0),
               dict(width_step=65, width_max=64), dict(margin=-0.01), dict(margin=1.01), dict(margin=float('nan'))):
        args = dict(h=8, width_max=2048, width_step=64, margin=0.125)
        args.update(kw)
        with pytest.raises(ValueError):
            S.strip_rows(q, **args)
    for h, width_max, width_step, margin in ((1, 1, 1, 0.0), (256, 8192, 8192, 1.0)):
        assert S.strip_rows(q, h, width_max, width_step, margin).status.tolist() == [0]
    with pytest.raises(ValueError):
        S.quad_strips_host([IMG, IMG], q)
