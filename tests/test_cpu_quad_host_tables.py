"""The host half that the five routes over match rows share (inferencing/quad_tables.py): the builder of padded batches on
ragged lists, the checker of the oracles' tables driven through all five ``*_host`` oracles, and the two ends of the device
wrappers - the capacity retry with a fake call, the device check.  No GPU."""
import numpy as np
import pytest

from tests import quad_match_cases as C
from vkit_ocr_model_adaptive_scaling_amd import inferencing as I
from vkit_ocr_model_adaptive_scaling_amd.inferencing import quad_tables as T

SQ = C.SQ
RAGGED = [np.zeros((0, 4, 2)), np.array([SQ(0, 0, 8, 8)], np.float64),
          np.array([SQ(0, 0, 8, 8), SQ(0, 4, 8, 8), SQ(20, 0, 8, 8)], np.float64)]  # images with 0, 1 and 3 quads
TOO_MANY = np.broadcast_to(np.zeros((1, 1, 1)), (T.MAX_QUADS + 1, 4, 2))  # a zero-stride view: it costs nothing


# ---- the builder -----------------------------------------------------------------------------------------------------

def test_padded_batch_of_ragged_lists():
    q = T.quad_lists([a.tolist() for a in RAGGED])
    assert [a.shape for a in q] == [(0, 4, 2), (1, 4, 2), (3, 4, 2)] and all(a.dtype == np.float64 for a in q)
    quads, count = T.pad_quads(q)
    assert quads.shape == (3, 3, 4, 2) and quads.dtype == np.float64
    assert count.dtype == np.int32 and count.tolist() == [0, 1, 3]
    for b, a in enumerate(RAGGED):
        assert np.array_equal(quads[b, :len(a)], a) and not quads[b, len(a):].any()
    probs = T.pad_values(q, [[], [0.5], [0.25, np.nan, 1.0]], np.float32, 'probs')
    assert probs.dtype == np.float32 and probs.shape == (3, 3)
    assert np.array_equal(probs, np.array([[0, 0, 0], [0.5, 0, 0], [0.25, np.nan, 1.0]], np.float32), equal_nan=True)
    ones = T.pad_values(q, None, np.uint8, 'valid')
    assert ones.dtype == np.uint8 and ones.tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 1]]
    rows, n = T.pad_rows([I.match_rows(a)[0] for a in q])
    assert rows.shape == (3, 3, 16) and rows.dtype == np.int32 and n.tolist() == [0, 1, 3]
    assert np.array_equal(rows[2], I.match_rows(RAGGED[2])[0]) and not rows[1, 1:].any() and not rows[0].any()


def test_the_builder_fills_views_it_is_given():
    q = T.quad_lists(RAGGED)
    up = np.zeros((3 * 3 * 64 + 3 * 4,), np.uint8)
    quads, count = T.pad_quads(q, up[:3 * 3 * 64].view(np.float64).reshape(3, 3, 4, 2), up[3 * 3 * 64:].view(np.int32))
    want, want_count = T.pad_quads(q)
    assert np.shares_memory(quads, up) and np.shares_memory(count, up)
    assert up.tobytes() == want.tobytes() + want_count.tobytes()


def test_an_empty_batch_has_one_column_and_no_counts():
    quads, count = T.pad_quads(T.quad_lists([]))
    assert quads.shape == (0, 1, 4, 2) and count.shape == (0,) and count.dtype == np.int32
    assert T.pad_values([], None, np.float32, 'probs').shape == (0, 1)
    assert T.pad_rows([])[0].shape == (0, 1, 16)
    pred, gt = T.quad_lists([], [])
    assert pred == [] and gt == []
    only_empty = T.pad_quads(T.quad_lists([np.zeros((0, 4, 2))]))
    assert only_empty[0].shape == (1, 1, 4, 2) and only_empty[1].tolist() == [0]


def test_lists_that_do_not_pair_up_raise():
    q = T.quad_lists(RAGGED)
    with pytest.raises(ValueError, match='one entry per image'):
        T.pad_values(q, [[], [0.5]], np.float32, 'probs')
    with pytest.raises(ValueError, match='pair up image by image'):
        T.pad_values(q, [[], [0.5], [0.25, 1.0]], np.float32, 'probs')
    with pytest.raises(ValueError, match='3 images of predictions against 2 of annotations'):
        T.quad_lists(RAGGED, RAGGED[:2])
    for bad in (dict(pred_scores=[np.zeros(0), np.zeros(1)]), dict(pred_scores=[np.zeros(0), np.zeros(1), np.zeros(2)]),
                dict(pred_scores=[np.zeros(0), np.zeros(1), np.zeros(3)], gt_care=[np.ones(0), np.ones(1)]),
                dict(pred_scores=[np.zeros(0), np.zeros(1), np.zeros(3)], gt_care=[np.ones(0), np.ones(1), np.ones(4)])):
        with pytest.raises(ValueError):
            I.evaluate_quads_ranked_host(RAGGED, RAGGED, **bad)
    for bad in ([np.ones(0), np.ones(1)], [np.ones(0), np.ones(2), np.ones(3)]):
        with pytest.raises(ValueError):
            I.evaluate_lines_host(RAGGED, RAGGED, gt_care=bad)
        with pytest.raises(ValueError):
            I.nms_quads_lists_host(RAGGED, bad)


def test_more_than_max_quads_raises_and_names_the_counts():
    with pytest.raises(ValueError, match=f'at most {T.MAX_QUADS} quads .* got {T.MAX_QUADS + 1}$'):
        T.quad_lists([RAGGED[1], TOO_MANY])
    with pytest.raises(ValueError, match=f'at most {T.MAX_QUADS} .* got 3 annotations / {T.MAX_QUADS + 1} predictions'):
        T.quad_lists([TOO_MANY], [RAGGED[2]])
    with pytest.raises(ValueError, match=f'got {T.MAX_QUADS + 1} annotations / 1 predictions'):
        T.quad_lists([RAGGED[1]], [TOO_MANY])
    assert len(T.quad_lists([TOO_MANY[:T.MAX_QUADS]])[0]) == T.MAX_QUADS
    scores = np.broadcast_to(np.float32(0.5), (T.MAX_QUADS + 1,))
    for call in (lambda: I.evaluate_quads_host([TOO_MANY], [RAGGED[1]]), lambda: I.nms_quads_lists_host([TOO_MANY], [scores]),
                 lambda: I.evaluate_quads_ranked_host([RAGGED[1]], [TOO_MANY], [np.zeros(1)]),
                 lambda: I.quad_lines_lists_host([TOO_MANY]), lambda: I.evaluate_lines_host([TOO_MANY], [RAGGED[1]])):
        with pytest.raises(ValueError, match=f'at most {T.MAX_QUADS}'):
            call()


def test_the_public_table_builders_return_what_the_builder_returns():
    gt, pred = RAGGED, RAGGED[::-1]
    scores = [np.array([0.9, 0.2, np.nan]), np.array([0.4]), np.zeros(0)]
    tables = I.evaluation_tables(pred, gt, scores, 0.3)
    keep = [np.array([True, False, False]), np.array([True]), np.zeros(0, bool)]
    want_g = T.pad_rows([I.match_rows(a)[0] for a in gt])
    want_p = T.pad_rows([I.match_rows(a, k)[0] for a, k in zip(pred, keep)])
    for got, want in zip(tables[:4], want_g + want_p):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert [v.tolist() for v in tables[5]] == [k.tolist() for k in keep]
    rows, count, probs, valid = I.nms_tables(pred, scores, 0.3)
    assert np.array_equal(rows, want_p[0]) and np.array_equal(count, want_p[1])
    assert [v.tolist() for v in valid] == [k.tolist() for k in keep]
    assert probs.tobytes() == T.pad_values(T.quad_lists(pred), scores, np.float32, 'probs').tobytes()
    sides = T.padded_sides(pred, gt, [np.zeros(0), [2], [0, 1, 0]], scores)
    assert [t.dtype for t in sides] == [np.float64, np.int32, np.uint8, np.float64, np.int32, np.float32]
    assert np.array_equal(sides[0], T.pad_quads(T.quad_lists(gt))[0]) and sides[1].tolist() == [0, 1, 3]
    assert sides[2].tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0]] and sides[4].tolist() == [3, 1, 0]
    assert len(T.padded_sides(pred, gt)) == 5 and T.padded_sides(pred, gt)[2].tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 1]]


# ---- the checker, through the five oracles -------------------------------------------------------------------------------

def z(shape, dtype=np.int32):
    return np.broadcast_to(np.zeros((1,) * len(shape), dtype), shape)


def two_sided(care, probs):
    def good(B=2, M=4, N=5):
        kw = dict(gt_rows=z((B, M, 16)), gt_count=z((B,)), pred_rows=z((B, N, 16)), pred_count=z((B,)))
        if care:
            kw['gt_care'] = z((B, M), np.uint8)
        if probs:
            kw.update(probs=z((B, N), np.float32), iou_thrs=(0.5, 0.75))
        return kw
    return good, ('gt_rows', 'pred_rows'), ('gt_count', 'pred_count')


def one_sided(probs):
    def good(B=2, M=4, N=None):
        kw = dict(rows=z((B, M, 16)), count=z((B,)))
        if probs:
            kw['probs'] = z((B, M), np.float32)
        return kw
    return good, ('rows',), ('count',)


ORACLES = {
    'match_quads_host': two_sided(False, False),
    'match_quads_ranked_host': two_sided(True, True),
    'match_lines_host': two_sided(True, False),
    'nms_quads_host': one_sided(True),
    'quad_lines_host': one_sided(False),
}
STATS = {'match_quads_host': 3, 'match_quads_ranked_host': 5, 'match_lines_host': 4, 'nms_quads_host': 2, 'quad_lines_host': 3}


def bad_calls(name):
    good, rows_keys, count_keys = ORACLES[name]
    ok = good()
    for k in rows_keys:
        B, K, _ = ok[k].shape
        yield f'{k} of rank 2', {**ok, k: z((K, 16))}
        yield f'{k} with 15 words', {**ok, k: z((B, K, 15))}
    for k in count_keys:
        yield f'{k} of the wrong length', {**ok, k: z((3,))}
    if 'gt_care' in ok:
        yield 'gt_care of the wrong shape', {**ok, 'gt_care': z((2, 5), np.uint8)}
    if 'probs' in ok:
        yield 'probs of the wrong shape', {**ok, 'probs': z((2, 9), np.float32)}
    if len(rows_keys) == 2:
        yield 'tables with differing B', {**ok, 'pred_rows': z((3, 5, 16)), 'pred_count': z((3,))}


CASES = [(name, label, kw) for name in ORACLES for label, kw in bad_calls(name)]


@pytest.mark.parametrize('name,label,kw', CASES, ids=[f'{n}-{l}' for n, l, _ in CASES])
def test_bad_table_raises(name, label, kw):
    with pytest.raises(ValueError):
        getattr(I, name)(**kw)


def test_ranked_pairs_and_line_pairs_use_the_checker():
    ranked, lines = ORACLES['match_quads_ranked_host'][0](), ORACLES['match_lines_host'][0]()
    for fn, ok in ((I.ranked_pairs, ranked), (I.line_pairs, lines)):
        assert len(fn(**ok)) == 2
        for bad in (dict(gt_rows=z((4, 16))), dict(pred_rows=z((2, 5, 15))), dict(gt_count=z((3,))),
                    dict(gt_care=z((2, 5), np.uint8))):
            with pytest.raises(ValueError):
                fn(**{**ok, **bad})


def _valid_tables(name, K=4):
    """B = 2 tables of K valid, well separated squares a side, with the counts -3 and K + 5"""
    rows = np.stack([I.match_rows(np.array([SQ(0, 40 * k, 8, 8) for k in range(K)], np.float64))[0]] * 2)
    count = np.array([-3, K + 5], np.int32)
    good = ORACLES[name][0](M=K, N=K)
    for k in good:
        if k.endswith('rows'):
            good[k] = rows
        elif k.endswith('count'):
            good[k] = count
        elif k == 'gt_care':
            good[k] = None
    return good


@pytest.mark.parametrize('name', ORACLES)
def test_counts_are_clamped(name):
    K = 4
    outs = getattr(I, name)(**_valid_tables(name, K))
    stats = outs[STATS[name]]
    if name == 'match_quads_host':      # tp, n_gt, n_pred
        assert stats[:, :3].tolist() == [[0, 0, 0], [K, K, K]]
    elif name == 'match_quads_ranked_host':  # per threshold: tp, fp, ignored, n_gt, n_pred
        assert stats[:, 0, :5].tolist() == [[0, 0, 0, 0, 0], [K, 0, 0, K, K]]
    elif name == 'match_lines_host':    # n_gt, n_pred, one_to_one
        assert stats[:, :3].tolist() == [[0, 0, 0], [K, K, K]]
    elif name == 'nms_quads_host':      # kept, n, n_valid
        assert stats[:, :3].tolist() == [[0, 0, 0], [K, K, K]]
    else:                               # n, n_part
        assert stats[:, :2].tolist() == [[0, 0], [K, K]]
    assert [T.clamped(c, K) for c in (-3, 0, 2, K, K + 5)] == [0, 0, 2, K, K]


def test_the_checker_returns_contiguous_typed_tables():
    rows = np.asfortranarray(np.arange(2 * 3 * 16, dtype=np.int64).reshape(2, 3, 16))
    (g, gc, p, pc, care, probs), B, M, N = T.host_tables(rows, [1, 2], rows[:, :2], (2, 0), None, np.ones((2, 2)))
    assert (B, M, N) == (2, 3, 2) and g.dtype == p.dtype == np.int32 and g.flags.c_contiguous and p.flags.c_contiguous
    assert np.array_equal(g, rows) and care.dtype == np.uint8 and care.shape == (2, 3) and care.all()
    assert probs.dtype == np.float32 and probs.shape == (2, 2) and gc.shape == pc.shape == (2,)
    (r, c, pr), B, K = T.host_table(rows, np.array([[1], [2]]))
    assert (B, K) == (2, 3) and r.dtype == np.int32 and c.tolist() == [1, 2] and pr is None


# ---- the ends of the device wrappers -------------------------------------------------------------------------------------

def _fake(stats_per_call):
    """a ``call`` that records its capacities and hands out the canned stats in turn, and its ``read_stats``"""
    caps, reads = [], []

    def call(cap):
        caps.append(cap)
        return ('outs', len(caps) - 1)

    def read_stats(outs):
        reads.append(outs[1])
        return stats_per_call[outs[1]]
    return call, read_stats, caps, reads


def _stats(status, candidates):
    st = np.zeros((len(status), 6), np.int64)
    st[:, 5], st[:, 4] = status, candidates
    return st


def test_with_capacity_calls_once_when_no_image_reports_status():
    call, read, caps, reads = _fake([_stats([0, 0, 0], [7, 19, 3])])
    outs, stats = T.with_capacity('who', call, read, np.s_[:, 5], np.s_[:, 4])
    assert caps == [None] and reads == [0] and outs == ('outs', 0) and stats[:, 4].tolist() == [7, 19, 3]


def test_with_capacity_retries_once_with_the_largest_reported_count():
    call, read, caps, reads = _fake([_stats([1, 0, 1], [7, 500, 19]), _stats([0, 0, 0], [7, 500, 19])])
    outs, stats = T.with_capacity('who', call, read, np.s_[:, 5], np.s_[:, 4])
    assert caps == [None, 500] and reads == [0, 1] and outs == ('outs', 1) and not stats[:, 5].any()
    # the capacity is the largest count reported, whichever image reports it: here the two images with status
    call, read, caps, reads = _fake([_stats([1, 1], [7, 19]), _stats([0, 0], [7, 19])])
    T.with_capacity('who', call, read, np.s_[:, 5], np.s_[:, 4])
    assert caps == [None, 19] and type(caps[1]) is int and reads == [0, 1]


def test_with_capacity_raises_on_a_second_overflow():
    call, read, caps, reads = _fake([_stats([1, 1], [7, 19]), _stats([0, 1], [7, 19]), _stats([0, 0], [7, 19])])
    with pytest.raises(RuntimeError, match='^who: .*overflowed again'):
        T.with_capacity('who', call, read, np.s_[:, 5], np.s_[:, 4])
    assert caps == [None, 19] and reads == [0, 1]


def test_with_capacity_reads_the_columns_it_is_given():
    first, second = np.zeros((2, 3, 8), np.int64), np.zeros((2, 3, 8), np.int64)
    first[1, 0, 7], first[:, 0, 6] = 1, (4, 11)
    first[0, 1, 7] = second[0, 1, 7] = 1  # beside the status column: not read
    call, read, caps, _ = _fake([first, second])
    T.with_capacity('who', call, read, np.s_[:, 0, 7], np.s_[:, 0, 6])
    assert caps == [None, 11]


def test_require_gpu_names_the_host_route():
    with pytest.raises(ValueError, match='GPU') as e:
        T.require_gpu('x', 'cpu', 'x_host')
    assert 'x_host' in str(e.value) and str(e.value).startswith('x runs on the GPU')
    assert T.require_gpu('x', 'cuda:1', 'x_host').index == 1


@pytest.mark.parametrize('name,args', [
    ('evaluate_quads', (RAGGED, RAGGED)), ('nms_quads', (RAGGED, [np.zeros(0), np.zeros(1), np.zeros(3)])),
    ('evaluate_quads_ranked', (RAGGED, RAGGED, [np.zeros(0), np.zeros(1), np.zeros(3)])), ('quad_lines', (RAGGED,)),
    ('evaluate_lines', (RAGGED, RAGGED))])
def test_every_device_wrapper_refuses_the_cpu_and_names_its_host_route(name, args):
    host = {'nms_quads': 'nms_quads_lists_host', 'quad_lines': 'quad_lines_lists_host'}.get(name, name + '_host')
    with pytest.raises(ValueError, match=f'^{name} runs on the GPU.*host route: {host}'):
        getattr(I, name)(*args, device='cpu')


def test_threshold_check_names_the_wrapper():
    from vkit_ocr_model_adaptive_scaling_amd import ops
    t = __import__('torch')
    zt = lambda shape, dtype=t.int32: t.zeros(shape, dtype=dtype)
    for bad in (0.0, 1.5, float('nan')):
        with pytest.raises(ValueError, match='^match_quads: iou_thr'):
            ops.match_quads(zt((1, 2, 16)), zt((1,)), zt((1, 2, 16)), zt((1,)), iou_thr=bad)
        with pytest.raises(ValueError, match='^nms_quads: iou_thr'):
            ops.nms_quads(zt((1, 2, 16)), zt((1,)), zt((1, 2), t.float32), iou_thr=bad)
        with pytest.raises(ValueError, match='^iou_thr'):
            I.check_iou_thr(bad)
    assert I.check_iou_thr(1) == 1.0 and type(I.check_iou_thr(1)) is float
