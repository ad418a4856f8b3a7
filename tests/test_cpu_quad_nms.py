"""inferencing/nms.py on the host: the oracle ``nms_quads_host`` on hand cases with ``==``, the sorted sequential form against
the rounds restatement of tests/quad_nms_cases.py on random graphs with exact prob ties, the list route with its score
threshold, the result filter, and the argument checks.  No GPU."""
import attrs
import numpy as np
import pytest

from tests import quad_nms_cases as Q
from vkit_ocr_model_adaptive_scaling_amd.inferencing import evaluation as E
from vkit_ocr_model_adaptive_scaling_amd.inferencing import nms as N


@pytest.mark.parametrize('name', list(Q.hand_cases()))
def test_hand_cases(name):
    rows, count, probs, thr, keep, suppressor, rounds = Q.hand_cases()[name]
    got = N.nms_quads_host(rows[None], [count], probs[None], thr)
    assert got[0][0].tolist() == keep and got[1][0].tolist() == suppressor
    assert got[2][0].tolist() == Q.hand_stats(name)
    assert got[0].dtype == np.uint8 and got[1].dtype == np.int32 and got[2].dtype == np.int64
    assert Q.rounds_of(rows, count, probs, thr) == rounds


def test_the_argument_order_decides():
    a, b, ab, ba = Q.asymmetric_pair()
    assert ab > ba > 0.2 and E.quad_iou_host(a, b) == ab and E.quad_iou_host(b, a) == ba
    thr = Q.order_threshold()
    assert ba < thr <= ab  # reached by iou(a, b) alone
    print(f'iou(a, b) = {ab!r}, iou(b, a) = {ba!r}, threshold {thr!r}')
    cases = Q.hand_cases()
    assert cases['order_a_judged'][4] == [0, 1] and cases['order_b_judged'][4] == [1, 1]


def test_a_b_c_needs_more_than_one_round():
    rows, count, probs, thr, keep, _, rounds = Q.hand_cases()['a_b_c']
    # A is kept in the first round, B suppressed in the second (it reads A's state of the first), C kept in the third: two
    # rounds after the one that decides the quads without neighbours
    assert rounds == 3 and keep == [1, 0, 1]
    ious = [E.quad_iou_host(rows[i], rows[j]) for i, j in ((1, 0), (2, 1), (2, 0))]
    assert ious == [44 / 84, 44 / 84, 24 / 104]


def test_counts_outside_the_table_are_clamped():
    rows, _, probs, thr, *_ = Q.hand_cases()['a_b_c']
    for count, want in ((-3, [0, 0, 0]), (0, [0, 0, 0]), (2, [1, 0, 0]), (99, [1, 0, 1])):
        keep, sup, stats = N.nms_quads_host(rows[None], [count], probs[None], thr)
        assert keep[0].tolist() == want and stats[0, 1] == min(max(count, 0), 3) and stats[0, 0] == sum(want)
        assert (sup[0, max(count, 0):] == -1).all()


def test_chain_of_forty():
    rows, probs, keep, suppressor, rounds = Q.chain_case()
    got = N.nms_quads_host(rows[None], [40], probs[None], 0.5)
    assert np.array_equal(got[0][0], keep) and np.array_equal(got[1][0], suppressor)
    assert got[2][0].tolist() == [20, 40, 40, 39 + 38 + 37, 39, 0]  # boxes of quads up to 60 px apart overlap
    assert Q.rounds_of(rows, 40, probs) == rounds == 40


def test_sorted_form_equals_the_rounds_on_random_graphs_with_ties():
    rng = np.random.default_rng(12)
    multi = 0
    for _ in range(1000):
        n = int(rng.integers(1, 13))
        probs = (rng.integers(0, 4, n) / 4).astype(np.float32)  # four values: ties in most graphs
        probs[rng.uniform(size=n) < 0.1] *= -1                  # and -0.0 beside +0.0
        part = rng.uniform(size=n) < 0.85
        edges = [(i, j) for i in range(n) for j in range(n)
                 if i != j and part[i] and part[j] and Q.outranks(probs, j, i) and rng.uniform() < 0.35]
        keep, sup = N.greedy_suppression(part, probs, edges)
        rkeep, rsup, rounds = Q.suppression_rounds(part, probs, edges)
        assert np.array_equal(keep, rkeep) and np.array_equal(sup, rsup), (n, probs, edges)
        assert rounds <= max(int(part.sum()), 0)
        # the greedy property itself: kept iff no kept neighbour; the suppressor outranks every other kept neighbour
        for i in range(n):
            kept = [j for (a, j) in edges if a == i and keep[j]]
            assert bool(keep[i]) == (not kept)
            assert sup[i] == (-1 if not kept else [j for j in kept if all(j == k or Q.outranks(probs, j, k) for k in kept)][0])
        multi += rounds > 2
    assert multi > 100, 'the graphs must need several rounds'


@pytest.mark.parametrize('seed,K', [(1, 1), (2, 40), (3, 129)])
def test_oracle_equals_the_rounds_on_random_tables(seed, K):
    rows, count, probs = Q.random_table(seed, 1, K)
    keep, sup, stats = N.nms_quads_host(rows, count, probs, 0.5)
    part, pi, pj = N.nms_pairs(rows[0], probs[0])
    edges = [(i, j) for i, j in zip(pi.tolist(), pj.tolist()) if E.quad_iou_host(rows[0, i], rows[0, j]) >= 0.5]
    rkeep, rsup, _ = Q.suppression_rounds(part, probs[0], edges)
    assert np.array_equal(keep[0], rkeep) and np.array_equal(sup[0], rsup)
    assert stats[0].tolist() == [int(rkeep.sum()), K, int(part.sum()), len(pi), len(edges), 0]
    if K > 8:
        assert 0 < len(edges) < len(pi) and part.sum() < K and (keep[0][~part] == 1).all() and (keep[0] == 0).any()


def test_page_is_not_vacuous():
    (rows, count, probs), (keep, sup, stats) = Q.page_reference(2)
    assert count[0] == 330 and stats[0, 1] == stats[0, 2] == 330
    assert 330 - stats[0, 0] >= 20 and stats[0, 0] >= 250
    assert ((sup[0] >= 0) == (keep[0] == 0)).all()


def test_list_route_and_score_thr():
    q = np.array([Q.SQ(3, 5, 8, 8)] * 3, np.float64)
    res, stats = N.nms_quads_lists_host([q], [np.array([0.9, 0.3, 0.8], np.float32)], 0.5, score_thr=0.5)
    assert res[0].keep.tolist() == [True, False, False] and res[0].suppressor.tolist() == [-1, -1, 0]
    assert res[0].valid.tolist() == [True, False, True] and stats.tolist() == [1, 3, 2, 1, 1, 0]
    res, stats = N.nms_quads_lists_host([q], [np.array([0.9, 0.3, 0.8], np.float32)], 0.5)
    assert res[0].keep.tolist() == [True, False, False] and res[0].suppressor.tolist() == [-1, 0, 0] and stats[3] == 3
    # an invalid quad without a threshold passes through; an image without quads; a NaN prob under a threshold is absent
    bad = q.copy()
    bad[1] = bad[1][::-1]  # anticlockwise
    res, _ = N.nms_quads_lists_host([bad, q[:0]], [np.array([0.9, 0.95, np.nan], np.float32), np.zeros((0,), np.float32)])
    assert res[0].keep.tolist() == [True, True, True] and res[0].valid.tolist() == [True, False, True]
    assert res[1].keep.shape == (0,)
    res, _ = N.nms_quads_lists_host([q], [np.array([0.9, np.nan, 0.8], np.float32)], 0.5, score_thr=0.1)
    assert res[0].keep.tolist() == [True, False, False]


def _result(points, probs, polygons):
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import AdaptiveScalingInferencingResult
    return AdaptiveScalingInferencingResult(
        image_shape=(100, 100), regions=None, packed=np.ones((len(probs),), bool), too_large=np.zeros((len(probs),), bool),
        placements=np.zeros((len(probs), 8), np.int32), placement_regions=np.arange(1, len(probs) + 1, dtype=np.int32),
        page_shape=(256, 256), page=None, region_labels=None, points=points, probs=probs, polygons=polygons)


def test_result_filter_on_duplicates_across_two_regions():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import filter_result, result_quads
    sq = lambda y, x: np.array(Q.SQ(y, x, 10, 8), np.float64)
    # region 1 holds characters a, b; region 2 holds b again (a shade weaker), c, and a second peak on c; region 3 is empty
    polygons = [np.stack([sq(10, 10), sq(10, 30)]), np.stack([sq(10, 30.5), sq(10, 50), sq(11, 50)]), np.zeros((0, 4, 2))]
    probs = [np.array([0.9, 0.8], np.float32), np.array([0.75, 0.85, 0.95], np.float32), np.zeros((0,), np.float32)]
    points = [np.array([[5, 5], [5, 15]], np.int32), np.array([[5, 16], [5, 25], [6, 25]], np.int32), np.zeros((0, 2), np.int32)]
    r = _result(points, probs, polygons)
    assert (r.num_suppressed, r.nms_status) == (0, 0)
    quads, pr = result_quads(r)
    res, stats = N.nms_quads_lists_host([quads], [pr], 0.5)
    assert res[0].keep.tolist() == [True, True, False, False, True] and res[0].suppressor.tolist() == [-1, -1, 1, 4, -1]
    out = filter_result(r, res[0].keep)
    assert out.num_suppressed == 2 and out.nms_status == 0 and len(out.polygons) == 3
    assert [p.tolist() for p in out.points] == [[[5, 5], [5, 15]], [[6, 25]], []]
    assert [p.tolist() for p in out.probs] == [probs[0].tolist(), [probs[1][2]], []]
    assert np.array_equal(out.polygons[0], polygons[0]) and np.array_equal(out.polygons[1], polygons[1][2:])
    assert [a.dtype for a in out.points + out.probs + out.polygons] == [a.dtype for a in points + probs + polygons]
    same = lambda a, b: all(getattr(a, f.name) is getattr(b, f.name) for f in attrs.fields(type(a))
                            if f.name not in ('points', 'probs', 'polygons', 'num_suppressed'))
    assert same(out, r) and r.num_suppressed == 0 and len(r.probs[1]) == 3  # a copy: the source is untouched
    sq2, p2 = result_quads(out)
    assert np.array_equal(sq2, quads[res[0].keep]) and np.array_equal(p2, pr[res[0].keep])
    with pytest.raises(ValueError):
        filter_result(r, np.ones((4,), bool))


def test_argument_checks():
    rows, count, probs, *_ = Q.hand_cases()['a_b_c']
    for thr in (0.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError):
            N.nms_quads_host(rows[None], [count], probs[None], thr)
    with pytest.raises(ValueError):
        N.nms_quads_host(rows, [count], probs[None])
    with pytest.raises(ValueError):
        N.nms_quads_host(rows[None], [count, count], probs[None])
    with pytest.raises(ValueError):
        N.nms_quads_host(rows[None], [count], probs[None, :2])
    q = np.zeros((2, 4, 2))
    with pytest.raises(ValueError):
        N.nms_quads_lists_host([q], [np.zeros((3,))])
    with pytest.raises(ValueError):
        N.nms_quads_lists_host([q, q], [np.zeros((2,))])
    with pytest.raises(ValueError):
        N.nms_quads_lists_host([np.zeros((8193, 4, 2))], [np.zeros((8193,))])
    with pytest.raises(ValueError, match='GPU'):
        N.nms_quads([q], [np.zeros((2,))], device='cpu')


def test_config_and_result_defaults():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import AdaptiveScalingInferencingConfig
    assert AdaptiveScalingInferencingConfig().precise_char_nms_iou_thr == 0.0
