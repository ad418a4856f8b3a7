"""The text-line score of inferencing/line_evaluation.py on the host: the sequential oracle on hand cases with ``==``, the
tests at equality and one Q8 step beyond, the sequential form against the rounds on random candidate graphs, the
intersection against an exact clip over fractions, the magnitude bounds, the score against fractions and the parameter
ranges."""
from fractions import Fraction

import numpy as np
import pytest

from tests import line_match_cases as Q
from tests import quad_match_cases as C
from vkit_ocr_model_adaptive_scaling_amd.inferencing import evaluation as E
from vkit_ocr_model_adaptive_scaling_amd.inferencing import line_evaluation as L
from vkit_ocr_model_adaptive_scaling_amd.inferencing import ranking as R

NAMES = ('gt_kind', 'gt_group', 'pred_kind', 'pred_group', 'stats')


def both_forms(t, params):
    pairs = L.line_pairs(*t, **params)
    seq = L.match_lines_host(*t, **params, pairs=pairs)
    rnd = L.match_lines_rounds_host(*t, **params, pairs=pairs)
    for name, a, b in zip(NAMES, seq, rnd):
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    assert np.array_equal(rnd[5], rnd[4][:, 12:14])
    return rnd


@pytest.mark.parametrize('name', list(Q.hand_cases()))
def test_hand_cases(name):
    t, params, gk, gg, pk, pg, stats = Q.hand_cases()[name]
    got = both_forms(t, params)
    assert got[0][0].tolist() == gk and got[1][0].tolist() == gg and got[2][0].tolist() == pk and got[3][0].tolist() == pg
    assert [d.dtype for d in got] == [np.uint8, np.int32, np.uint8, np.int32, np.int64, np.int32]
    for key, value in stats.items():
        assert got[4][0, L.STAT_NAMES.index(key)] == value, (key, got[4][0].tolist())
    assert got[4][0, 11] == 0 and not got[4][0, 14:].any()


@pytest.mark.parametrize('name', list(Q.equality_cases()))
def test_comparisons_at_equality_and_one_step_beyond(name):
    t, params, gk, pk = Q.equality_cases()[name]
    got = both_forms(t, params)
    assert got[0][0].tolist() == gk and got[2][0].tolist() == pk, (got[0][0].tolist(), got[2][0].tolist())


def test_chains_take_one_round_per_link():
    for case in (Q.split_chain(40), Q.split_chain(3), Q.merge_chain(5)):
        t, params, gk, gg, pk, pg, rounds = case
        got = both_forms(t, params)
        assert np.array_equal(got[0][0], gk) and np.array_equal(got[1][0], gg)
        assert np.array_equal(got[2][0], pk) and np.array_equal(got[3][0], pg) and got[5][0].tolist() == rounds


def test_sequential_form_equals_the_rounds_on_random_graphs():
    rng = np.random.default_rng(20)
    kinds, most_split, most_merge = set(), 0, 0
    for _ in range(1000):
        args = Q.random_graph(rng)
        seq = L.line_matching(*args)
        rnd = L.line_matching_rounds(*args)
        for a, b in zip(seq, rnd[:4]):
            assert a.dtype == b.dtype and np.array_equal(a, b), (args, seq, rnd)
        M, N = len(args[0]), len(args[1])
        assert rnd[4][0] <= min(M, N // 2) and rnd[4][1] <= min(N, M // 2)
        # what the outputs must satisfy whatever the graph: groups and kinds agree
        gk, gg, pk, pg = seq
        for g in range(M):
            assert (gg[g] >= 0) == (gk[g] in (2, 3, 4)) and (gk[g] != 3 or gg[g] == g)
            assert gk[g] not in (2, 4) or (pk[gg[g]] == gk[g] and (gk[g] == 4 or pg[gg[g]] == g))
        for p in range(N):
            assert (pg[p] >= 0) == (pk[p] in (2, 3, 4)) and (pk[p] != 4 or pg[p] == p)
            assert pk[p] != 3 or gk[pg[p]] == 3
        kinds |= set(gk.tolist()) | {10 + k for k in pk.tolist()}
        most_split, most_merge = max(most_split, rnd[4][0]), max(most_merge, rnd[4][1])
    assert kinds == {0, 1, 2, 3, 4, 5, 10, 11, 12, 13, 14, 15} and most_split >= 3 and most_merge >= 2, (kinds, most_split,
                                                                                                      most_merge)


def test_intersection_against_an_exact_clip():
    rng = np.random.default_rng(3)
    far, exact_floor = 0, 0
    for _ in range(500):
        g, p = C.random_pair(rng)
        rows, ok = E.match_rows(np.stack([g, p]))
        if not ok.all():
            continue
        inter2, _ = R.quad_inter2_host(rows[0], rows[1])
        exact = C.exact_inter2(rows[0], rows[1])
        if rows[0][8] > rows[1][10] or rows[1][8] > rows[0][10] or rows[0][9] > rows[1][11] or rows[1][9] > rows[0][11]:
            assert exact == 0 and inter2 == 0.0
        assert abs(Fraction(inter2) - exact) < Fraction(1, 10 ** 6), (inter2, float(exact))
        nearest = round(exact)
        if abs(exact - nearest) > Fraction(1, 10 ** 6):  # not within 1e-6 of an integer: the floor must be the exact one
            far += 1
            assert L.inter_floor(inter2) == exact.numerator // exact.denominator
            exact_floor += 1
    assert far >= 450 and exact_floor == far, far  # at least 90 % of the pairs qualify: a condition on the inputs


def test_magnitude_bounds_in_python_integers():
    big = 1 << 19
    quad = np.array([[[-big, -big], [-big, big], [big, big], [big, -big]]], np.float64) / 16  # Q4 corners at +-2^19
    rows, ok = E.match_rows(quad)
    assert ok.all()
    area2 = E._area2(rows[0])
    assert area2 == 2 * (2 * big) ** 2 == L.AREA_MAX == 1 << 41
    inter2, _ = R.quad_inter2_host(rows[0], rows[0])
    I = L.inter_floor(inter2)
    assert I == area2 and 8192 * I <= 1 << 54 and 256 * 8192 * I <= 1 << 62 < (1 << 63) - 1
    assert 256 * area2 <= 1 << 49
    # the clamps are what holds the bounds for a table that lies
    assert L.inter_floor(1e30) == L.AREA_MAX and L.inter_floor(float(L.AREA_MAX) - 0.5) == L.AREA_MAX - 1
    assert L.clamp_area(-5) == 0 and L.clamp_area(1 << 62) == L.AREA_MAX and L.clamp_area(77) == 77
    # a candidate word holds I above 15 bits
    assert (L.AREA_MAX << 15) < 1 << 64
    t = Q.table(rows, rows)
    got = both_forms(t, {})
    assert got[0][0].tolist() == [2] and got[4][0, :3].tolist() == [1, 1, 1]


def test_lying_rows_are_used_as_they_are():
    t = list(Q.random_tables(5, 1, 20, 20))
    for lie in (t[0], t[3]):
        lie[:, 0::4, 8:12] = (0, 0, 40000, 40000)
        lie[0, 3, 8:12] = (-(1 << 30), -(1 << 30), 1 << 30, 1 << 30)
        lie[0, 7, 12:14] = (-5, -1)
        lie[:, 0::5, 12:14] = (0, 0)
        lie[0, 9, 12:14] = (0, 1 << 30)  # 2^62
        lie[:, 11, 14] = -3
    got = both_forms(tuple(t), {})
    assert got[4][0, 9] > 100


def test_line_score_against_fractions():
    s = L.LineScore()
    stats = [[10, 12, 4, 2, 5, 2, 1, 3, 1, 0, 0, 0, 0, 0, 0, 0], [7, 5, 3, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]]
    for st in stats:
        s.add(np.array(st, np.int64))
    credit = Fraction(4, 5)
    recall = (7 + credit * 3 + credit * 2) / 17
    precision = (7 + credit * 7 + credit * 1) / 17
    assert (s.n_gt, s.n_pred, s.one_to_one, s.split_gt, s.split_pred, s.merged_gt, s.merge_pred, s.n_dc, s.n_ignored) == (
        17, 17, 7, 3, 7, 2, 1, 3, 1)
    assert abs(s.recall - float(recall)) < 1e-15 and abs(s.precision - float(precision)) < 1e-15
    assert abs(s.f1 - float(2 * precision * recall / (precision + recall))) < 1e-15
    other = L.LineScore(split_credit=1.0, merge_credit=0.0).add(stats[0])
    assert other.recall == (4 + 2) / 10 and other.precision == (4 + 5) / 12
    empty = L.LineScore()
    assert empty.recall == 0.0 and empty.precision == 0.0 and empty.f1 == 0.0
    with pytest.raises(ValueError):
        L.LineScore().add([1, 1, 2, 0, 0, 0, 0, 0, 0])


def test_evaluate_lines_host_on_lists():
    gt, care, pred = Q.page(7, 30)
    res, score = L.evaluate_lines_host([pred, pred[:0], pred[:4]], [gt, gt[:3], gt[:0]], [care, care[:3], care[:0]])
    assert len(res) == 3 and res[1].pred_kind.shape == (0,) and res[2].gt_kind.shape == (0,)
    assert res[0].stat('one_to_one') > 3 and res[0].stat('split_gt') > 3 and res[0].stat('merged_gt') >= 2
    assert score.n_gt == int(care.sum()) + int(care[:3].sum()) and 0.5 < score.recall < 1 and 0.5 < score.precision < 1
    assert res[1].stats[:9].tolist() == [int(care[:3].sum()), 0, 0, 0, 0, 0, 0, 3 - int(care[:3].sum()), 0]
    # line polygons scored by one-to-one IoU miss what the line score credits
    _, plain = E.evaluate_quads_host([pred], [gt[care != 0]])
    assert plain.tp < res[0].stat('one_to_one') + res[0].stat('split_gt') + res[0].stat('merged_gt')


def test_parameter_ranges():
    assert L.check_line_thresholds() == (205, 102, 0.5)
    assert L.check_line_thresholds(1.0, 1 / 256, 1.0) == (256, 1, 1.0)
    assert L.check_line_thresholds(0.5 + 1 / 512, 0.5 + 3 / 512)[:2] == (128, 130)  # half to even
    for bad in (dict(recall_thr=0.0), dict(recall_thr=1.01), dict(recall_thr=float('nan')), dict(precision_thr=-0.1),
                dict(precision_thr=0.001), dict(precision_thr=2), dict(cover_thr=0.0), dict(cover_thr=1.5),
                dict(cover_thr=float('nan'))):
        with pytest.raises(ValueError):
            L.check_line_thresholds(**bad)
    t = Q.hand_cases()['split'][0]
    with pytest.raises(ValueError):
        L.match_lines_host(*t, recall_thr=0.0)
    with pytest.raises(ValueError):
        L.match_lines_host(t[0], t[1], np.ones((1, 3), np.uint8), t[3], t[4])
    with pytest.raises(ValueError):
        L.match_lines_host(t[0][0], t[1], None, t[3], t[4])
    with pytest.raises(ValueError):
        L.evaluate_lines_host([np.zeros((1, 4, 2))], [])
    with pytest.raises(ValueError):
        L.evaluate_lines([np.zeros((1, 4, 2))], [np.zeros((1, 4, 2))], device='cpu')
