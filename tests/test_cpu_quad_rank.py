"""The rule of inferencing/ranking.py on the host: the pair quantities against quad_iou_host and an exact clip, the hand
cases, the sorted form against the rounds restatement on random graphs with exact ties, average precision against an exact
restatement over fractions, and the argument checks.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import quad_match_cases as C
from tests import quad_rank_cases as Q
from vkit_ocr_model_adaptive_scaling_amd.inferencing import evaluation as E
from vkit_ocr_model_adaptive_scaling_amd.inferencing import ranking as R


def test_inter2_and_iou_of_one_clip_on_2000_seeded_pairs():
    """iou: == quad_iou_host.  inter2 against the exact clip: tests/test_cpu_quad_match.py pins the IoU's absolute error at
    1e-12 (clipped vertices carry a few 2^-53 relative on coordinates of up to 2^16 Q4 units, then a shoelace sum of at most
    eight terms and one quotient).  inter2 is that quotient's numerator: the same error sources without the division,
    relative to the areas, so |inter2 - exact| <= 1e-12 * (area2_g + area2_p), the union's upper bound.  The measured worst
    is printed below."""
    rng = np.random.default_rng(20)
    worst, overlapping = 0.0, 0
    for _ in range(2000):
        g, p = C.random_pair(rng)
        rows, ok = E.match_rows(np.stack([g, p]))
        if not ok.all():
            continue
        inter2, iou = R.quad_inter2_host(rows[0], rows[1])
        assert iou == E.quad_iou_host(rows[0], rows[1])
        boxes_meet = not (rows[0][8] > rows[1][10] or rows[1][8] > rows[0][10] or rows[0][9] > rows[1][11] or
                          rows[1][9] > rows[0][11])
        exact = C.exact_inter2(rows[0], rows[1]) if boxes_meet else Fraction(0)
        scale = E._area2(rows[0]) + E._area2(rows[1])
        err = abs(Fraction(inter2) - exact) / scale
        assert err <= Fraction(1, 10 ** 12), float(err)
        worst, overlapping = max(worst, float(err)), overlapping + (inter2 > 0)
    assert overlapping > 1000
    print(f'inter2: worst distance from the exact clip {worst:.3g} of area2_g + area2_p')
    assert R.quad_inter2_host(*C.hand_rows('disjoint')[:2]) == (0.0, 0.0)
    g, p, _ = C.hand_rows('half_inside')
    assert R.quad_inter2_host(g[0], p[0]) == (2.0 * 2 * 4 * 256, 0.5)


@pytest.mark.parametrize('name', list(Q.hand_cases()))
def test_hand_cases(name):
    table, thrs, cover, states, match, covered, n_gt, dc_stats, rounds = Q.hand_cases()[name]
    seq = R.match_quads_ranked_host(*table, thrs, cover)
    rnd = R.match_quads_ranked_rounds_host(*table, thrs, cover)
    for a, b in zip(seq, rnd):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert seq[1][0].tolist() == states and seq[0][0].tolist() == match and seq[4][0].tolist() == covered
    assert seq[5][0, :, 3].tolist() == [n_gt] * len(thrs) and seq[6][0].tolist() == dc_stats and rnd[7][0].tolist() == rounds
    for t in range(len(thrs)):  # the matches are mutual and the statistics count the states
        for p_, g_ in enumerate(seq[0][0, t]):
            assert g_ < 0 or (seq[2][0, t, g_] == p_ and table[2][0, g_] != 0 and seq[3][0, t, p_] >= thrs[t])
        assert seq[5][0, t, :3].tolist() == [states[t].count(k) for k in (Q.TP, Q.FP, Q.IGNORED)]


def test_score_order_beats_iou_order():
    table, thrs, *_ = Q.hand_cases()['score_beats_iou']
    ranked = R.match_quads_ranked_host(*table, thrs)
    greedy = E.match_quads_host(table[0], table[1], table[3], table[4], 0.5)
    assert ranked[2][0, 0].tolist() == [1] and greedy[0][0].tolist() == [0]  # the gt's partner: by score, by IoU
    assert ranked[3][0, 0, 1] == 44 / 84 and greedy[2][0, 0] == 54 / 74


def test_coverage_is_inclusive_at_cover_thr_and_independent_of_the_iou_threshold():
    table, _, _, _, _, covered, _, _, _ = Q.hand_cases()['coverage_at_cover_thr_is_inclusive']
    inter2, _ = R.quad_inter2_host(table[0][0, 0], table[3][0, 0])
    assert inter2 == 0.5 * E._area2(table[3][0, 0])  # exactly at the threshold
    for thrs in ((0.1,), (0.5, 0.9), (1.0,)):
        assert R.match_quads_ranked_host(*table, thrs)[4][0].tolist() == covered
    above = math.nextafter(0.5, 1.0)
    assert R.match_quads_ranked_host(*table, (0.5,), above)[4][0].tolist() == [0, 0]


def test_chain_of_forty():
    table, thrs, states, match, rounds = Q.chain_case()
    rnd = R.match_quads_ranked_rounds_host(*table, thrs)
    seq = R.match_quads_ranked_host(*table, thrs)
    assert np.array_equal(rnd[1][0], states) and np.array_equal(rnd[0][0], match) and rnd[7][0].tolist() == rounds == [40, 1]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(seq, rnd))
    for n in (1, 2, 7):
        assert R.match_quads_ranked_rounds_host(*Q.chain_case(n)[0], thrs)[7][0].tolist() == [n, 1]


def test_sorted_form_equals_rounds_on_1000_random_graphs_with_ties():
    rng = np.random.default_rng(1234)
    tied_probs = tied_ious = many_rounds = 0
    for _ in range(1000):
        part, probs, covered, edges, M = Q.random_graph(rng)
        for thr in (0.25, 0.5, 0.75):
            seq = R.ranked_matching(part, probs, covered, edges, M, thr)
            rnd = R.ranked_matching_rounds(part, probs, covered, edges, M, thr)
            for a, b in zip(seq, rnd[:4]):
                assert np.array_equal(a, b), (edges, probs.tolist(), thr)
            assert 0 <= rnd[4] <= int(part.sum()) and (rnd[4] > 0) == bool(part.any())
            many_rounds += rnd[4] > 2
            assert ((seq[1] == Q.ABSENT) == ~part).all() and ((seq[1] == Q.IGNORED) <= (covered != 0)).all()
        live = probs[part]
        tied_probs += len(set(live.tolist())) < len(live)
        tied_ious += any(len({w for g, p, w in edges if p == q}) < sum(1 for g, p, w in edges if p == q) for q in range(len(part)))
    assert tied_probs > 900 and tied_ious > 300 and many_rounds > 300


def test_random_tables_through_both_oracles():
    table = Q.random_tables(3, 2, 40, 45)
    thrs = (0.3, 0.5, 0.7)
    pairs = R.ranked_pairs(*table, thrs)
    seq = R.match_quads_ranked_host(*table, thrs, pairs=pairs)
    rnd = R.match_quads_ranked_rounds_host(*table, thrs, pairs=pairs)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(seq, rnd))
    stats, dc = seq[5], seq[6]
    assert (dc[:, 0] > 2).all() and (dc[:, 2] > 0).all() and (stats[:, 0, 4] < 45).all() and (stats[:, :, 2] > 0).all()
    assert (np.diff(stats[:, :, 6], axis=1) <= 0).all() and (stats[:, :, 0] + stats[:, :, 1] + stats[:, :, 2] ==
                                                              stats[:, :, 4]).all()
    part = (seq[1][:, 0] != Q.ABSENT)
    assert (seq[1] != Q.ABSENT).all(axis=1).sum() == part.sum() and rnd[7].max() > 1
    none = R.match_quads_ranked_host(table[0], table[1], None, *table[3:], thrs)
    assert not none[6].any() and (none[5][:, 0, 3] > stats[:, 0, 3]).all()


def test_average_precision_against_fractions_on_200_seeded_state_vectors():
    rng = np.random.default_rng(99)
    worst = 0.0
    for _ in range(200):
        images = int(rng.integers(1, 4))
        states = [rng.integers(0, 4, int(rng.integers(0, 30))).astype(np.uint8) for _ in range(images)]
        probs = [(rng.integers(0, 8, len(s)) / np.float32(8)).astype(np.float32) for s in states]  # ties, and zeros
        for s, p in zip(states, probs):
            p[(s == Q.ABSENT) & (rng.uniform(size=len(s)) < 0.5)] = np.nan
            p[rng.uniform(size=len(p)) < 0.1] *= np.float32(-1.0)  # -0.0 among them
        n_tp = sum(int((s == Q.TP).sum()) for s in states)
        n_gt = n_tp + int(rng.integers(0, 10))
        curve = R.average_precision_host(states, probs, n_gt)
        ap, best = Q.exact_average_precision(states, probs, n_gt)
        worst = max(worst, abs(float(Fraction(curve.ap) - ap)))
        assert abs(Fraction(curve.ap) - ap) <= Fraction(1, 10 ** 12)
        assert 0.0 <= curve.ap <= 1.0 and len(curve.probs) == sum(int(((s == Q.TP) | (s == Q.FP)).sum()) for s in states)
        assert (np.diff(curve.probs) <= 0).all() and (curve.tp + curve.fp == np.arange(1, len(curve.probs) + 1)).all()
        if best is None:
            assert curve.best == R.OperatingPoint(math.inf, 0.0, 0.0, 0.0)
        else:
            b = curve.best
            assert b.score_thr == best[0] and (b.precision, b.recall, b.f1) == tuple(float(v) for v in best[1:])
            # the cut never splits equal probs: every pred at the threshold's prob is in, and the counts are those of a cut
            k = int((curve.probs >= np.float32(b.score_thr)).sum())
            assert k > 0 and b.precision == curve.tp[k - 1] / k and (k == len(curve.probs) or curve.probs[k] < b.score_thr)
    print(f'average precision: worst distance from the exact value {worst:.3g} (bound 1e-12)')


def test_average_precision_of_perfect_and_degenerate_rankings():
    s = np.array([Q.TP] * 5 + [Q.FP] * 3 + [Q.IGNORED, Q.ABSENT], np.uint8)
    p = np.array([0.9, 0.9, 0.8, 0.7, 0.7, 0.6, 0.6, 0.5, 0.99, np.nan], np.float32)
    c = R.average_precision_host(s, p, 5)
    assert c.ap == 1.0 and c.best == R.OperatingPoint(float(np.float32(0.7)), 1.0, 1.0, 1.0)
    c = R.average_precision_host(s, p, 10)
    assert c.ap == 0.5 and c.best.recall == 0.5
    with pytest.raises(ValueError):
        R.average_precision_host(s, p, 4)  # more TPs than gts
    c = R.average_precision_host(np.where(s == Q.TP, Q.FP, s).astype(np.uint8), p, 0)
    assert c.ap == 0.0 and c.best.f1 == 0.0 and not c.recall.any() and len(c.probs) == 8
    # one TP among three equal probs: the only cut takes all three
    c = R.average_precision_host(np.array([Q.FP, Q.TP, Q.FP], np.uint8), np.full(3, 0.5, np.float32), 1)
    assert c.ap == 0.5 and c.best == R.OperatingPoint(0.5, 1 / 3, 1.0, 0.5)  # (FP, TP, FP) by index: precision 1 / 2 at the TP
    assert R.average_precision_host([], [], 3).best.score_thr == math.inf
    # the first maximum: two cuts with F1 = 2 / 3
    c = R.average_precision_host(np.array([Q.TP, Q.FP, Q.TP, Q.FP], np.uint8), np.array([.9, .8, .7, .6], np.float32), 2)
    assert c.best.score_thr == float(np.float32(0.7)) and c.best.f1 == 0.8


def test_ranked_score_over_a_batch():
    table = Q.random_tables(8, 3, 30, 30, (30, 0, 12), (30, 5, 30))
    thrs = (0.3, 0.6)
    outs = R.match_quads_ranked_host(*table, thrs)
    score = R.ranked_score(outs, np.clip(table[4], 0, 30), table[5], thrs)
    assert score.n_gt == outs[5][:, 0, 3].sum() and score.tp.tolist() == outs[5][:, :, 0].sum(axis=0).tolist()
    assert score.map == math.fsum(score.ap.tolist()) / 2 and score.ap[0] >= score.ap[1] > 0 and len(score.best) == 2
    assert [len(c.probs) for c in score.curves] == (outs[5][:, :, 0] + outs[5][:, :, 1]).sum(axis=0).tolist()


def test_evaluate_quads_ranked_host_on_lists():
    gt, care, pred, probs = Q.page(5)
    res, score = R.evaluate_quads_ranked_host([pred[:60], pred[:0]], [gt[:50], gt[:3]], [probs[:60], probs[:0]],
                                              [care[:50], care[:3]], iou_thrs=(0.5, 0.75))
    assert len(res) == 2 and res[0].pred_state.shape == (2, 60) and res[1].gt_match.shape == (2, 3)
    assert score.n_gt == int(care[:50].sum() + care[:3].sum()) and 0 <= score.ap[1] <= score.ap[0] <= 1
    allcare, score2 = R.evaluate_quads_ranked_host([pred[:60]], [gt[:50]], [probs[:60]], iou_thrs=(0.5,))
    assert score2.n_gt == 50 and not allcare[0].covered.any() and allcare[0].gt_care.all()
    assert R.DEFAULT_IOU_THRS[0] == 0.5 and len(R.DEFAULT_IOU_THRS) == 10


def test_argument_checks():
    table = Q.random_tables(1, 1, 6, 6)
    for thrs in ((0.5, 0.5), (0.6, 0.5), (0.0,), (-0.1, 0.5), (0.5, 1.01), (float('nan'),), (), tuple(0.05 * (i + 1) for i in range(17))):
        with pytest.raises(ValueError):
            R.match_quads_ranked_host(*table, thrs)
        with pytest.raises(ValueError):
            R.match_quads_ranked_rounds_host(*table, thrs)
    R.match_quads_ranked_host(*table, tuple(0.05 * (i + 1) for i in range(16)))
    R.match_quads_ranked_host(*table, (1.0,), 1.0)
    for cover in (0.0, -1.0, 1.5, float('nan')):
        with pytest.raises(ValueError):
            R.match_quads_ranked_host(*table, (0.5,), cover)
    with pytest.raises(ValueError):
        R.match_quads_ranked_host(table[0][:, :, :15], *table[1:], (0.5,))
    with pytest.raises(ValueError):
        R.match_quads_ranked_host(*table[:5], table[5][:, :4], (0.5,))
    with pytest.raises(ValueError):
        R.match_quads_ranked_host(table[0], table[1], table[2][:, :4], *table[3:], (0.5,))
    with pytest.raises(ValueError):
        R.evaluate_quads_ranked([], [], [], device='cpu')
    with pytest.raises(ValueError):
        R.evaluate_quads_ranked_host([np.zeros((2, 4, 2))], [np.zeros((1, 4, 2))], [np.zeros(3)])


def test_the_op_checks_its_arguments_and_has_no_cpu_fallback():
    from vkit_ocr_model_adaptive_scaling_amd import ops
    gt, cg, care, pred, cp, probs = (torch.from_numpy(t) for t in Q.random_tables(1, 1, 6, 6))
    ok = lambda **kw: dict(dict(gt_rows=gt, gt_count=cg, gt_care=care, pred_rows=pred, pred_count=cp, probs=probs,
                                iou_thrs=(0.5, 0.75)), **kw)
    for bad in (ok(iou_thrs=(0.5, 0.5)), ok(iou_thrs=(0.75, 0.5)), ok(iou_thrs=(0.0,)), ok(iou_thrs=(1.5,)), ok(iou_thrs=()),
                ok(iou_thrs=tuple(0.05 * (i + 1) for i in range(17))), ok(cover_thr=0.0), ok(probs=probs.double()),
                ok(probs=probs[:, :4]), ok(gt_care=care.int()), ok(gt_care=care[:, :3]), ok(gt_rows=gt[:, :, :8]),
                ok(gt_count=cg.long()), ok(pred_count=torch.zeros((2,), dtype=torch.int32)), ok(max_pairs=-1),
                ok(rounds=torch.zeros((1, 3), dtype=torch.int32)), ok(pred_rows=torch.zeros((1, 8193, 16), dtype=torch.int32),
                                                                       probs=torch.zeros((1, 8193)))):
        with pytest.raises(ValueError):
            ops.match_quads_ranked(**bad)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.match_quads_ranked(**ok())
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.match_quads_ranked(**ok(gt_care=None))
