"""The quad-matching rule on the host (inferencing/evaluation.py): the binary64 IoU oracle against exact arithmetic, the
hand cases with ``==``, the row and validity rules, the sorted greedy matching against a mutual-best-rounds restatement, the
scores, ``result_quads`` and the argument checks of the C ABI and of ``ops.match_quads``, which run before anything touches
the device.  The exact clip and the rounds are tests/quad_match_cases.py's, written apart from the module under test."""
import ctypes
import types
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import quad_match_cases as C
from vkit_ocr_model_adaptive_scaling_amd.inferencing import evaluation as E

# |quad_iou_host - exact IoU| on rotated, jittered quads of 4 to 60 px with centres up to 3000 px.  The intersection's
# vertices carry a relative rounding error of a few 2^-53 on coordinates of up to 2^16 Q4 units, the shoelace sum of at
# most eight terms and the quotient a few more: measured 7.8e-16 on 4000 such pairs; the pin leaves three orders of
# magnitude for other seeds.
IOU_ABS = 1e-12


def test_oracle_matches_exact_arithmetic():
    rng = np.random.default_rng(20261019)
    worst, overlapping = 0.0, 0
    for _ in range(2000):
        g, p = C.random_pair(rng)
        (gr, pr), ok = zip(*(E.match_rows(q[None]) for q in (g, p)))
        gr, pr = gr[0], pr[0]
        assert ok[0][0] and ok[1][0]
        exact = C.exact_iou(gr, pr)
        assert exact == C.exact_iou(pr, gr), 'the exact IoU is symmetric'
        got = E.quad_iou_host(gr, pr)
        boxes_apart = gr[8] > pr[10] or pr[8] > gr[10] or gr[9] > pr[11] or pr[9] > gr[11]
        assert (got == 0.0 and exact == 0) if boxes_apart else True
        worst = max(worst, abs(got - float(exact)), abs(E.quad_iou_host(pr, gr) - float(exact)))
        overlapping += exact > 0
    print(f'largest |oracle - exact| {worst:.3e} over 2000 pairs, {overlapping} of them overlapping')
    assert overlapping > 1500 and worst <= IOU_ABS


@pytest.mark.parametrize('name', list(C.HAND))
def test_hand_cases(name):
    g, p, want = C.hand_rows(name)
    got = E.quad_iou_host(g[0], p[0])
    if want is not None:
        assert got == float(want) and C.exact_iou(g[0], p[0]) == want
    else:  # the square against itself turned by 45 degrees: an octagon
        ring_exact = C.exact_iou(g[0], p[0])
        assert abs(got - float(ring_exact)) <= IOU_ABS and 0.6 < got < 0.75
    out = E.match_quads_host(g[None], [1], p[None], [1], 0.5)
    matched = want is None or want >= Fraction(1, 2)  # 'half_inside' and the diamonds sit exactly on the threshold: >=
    assert int(out[0][0, 0]) == (0 if matched else -1) and int(out[3][0, 0]) == int(matched)
    assert int(out[3][0, 3]) == (0 if name == 'disjoint' else 1), 'touching boxes are a pair, disjoint ones are not'


def test_turned_square_has_eight_vertices():
    g, p, _ = C.hand_rows('turned')
    ring = [(float(p[0][2 * k] - 64), float(p[0][2 * k + 1] - 64)) for k in range(4)]
    gq = [(float(g[0][2 * k] - 64), float(g[0][2 * k + 1] - 64)) for k in range(4)]
    for k in range(4):
        ring = E._clip(ring, *gq[k], *gq[(k + 1) % 4])
    assert len(ring) == 8


def test_rows_and_validity():
    good = np.array(C.SQ(1.5, 2.25, 3, 5), dtype=np.float64)
    quads = np.stack([good,
                      good[::-1],                                            # counter-clockwise
                      np.array([[0, 0], [0, 4], [1, 1], [4, 0]], float),     # non-convex
                      np.array([[0, 0], [0, 4], [0, 8], [4, 0]], float),     # three corners in line: not strictly convex
                      np.where(np.eye(4, 2, dtype=bool), np.nan, good),      # NaN
                      good + 2.0 ** 15,                                      # 16 * (2^15 + 1.5) > 2^19
                      good])
    rows, ok = E.match_rows(quads, valid=[1, 1, 1, 1, 1, 1, 0])
    assert ok.tolist() == [True, False, False, False, False, False, False]
    assert not rows[1:].any(), 'invalid quads get zero rows'
    r = rows[0]
    assert r[:8].tolist() == [24, 36, 24, 116, 72, 116, 72, 36] and r[8:12].tolist() == [24, 36, 72, 116]
    assert E._area2(r) == 2 * 48 * 80 and r[14] == 1 and r[15] == 0
    assert E.match_rows(np.array(C.SQ(0.03125, 0.09375, 1, 1), float))[0][0, :2].tolist() == [0, 2], 'rint: half to even'
    edge = np.array(C.SQ(-2.0 ** 15, -2.0 ** 15, 2.0 ** 16, 2.0 ** 16))
    rows, ok = E.match_rows(edge[None])
    assert ok[0] and rows[0, 8:12].tolist() == [-(1 << 19), -(1 << 19), 1 << 19, 1 << 19] and E._area2(rows[0]) == 1 << 41
    assert E.quad_iou_host(rows[0], rows[0]) == 1.0
    assert E.match_rows(np.zeros((0, 4, 2)))[0].shape == (0, 16)
    with pytest.raises(ValueError):
        E.match_rows(good[None], valid=[1, 1])


def test_greedy_equals_mutual_best_rounds():
    rng = np.random.default_rng(7)
    most = 0
    for _ in range(1000):
        M, N = rng.integers(1, 13, 2)
        k = int(rng.integers(0, 3 * max(M, N)))
        pairs = {(int(g), int(p)) for g, p in zip(rng.integers(0, M, k), rng.integers(0, N, k))}
        edges = [(g, p, float(rng.integers(5, 9)) / 8.0) for g, p in sorted(pairs)]  # four weights: many exact ties
        gm, pm, gw = E.greedy_matching(edges, M, N)
        rgm, rpm, rounds = C.mutual_best_rounds(edges, M, N)
        assert np.array_equal(gm, rgm) and np.array_equal(pm, rpm)
        assert rounds <= min(M, N)
        weight = {(g, p): w for g, p, w in edges}
        assert all(gw[g] == (weight[(g, gm[g])] if gm[g] >= 0 else 0.0) for g in range(M))
        most = max(most, rounds)
    assert most >= 3


def _match(gt, pred, thr=0.5):
    t = E.evaluation_tables([pred], [gt])
    return E.match_quads_host(*t[:4], thr), t


def test_ties_go_to_the_lower_index():
    cases = C.tie_cases()
    out, _ = _match(*cases['two_preds'])
    assert out[0][0].tolist() == [0] and out[1][0].tolist() == [0, -1]
    out, _ = _match(*cases['two_gts'])
    assert out[0][0].tolist() == [0, -1] and out[1][0].tolist() == [0]
    assert out[3][0].tolist() == [1, 2, 1, 2, 2, 0]


def test_chain_needs_three_rounds():
    gt, pred, want, rounds = C.chain_case()
    out, t = _match(gt, pred)
    assert out[0][0].tolist() == want.tolist() and out[3][0, 0] == 3 and out[3][0, 4] == 6
    g, p = t[0][0], t[2][0]
    edges = [(a, c, E.quad_iou_host(g[a], p[c])) for a in range(4) for c in range(3)]
    edges = [e for e in edges if e[2] >= 0.5]
    chain = sorted(e[2] for e in edges)
    assert len(edges) == 6 and all(a < b for a, b in zip(chain, chain[1:]))
    assert C.mutual_best_rounds(edges, 4, 3)[2] == rounds == 3
    assert [e[2] for e in edges if e[:2] == (0, 0)] == [43.0 / 85.0]


def test_counts_are_clamped_and_invalid_rows_skipped():
    gt, cg, pred, cp = C.random_tables(3, 2, 6, 5)
    ref = E.match_quads_host(gt, cg, pred, cp)
    over = E.match_quads_host(gt, [99, 99], pred, [77, 77])
    assert all(np.array_equal(a, b) for a, b in zip(ref, over))
    none = E.match_quads_host(gt, [-3, 0], pred, cp)
    assert (none[0] == -1).all() and none[3][:, [0, 1, 3, 4]].sum() == 0 and none[3][:, 2].tolist() == [5, 5]
    dead = gt.copy()
    dead[:, :, 14] = 0
    assert E.match_quads_host(dead, cg, pred, cp)[3][:, [0, 1, 3]].sum() == 0


def test_detection_score():
    s = E.DetectionScore()
    assert (s.precision, s.recall, s.f1, s.mean_iou) == (0.0, 0.0, 0.0, 0.0)
    s.add(3, 4, 6, 2.25).add(0, 2, 0)
    assert (s.tp, s.fp, s.fn) == (3, 3, 3) and s.precision == 0.5 and s.recall == 0.5 and s.f1 == 0.5 and s.mean_iou == 0.75
    s = E.DetectionScore().add(0, 0, 5)
    assert (s.precision, s.recall, s.f1) == (0.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        E.DetectionScore().add(3, 2, 5)


def test_evaluate_quads_host_and_score_threshold():
    gt, pred = C.page(11, lines=3, per_line=8)
    res, score = E.evaluate_quads_host([pred, pred[:0]], [gt, gt])
    assert len(res) == 2 and res[1].tp == 0 and res[1].n_pred == 0 and res[1].n_gt == len(gt)
    assert score.tp == res[0].tp and score.fn == 2 * len(gt) - res[0].tp and score.fp == len(pred) - res[0].tp
    assert res[0].tp > 15 and np.isclose(score.mean_iou, res[0].gt_iou.sum() / res[0].tp)
    scores = np.linspace(0.0, 1.0, len(pred))
    cut, _ = E.evaluate_quads_host([pred], [gt], pred_scores=[scores], score_thr=0.5)
    assert cut[0].n_pred == int((scores >= 0.5).sum()) and cut[0].pred_valid.tolist() == (scores >= 0.5).tolist()
    assert (cut[0].pred_match[scores < 0.5] == -1).all()
    with pytest.raises(ValueError):
        E.evaluate_quads_host([pred], [gt, gt])
    with pytest.raises(ValueError):
        E.evaluate_quads_host([pred], [gt], pred_scores=[scores])
    with pytest.raises(ValueError):
        E.evaluate_quads_host([pred], [gt], iou_thr=0.0)
    with pytest.raises(ValueError, match='GPU'):
        E.evaluate_quads([pred], [gt], device='cpu')


def test_result_quads_flattens_regions():
    from vkit_ocr_model_adaptive_scaling_amd import inferencing as I
    a, b = np.arange(16, dtype=np.float64).reshape(2, 4, 2), np.arange(8, dtype=np.float64).reshape(1, 4, 2) + 100
    r = types.SimpleNamespace(polygons=[a, np.zeros((0, 4, 2)), b],
                              probs=[np.array([0.9, 0.8], np.float32), np.zeros((0,), np.float32), np.array([0.7], np.float32)])
    quads, probs = I.result_quads(r)
    assert quads.shape == (3, 4, 2) and np.array_equal(quads[2], b[0]) and probs.tolist() == [np.float32(0.9), np.float32(0.8),
                                                                                              np.float32(0.7)]
    empty = I.result_quads(types.SimpleNamespace(polygons=[], probs=[]))
    assert empty[0].shape == (0, 4, 2) and empty[1].shape == (0,)
    with pytest.raises(ValueError):
        I.result_quads(types.SimpleNamespace(polygons=[a], probs=[np.zeros((3,), np.float32)]))
    for name in ('DetectionScore', 'evaluate_quads', 'match_rows', 'match_quads_host', 'quad_iou_host', 'result_quads'):
        assert hasattr(I, name), name


def test_c_abi_validates_before_touching_anything():
    from vkit_ocr_model_adaptive_scaling_amd import _lib
    L = _lib.lib
    err = lambda: L.vkas_last_error()
    assert L.vkas_quad_match_workspace_bytes(2, 65, 63, 100) > 2 * 2 * 128 * 8
    assert L.vkas_quad_match_workspace_bytes(1, 0, 4, 8) == -1 and b'1..8192' in err()
    assert L.vkas_quad_match_workspace_bytes(1, 4, 8193, 8) == -1 and b'1..8192' in err()
    assert L.vkas_quad_match_workspace_bytes(-1, 4, 4, 8) == -1 and b'bad B' in err()
    assert L.vkas_quad_match_workspace_bytes(1, 4, 4, -1) == -1 and b'max_pairs' in err()
    assert L.vkas_quad_match_workspace_bytes(3, 4, 4, 1 << 30) == -1 and b'2^31' in err()
    nb = L.vkas_quad_match_workspace_bytes(1, 4, 4, 8)
    a = lambda: ctypes.c_void_p(256)  # any aligned non-null address: the checks run before anything is dereferenced

    def call(gt=None, B=1, M=4, N=4, thr=0.5, cap=8, ws=None, nbytes=nb, iou=None, stats=None):
        return L.vkas_quad_match(gt or a(), a(), a(), a(), B, M, N, thr, cap, ws or a(), nbytes, a(), a(), iou or a(),
                                 stats or a(), None, None)
    assert L.vkas_quad_match(None, a(), a(), a(), 1, 4, 4, 0.5, 8, a(), nb, a(), a(), a(), a(), None, None) == -1 \
        and b'null' in err()
    assert call(M=8193) == -1 and b'1..8192' in err()
    assert call(N=0) == -1 and b'1..8192' in err()
    assert call(B=-2) == -1 and b'bad B' in err()
    assert call(cap=-1) == -1 and b'max_pairs' in err()
    for thr in (0.0, -0.5, 1.5, float('nan')):
        assert call(thr=thr) == -1 and b'iou_thr' in err()
    assert call(nbytes=nb - 1) == -1 and b'needed' in err()
    assert call(ws=ctypes.c_void_p(264)) == -1 and b'16-byte' in err()
    assert call(gt=ctypes.c_void_p(260)) == -1 and b'16-byte' in err()
    assert call(iou=ctypes.c_void_p(260)) == -1 and b'8-byte' in err()
    assert call(B=0) == 0  # nothing to do, nothing launched


def test_ops_match_quads_validates_before_launch():
    from vkit_ocr_model_adaptive_scaling_amd import ops
    z = lambda *s: torch.zeros(s, dtype=torch.int32)
    good = lambda: [z(2, 4, 16), z(2), z(2, 5, 16), z(2)]
    for i, bad in ((0, z(2, 4, 20)), (0, z(2, 4, 16).long()), (1, z(3)), (2, z(3, 5, 16)), (3, z(2).long()), (2, z(2, 0, 16)),
                   (0, z(2, 8193, 16))):
        args = good()
        args[i] = bad
        with pytest.raises(ValueError):
            ops.match_quads(*args)
    for kw in ({'iou_thr': 0.0}, {'iou_thr': 1.01}, {'max_pairs': -1}, {'rounds': z(3)}, {'rounds': torch.zeros(2)}):
        with pytest.raises(ValueError):
            ops.match_quads(*good(), **kw)
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.match_quads(*good())  # valid arguments: no CPU fallback
