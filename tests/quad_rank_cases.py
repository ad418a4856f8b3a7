"""Shared inputs of the ranked-matching tests (test_cpu_quad_rank.py, test_gpu_quad_rank.py, test_gpu_quad_rank_infer.py):
the hand cases with their expected answers, the chain, random tables with exact prob ties, don't-care flags and rows that
take no part, the seeded page with don't-care boxes, and an exact restatement of average precision over fractions."""
from fractions import Fraction
from functools import lru_cache

import numpy as np

from tests import quad_match_cases as C
from vkit_ocr_model_adaptive_scaling_amd.inferencing import evaluation as E
from vkit_ocr_model_adaptive_scaling_amd.inferencing import ranking as R

SQ = C.SQ
ABSENT, TP, FP, IGNORED = 0, 1, 2, 3


def _rows(quads):
    rows, ok = E.match_rows(np.array(quads, dtype=np.float64))
    assert ok.all()
    return rows


def table(gt, care, pred, probs, gt_count=None, pred_count=None):
    """one image -> the batched arguments of the oracles and the op (B = 1), without thresholds"""
    g, p = (gt if isinstance(gt, np.ndarray) and gt.ndim == 2 else _rows(gt)), \
        (pred if isinstance(pred, np.ndarray) and pred.ndim == 2 else _rows(pred))
    return (g[None], np.array([len(g) if gt_count is None else gt_count], np.int32), np.array(care, np.uint8)[None], p[None],
            np.array([len(p) if pred_count is None else pred_count], np.int32), np.array(probs, np.float32)[None])


# ---- hand cases: name -> (table, iou_thrs, cover_thr, states (T, N), pred_match (T, N), covered (N,), n_gt, dc_stats, rounds (T,))

def hand_cases():
    g = SQ(0, 0, 64, 64)
    near, far = SQ(0, 10, 64, 64), SQ(0, 20, 64, 64)  # IoU 54 / 74 and 44 / 84 with g
    cases = {}
    # the higher prob wins the gt although its IoU is the lower one; the loser is decided a round later
    cases['score_beats_iou'] = (table([g], [1], [near, far], [0.6, 0.9]), (0.5,), 0.5, [[FP, TP]], [[-1, 0]], [0, 0], 1,
                                [0, 0, 0], [2])
    cases['equal_probs_lower_index_first'] = (table([g], [1], [far, near], [0.9, 0.9]), (0.5,), 0.5, [[TP, FP]], [[0, -1]],
                                              [0, 0], 1, [0, 0, 0], [2])
    cases['signed_zero_probs_are_equal'] = (table([g], [1], [far, near], [-0.0, 0.0]), (0.5,), 0.5, [[TP, FP]], [[0, -1]],
                                            [0, 0], 1, [0, 0, 0], [2])
    cases['zero_probs_the_other_way'] = (table([g], [1], [far, near], [0.0, -0.0]), (0.5,), 0.5, [[TP, FP]], [[0, -1]],
                                         [0, 0], 1, [0, 0, 0], [2])
    cases['tp_at_050_fp_at_075'] = (table([g], [1], [far], [0.8]), (0.5, 0.75), 0.5, [[TP], [FP]], [[0], [-1]], [0], 1,
                                    [0, 0, 0], [1, 1])
    inside = SQ(10, 10, 20, 20)
    cases['covered_unmatched_is_ignored'] = (table([g], [0], [inside], [0.8]), (0.5,), 0.5, [[IGNORED]], [[-1]], [1], 0,
                                             [1, 1, 1], [1])
    cases['covered_but_matched_is_tp'] = (table([SQ(0, 0, 100, 100), inside], [0, 1], [inside], [0.8]), (0.5, 0.95), 0.5,
                                          [[TP], [TP]], [[1], [1]], [1], 1, [1, 1, 1], [1, 1])
    # half of the first pred lies inside the don't-care box: exactly cover_thr, inclusive; 31 / 64 of the second: not covered
    cases['coverage_at_cover_thr_is_inclusive'] = (table([g], [0], [SQ(0, 32, 64, 64), SQ(0, 33, 64, 64)], [0.8, 0.7]), (0.5,),
                                                   0.5, [[IGNORED, FP]], [[-1, -1]], [1, 0], 0, [1, 2, 1], [1])
    # the don't-care box equals the pred: never matched, not in n_gt; the care gt far away stays unmatched
    cases['dont_care_is_never_matched'] = (table([g, SQ(500, 500, 64, 64)], [0, 1], [g], [0.9]), (0.5,), 0.5, [[IGNORED]],
                                           [[-1]], [1], 1, [1, 1, 1], [1])
    six = _rows([SQ(3, 5, 8, 8)] * 6)
    six[1] = 0  # an invalid quad: a zero row
    nan, inf = float('nan'), float('inf')
    # rows 0 and 4 take part; 1 is invalid, 2 and 3 have no finite prob, 5 lies beyond the count
    cases['absent'] = (table([SQ(3, 5, 8, 8)], [1], six, [0.5, 0.9, nan, inf, 0.7, 0.8], pred_count=5), (0.5,), 0.5,
                       [[FP, ABSENT, ABSENT, ABSENT, TP, ABSENT]], [[-1, -1, -1, -1, 0, -1]], [0] * 6, 1, [0, 0, 0], [2])
    return cases


def chain_case(n=40):
    """n 64 x 64 gts 36 px apart and n preds 19 px to the right of them with descending probs: p_i overlaps g_i (IoU 45 / 83)
    and g_(i+1) (47 / 81) and nothing else above 0.1.  At 0.5 every pred is blocked by the one before it, p_i takes g_(i+1)
    and the last pred finds its only gt taken: n rounds.  At 0.56 each pred has the one candidate g_(i+1): one round.
    -> (table, iou_thrs, states (2, n), pred_match (2, n), rounds)"""
    gt = [SQ(0, 36 * k, 64, 64) for k in range(n)]
    pred = [SQ(0, 36 * k + 19, 64, 64) for k in range(n)]
    probs = [1.0 - 0.01 * k for k in range(n)]
    states = np.full((2, n), TP, np.uint8)
    states[:, n - 1] = FP
    match = np.tile(np.arange(1, n + 1, dtype=np.int32), (2, 1))
    match[:, n - 1] = -1
    return table(gt, [1] * n, pred, probs), (0.5, 0.56), states, match, [n, 1]


# ---- random tables and graphs ------------------------------------------------------------------------------------------

def random_tables(seed, B, M, N, counts_g=None, counts_p=None):
    """``quad_match_cases.random_tables`` with probs from eleven values (exact ties abound), one gt in six a don't-care one,
    and, from 9 rows on, a few rows invalid and a few probs not finite -> (gt_rows, gt_count, gt_care, pred_rows, pred_count,
    probs)"""
    gt, cg, pred, cp = C.random_tables(seed, B, M, N, counts_g, counts_p)
    rng = np.random.default_rng(7000 + seed)
    probs = (rng.integers(0, 11, (B, N)) / np.float32(10)).astype(np.float32)
    care = (rng.uniform(size=(B, M)) >= 1 / 6).astype(np.uint8) * rng.integers(1, 256, (B, M)).astype(np.uint8)
    if N > 8:
        pred[:, 5::17] = 0
        probs[:, 7::19] = np.nan
        probs[:, 8::23] = -np.inf
    if M > 8:
        gt[:, 3::13] = 0
    return gt, cg, care, pred, cp, probs


def random_graph(rng, M=7, N=9):
    """a small bipartite graph with exact prob and IoU ties -> (part, probs, covered, edges, M)"""
    part = rng.uniform(size=N) < 0.85
    probs = (rng.integers(0, 4, N) / np.float32(4)).astype(np.float32)
    probs[rng.uniform(size=N) < 0.1] *= np.float32(-0.0)  # signed zeros among the zeros
    covered = (rng.uniform(size=N) < 0.3).astype(np.uint8)
    edges = [(g, p, float(rng.integers(2, 9)) / 8) for g in range(M) for p in range(N) if part[p] and rng.uniform() < 0.3]
    return part, probs, covered, edges, M


# ---- the seeded page -----------------------------------------------------------------------------------------------------

def page(seed, boxes=15, per_box=3):
    """``quad_match_cases.page`` (300 characters in 12 lines; jittered, missing, duplicated and spurious preds) with ``boxes``
    runs of ``per_box`` neighbouring characters replaced by one don't-care box over them, and random probs
    -> (gt (n, 4, 2), care (n,), pred (m, 4, 2), probs (m,) float32)"""
    gt, pred = C.page(seed)
    rng = np.random.default_rng(2000 + seed)
    per_line = 25
    starts = rng.permutation(len(gt) // per_line * (per_line // (per_box + 1)))[:boxes]
    gone, dc = [], []
    for s in starts.tolist():
        line, slot = divmod(s, per_line // (per_box + 1))
        first = line * per_line + slot * (per_box + 1)
        run = gt[first:first + per_box].reshape(-1, 2)
        y0, x0, y1, x1 = run[:, 0].min() - 1, run[:, 1].min() - 1, run[:, 0].max() + 1, run[:, 1].max() + 1
        dc.append(np.array(SQ(y0, x0, y1 - y0, x1 - x0), np.float64))
        gone += list(range(first, first + per_box))
    keep = np.setdiff1d(np.arange(len(gt)), gone)
    quads = np.concatenate([gt[keep], np.stack(dc)])
    care = np.r_[np.ones(len(keep), np.uint8), np.zeros(len(dc), np.uint8)]
    order = rng.permutation(len(quads))
    probs = rng.uniform(0.3, 1.0, len(pred)).astype(np.float32)
    return quads[order], care[order], pred, probs


PAGE_THRS = tuple(0.5 + 0.05 * i for i in range(10))


@lru_cache(maxsize=None)
def page_reference(seed):
    """the page's tables, its clipped pairs and the rounds oracle's answer on them at ``PAGE_THRS``, computed once and
    shared: do not modify"""
    gt, care, pred, probs = page(seed)
    t = table(E.match_rows(gt)[0], care, E.match_rows(pred)[0], probs)
    pairs = R.ranked_pairs(*t, PAGE_THRS)
    return t, pairs, R.match_quads_ranked_rounds_host(*t, PAGE_THRS, pairs=pairs)


# ---- average precision, exactly ------------------------------------------------------------------------------------------

def exact_average_precision(states, probs, n_gt):
    """all-point interpolated AP and the best operating point over fractions.Fraction, written apart from
    ``average_precision_host`` -> (AP, (score_thr, precision, recall, f1) or None)"""
    items = []
    for img, (s, p) in enumerate(zip(states, probs)):
        for k in range(len(s)):
            if s[k] in (TP, FP):
                items.append((np.float32(p[k]), img, k, int(s[k] == TP)))
    done, rest = [], list(items)
    while rest:  # selection by the rule's order, one at a time
        top = rest[0]
        for it in rest[1:]:
            if it[0] > top[0] or (it[0] == top[0] and it[1:3] < top[1:3]):
                top = it
        rest.remove(top)
        done.append(top)
    prec, tps = [], 0
    for k, it in enumerate(done, 1):
        tps += it[3]
        prec.append(Fraction(tps, k))
    ap = Fraction(0)
    if n_gt:
        for k, it in enumerate(done):
            if it[3]:
                ap += max(prec[k:])
        ap /= n_gt
    best, tps = None, 0
    for k, it in enumerate(done, 1):
        tps += it[3]
        if k < len(done) and done[k][0] == it[0]:
            continue
        f1 = Fraction(2 * tps, k + n_gt)
        if best is None or f1 > best[3]:
            best = (float(it[0]), Fraction(tps, k), Fraction(tps, n_gt) if n_gt else Fraction(0), f1)
    return ap, best
