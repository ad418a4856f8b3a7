"""Average precision of character quadrilaterals: matching in score order at several IoU thresholds with don't-care
annotations - the rule, its host oracles, the device route and the curve.

The rule is THIS PROJECT'S OWN, stated on the match rows and the clip of inferencing/evaluation.py in integers and IEEE
binary64 without contraction, so that the device kernels (csrc/quadmatch.hip) and the host oracles are held to each other
for equality.

Inputs, per image: ``gt_rows`` (M, 16) and ``gt_count``; ``gt_care`` (M,) uint8, 0 = don't care; ``pred_rows`` (N, 16) and
``pred_count``; ``probs`` (N,) float32; ``iou_thrs`` (T,) binary64, strictly ascending in (0, 1], 1 <= T <= 16; ``cover_thr``
binary64 in (0, 1], 0.5 by default.  Counts are clamped to [0, K].

Taking part: a pred takes part iff it lies within the count, its ``valid`` word is set and its prob is finite (the test of
inferencing/nms.py); a gt iff it lies within the count and its ``valid`` word is set.  A gt that takes part is a CARE gt iff
``gt_care != 0`` and a DON'T-CARE gt otherwise.

Rank: q OUTRANKS p iff ``probs[q] > probs[p]``, or they are equal and ``q < p`` (float32 comparisons, so -0 equals +0): the
order of inferencing/nms.py.

Pair quantities, for the pairs whose Q4 boxes overlap (the inclusive test of ``box_pairs``, both rows taking part): ONE clip
of p against g in ``quad_iou_host``'s order of operations gives ``inter2`` after its clamp, and
``iou = inter2 / ((area2_g + area2_p) - inter2)``: ``quad_inter2_host`` of inferencing/evaluation.py, whose second result
``quad_iou_host`` is.  The pass over the pairs (``care_pairs``) is shared with inferencing/line_evaluation.py.

Covered: pred p is covered iff some don't-care gt g has ``inter2(g, p) >= cover_thr * area2_p`` (the product rounded once,
the comparison inclusive).  Coverage does not depend on the IoU threshold.  A don't-care gt is never matched and does not
count in ``n_gt``.

Candidates: the (care gt, pred) pairs with ``iou >= iou_thrs[0]``; at threshold t only those with ``iou >= iou_thrs[t]``.

Matching at threshold t, independently per threshold: going down the ranks, pred p takes the free care gt among its
candidates at t with the highest iou, ties to the lowest gt index; a taken gt is no longer free.  p is TP (1) if it took
one, else IGNORED (3) if it is covered, else FP (2).  A pred that does not take part is ABSENT (0).

The same as rounds: a round reads the states the previous round left.  An undecided pred p is decided in a round iff no
undecided pred that outranks p shares with p a gt that is free and a candidate of both at t; a decided pred takes its best
free candidate, or none.  Two preds decided in one round cannot want the same gt (the lower-ranked of them would not have
been decided), and a pred's free candidates can only be taken by preds that outrank it, all of which are decided when it
is: so what a pred takes is what the sequential rule gives it, by induction down the ranks.  The top-ranked undecided pred
can always be decided, so the rounds end after at most n.  The count of rounds that decided a pred is part of the rule:
preds without shared candidates are decided in round 1; a chain p_0 > p_1 > ... by rank with p_i overlapping g_i and
g_(i+1) takes one round per pred.  ``match_quads_ranked_host`` is the sorted sequential form,
``match_quads_ranked_rounds_host`` the rounds, written apart (tests/test_cpu_quad_rank.py holds them to each other on
random graphs with exact prob and IoU ties); the device runs the rounds.

Per image and threshold: ``pred_match`` (N,) int32 gt index or -1, ``pred_state`` (N,) uint8, ``gt_match`` (M,) int32,
``pred_iou`` (N,) float64 (0 unless TP), ``stats`` (8,) int64 = tp, fp, ignored, n_gt (care gts), n_pred (preds taking
part), pairs (care box pairs, the same for every t), candidates (those at or above ``iou_thrs[t]``), status.  Per image:
``covered`` (N,) uint8 and ``dc_stats`` (3,) int64 = n_dc, dc_pairs, n_covered.

Curve and AP at threshold t, over a batch, on the host in binary64 (``average_precision_host``): the preds of all images
that are TP or FP at t, ordered by prob descending, then image ascending, then index ascending; ``tp_k`` and ``fp_k``
cumulative integers; ``n_gt`` the care gts of the batch; ``precision_k = tp_k / k``, ``recall_k = tp_k / n_gt``;
``AP_t = (1 / n_gt) * sum over the TP ranks k of max_{j >= k} precision_j`` (all-point interpolation), summed with
``math.fsum``, 0 when ``n_gt = 0``; ``mAP`` the mean of the AP_t.  Best operating point at t: among the cuts k where the next
prob is strictly lower or k is the last (a threshold cannot split equal probs), the first maximum of
``F1_k = 2 tp_k / (k + n_gt)``, reported as ``score_thr`` (the prob at k), precision, recall and F1; without a TP or FP pred
it is (inf, 0, 0, 0).

Differences from COCO / ICDAR practice: a prediction on a don't-care annotation is ignored by COVERAGE (the share of the
prediction's own area inside the annotation), not by IoU, because illegible text is annotated as one box over many
characters; every threshold is matched independently, so a pred may take different gts at different thresholds (COCO does
the same, ICDAR matches once); a don't-care annotation is never matched, so a pred is first offered the care gts and only
then ignored; everything is measured on the Q4 grid of the match rows; precision is interpolated at all points, not at 101
recall levels.

Text lines and words, scored with one-to-many splits and many-to-one merges: inferencing/line_evaluation.py."""
import math
from typing import List, Optional, Sequence, Tuple

import attrs
import numpy as np
import torch

from .evaluation import ROW_VALID, care_pairs, quad_inter2_host, quad_rows_host  # noqa: F401 (the clip: importable here too)
from .quad_tables import clamped, host_tables, padded_sides, require_gpu, with_capacity

ABSENT, TP, FP, IGNORED = 0, 1, 2, 3
MAX_THRS = 16
DEFAULT_IOU_THRS = tuple(0.5 + 0.05 * i for i in range(10))


def check_thresholds(iou_thrs, cover_thr=0.5) -> Tuple[Tuple[float, ...], float]:
    thrs = tuple(float(v) for v in iou_thrs)
    if not 1 <= len(thrs) <= MAX_THRS:
        raise ValueError(f'between 1 and {MAX_THRS} IoU thresholds, got {len(thrs)}')
    if not all(0.0 < v <= 1.0 for v in thrs):
        raise ValueError(f'every IoU threshold must lie in (0, 1], got {thrs}')
    if any(b <= a for a, b in zip(thrs, thrs[1:])):
        raise ValueError(f'the IoU thresholds must ascend strictly, got {thrs}')
    cover_thr = float(cover_thr)
    if not (cover_thr > 0.0 and cover_thr <= 1.0):
        raise ValueError(f'cover_thr must lie in (0, 1], got {cover_thr}')
    return thrs, cover_thr


def _rank_order(part: np.ndarray, probs: np.ndarray) -> List[int]:
    p = np.asarray(probs, dtype=np.float32)
    return sorted(np.flatnonzero(part).tolist(), key=lambda k: (-float(p[k]), k))  # -0.0 == 0.0: the index decides


def ranked_matching(part, probs, covered, edges, M: int, thr: float):
    """One image at one threshold by the sorted sequential rule.  ``part`` (N,) bool: the preds that take part; ``covered``
    (N,); ``edges`` = (g, p, iou) care candidates -> ``(pred_match (N,), pred_state (N,), gt_match (M,), pred_iou (N,))``."""
    N = len(part)
    pred_match, gt_match = np.full((N,), -1, np.int32), np.full((M,), -1, np.int32)
    pred_state, pred_iou = np.zeros((N,), np.uint8), np.zeros((N,), np.float64)
    cands: List[List[Tuple[int, float]]] = [[] for _ in range(N)]
    for g, p, w in edges:
        if w >= thr:
            cands[p].append((g, w))
    for p in _rank_order(part, probs):
        free = [(w, -g) for g, w in cands[p] if gt_match[g] < 0]
        if free:
            w, mg = max(free)
            pred_match[p], gt_match[-mg], pred_iou[p], pred_state[p] = -mg, p, w, TP
        else:
            pred_state[p] = IGNORED if covered[p] else FP
    return pred_match, pred_state, gt_match, pred_iou


def ranked_matching_rounds(part, probs, covered, edges, M: int, thr: float):
    """The same by the rule's rounds, written apart from ``ranked_matching`` -> its four arrays and the count of rounds
    that decided a pred."""
    N = len(part)
    pr = np.asarray(probs, dtype=np.float32)
    outranks = lambda q, p: bool(pr[q] > pr[p] or (pr[q] == pr[p] and q < p))
    of_pred = {p: {} for p in range(N) if part[p]}
    of_gt = {}
    for g, p, w in edges:
        if w >= thr and p in of_pred:
            of_pred[p][g] = w
            of_gt.setdefault(g, set()).add(p)
    undecided, taken, took, rounds = set(of_pred), {}, {}, 0
    while undecided:
        decided = []
        for p in undecided:  # reads the states the previous round left
            rivals = set()
            for g in of_pred[p]:
                if g not in taken:
                    rivals |= of_gt[g] & undecided
            if not any(outranks(q, p) for q in rivals if q != p):
                decided.append(p)
        assert decided, 'the top-ranked undecided pred can always be decided'
        wants = {}
        for p in decided:
            free = [g for g in of_pred[p] if g not in taken]
            if free:
                best = max(of_pred[p][g] for g in free)
                wants[p] = min(g for g in free if of_pred[p][g] == best)
            else:
                wants[p] = None
        assert len({g for g in wants.values() if g is not None}) == sum(g is not None for g in wants.values())
        for p, g in wants.items():
            took[p] = g
            if g is not None:
                taken[g] = p
        undecided -= set(decided)
        rounds += 1
    pred_match, gt_match = np.full((N,), -1, np.int32), np.full((M,), -1, np.int32)
    pred_state, pred_iou = np.zeros((N,), np.uint8), np.zeros((N,), np.float64)
    for p, g in took.items():
        if g is None:
            pred_state[p] = IGNORED if covered[p] else FP
        else:
            pred_match[p], gt_match[g], pred_iou[p], pred_state[p] = g, p, of_pred[p][g], TP
    return pred_match, pred_state, gt_match, pred_iou, rounds


@attrs.define
class RankedPairs:
    """One image of ``ranked_pairs``: what the matching at every threshold starts from."""
    part: np.ndarray      # (N,) bool: the preds that take part
    covered: np.ndarray   # (N,) uint8
    edges: list           # (g, p, iou): the care pairs with iou >= iou_thrs[0], gt-major ascending
    ious: np.ndarray      # the iou of every care box pair
    cover_margin: float   # the least |inter2 - cover_thr * area2_p| / area2_p over the don't-care pairs (inf without one)
    n_gt: int
    n_dc: int
    pairs: int
    dc_pairs: int


def ranked_pairs(gt_rows, gt_count, gt_care, pred_rows, pred_count, probs, iou_thrs, cover_thr: float = 0.5
                 ) -> List[RankedPairs]:
    """The clip of every box pair, once: per image the preds that take part, the coverage and the care candidates.  Both
    oracles take its result as ``pairs=`` so that a test computes it once."""
    (gt_rows, gt_count, pred_rows, pred_count, gt_care, probs), B, M, N = host_tables(gt_rows, gt_count, pred_rows, pred_count,
                                                                                      gt_care, probs)
    thrs, cover_thr = check_thresholds(iou_thrs, cover_thr)
    out = []
    for b in range(B):
        ng, npred = clamped(gt_count[b], M), clamped(pred_count[b], N)
        g, care = gt_rows[b, :ng], gt_care[b, :ng] != 0
        part = np.zeros((N,), dtype=bool)
        part[:npred] = (pred_rows[b, :npred, ROW_VALID] != 0) & np.isfinite(probs[b, :npred])
        p = pred_rows[b, :npred].copy()
        p[~part[:npred], ROW_VALID] = 0  # a pred without a finite prob takes no part: before the box pairs
        pairs, cover, margin, dc_pairs = care_pairs(g, p, care, cover_thr)
        covered = np.zeros((N,), np.uint8)
        covered[:npred] = cover
        valid_g = g[:, ROW_VALID] != 0
        out.append(RankedPairs(part, covered, [(a, c, iou) for a, c, _, iou in pairs if iou >= thrs[0]],
                               np.array([iou for _, _, _, iou in pairs], np.float64), margin, int((valid_g & care).sum()),
                               int((valid_g & ~care).sum()), len(pairs), dc_pairs))
    return out


def _ranked_host(matching, with_rounds, gt_rows, gt_count, gt_care, pred_rows, pred_count, probs, iou_thrs, cover_thr, pairs):
    (gt_rows, gt_count, pred_rows, pred_count, gt_care, probs), B, M, N = host_tables(gt_rows, gt_count, pred_rows, pred_count,
                                                                                      gt_care, probs)
    thrs, cover_thr = check_thresholds(iou_thrs, cover_thr)
    if pairs is None:
        pairs = ranked_pairs(gt_rows, gt_count, gt_care, pred_rows, pred_count, probs, thrs, cover_thr)
    T = len(thrs)
    pred_match, gt_match = np.full((B, T, N), -1, np.int32), np.full((B, T, M), -1, np.int32)
    pred_state, pred_iou = np.zeros((B, T, N), np.uint8), np.zeros((B, T, N), np.float64)
    covered, stats, dc_stats = np.zeros((B, N), np.uint8), np.zeros((B, T, 8), np.int64), np.zeros((B, 3), np.int64)
    rounds = np.zeros((B, T), np.int32)
    for b, im in enumerate(pairs):
        covered[b] = im.covered
        dc_stats[b] = (im.n_dc, im.dc_pairs, int(im.covered.sum()))
        for t, thr in enumerate(thrs):
            got = matching(im.part, probs[b], im.covered, im.edges, M, thr)
            pred_match[b, t], pred_state[b, t], gt_match[b, t], pred_iou[b, t] = got[:4]
            if with_rounds:
                rounds[b, t] = got[4]
            st = pred_state[b, t]
            stats[b, t] = (int((st == TP).sum()), int((st == FP).sum()), int((st == IGNORED).sum()), im.n_gt,
                           int(im.part.sum()), im.pairs, sum(1 for e in im.edges if e[2] >= thr), 0)
    outs = (pred_match, pred_state, gt_match, pred_iou, covered, stats, dc_stats)
    return outs + (rounds,) if with_rounds else outs


def match_quads_ranked_host(gt_rows, gt_count, gt_care, pred_rows, pred_count, probs, iou_thrs, cover_thr: float = 0.5,
                            pairs: Optional[List[RankedPairs]] = None):
    """The oracle of ``ops.match_quads_ranked`` in the sorted sequential form -> ``(pred_match (B, T, N) int32, pred_state
    (B, T, N) uint8, gt_match (B, T, M) int32, pred_iou (B, T, N) float64, covered (B, N) uint8, stats (B, T, 8) int64,
    dc_stats (B, 3) int64)``; status is always 0 here: the host has no capacity.  ``gt_care=None``: every gt is a care gt.
    Every field of a row is used as it is, as on the device."""
    return _ranked_host(ranked_matching, False, gt_rows, gt_count, gt_care, pred_rows, pred_count, probs, iou_thrs, cover_thr,
                        pairs)


def match_quads_ranked_rounds_host(gt_rows, gt_count, gt_care, pred_rows, pred_count, probs, iou_thrs,
                                   cover_thr: float = 0.5, pairs: Optional[List[RankedPairs]] = None):
    """The same through the rounds restatement, with ``rounds (B, T)`` int32 as an eighth result."""
    return _ranked_host(ranked_matching_rounds, True, gt_rows, gt_count, gt_care, pred_rows, pred_count, probs, iou_thrs,
                        cover_thr, pairs)


# ---- the curve ---------------------------------------------------------------------------------------------------------

@attrs.define
class OperatingPoint:
    score_thr: float
    precision: float
    recall: float
    f1: float


@attrs.define
class PRCurve:
    """One threshold: the TP / FP preds of a batch in rank order."""
    ap: float
    n_gt: int
    probs: np.ndarray      # (K,) float32, descending
    tp: np.ndarray         # (K,) int64, cumulative
    fp: np.ndarray         # (K,) int64, cumulative
    precision: np.ndarray  # (K,) float64: tp_k / k
    recall: np.ndarray     # (K,) float64: tp_k / n_gt
    best: OperatingPoint


def average_precision_host(states, probs, n_gt: int) -> PRCurve:
    """``states`` and ``probs``: one (n,) array per image (or one array: a single image) of the states at ONE threshold and
    the float32 probs; ``n_gt``: the care gts of the batch -> the curve, AP and the best operating point of the rule."""
    if isinstance(states, np.ndarray) and states.ndim == 1:
        states, probs = [states], [probs]
    n_gt = int(n_gt)
    if n_gt < 0 or len(states) != len(probs):
        raise ValueError('average_precision_host: n_gt >= 0 and one probs array per states array')
    pr, im, ix, hit = [], [], [], []
    for img, (s, p) in enumerate(zip(states, probs)):
        s, p = np.asarray(s).reshape(-1), np.asarray(p, dtype=np.float32).reshape(-1)
        if len(s) != len(p):
            raise ValueError('average_precision_host: states and probs of an image must pair up')
        k = np.flatnonzero((s == TP) | (s == FP))
        if not np.isfinite(p[k]).all():
            raise ValueError('average_precision_host: a TP or FP pred without a finite prob')
        pr.append(p[k])
        im.append(np.full(len(k), img, np.int64))
        ix.append(k.astype(np.int64))
        hit.append((s[k] == TP).astype(np.int64))
    cat = lambda parts, dtype: np.concatenate(parts) if parts else np.zeros((0,), dtype)
    pr, im, ix, hit = cat(pr, np.float32), cat(im, np.int64), cat(ix, np.int64), cat(hit, np.int64)
    order = np.lexsort((ix, im, -pr))  # prob descending (-0 equals +0), then image, then index
    pr, hit = pr[order], hit[order]
    K = len(pr)
    if int(hit.sum()) > n_gt:
        raise ValueError(f'average_precision_host: {int(hit.sum())} TP preds for n_gt = {n_gt}')
    ks = np.arange(1, K + 1, dtype=np.int64)
    tp = np.cumsum(hit, dtype=np.int64)
    fp = ks - tp
    # integers below 2^53: exact in binary64, so each quotient is the one correctly rounded division of the rule
    precision = tp.astype(np.float64) / ks.astype(np.float64)
    recall = tp.astype(np.float64) / float(n_gt) if n_gt else np.zeros((K,), np.float64)
    interpolated = np.maximum.accumulate(precision[::-1])[::-1]
    ap = math.fsum(interpolated[hit != 0].tolist()) / n_gt if n_gt else 0.0
    best = OperatingPoint(math.inf, 0.0, 0.0, 0.0)
    if K:
        cut = np.r_[pr[1:] < pr[:-1], True]  # a threshold cannot split equal probs
        f1 = (2 * tp).astype(np.float64) / (ks + n_gt).astype(np.float64)
        k = int(np.argmax(np.where(cut, f1, -1.0)))  # the first maximum
        best = OperatingPoint(float(pr[k]) + 0.0, float(precision[k]), float(recall[k]), float(f1[k]))
    return PRCurve(ap, n_gt, pr, tp, fp, precision, recall, best)


@attrs.define
class RankedScore:
    """Average precision over a batch: per threshold the counts, AP, curve and best operating point; ``map`` their mean."""
    iou_thrs: Tuple[float, ...]
    ap: np.ndarray       # (T,) float64
    map: float
    tp: np.ndarray       # (T,) int64
    fp: np.ndarray
    ignored: np.ndarray
    n_gt: int
    curves: List[PRCurve]

    @property
    def best(self) -> List[OperatingPoint]:
        return [c.best for c in self.curves]


@attrs.define
class RankedMatchResult:
    """One image of ``evaluate_quads_ranked``; indices are those of the image's own ``gt`` / ``pred`` arrays."""
    pred_state: np.ndarray  # (T, n) uint8: 0 ABSENT, 1 TP, 2 FP, 3 IGNORED
    pred_match: np.ndarray  # (T, n) int32: the gt index, or -1
    gt_match: np.ndarray    # (T, m) int32: the pred index, or -1
    pred_iou: np.ndarray    # (T, n) float64, 0 unless TP
    covered: np.ndarray     # (n,) bool
    gt_valid: np.ndarray    # (m,) bool: the rule's validity
    gt_care: np.ndarray     # (m,) bool
    pred_valid: np.ndarray  # (n,) bool: takes part (valid, finite prob)
    stats: np.ndarray       # (T, 8) int64
    dc_stats: np.ndarray    # (3,) int64


def ranked_score(outs, pred_count, probs, iou_thrs) -> RankedScore:
    """The outputs of the op or of an oracle, the counts and the (B, N) probs -> the batch's ``RankedScore``."""
    pred_state, stats = np.asarray(outs[1]), np.asarray(outs[5])
    B, T = pred_state.shape[0], len(iou_thrs)
    n_gt = int(stats[:, 0, 3].sum()) if B else 0
    curves = [average_precision_host([pred_state[b, t, :pred_count[b]] for b in range(B)],
                                     [probs[b, :pred_count[b]] for b in range(B)], n_gt) for t in range(T)]
    ap = np.array([c.ap for c in curves], np.float64)
    total = stats.sum(axis=0) if B else np.zeros((T, 8), np.int64)
    return RankedScore(tuple(iou_thrs), ap, math.fsum(ap.tolist()) / T, total[:, 0].copy(), total[:, 1].copy(),
                       total[:, 2].copy(), n_gt, curves)


def _ranked_results(tables, gt_valid, pred_valid, outs, iou_thrs) -> Tuple[List[RankedMatchResult], RankedScore]:
    _, gt_count, care, _, pred_count, probs = tables
    pred_match, pred_state, gt_match, pred_iou, covered, stats, dc_stats = (np.asarray(o) for o in outs[:7])
    results = []
    for b in range(len(gt_count)):
        m, n = int(gt_count[b]), int(pred_count[b])
        results.append(RankedMatchResult(pred_state[b, :, :n].copy(), pred_match[b, :, :n].copy(), gt_match[b, :, :m].copy(),
                                         pred_iou[b, :, :n].copy(), covered[b, :n] != 0, gt_valid[b, :m].copy(),
                                         care[b, :m] != 0, pred_valid[b, :n].copy(), stats[b].copy(), dc_stats[b].copy()))
    return results, ranked_score(outs, pred_count, probs, iou_thrs)


def evaluate_quads_ranked_host(pred: Sequence, gt: Sequence, pred_scores: Sequence, gt_care: Optional[Sequence] = None,
                               iou_thrs=DEFAULT_IOU_THRS, cover_thr: float = 0.5):
    """What ``evaluate_quads_ranked`` returns, through ``match_rows`` and ``match_quads_ranked_host``: the slow route, for
    checks and for timing against."""
    thrs, cover_thr = check_thresholds(iou_thrs, cover_thr)
    tables = padded_sides(pred, gt, gt_care, pred_scores)
    h_gt, gt_count, care, h_pred, pred_count, probs = tables
    gt_rows, pred_rows = quad_rows_host(h_gt), quad_rows_host(h_pred)
    outs = match_quads_ranked_host(gt_rows, gt_count, care, pred_rows, pred_count, probs, thrs, cover_thr)
    return _ranked_results(tables, gt_rows[:, :, ROW_VALID] != 0, (pred_rows[:, :, ROW_VALID] != 0) & np.isfinite(probs), outs,
                           thrs)


def evaluate_quads_ranked(pred: Sequence, gt: Sequence, pred_scores: Sequence, gt_care: Optional[Sequence] = None,
                          iou_thrs=DEFAULT_IOU_THRS, cover_thr: float = 0.5, device='cuda'):
    """Average precision of predicted character quads against annotated ones on the device.  ``pred``, ``gt`` and
    ``pred_scores`` are lists with one (n, 4, 2) ``(y, x)`` array, one (m, 4, 2) array and one (n,) array per image;
    ``gt_care`` a list of (m,) arrays, 0 = don't care, or None.  The padded quads, scores, care flags and counts go up once,
    both row tables are built on the device (``ops.quad_rows``), ``ops.match_quads_ranked`` is called once and the results
    are read back; if an image reports ``status`` the call is repeated once with the reported candidate count as capacity.
    Returns ``(per-image RankedMatchResult list, RankedScore over the batch)``."""
    from .. import ops
    device = require_gpu('evaluate_quads_ranked', device, 'evaluate_quads_ranked_host')
    thrs, cover_thr = check_thresholds(iou_thrs, cover_thr)
    tables = padded_sides(pred, gt, gt_care, pred_scores)
    if len(tables[1]) == 0:
        return [], ranked_score((None, np.zeros((0, len(thrs), 1), np.uint8), None, None, None,
                                 np.zeros((0, len(thrs), 8), np.int64)), tables[4], tables[5], thrs)
    d_gt, d_gt_count, d_care, d_pred, d_pred_count, d_probs = (torch.from_numpy(t).to(device, non_blocking=True)
                                                               for t in tables)
    d_gt_rows, d_pred_rows = ops.quad_rows(d_gt), ops.quad_rows(d_pred)
    call = lambda cap: ops.match_quads_ranked(d_gt_rows, d_gt_count, d_care, d_pred_rows, d_pred_count, d_probs, thrs,
                                              cover_thr, max_pairs=cap)
    outs, _ = with_capacity('evaluate_quads_ranked', call, lambda o: o[5].cpu().numpy(), np.s_[:, 0, 7], np.s_[:, 0, 6])
    gt_valid = (d_gt_rows[:, :, ROW_VALID] != 0).cpu().numpy()
    pred_valid = (d_pred_rows[:, :, ROW_VALID] != 0).cpu().numpy() & np.isfinite(tables[5])
    return _ranked_results(tables, gt_valid, pred_valid, [o.cpu().numpy() for o in outs], thrs)
