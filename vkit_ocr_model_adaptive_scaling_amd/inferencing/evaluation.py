"""Detection quality of character quadrilaterals: the rule, its host oracles, and the device route.

Neither the reference nor this project scored what ``infer`` reads off an image; the rule below is THIS PROJECT'S OWN.  It is
stated in integers and in IEEE binary64 without contraction, one rounding per operation in the order ``quad_iou_host``
writes them, so that the device kernels (csrc/quadmatch.hip) and the host oracles are held to each other.

A quadrilateral is ``(4, 2)`` ``(y, x)`` in image pixels, corners up-left, up-right, down-right, down-left (clockwise with y
down) - the order ``infer`` and ``ops.char_polygons`` emit.

A match row is 16 int32 (64 bytes, four 16-byte loads):
    0..7    the corners in Q4: ``rint(c * 16)`` (half to even)
    8..11   the inclusive Q4 box (y0, x0, y1, x1): the min and max of the Q4 corners
    12, 13  twice the area in Q4^2 as one int64 (low word first): the exact integer shoelace sum
            sum_k x_k * y_(k+1) - x_(k+1) * y_k, positive for a valid quad
    14      valid
    15      zero

A quad is valid iff its Q4 corners lie within +-2^19 and all four int64 cross products of successive edges are positive
(strictly convex, clockwise with y down): the test of ``dataset.quad_rows``.  A caller's ``valid`` is and-ed with it; this is
how a score threshold acts.  An invalid quad gets a zero row and is reported; nothing is clamped or repaired.

IoU of a valid pair (g, p) whose boxes overlap (inclusive test on the Q4 boxes; other pairs have iou = 0 and are never
clipped):
    * the origin is the integer minimum of the two boxes; the eight corners relative to it (int64 differences) become
      binary64.  For rows of ``match_rows`` their magnitudes stay below 2^21, so every edge function of an input corner is
      exact;
    * p is clipped against the four edges of g by Sutherland-Hodgman, edges in the order ul->ur, ur->dr, dr->dl, dl->ul, the
      vertices of the running polygon in ring order.  For the edge a -> b with e = b - a, a vertex v is inside iff
          d(v) = ex * (vy - ay) - ey * (vx - ax) >= 0                                    (inclusive)
      For successive vertices v, w: v is emitted when it is inside, then, when exactly one of v, w is inside, the crossing
          t = dv / (dv - dw),   (vy + t * (wy - vy),  vx + t * (wx - vx)).
      A polygon holds at most eight vertices: a ninth would be dropped (it cannot arise from two convex quads in exact
      arithmetic; the bound is what keeps the device's ring inside its slots);
    * inter2 = the shoelace sum  acc = acc + (x_k * y_(k+1) - x_(k+1) * y_k)  over the ring, from acc = 0, then
      ``inter2 = hi if inter2 > hi``, ``inter2 = 0 if inter2 < 0`` with hi = min(area2_g, area2_p);
    * den = (area2_g + area2_p) - inter2;  iou = inter2 / den  if den > 0  else 0.

Matching, per image: the candidate edges are the box-overlapping valid pairs with ``iou >= iou_thr`` (iou_thr in (0, 1],
binary64).  The matching is the greedy one under the strict total order (iou descending, gt index ascending, pred index
ascending): an edge is taken iff both its ends are free.  This equals repeated mutual-best rounds: in a round, g takes p iff
p is g's best free candidate (highest iou, then lowest p) and g is p's best free candidate (highest iou, then lowest g).
The first edge of the order among free ends is always mutual-best, so every round that has a free edge takes at least one
and the rounds end after at most min(M, N); an edge taken in a round is one the greedy order takes (no earlier edge of the
order shares an end with it among free ends), by induction over the rounds.  ``match_quads_host`` is the sorted greedy
form; the device runs the rounds, so the two are written differently (and tests/test_cpu_quad_match.py holds them to each
other on random graphs with exact ties).

Per image: ``gt_match`` (M,) int32 pred index or -1, ``pred_match`` (N,) int32, ``gt_iou`` (M,) float64 (0 where
unmatched), ``tp``, ``n_gt`` / ``n_pred`` (the valid rows within the count), ``pairs`` (box-overlapping valid pairs),
``candidates`` (those at or above iou_thr).  fp = n_pred - tp, fn = n_gt - tp.

Lists of per-image quads -> padded tables, the checker of the oracles' tables and the two ends of the device wrappers are
shared with the other routes over match rows: inferencing/quad_tables.py.

Average precision over the scores, several IoU thresholds at once and don't-care annotations: inferencing/ranking.py.

Text lines and words, scored with one-to-many splits and many-to-one merges: inferencing/line_evaluation.py."""
import math
from typing import List, Optional, Sequence, Tuple

import attrs
import numpy as np
import torch

from .quad_tables import (MAX_QUADS, ROW_WORDS, clamped, host_tables, pad_rows, quad_lists, require_gpu, with_capacity)

ROW_BOX, ROW_AREA, ROW_VALID = 8, 12, 14
COORD_MAX = 1 << 19
RING_MAX = 8


def match_rows(quads, valid=None) -> Tuple[np.ndarray, np.ndarray]:
    """``quads`` (n, 4, 2) -> ``(rows (n, 16) int32, valid (n,) bool)``; ``valid`` (n,) is and-ed with the rule's test."""
    q = np.asarray(quads, dtype=np.float64).reshape(-1, 4, 2)
    n = len(q)
    rows = np.zeros((n, ROW_WORDS), dtype=np.int32)
    if valid is None:
        ok = np.ones((n,), dtype=bool)
    else:
        ok = np.asarray(valid, dtype=bool).reshape(-1).copy()
        if len(ok) != n:
            raise ValueError(f'valid must be ({n},), got {ok.shape}')
    if n == 0:
        return rows, ok
    with np.errstate(all='ignore'):
        c16 = np.rint(q * 16.0)
        ok &= (np.abs(c16) <= COORD_MAX).all(axis=(1, 2))  # NaN and inf compare false
        ci = np.where(ok[:, None, None], c16, 0.0).astype(np.int64)
    e = np.roll(ci, -1, axis=1) - ci                       # ul->ur, ur->dr, dr->dl, dl->ul as (dy, dx)
    en = np.roll(e, -1, axis=1)
    ok &= (e[..., 1] * en[..., 0] - e[..., 0] * en[..., 1] > 0).all(axis=1)
    nxt = np.roll(ci, -1, axis=1)
    area2 = (ci[..., 1] * nxt[..., 0] - nxt[..., 1] * ci[..., 0]).sum(axis=1)
    rows[:, 0:8] = ci.reshape(n, 8)
    rows[:, ROW_BOX:ROW_BOX + 2] = ci.min(axis=1)
    rows[:, ROW_BOX + 2:ROW_BOX + 4] = ci.max(axis=1)
    rows[:, ROW_AREA:ROW_AREA + 2] = area2.astype('<i8').view('<i4').reshape(n, 2)
    rows[:, ROW_VALID] = 1
    rows[~ok] = 0
    return rows, ok


def quad_rows_host(quads: np.ndarray) -> np.ndarray:
    """``ops.quad_rows`` on the host: padded quads (B, K, 4, 2) -> (B, K, 16) int32 match rows"""
    B, K = quads.shape[:2]
    return match_rows(quads.reshape(-1, 4, 2))[0].reshape(B, K, ROW_WORDS)


def _area2(row: np.ndarray) -> int:
    return int(np.ascontiguousarray(row[ROW_AREA:ROW_AREA + 2], dtype='<i4').view('<i8')[0])


def _clip(ring: List[Tuple[float, float]], ay: float, ax: float, by: float, bx: float) -> List[Tuple[float, float]]:
    """One Sutherland-Hodgman step of the rule: ``ring`` against the edge a -> b; Python floats are IEEE binary64 and
    every line below is one rounded operation per operator."""
    ey = by - ay
    ex = bx - ax
    out: List[Tuple[float, float]] = []
    n = len(ring)
    d = []
    for vy, vx in ring:
        m0 = ex * (vy - ay)
        m1 = ey * (vx - ax)
        d.append(m0 - m1)
    for k in range(n):
        (vy, vx), (wy, wx) = ring[k], ring[(k + 1) % n]
        dv, dw = d[k], d[(k + 1) % n]
        if dv >= 0.0 and len(out) < RING_MAX:
            out.append((vy, vx))
        if (dv >= 0.0) != (dw >= 0.0) and len(out) < RING_MAX:
            t = dv / (dv - dw)
            sy = t * (wy - vy)
            sx = t * (wx - vx)
            out.append((vy + sy, vx + sx))
    return out


def quad_inter2_host(g_row, p_row) -> Tuple[float, float]:
    """The oracle of the pair quantities: two match rows (16 int32 each), both taken as valid -> ``(inter2, iou)``: twice the
    area of the intersection after the rule's clamp and the rule's binary64 IoU, from one clip (``(0.0, 0.0)`` when the rows'
    boxes do not overlap).  Everything is read from the rows as they are, as the device does."""
    g = [int(v) for v in np.asarray(g_row).reshape(ROW_WORDS)]
    p = [int(v) for v in np.asarray(p_row).reshape(ROW_WORDS)]
    if g[8] > p[10] or p[8] > g[10] or g[9] > p[11] or p[9] > g[11]:
        return 0.0, 0.0
    oy, ox = min(g[8], p[8]), min(g[9], p[9])
    gq = [(float(g[2 * k] - oy), float(g[2 * k + 1] - ox)) for k in range(4)]
    ring = [(float(p[2 * k] - oy), float(p[2 * k + 1] - ox)) for k in range(4)]
    for k in range(4):
        (ay, ax), (by, bx) = gq[k], gq[(k + 1) % 4]
        ring = _clip(ring, ay, ax, by, bx)
    acc = 0.0
    n = len(ring)
    for k in range(n):
        (y0, x0), (y1, x1) = ring[k], ring[(k + 1) % n]
        m0 = x0 * y1
        m1 = x1 * y0
        acc = acc + (m0 - m1)
    ag, ap = float(_area2(np.asarray(g_row))), float(_area2(np.asarray(p_row)))
    hi = ap if ap < ag else ag
    inter2 = acc
    if inter2 > hi:
        inter2 = hi
    if inter2 < 0.0:
        inter2 = 0.0
    den = (ag + ap) - inter2
    return inter2, (inter2 / den if den > 0.0 else 0.0)


def quad_iou_host(g_row, p_row) -> float:
    """The oracle of the pair IoU: the second result of ``quad_inter2_host``."""
    return quad_inter2_host(g_row, p_row)[1]


def box_pairs(gt_rows: np.ndarray, pred_rows: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The box-overlapping valid pairs of two (m, 16) / (n, 16) tables as ``(gi, pi)``, gt-major ascending."""
    g, p = np.asarray(gt_rows, dtype=np.int64), np.asarray(pred_rows, dtype=np.int64)
    if len(g) == 0 or len(p) == 0:
        return np.zeros((0,), np.int64), np.zeros((0,), np.int64)
    hit = ((g[:, None, 8] <= p[None, :, 10]) & (p[None, :, 8] <= g[:, None, 10]) &
           (g[:, None, 9] <= p[None, :, 11]) & (p[None, :, 9] <= g[:, None, 11]) &
           (g[:, None, ROW_VALID] != 0) & (p[None, :, ROW_VALID] != 0))
    return np.nonzero(hit)


def care_pairs(g: np.ndarray, p: np.ndarray, care: np.ndarray, cover_thr: float):
    """The don't-care pass over one image, every box pair clipped once: ``g`` (m, 16) and ``p`` (n, 16) cut to their counts,
    ``care`` (m,) bool, ``cover_thr`` binary64 -> ``(pairs, covered, cover_margin, dc_pairs)``.  ``pairs`` are the pairs of a
    care gt as ``(a, c, inter2, iou)``, gt-major ascending; ``covered`` (n,) bool marks the preds for which some don't-care gt
    has ``inter2 >= cover_thr * area2_p`` (the product rounded once, the comparison inclusive); ``cover_margin`` is the least
    ``|inter2 - cover_thr * area2_p| / area2_p`` over the ``dc_pairs`` pairs of a don't-care gt (inf without one)."""
    gi, pi = box_pairs(g, p)
    pairs, covered, margin, dc_pairs = [], np.zeros((len(p),), bool), math.inf, 0
    for a, c in zip(gi.tolist(), pi.tolist()):
        inter2, iou = quad_inter2_host(g[a], p[c])
        if care[a]:
            pairs.append((a, c, inter2, iou))
        else:
            dc_pairs += 1
            ap = float(_area2(p[c]))
            need = cover_thr * ap
            if inter2 >= need:
                covered[c] = True
            if ap > 0:
                margin = min(margin, abs(inter2 - need) / ap)
    return pairs, covered, margin, dc_pairs


def check_iou_thr(iou_thr, who: str = '') -> float:
    """an IoU threshold of the rule: binary64 in (0, 1]; ``who`` names the caller in the error"""
    thr = float(iou_thr)
    if not (thr > 0.0 and thr <= 1.0):
        raise ValueError(f'{who + ": " if who else ""}iou_thr must lie in (0, 1], got {iou_thr}')
    return thr


def greedy_matching(edges, M: int, N: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``edges`` = (g, p, iou) triples -> ``(gt_match (M,), pred_match (N,), gt_iou (M,))`` by the sorted greedy rule."""
    gt_match = np.full((M,), -1, dtype=np.int32)
    pred_match = np.full((N,), -1, dtype=np.int32)
    gt_iou = np.zeros((M,), dtype=np.float64)
    for g, p, w in sorted(edges, key=lambda e: (-e[2], e[0], e[1])):
        if gt_match[g] < 0 and pred_match[p] < 0:
            gt_match[g], pred_match[p], gt_iou[g] = p, g, w
    return gt_match, pred_match, gt_iou


def match_quads_host(gt_rows, gt_count, pred_rows, pred_count, iou_thr: float = 0.5):
    """The oracle of ``ops.match_quads``: ``gt_rows`` (B, M, 16) / ``gt_count`` (B,), ``pred_rows`` (B, N, 16) /
    ``pred_count`` (B,) -> ``(gt_match (B, M) int32, pred_match (B, N) int32, gt_iou (B, M) float64, stats (B, 6) int64)``
    with ``stats`` = tp, n_gt, n_pred, pairs, candidates, status (always 0 here: the host has no capacity).  As on the device
    the counts are clamped to [0, K], a row with ``valid == 0`` takes no part and every field of a row is used as it is."""
    (gt_rows, gt_count, pred_rows, pred_count, _, _), B, M, N = host_tables(gt_rows, gt_count, pred_rows, pred_count)
    thr = check_iou_thr(iou_thr)
    gt_match = np.full((B, M), -1, dtype=np.int32)
    pred_match = np.full((B, N), -1, dtype=np.int32)
    gt_iou = np.zeros((B, M), dtype=np.float64)
    stats = np.zeros((B, 6), dtype=np.int64)
    for b in range(B):
        g, p = gt_rows[b, :clamped(gt_count[b], M)], pred_rows[b, :clamped(pred_count[b], N)]
        gi, pi = box_pairs(g, p)
        edges = []
        for a, c in zip(gi.tolist(), pi.tolist()):
            w = quad_iou_host(g[a], p[c])
            if w >= thr:
                edges.append((a, c, w))
        gt_match[b], pred_match[b], gt_iou[b] = greedy_matching(edges, M, N)
        stats[b] = (int((gt_match[b] >= 0).sum()), int((g[:, ROW_VALID] != 0).sum()), int((p[:, ROW_VALID] != 0).sum()),
                    len(gi), len(edges), 0)
    return gt_match, pred_match, gt_iou, stats


@attrs.define
class DetectionScore:
    """tp / fp / fn over images and the sum of the matches' IoUs; 0 / 0 is 0."""
    tp: int = 0
    fp: int = 0
    fn: int = 0
    iou_sum: float = 0.0

    def add(self, tp: int, n_gt: int, n_pred: int, iou_sum: float = 0.0) -> 'DetectionScore':
        tp, n_gt, n_pred = int(tp), int(n_gt), int(n_pred)
        if tp < 0 or tp > n_gt or tp > n_pred:
            raise ValueError(f'tp = {tp} outside [0, min(n_gt = {n_gt}, n_pred = {n_pred})]')
        self.tp += tp
        self.fp += n_pred - tp
        self.fn += n_gt - tp
        self.iou_sum += float(iou_sum)
        return self

    @property
    def precision(self) -> float:
        return self.tp / (self.tp + self.fp) if self.tp + self.fp else 0.0

    @property
    def recall(self) -> float:
        return self.tp / (self.tp + self.fn) if self.tp + self.fn else 0.0

    @property
    def f1(self) -> float:
        return 2 * self.tp / (2 * self.tp + self.fp + self.fn) if 2 * self.tp + self.fp + self.fn else 0.0

    @property
    def mean_iou(self) -> float:
        return self.iou_sum / self.tp if self.tp else 0.0


@attrs.define
class QuadMatchResult:
    """One image of ``evaluate_quads``; indices are those of the image's own ``gt`` / ``pred`` arrays."""
    gt_match: np.ndarray    # (m,) int32: the pred index, or -1
    pred_match: np.ndarray  # (n,) int32: the gt index, or -1
    gt_iou: np.ndarray      # (m,) float64, 0 where unmatched
    gt_valid: np.ndarray    # (m,) bool: the rule's validity
    pred_valid: np.ndarray  # (n,) bool: the rule's validity and the score threshold
    tp: int
    n_gt: int
    n_pred: int
    pairs: int
    candidates: int


def result_quads(result) -> Tuple[np.ndarray, np.ndarray]:
    """An ``AdaptiveScalingInferencingResult`` (``infer``, or an entry of ``infer_batch().results``) -> ``(quads (n, 4, 2)
    float64, probs (n,) float32)``: its per-region lists flattened in region order."""
    polys = [np.asarray(p, dtype=np.float64).reshape(-1, 4, 2) for p in result.polygons]
    probs = [np.asarray(p, dtype=np.float32).reshape(-1) for p in result.probs]
    if len(polys) != len(probs) or any(len(a) != len(b) for a, b in zip(polys, probs)):
        raise ValueError('result_quads: polygons and probs of a result must pair up region by region')
    if not polys:
        return np.zeros((0, 4, 2), np.float64), np.zeros((0,), np.float32)
    return np.concatenate(polys, axis=0), np.concatenate(probs, axis=0)


def fitting_quads(results: Sequence) -> Tuple[list, List[int]]:
    """What the steps of ``infer`` / ``infer_batch`` over a result's characters start from: ``result_quads`` of every result,
    and the indices of those with at most ``MAX_QUADS`` characters (the others keep their step's status 2)."""
    tabs = [result_quads(r) for r in results]
    return tabs, [i for i, (q, _) in enumerate(tabs) if len(q) <= MAX_QUADS]


def evaluation_tables(pred: Sequence, gt: Sequence, pred_scores: Optional[Sequence] = None,
                      score_thr: Optional[float] = None):
    """The host half of ``evaluate_quads``: per-image quad arrays -> ``(gt_rows (B, M, 16), gt_count (B,), pred_rows
    (B, N, 16), pred_count (B,), gt_valid, pred_valid)`` with M, N the batch's largest counts (at least 1)."""
    pq, gq = quad_lists(pred, gt)
    if (pred_scores is None) != (score_thr is None):
        raise ValueError('pred_scores and score_thr go together')
    if pred_scores is not None and len(pred_scores) != len(pq):
        raise ValueError(f'pred_scores must have one entry per image, got {len(pred_scores)}')
    # compared in binary64: NaN compares false
    keep = [None if pred_scores is None else np.asarray(pred_scores[i], dtype=np.float64).reshape(-1) >= float(score_thr)
            for i in range(len(pq))]
    g_tabs, p_tabs = [match_rows(q) for q in gq], [match_rows(q, k) for q, k in zip(pq, keep)]
    return (*pad_rows([r for r, _ in g_tabs]), *pad_rows([r for r, _ in p_tabs]), [v for _, v in g_tabs],
            [v for _, v in p_tabs])


def _results(tables, outs, iou_dtype=np.float64) -> Tuple[List[QuadMatchResult], DetectionScore]:
    _, gt_count, _, pred_count, gt_valid, pred_valid = tables
    gt_match, pred_match, gt_iou, stats = outs
    score, results = DetectionScore(), []
    for b in range(len(gt_count)):
        m, n = int(gt_count[b]), int(pred_count[b])
        tp, n_gt, n_pred, pairs, cand, _ = (int(v) for v in stats[b])
        r = QuadMatchResult(gt_match[b, :m].copy(), pred_match[b, :n].copy(), gt_iou[b, :m].astype(iou_dtype), gt_valid[b],
                            pred_valid[b], tp, n_gt, n_pred, pairs, cand)
        score.add(tp, n_gt, n_pred, float(r.gt_iou.sum()))
        results.append(r)
    return results, score


def evaluate_quads_host(pred: Sequence, gt: Sequence, iou_thr: float = 0.5, pred_scores: Optional[Sequence] = None,
                        score_thr: Optional[float] = None) -> Tuple[List[QuadMatchResult], DetectionScore]:
    """What ``evaluate_quads`` returns, through ``match_quads_host``: the slow route, for checks and for timing against."""
    tables = evaluation_tables(pred, gt, pred_scores, score_thr)
    return _results(tables, match_quads_host(*tables[:4], iou_thr))


def evaluate_quads(pred: Sequence, gt: Sequence, iou_thr: float = 0.5, pred_scores: Optional[Sequence] = None,
                   score_thr: Optional[float] = None, device='cuda') -> Tuple[List[QuadMatchResult], DetectionScore]:
    """Scores predicted character quads against annotated ones on the device.  ``pred`` and ``gt`` are lists with one
    (n, 4, 2) ``(y, x)`` array per image; with ``pred_scores`` (one (n,) array per image) and ``score_thr`` a prediction below
    the threshold is invalid, i.e. absent.  The rows are built on the host and uploaded once, ``ops.match_quads`` is called
    once and the statistics are read back; if an image reports ``status`` the call is repeated once with the reported
    candidate count as capacity.  Returns ``(per-image QuadMatchResult list, DetectionScore over the batch)``."""
    from .. import ops
    device = require_gpu('evaluate_quads', device, 'evaluate_quads_host')
    check_iou_thr(iou_thr)
    tables = evaluation_tables(pred, gt, pred_scores, score_thr)
    if len(tables[1]) == 0:
        return [], DetectionScore()
    dev = [torch.from_numpy(t).to(device, non_blocking=True) for t in tables[:4]]
    outs, stats = with_capacity('evaluate_quads', lambda cap: ops.match_quads(*dev, iou_thr=iou_thr, max_pairs=cap),
                                lambda o: o[3].cpu().numpy(), np.s_[:, 5], np.s_[:, 4])
    return _results(tables, (outs[0].cpu().numpy(), outs[1].cpu().numpy(), outs[2].cpu().numpy(), stats))
