"""Suppression of duplicate character quadrilaterals by IoU: the rule, its host oracle, the device route and the filter
that ``infer`` / ``infer_batch`` apply to a result.

The rule is THIS PROJECT'S OWN, stated on the match rows and the pair IoU of inferencing/evaluation.py so that the device
kernels (csrc/quadmatch.hip) and the host oracle are held to each other for equality.

Inputs, per image: K match rows (``match_rows``: 16 int32 each), ``count``, float32 ``probs`` (K,), ``iou_thr`` in (0, 1] as
binary64.  ``count`` is clamped to [0, K].  A row TAKES PART iff it lies within the count, its ``valid`` word is set and its
prob is finite.  Every other row within the count passes through as kept: it neither suppresses nor is suppressed, and
nothing is repaired.

Rank: j OUTRANKS i iff ``probs[j] > probs[i]``, or ``probs[j] == probs[i]`` and ``j < i`` (float32 comparisons, so -0 equals
+0): a strict total order on the rows that take part.

Neighbours: j is a neighbour of i iff both take part, j outranks i, their Q4 boxes overlap (the inclusive test of
``box_pairs``) and ``quad_iou_host(rows[i], rows[j]) >= iou_thr`` - the row that is judged is the ``g`` argument and the
outranker the ``p`` argument: the clip is not symmetric to the last bit, so the order is part of the rule.

Result: the greedy one - going down the rank order, a quad is kept iff none of its neighbours was kept.  The same as a
fixpoint: an undecided quad becomes suppressed as soon as one neighbour is kept, and kept as soon as all its neighbours are
suppressed.  The top-ranked undecided quad has only decided neighbours, none of them kept (or it would be suppressed
already), so it can always be decided and the rounds end after at most n of them; a decision, once taken, is the greedy
one by induction down the ranks, so the fixpoint is unique.  ``nms_quads_host`` is the sorted sequential form; the device
runs the rounds, each reading the states the previous round left (tests/test_cpu_quad_nms.py holds the two forms to each
other on random graphs with exact prob ties).

Outputs, per image: ``keep`` (K,) uint8, 0 beyond the count; ``suppressor`` (K,) int32, the highest-ranked kept neighbour of
a suppressed quad and -1 otherwise; ``stats`` (6,) int64 = ``kept`` (rows with keep = 1), ``n`` (the clamped count),
``n_valid`` (the rows that take part), ``pairs`` (box-overlapping pairs of them with j outranking i), ``candidates`` (those
at or above ``iou_thr``), ``status``; ``rounds``: the rounds that decided at least one quad (a quad without neighbours is
decided in the first, so an image with a quad that takes part has at least one).

Differences from common practice: the IoU is asymmetric in the last bit and its argument order is fixed; the comparison is
``>=``, as in the matching, not ``>``; an invalid quad passes through instead of being dropped; the scope in ``infer`` is
the image, not the text region, because the duplicates come from two regions' boxes sharing a character as well as from two
peaks on one."""
from typing import List, Optional, Sequence, Tuple

import attrs
import numpy as np
import torch

from .evaluation import ROW_VALID, ROW_WORDS, check_iou_thr, fitting_quads, match_rows, quad_iou_host
from .quad_tables import clamped, host_table, pad_quads, pad_rows, pad_values, quad_lists, require_gpu, with_capacity


def nms_pairs(rows: np.ndarray, probs: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """One image, already cut to its count: ``(part (n,) bool, i, j)`` - the rows that take part and the box-overlapping pairs
    of them with j outranking i, i-major ascending."""
    r = np.asarray(rows, dtype=np.int64).reshape(-1, ROW_WORDS)
    p = np.asarray(probs, dtype=np.float32).reshape(-1)
    part = (r[:, ROW_VALID] != 0) & np.isfinite(p)
    if len(r) == 0:
        return part, np.zeros((0,), np.int64), np.zeros((0,), np.int64)
    idx = np.arange(len(r))
    with np.errstate(invalid='ignore'):
        outranks = (p[None, :] > p[:, None]) | ((p[None, :] == p[:, None]) & (idx[None, :] < idx[:, None]))  # [i, j]
    hit = ((r[:, None, 8] <= r[None, :, 10]) & (r[None, :, 8] <= r[:, None, 10]) &
           (r[:, None, 9] <= r[None, :, 11]) & (r[None, :, 9] <= r[:, None, 11]) &
           part[:, None] & part[None, :] & outranks)
    i, j = np.nonzero(hit)
    return part, i, j


def greedy_suppression(part: np.ndarray, probs: np.ndarray, edges) -> Tuple[np.ndarray, np.ndarray]:
    """``edges`` = (i, j) with j a neighbour of i -> ``(keep (n,) uint8, suppressor (n,) int32)`` by the sorted sequential
    rule; a row that takes no part is kept."""
    n = len(part)
    p = np.asarray(probs, dtype=np.float32)
    keep = np.ones((n,), dtype=np.uint8)
    suppressor = np.full((n,), -1, dtype=np.int32)
    nbrs: List[List[int]] = [[] for _ in range(n)]
    for i, j in edges:
        nbrs[i].append(j)
    order = sorted(np.flatnonzero(part).tolist(), key=lambda k: (-float(p[k]), k))  # -0.0 == 0.0: the index decides
    rank = {k: at for at, k in enumerate(order)}
    for i in order:
        kept = [j for j in nbrs[i] if keep[j]]  # every neighbour outranks i: decided already
        if kept:
            keep[i] = 0
            suppressor[i] = min(kept, key=rank.__getitem__)
    return keep, suppressor


def nms_quads_host(rows, count, probs, iou_thr: float = 0.5):
    """The oracle of ``ops.nms_quads``: ``rows`` (B, K, 16), ``count`` (B,), ``probs`` (B, K) -> ``(keep (B, K) uint8,
    suppressor (B, K) int32, stats (B, 6) int64)`` with ``stats`` = kept, n, n_valid, pairs, candidates, status (always 0
    here: the host has no capacity).  Every field of a row is used as it is, as on the device."""
    (rows, count, probs), B, K = host_table(rows, count, probs)
    thr = check_iou_thr(iou_thr)
    keep = np.zeros((B, K), dtype=np.uint8)
    suppressor = np.full((B, K), -1, dtype=np.int32)
    stats = np.zeros((B, 6), dtype=np.int64)
    for b in range(B):
        n = clamped(count[b], K)
        r, p = rows[b, :n], probs[b, :n]
        part, pi, pj = nms_pairs(r, p)
        edges = [(i, j) for i, j in zip(pi.tolist(), pj.tolist()) if quad_iou_host(r[i], r[j]) >= thr]
        keep[b, :n], suppressor[b, :n] = greedy_suppression(part, p, edges)
        stats[b] = (int(keep[b].sum()), n, int(part.sum()), len(pi), len(edges), 0)
    return keep, suppressor, stats


@attrs.define
class QuadNmsResult:
    """One image of ``nms_quads``; indices are those of the image's own arrays."""
    keep: np.ndarray        # (n,) bool
    suppressor: np.ndarray  # (n,) int32: the highest-ranked kept neighbour of a suppressed quad, or -1
    valid: np.ndarray       # (n,) bool: the rule's validity and the score threshold


def nms_tables(quads: Sequence, probs: Sequence, score_thr: Optional[float] = None):
    """The host half of ``nms_quads_lists_host`` (the device route builds its rows on the device): per-image arrays ->
    ``(rows (B, K, 16), count (B,), probs (B, K) float32, valid)`` with K the batch's largest count (at least 1)."""
    q, pr, present = _scored(quads, probs, score_thr)
    tabs = [match_rows(a, None if present is None else present[b]) for b, a in enumerate(q)]
    return (*pad_rows([r for r, _ in tabs]), pr, [v for _, v in tabs])


def _scored(quads: Sequence, probs: Sequence, score_thr: Optional[float]):
    """-> ``(quad lists, probs (B, K) float32, present)``: per image the quads at or above ``score_thr``, None without one"""
    q = quad_lists(quads)
    pr = pad_values(q, probs, np.float32, 'probs')
    # as in evaluation_tables: compared in binary64, NaN compares false
    present = None if score_thr is None else [pr[b, :len(a)].astype(np.float64) >= float(score_thr) for b, a in enumerate(q)]
    return q, pr, present


def _nms_results(counts, present, valid, keep, suppressor, stats):
    results = []
    for b, n in enumerate(int(c) for c in counts):
        k = keep[b, :n].astype(bool)
        if present is not None:  # below the score threshold: absent, not passed through
            k &= present[b]
        results.append(QuadNmsResult(k, suppressor[b, :n].copy(), np.asarray(valid[b], dtype=bool)))
    total = stats.sum(axis=0) if len(stats) else np.zeros((6,), np.int64)
    total[0] = sum(int(r.keep.sum()) for r in results)
    total[5] = int(stats[:, 5].max()) if len(stats) else 0
    return results, total


def nms_quads_lists_host(quads: Sequence, probs: Sequence, iou_thr: float = 0.5, score_thr: Optional[float] = None):
    """What ``nms_quads`` returns, through ``match_rows`` and ``nms_quads_host``: the slow route, for checks and for timing
    against."""
    rows, count, pr, valid = nms_tables(quads, probs, score_thr)
    return _nms_results(count, _scored(quads, probs, score_thr)[2], valid, *nms_quads_host(rows, count, pr, iou_thr))


def nms_quads(quads: Sequence, probs: Sequence, iou_thr: float = 0.5, score_thr: Optional[float] = None, device='cuda'):
    """Suppresses duplicate character quads on the device.  ``quads`` and ``probs`` are lists with one (n, 4, 2) ``(y, x)``
    array and one (n,) array per image.  With ``score_thr`` a quad whose prob is below it (or NaN) is absent: it takes no
    part and its ``keep`` is False.  Any other invalid quad passes through as kept.  The padded quads, probs and counts go
    up once, ``ops.quad_rows`` and ``ops.nms_quads`` are called once and the results are read back; if an image reports
    ``status`` the suppression is repeated once with the reported candidate count as capacity.  Returns ``(per-image
    QuadNmsResult list, stats (6,) int64 summed over the images: kept, n, n_valid, pairs, candidates, status)``."""
    from .. import ops
    device = require_gpu('nms_quads', device, 'nms_quads_lists_host')
    check_iou_thr(iou_thr)
    q, h_probs, present = _scored(quads, probs, score_thr)
    B = len(q)
    if B == 0:
        return [], np.zeros((6,), np.int64)
    h_quads, count = pad_quads(q)
    h_valid = pad_values(q, present, np.uint8, 'valid')
    d_quads, d_probs, d_valid, d_count = (torch.from_numpy(t).to(device, non_blocking=True)
                                          for t in (h_quads, h_probs, h_valid, count))
    d_rows = ops.quad_rows(d_quads, d_valid)
    outs, stats = with_capacity('nms_quads', lambda cap: ops.nms_quads(d_rows, d_count, d_probs, iou_thr=iou_thr, max_pairs=cap),
                                lambda o: o[2].cpu().numpy(), np.s_[:, 5], np.s_[:, 4])
    valid = (d_rows[:, :, ROW_VALID] != 0).cpu().numpy()
    return _nms_results(count, present, [valid[b, :count[b]] for b in range(B)], outs[0].cpu().numpy(),
                        outs[1].cpu().numpy(), stats)


def filter_result(result, keep):
    """An ``AdaptiveScalingInferencingResult`` and a keep mask over its characters in ``result_quads`` order (the per-region
    lists flattened in region order) -> a copy whose per-region ``points`` / ``probs`` / ``polygons`` hold the survivors in
    their present order, with ``num_suppressed`` raised by the number dropped.  Nothing else changes."""
    keep = np.asarray(keep, dtype=bool).reshape(-1)
    sizes = [len(p) for p in result.probs]
    if len(keep) != sum(sizes):
        raise ValueError(f'filter_result: a keep mask of {len(keep)} for {sum(sizes)} characters')
    points, probs, polygons, at = [], [], [], 0
    for r, k in enumerate(sizes):
        sel = keep[at:at + k]
        at += k
        points.append(np.ascontiguousarray(np.asarray(result.points[r])[sel]))
        probs.append(np.asarray(result.probs[r])[sel])
        polygons.append(np.asarray(result.polygons[r])[sel])
    return attrs.evolve(result, points=points, probs=probs, polygons=polygons,
                        num_suppressed=int(result.num_suppressed) + int((~keep).sum()))


def suppress_results(results: Sequence, iou_thr: float, device='cuda') -> list:
    """The step of ``infer`` / ``infer_batch``: the characters of every result go through ONE ``nms_quads`` call, each image
    on its own; an image with more than ``MAX_QUADS`` characters is left as it is with ``nms_status = 2``."""
    tabs, fits = fitting_quads(results)
    out = [attrs.evolve(r, nms_status=2) for r in results]
    if any(len(tabs[i][0]) for i in fits):
        res, _ = nms_quads([tabs[i][0] for i in fits], [tabs[i][1] for i in fits], iou_thr, device=device)
        for i, r in zip(fits, res):
            out[i] = filter_result(results[i], r.keep)
    else:
        for i in fits:
            out[i] = results[i]
    return out
