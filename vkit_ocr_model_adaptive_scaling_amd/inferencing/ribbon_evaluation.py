"""Detection quality of curved text lines: a line is a RIBBON of quads, scored by the rule of inferencing/line_evaluation.py
with the intersection of two lines summed over their segments - the rule, its host oracles, and the device route.

``evaluate_lines`` takes one convex quad per line, which for an arched headline, a seal or a line of a warped page is a
chord rectangle that is mostly background, and two neighbouring arcs can overlap in their rectangles without sharing a
pixel.  The benchmarks that annotate curved text give an even number of vertices along the two long sides of a line, and
``infer`` with ``precise_line_strip_curved`` gives ``line_spines``: both are ribbons.  The rule below is THIS PROJECT'S OWN:
no agreement with any published script's numbers is claimed.  It is stated on the match rows and the clip of
inferencing/evaluation.py; after the clip of a segment pair everything is integer arithmetic, so the device kernels
(csrc/ribbonmatch.hip) and the host oracles are held to each other for equality.

The shape.  A ribbon is a (K, 2, 2) float64 array, 2 <= K <= 257: ``[k, 0]`` is the k-th point of the top rail, ``[k, 1]``
of the bottom rail, each ``(y, x)`` in image pixels.  Segment k, 0 <= k < K - 1, is the quad (T_k, T_(k+1), B_(k+1), B_k):
up-left, up-right, down-right, down-left, the corner order of ``match_rows``.  A ribbon of one segment is a quad.

1. Segment rows.  Every segment becomes a match row by ``match_rows``: corners ``rint(c * 16)``, the box, the exact integer
   area, the valid test.  A point shared by two segments rounds once, so neighbouring segments share their edge exactly.
2. Orientation.  ``turn`` = the sum over the segments of the signed integer shoelace sums of their Q4 corners, computed
   whether or not the segments are valid.  If ``turn < 0`` the two rails are exchanged before anything else: a mirrored
   line gives the mirrored ribbon, as the ``sgn`` of inferencing/spines.py does.
3. Validity.  A ribbon is valid iff every corner is finite and within +-2^19 in Q4 and every segment row is valid
   (strictly convex, clockwise with y down).  An invalid ribbon gets a zero ribbon row and no segments and is reported to
   the caller; nothing is repaired.  A caller's ``valid`` is and-ed in, as in ``match_rows``.
4. Ribbon row: 16 int32, read by the scan and the phases of the line score as a match row.
       0       seg_start, an index into the image's segment table
       1       seg_count, in 1..256
       2..7    zero
       8..11   the union of the segment boxes (y0, x0, y1, x1)
       12, 13  the sum of the segments' area2 as one int64 (low word first)
       14      valid
       15      zero
5. Pair quantity, for every pair of ribbons that both take part (within the clamped count, valid word set) and whose
   ribbon boxes overlap (the inclusive test of ``box_pairs``):
       I = min( sum_{i, j} I_seg(i, j), 2^41 )   over all segments i of the gt and j of the pred,
       I_seg = inter_floor(quad_inter2_host(gseg_i, pseg_j)[0])
   - the one clip of the two segment rows, its clamp, then the floor of the line score.  A segment pair whose boxes do not
   overlap contributes 0.  The sum is over integers, so its order does not matter, and it stays below 2^16 * 2^41.
   ``A_g`` and ``A_p`` are the line score's clamped areas, read from the ribbon rows.
6. Don't care.  A pred is IGNORED iff some don't-care gt has ``float(I) >= cover_thr * float(area2_p)``: the coverage test
   of inferencing/ranking.py with ``float(I)`` in place of ``inter2`` - binary64, the product rounded once, inclusive.
7. Everything after this is the line score's, word for word: ``rec_ok``, ``prec_ok``, candidates, phases A, B and C in both
   forms, the round counts, the outputs ``gt_kind``, ``gt_group``, ``pred_kind``, ``pred_group`` and ``stats (16,)``, capacity
   with ``status = 1``, ``LineScore`` and the credits.  The oracles here call ``line_matching``, ``line_matching_rounds`` and
   ``line_stats`` (through ``match_lines_host(pairs=...)``) on the ``LinePairs`` that ``ribbon_pairs`` builds.
8. What a table may hold.  The oracle and the device read the tables as they are.  A ribbon row with ``seg_count`` outside
   1..256, ``seg_start < 0`` or ``seg_start + seg_count > S`` has no segments: every I with it is 0; it still takes part as
   its valid word says.  A segment row whose valid word is 0 contributes 0.  Segment boxes and areas are believed as
   written.

What the rule does NOT do.  Segments of one ribbon are summed, not united: a bend tighter than half the line's height
makes a segment non-convex and the ribbon invalid, and a ribbon that overlaps itself counts the overlap twice.  I can fall
short of the true area by up to one Q4^2 unit per clipped segment pair (each floor).  With every ribbon of one segment
the rule is the line score's, except that the coverage test sees ``floor(inter2)``: tests stay clear of that gap by
``LinePairs.cover_margin``.

Tables: per image and side a ribbon table (B, M, 16) with counts (B,) and a segment table (B, S, 16), int32; M and N at
most 8192, a ribbon of 1..256 segments, S in 1..2^21, B at most 65535.  ``ribbon_tables`` builds both tables of a side on
the host."""
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .evaluation import COORD_MAX, ROW_AREA, ROW_BOX, ROW_VALID, _area2, box_pairs, match_rows, quad_inter2_host
from .line_evaluation import (ABSENT, APART, AREA_MAX, UNMATCHED, LineMatchResult, LinePairs, LineScore, _line_results,
                              check_line_thresholds, clamp_area, inter_floor, match_lines_host, match_lines_rounds_host)
from .quad_tables import MAX_QUADS, ROW_WORDS, capacity, clamped, host_tables, pad_values, require_gpu, with_capacity

KNOTS_MAX = 257               # points per rail
SEG_MAX = KNOTS_MAX - 1       # segments of a ribbon
SEG_TABLE_MAX = 1 << 21       # rows of an image's segment table
ROW_SEG_START, ROW_SEG_COUNT = 0, 1


# ---- builders ------------------------------------------------------------------------------------------------------------

def _checked(ribbon) -> np.ndarray:
    r = np.asarray(ribbon, dtype=np.float64)
    if r.ndim != 3 or r.shape[1:] != (2, 2):
        raise ValueError(f'a ribbon is (K, 2, 2), got {r.shape}')
    if not 2 <= len(r) <= KNOTS_MAX:
        raise ValueError(f'a ribbon has 2..{KNOTS_MAX} points per rail, got K = {len(r)}')
    return r


def polygon_ribbon(polygon) -> np.ndarray:
    """A (2K, 2) ``(y, x)`` outline in ring order - the first K vertices one long side, the last K the other long side
    backwards: the convention of the curved-text benchmarks and of ``spine_polygon`` - -> the (K, 2, 2) ribbon."""
    p = np.asarray(polygon, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f'an outline is (2K, 2), got {p.shape}')
    if len(p) < 4 or len(p) % 2:
        raise ValueError(f'an outline has an even number of vertices, at least 4; got {len(p)}')
    K = len(p) // 2
    return _checked(np.stack([p[:K], p[K:][::-1]], axis=1))


def spine_ribbon(spine) -> np.ndarray:
    """The (K, 2, 2) centres C and down vectors V of ``line_spines`` / ``SpineStrips.spine(k)`` -> the ribbon with the rails
    ``C - V/2`` and ``C + V/2``."""
    s = np.asarray(spine, dtype=np.float64)
    if s.ndim != 3 or s.shape[1:] != (2, 2):
        raise ValueError(f'a spine is (K, 2, 2), got {s.shape}')
    C, V = s[:, 0], s[:, 1]
    return _checked(np.stack([C - V / 2, C + V / 2], axis=1))


def quad_ribbon(quad) -> np.ndarray:
    """a (4, 2) quad, corners up-left, up-right, down-right, down-left -> the ribbon of one segment"""
    return polygon_ribbon(np.asarray(quad, dtype=np.float64).reshape(4, 2))


def result_ribbons(result) -> List[np.ndarray]:
    """One ribbon per line of an ``infer`` / ``infer_batch`` result: its spine's ribbon for a line that has a spine of 2..257
    knots, else its ``line_polygons`` quad as a ribbon of one segment (a (0, 2, 2) spine, a spine longer than a ribbon can
    be, or a result without ``line_spines``: the curved flag off)."""
    quads = np.asarray(result.line_polygons, dtype=np.float64).reshape(-1, 4, 2)
    spines = list(getattr(result, 'line_spines', None) or [])
    if spines and len(spines) != len(quads):
        raise ValueError(f'result_ribbons: {len(spines)} spines for {len(quads)} lines')
    out = []
    for k, q in enumerate(quads):
        s = np.asarray(spines[k], dtype=np.float64) if spines else np.zeros((0, 2, 2))
        out.append(spine_ribbon(s) if s.ndim == 3 and 2 <= len(s) <= KNOTS_MAX else quad_ribbon(q))
    return out


def ribbon_list(entries) -> List[np.ndarray]:
    """The lines of one image as ribbons: an (n, 4, 2) array of quads stands for n ribbons of one segment each; any other
    sequence holds one entry per line, a ribbon (K, 2, 2) or an outline (2K, 2), told apart by ``ndim``."""
    if isinstance(entries, np.ndarray) and entries.ndim == 3 and entries.shape[1:] == (4, 2):
        return [quad_ribbon(q) for q in entries]
    out = []
    for e in entries:
        a = np.asarray(e, dtype=np.float64)
        out.append(_checked(a) if a.ndim == 3 else polygon_ribbon(a))
    return out


# ---- rows and tables -----------------------------------------------------------------------------------------------------

def ribbon_rows(ribbon, valid: bool = True) -> Tuple[np.ndarray, np.ndarray, bool]:
    """Rules 1..4 for one ribbon -> ``(row (16,) int32 with seg_start = 0, segment rows (K - 1, 16) int32, ok)``; an invalid
    ribbon gives a zero row and a (0, 16) table."""
    r = _checked(ribbon)
    with np.errstate(all='ignore'):
        c16 = np.rint(r * 16.0)
        inside = bool((np.abs(c16) <= COORD_MAX).all())  # NaN and inf compare false
        ci = np.where(np.abs(c16) <= COORD_MAX, c16, 0.0).astype(np.int64)
    quads = lambda a: np.stack([a[:-1, 0], a[1:, 0], a[1:, 1], a[:-1, 1]], axis=1)  # (K - 1, 4, 2)
    qi = quads(ci)
    nxt = np.roll(qi, -1, axis=1)
    turn = int((qi[..., 1] * nxt[..., 0] - nxt[..., 1] * qi[..., 0]).sum())
    if turn < 0:
        r = r[:, ::-1]
    segs, seg_ok = match_rows(quads(r))
    ok = bool(valid) and inside and bool(seg_ok.all())
    row = np.zeros((ROW_WORDS,), np.int32)
    if not ok:
        return row, np.zeros((0, ROW_WORDS), np.int32), False
    row[ROW_SEG_COUNT] = len(segs)
    row[ROW_BOX:ROW_BOX + 2] = segs[:, ROW_BOX:ROW_BOX + 2].min(axis=0)
    row[ROW_BOX + 2:ROW_BOX + 4] = segs[:, ROW_BOX + 2:ROW_BOX + 4].max(axis=0)
    area2 = sum(_area2(s) for s in segs)
    row[ROW_AREA:ROW_AREA + 2] = np.array([area2], '<i8').view('<i4')
    row[ROW_VALID] = 1
    return row, segs, True


def ribbon_tables(lists: Sequence, valid: Optional[Sequence] = None):
    """Both tables of one side: ``lists[b]`` holds the lines of image b as ``ribbon_list`` takes them, ``valid[b]`` (n,) flags
    that are and-ed with the rule's test -> ``(rows (B, M, 16) int32, count (B,) int32, segs (B, S, 16) int32, invalid)`` with
    M and S the batch's largest counts (at least 1) and ``invalid`` the ``(image, index)`` pairs of the ribbons the rule
    (or the caller) calls invalid."""
    images = [ribbon_list(e) for e in lists]
    if valid is not None and (len(valid) != len(images) or any(len(np.asarray(v).reshape(-1)) != len(im)
                                                                 for v, im in zip(valid, images))):
        raise ValueError('ribbon_tables: valid must pair up with the ribbons image by image')
    if max([0] + [len(im) for im in images]) > MAX_QUADS:
        raise ValueError(f'at most {MAX_QUADS} ribbons per image and side')
    built = [[ribbon_rows(r, True if valid is None else bool(np.asarray(valid[b]).reshape(-1)[i])) for i, r in enumerate(im)]
             for b, im in enumerate(images)]
    S = max([1] + [sum(len(s) for _, s, _ in im) for im in built])
    if S > SEG_TABLE_MAX:
        raise ValueError(f'at most {SEG_TABLE_MAX} segments per image and side, got {S}')
    B, M = len(images), capacity(images)
    rows, count, segs = np.zeros((B, M, ROW_WORDS), np.int32), np.zeros((B,), np.int32), np.zeros((B, S, ROW_WORDS), np.int32)
    invalid = []
    for b, im in enumerate(built):
        count[b], at = len(im), 0
        for i, (row, s, ok) in enumerate(im):
            if not ok:
                invalid.append((b, i))
                continue
            rows[b, i] = row
            rows[b, i, ROW_SEG_START] = at
            segs[b, at:at + len(s)] = s
            at += len(s)
    return rows, count, segs, invalid


# ---- the pair quantity and the oracles -------------------------------------------------------------------------------------

def ribbon_segments(row, segs: np.ndarray) -> np.ndarray:
    """the segment rows of a ribbon row in its image's (S, 16) table: none for a run the table does not hold (rule 8)"""
    start, cnt = int(row[ROW_SEG_START]), int(row[ROW_SEG_COUNT])
    if not (1 <= cnt <= SEG_MAX and start >= 0 and start + cnt <= len(segs)):
        return segs[:0]
    return segs[start:start + cnt]


def ribbon_inter(g_row, g_segs, p_row, p_segs) -> int:
    """I of rule 5 for two ribbon rows and their images' segment tables, in Python integers."""
    g, p = ribbon_segments(g_row, g_segs), ribbon_segments(p_row, p_segs)
    gi, pi = box_pairs(g, p)  # box-overlapping pairs of segment rows whose valid words are set
    total = 0
    for a, c in zip(gi.tolist(), pi.tolist()):
        total += inter_floor(quad_inter2_host(g[a], p[c])[0])
    return min(total, AREA_MAX)


def _seg_table(name: str, segs, B: int) -> np.ndarray:
    segs = np.ascontiguousarray(segs, dtype=np.int32)
    if segs.ndim != 3 or segs.shape[0] != B or segs.shape[2] != ROW_WORDS or not 1 <= segs.shape[1] <= SEG_TABLE_MAX:
        raise ValueError(f'{name} must be ({B}, S, {ROW_WORDS}) with S in 1..{SEG_TABLE_MAX}, got {segs.shape}')
    return segs


def ribbon_pairs(gt_rows, gt_count, gt_care, gt_segs, pred_rows, pred_count, pred_segs, recall_thr=0.8, precision_thr=0.4,
                 cover_thr=0.5) -> List[LinePairs]:
    """Rules 5 and 6 for every box pair of ribbons, once: per image what the phases start from, in the form ``line_pairs``
    gives it.  ``cover_margin`` is the least ``|float(I) - cover_thr * area2_p| / area2_p`` over the don't-care pairs."""
    (gt_rows, gt_count, pred_rows, pred_count, gt_care, _), B, M, N = host_tables(gt_rows, gt_count, pred_rows, pred_count,
                                                                                  gt_care)
    gt_segs, pred_segs = _seg_table('gt_segs', gt_segs, B), _seg_table('pred_segs', pred_segs, B)
    tr, tp, cover_thr = check_line_thresholds(recall_thr, precision_thr, cover_thr)
    out = []
    for b in range(B):
        ng, npred = clamped(gt_count[b], M), clamped(pred_count[b], N)
        g, p = gt_rows[b, :ng], pred_rows[b, :npred]
        care = gt_care[b, :ng] != 0
        gt_kind, pred_kind = np.zeros((M,), np.uint8), np.zeros((N,), np.uint8)
        gt_kind[:ng] = np.where(g[:, ROW_VALID] != 0, np.where(care, UNMATCHED, APART), ABSENT)
        pred_kind[:npred] = np.where(p[:, ROW_VALID] != 0, UNMATCHED, ABSENT)
        area_g = [clamp_area(_area2(r)) for r in gt_rows[b]]
        area_p = [clamp_area(_area2(r)) for r in pred_rows[b]]
        gi, pi = box_pairs(g, p)
        floors, margin, dc_pairs = [], float('inf'), 0
        for a, c in zip(gi.tolist(), pi.tolist()):
            I = ribbon_inter(g[a], gt_segs[b], p[c], pred_segs[b])
            if care[a]:
                floors.append((a, c, I))
                continue
            dc_pairs += 1
            ap = float(_area2(p[c]))
            need = cover_thr * ap
            if float(I) >= need:
                pred_kind[c] = APART
            if ap > 0:
                margin = min(margin, abs(float(I) - need) / ap)
        edges = []
        for a, c, I in floors:
            rec, prec = 256 * I >= tr * area_g[a], 256 * I >= tp * area_p[c]
            if pred_kind[c] == UNMATCHED and I > 0 and (rec or prec):
                edges.append((a, c, I, rec, prec))
        out.append(LinePairs(gt_kind, pred_kind, area_g, area_p, edges, len(floors) + dc_pairs, floors, margin))
    return out


def match_ribbons_host(gt_rows, gt_count, gt_care, gt_segs, pred_rows, pred_count, pred_segs, recall_thr=0.8,
                       precision_thr=0.4, cover_thr=0.5, pairs: Optional[List[LinePairs]] = None):
    """The oracle of ``ops.match_ribbons`` in the sequential form, the definition -> what ``match_lines_host`` returns: the
    phases and the statistics are its own, run on the ``LinePairs`` of ``ribbon_pairs``."""
    if pairs is None:
        pairs = ribbon_pairs(gt_rows, gt_count, gt_care, gt_segs, pred_rows, pred_count, pred_segs, recall_thr, precision_thr,
                             cover_thr)
    return match_lines_host(gt_rows, gt_count, gt_care, pred_rows, pred_count, recall_thr, precision_thr, cover_thr, pairs=pairs)


def match_ribbons_rounds_host(gt_rows, gt_count, gt_care, gt_segs, pred_rows, pred_count, pred_segs, recall_thr=0.8,
                              precision_thr=0.4, cover_thr=0.5, pairs: Optional[List[LinePairs]] = None):
    """The same through the rounds form, with ``rounds (B, 2)`` int32 as a sixth result."""
    if pairs is None:
        pairs = ribbon_pairs(gt_rows, gt_count, gt_care, gt_segs, pred_rows, pred_count, pred_segs, recall_thr, precision_thr,
                             cover_thr)
    return match_lines_rounds_host(gt_rows, gt_count, gt_care, pred_rows, pred_count, recall_thr, precision_thr, cover_thr,
                                   pairs=pairs)


# ---- lists of lines -> the score -------------------------------------------------------------------------------------------

def evaluation_ribbon_tables(pred: Sequence, gt: Sequence, gt_care: Optional[Sequence] = None):
    """The host half of ``evaluate_ribbons`` -> ``(gt_rows, gt_count, gt_care (B, M) uint8, gt_segs, pred_rows, pred_count,
    pred_segs)``"""
    if len(pred) != len(gt):
        raise ValueError(f'{len(pred)} images of predictions against {len(gt)} of annotations')
    g_rows, g_count, g_segs, _ = ribbon_tables(gt)
    p_rows, p_count, p_segs, _ = ribbon_tables(pred)
    care = None if gt_care is None else [np.asarray(c).reshape(-1) != 0 for c in gt_care]
    lines = [np.zeros((int(n),), np.uint8) for n in g_count]
    return g_rows, g_count, pad_values(lines, care, np.uint8, 'gt_care'), g_segs, p_rows, p_count, p_segs


def evaluate_ribbons_host(pred: Sequence, gt: Sequence, gt_care: Optional[Sequence] = None, recall_thr: float = 0.8,
                          precision_thr: float = 0.4, cover_thr: float = 0.5, split_credit: float = 0.8,
                          merge_credit: float = 0.8) -> Tuple[List[LineMatchResult], LineScore]:
    """What ``evaluate_ribbons`` returns, through ``ribbon_tables`` and ``match_ribbons_host``: the slow route, for checks
    and for timing against."""
    check_line_thresholds(recall_thr, precision_thr, cover_thr)
    t = evaluation_ribbon_tables(pred, gt, gt_care)
    outs = match_ribbons_host(*t, recall_thr, precision_thr, cover_thr)
    return _line_results(t[1], t[5], outs, split_credit, merge_credit)


def evaluate_ribbons(pred: Sequence, gt: Sequence, gt_care: Optional[Sequence] = None, recall_thr: float = 0.8,
                     precision_thr: float = 0.4, cover_thr: float = 0.5, split_credit: float = 0.8, merge_credit: float = 0.8,
                     device='cuda') -> Tuple[List[LineMatchResult], LineScore]:
    """Scores detected text lines against annotated ones as ribbons on the device.  ``pred`` and ``gt`` hold one entry per
    image as ``ribbon_list`` takes it: a list of ribbons (K, 2, 2) and outlines (2K, 2) - ``result_ribbons`` of a result, the
    polygons of a curved-text annotation - or an (n, 4, 2) array of quads; ``gt_care`` a list of (m,) arrays, 0 = don't
    care, or None.  The tables are built on the host (``ribbon_tables``) and go up once, ``ops.match_ribbons`` is called once
    and the results are read back; if an image reports ``status`` the call is repeated once with the reported candidate
    count as capacity.  Returns ``(per-image LineMatchResult list, LineScore over the batch)``; an invalid ribbon is absent
    (kind 0)."""
    from .. import ops
    device = require_gpu('evaluate_ribbons', device, 'evaluate_ribbons_host')
    check_line_thresholds(recall_thr, precision_thr, cover_thr)
    t = evaluation_ribbon_tables(pred, gt, gt_care)
    if len(t[1]) == 0:
        return [], LineScore(float(split_credit), float(merge_credit))
    d = [torch.from_numpy(a).to(device, non_blocking=True) for a in t]
    call = lambda cap: ops.match_ribbons(*d, recall_thr, precision_thr, cover_thr, max_pairs=cap)
    outs, stats = with_capacity('evaluate_ribbons', call, lambda o: o[4].cpu().numpy(), np.s_[:, 11], np.s_[:, 10])
    return _line_results(t[1], t[5], [o.cpu().numpy() for o in outs[:4]] + [stats], split_credit, merge_credit)
