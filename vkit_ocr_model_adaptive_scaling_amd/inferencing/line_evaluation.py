"""Detection quality of text lines: an area-based score with one-to-one matches, splits and merges - the rule, its host
oracles, and the device route.

Public OCR ground truth annotates words or lines, and a detector may find an annotated line as two words or two annotated
words as one line.  The one-to-one IoU matching of inferencing/evaluation.py and inferencing/ranking.py scores both as
misses.  The rule below, in the manner of Wolf and Jolion's DetEval, also accepts one-to-many "splits" and many-to-one
"merges".  It is THIS PROJECT'S OWN: no agreement with any published script's numbers is claimed.  It is stated on the match
rows and the clip of inferencing/evaluation.py; after the one clip of a pair everything is integer arithmetic, so that the
device kernels (csrc/linematch.hip) and the host oracles are held to each other for equality.

Inputs, per image: ``gt_rows`` (M, 16) and ``gt_count``; ``gt_care`` (M,) uint8, 0 = don't care (None: every annotation
counts); ``pred_rows`` (N, 16) and ``pred_count``.  Rows are match rows (``match_rows`` / ``ops.quad_rows``); counts are
clamped to [0, K].  A row TAKES PART iff it lies within the count and its ``valid`` word is set.  A gt that takes part is a
CARE gt iff its care byte is set and a DON'T-CARE gt otherwise.

Parameters: ``recall_thr`` and ``precision_thr``, floats in (0, 1], 0.8 and 0.4 by default, become the Q8 integers
``tr_q8 = rint(recall_thr * 256)`` and ``tp_q8`` likewise (half to even), which must lie in 1..256; ``cover_thr`` is
binary64 in (0, 1], 0.5 by default, the one of inferencing/ranking.py.  Anything else raises.

Pair quantity, for every pair whose Q4 boxes overlap (the inclusive test of ``box_pairs``, both rows taking part): ONE clip
in ``quad_iou_host``'s order of operations gives ``inter2`` after its clamp (``quad_inter2_host``).  Then
    I   = int64(floor(min(inter2, 2^41)))
    A_g = min(max(area2_g, 0), 2^41),   A_p likewise
and everything after this point is integer arithmetic on I, A_g and A_p: every sum is exact and independent of its order.
For rows of ``match_rows`` the two clamps change nothing (corners within +-2^19 give area2 <= 2^41 and inter2 <= area2);
they are what keeps the bounds whatever a table holds: a sum over at most 8192 partners stays <= 2^54 and times 256
<= 2^62, inside int64.

Pair tests:  rec_ok(g, p) <=> 256 I >= tr_q8 A_g;  prec_ok(g, p) <=> 256 I >= tp_q8 A_p.

Phase 0, don't care: pred p is IGNORED iff some don't-care gt g has ``inter2(g, p) >= cover_thr * area2_p`` (binary64, the
product rounded once, inclusive: the coverage test of inferencing/ranking.py bit for bit).  Don't-care gts and ignored preds
take no further part and count in neither ``n_gt`` nor ``n_pred``.  A pair of a care gt and a pred that is not ignored is a
CANDIDATE iff I > 0 and at least one of rec_ok, prec_ok holds; only candidates matter below.

Phase A, one to one: Q(g, p) <=> rec_ok and prec_ok.  (g, p) match one to one iff Q(g, p), row g holds exactly one Q and
column p holds exactly one Q.  No order is involved.

Phase B, splits (one annotation found as several detections): going over the still-free care gts g in ascending index,
S_g = the still-free preds p with prec_ok(g, p) (candidates, so I > 0).  The split is accepted iff |S_g| >= 2 and
``256 * sum_{p in S_g} I(g, p) >= tr_q8 * A_g``; then g becomes SPLIT and every p in S_g a SPLIT PART of g.  Overlapping
detections are SUMMED, not united: two copies of one detection would count twice, so suppress duplicates first
(inferencing/nms.py).

Phase C, merges (several annotations found as one detection), the transpose: going over the still-free preds p in
ascending index, M_p = the still-free care gts g with rec_ok(g, p); accepted iff |M_p| >= 2 and
``256 * sum_{g in M_p} I(g, p) >= tp_q8 * A_p``; then p becomes a MERGE and every g in M_p MERGED into p.

Phases B and C as rounds (the form the device runs; B is stated, C is its transpose): a round reads the state the previous
round left.  A free gt is READY iff its S_g over the currently free preds passes the acceptance test.  Every ready gt
offers itself to each pred of its S_g; a pred keeps the lowest offering gt; a ready gt takes its set iff it holds every pred
of it.  The rounds end when no gt is ready.  Why this equals the sequential form:
    * readiness can only be lost, never gained: free preds only leave, so sets and sums only shrink;
    * the lowest ready gt of a round holds every pred it offers to, so it takes its set: every round with a ready gt takes
      at least one gt and two preds;
    * when g takes S in round r, no lower gt ever takes a pred of S: a lower gt that is ready in round r and shares a pred
      with S would have kept g from holding it, and one that is not ready never will be.  No higher gt has taken, before
      round r, a pred that g's test would accept: g was ready in every earlier round (readiness is only lost), offered
      itself to that pred and is the lower of the two.  So S is the set of prec_ok preds that no lower gt takes: what the
      sequential rule gives g, by induction up the indices.  A gt the sequential rule accepts stays ready until it is the
      lowest ready one, for the same two reasons.
The number of rounds of each phase - the rounds in which some gt (pred) was ready - is part of the rule.  Independent
splits take one round; a chain g_0 < g_1 < ... in which g_i and g_(i+1) share a pred, every g_i passing without the pred it
loses, takes one round per gt.  Split rounds are at most min(M, floor(N / 2)), merge rounds at most min(N, floor(M / 2)); the
device caps its loops one above that.  ``match_lines_host`` is the sequential form and the definition;
``match_lines_rounds_host`` the rounds, written apart (tests/test_cpu_line_match.py holds them to each other on random
candidate graphs).

Outputs per image:
    gt_kind (M,) uint8      0 absent, 1 unmatched, 2 one-to-one, 3 split, 4 merged, 5 don't care
    gt_group (M,) int32     the pred for kinds 2 and 4, g itself for kind 3, else -1
    pred_kind (N,) uint8    0 absent, 1 unmatched, 2 one-to-one, 3 split part, 4 merge, 5 ignored
    pred_group (N,) int32   the gt for kinds 2 and 3, p itself for kind 4, else -1
    stats (16,) int64       n_gt (care gts), n_pred (preds taking part and not ignored), one_to_one, split_gt, split_pred,
                            merged_gt, merge_pred, n_dc, n_ignored, pairs (box-overlapping pairs of rows taking part,
                            don't-care gts included), candidates, status, rounds_split, rounds_merge, 0, 0

Capacity (the device only): at most ``max_pairs`` stored candidates per image, ``4 * max(M, N)`` by default.  An image with
more keeps its true counts and gets ``status = 1``; all its kinds stay at absent / unmatched / don't care / ignored, with no
match and both round counts 0: never a partial result.  ``evaluate_lines`` retries once with the reported count.

Score, on the host: ``LineScore`` accumulates the integer stats over a batch.  With ``split_credit`` = ``merge_credit`` =
0.8 by default (Wolf and Jolion's constant for fragmented matches; for merges this project's choice):
    recall    = (one_to_one + split_credit * split_gt + merge_credit * merged_gt) / n_gt
    precision = (one_to_one + split_credit * split_pred + merge_credit * merge_pred) / n_pred
    f1        = 2 * precision * recall / (precision + recall),          every 0 / 0 = 0.
The counts are in the stats, so a caller can apply any other credit.

Differences from DetEval / ICDAR practice: areas are those of convex quads on the Q4 grid, not of axis-aligned boxes or
pixel masks; the thresholds are Q8 integers; a split sums the parts' intersections instead of uniting them; phase A
requires a pair to be alone in its row AND its column among the pairs passing both tests, and the pairs it leaves go on to
phases B and C; splits are settled before merges, each in ascending index; a detection on a don't-care annotation is
ignored by coverage of its own area."""
from collections import Counter
from typing import List, Optional, Sequence, Tuple

import attrs
import numpy as np
import torch

from .evaluation import ROW_VALID, _area2, care_pairs, quad_rows_host
from .quad_tables import clamped, host_tables, padded_sides, require_gpu, with_capacity

ABSENT, UNMATCHED, ONE_TO_ONE, SPLIT, MERGE, APART = 0, 1, 2, 3, 4, 5  # SPLIT: a split gt / a split part; APART: 5
AREA_MAX = 1 << 41
STATS = 16
STAT_NAMES = ('n_gt', 'n_pred', 'one_to_one', 'split_gt', 'split_pred', 'merged_gt', 'merge_pred', 'n_dc', 'n_ignored',
              'pairs', 'candidates', 'status', 'rounds_split', 'rounds_merge')


def check_line_thresholds(recall_thr=0.8, precision_thr=0.4, cover_thr=0.5) -> Tuple[int, int, float]:
    """-> ``(tr_q8, tp_q8, cover_thr)``; raises on anything outside the rule."""
    out = []
    for name, v in (('recall_thr', recall_thr), ('precision_thr', precision_thr)):
        x = float(v)
        if not (x > 0.0 and x <= 1.0):
            raise ValueError(f'{name} must lie in (0, 1], got {v}')
        q = int(np.rint(x * 256.0))
        if not 1 <= q <= 256:
            raise ValueError(f'{name} = {v} becomes {q} in Q8, outside 1..256')
        out.append(q)
    c = float(cover_thr)
    if not (c > 0.0 and c <= 1.0):
        raise ValueError(f'cover_thr must lie in (0, 1], got {cover_thr}')
    return out[0], out[1], c


def clamp_area(a: int) -> int:
    return min(max(int(a), 0), AREA_MAX)


def inter_floor(inter2: float) -> int:
    """I of the rule: ``inter2`` is ``quad_inter2_host``'s, clamped at 0 already."""
    x = inter2 if inter2 < float(AREA_MAX) else float(AREA_MAX)
    return int(np.floor(x))


@attrs.define
class LinePairs:
    """One image of ``line_pairs``: what the phases start from."""
    gt_kind: np.ndarray    # (M,) uint8: ABSENT, UNMATCHED (a care gt) or APART (don't care)
    pred_kind: np.ndarray  # (N,) uint8: ABSENT, UNMATCHED or APART (ignored)
    area_g: List[int]      # (M,) the clamped areas
    area_p: List[int]      # (N,)
    edges: list            # (g, p, I, rec_ok, prec_ok): the candidates, gt-major ascending
    pairs: int
    care_pairs: list       # (g, p, I) of every care box pair, ignored preds included: what the margin checks of tests read
    cover_margin: float    # the least |inter2 - cover_thr * area2_p| / area2_p over the don't-care pairs (inf without one)


def line_pairs(gt_rows, gt_count, gt_care, pred_rows, pred_count, recall_thr=0.8, precision_thr=0.4, cover_thr=0.5
               ) -> List[LinePairs]:
    """The clip of every box pair, once: per image phase 0 and the candidates.  Both oracles take its result as ``pairs=``
    so that a test computes it once."""
    (gt_rows, gt_count, pred_rows, pred_count, gt_care, _), B, M, N = host_tables(gt_rows, gt_count, pred_rows, pred_count,
                                                                                  gt_care)
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
        pairs, covered, margin, dc_pairs = care_pairs(g, p, care, cover_thr)
        pred_kind[:npred][covered] = APART
        floors = [(a, c, inter_floor(inter2)) for a, c, inter2, _ in pairs]
        edges = []
        for a, c, I in floors:
            rec, prec = 256 * I >= tr * area_g[a], 256 * I >= tp * area_p[c]
            if pred_kind[c] == UNMATCHED and I > 0 and (rec or prec):
                edges.append((a, c, I, rec, prec))
        out.append(LinePairs(gt_kind, pred_kind, area_g, area_p, edges, len(pairs) + dc_pairs, floors, margin))
    return out


def line_matching(gt_kind0, pred_kind0, area_g, area_p, edges, tr_q8: int, tp_q8: int):
    """Phases A, B and C of one image by the sequential rule: the definition.  ``gt_kind0`` / ``pred_kind0``: the kinds
    phase 0 leaves; ``edges`` = (g, p, I, rec_ok, prec_ok) -> ``(gt_kind, gt_group, pred_kind, pred_group)``."""
    gk, pk = np.array(gt_kind0, np.uint8), np.array(pred_kind0, np.uint8)
    M, N = len(gk), len(pk)
    gg, pg = np.full((M,), -1, np.int32), np.full((N,), -1, np.int32)
    edges = [e for e in edges if gk[e[0]] == UNMATCHED and pk[e[1]] == UNMATCHED and e[2] > 0]
    q = [(g, p) for g, p, _, rec, prec in edges if rec and prec]
    row, col = np.zeros((M,), np.int64), np.zeros((N,), np.int64)
    for g, p in q:
        row[g] += 1
        col[p] += 1
    for g, p in q:
        if row[g] == 1 and col[p] == 1:
            gk[g], pk[p], gg[g], pg[p] = ONE_TO_ONE, ONE_TO_ONE, p, g
    of_gt = [[] for _ in range(M)]
    of_pred = [[] for _ in range(N)]
    for g, p, I, rec, prec in edges:
        if prec:
            of_gt[g].append((p, I))
        if rec:
            of_pred[p].append((g, I))
    for g in range(M):
        if gk[g] != UNMATCHED:
            continue
        S = [(p, I) for p, I in of_gt[g] if pk[p] == UNMATCHED]
        if len(S) >= 2 and 256 * sum(I for _, I in S) >= tr_q8 * area_g[g]:
            gk[g], gg[g] = SPLIT, g
            for p, _ in S:
                pk[p], pg[p] = SPLIT, g
    for p in range(N):
        if pk[p] != UNMATCHED:
            continue
        S = [(g, I) for g, I in of_pred[p] if gk[g] == UNMATCHED]
        if len(S) >= 2 and 256 * sum(I for _, I in S) >= tp_q8 * area_p[p]:
            pk[p], pg[p] = MERGE, p
            for g, _ in S:
                gk[g], gg[g] = MERGE, p
    return gk, gg, pk, pg


def _take_rounds(owners, sets_of, free_member, need):
    """The rounds of one phase, for either orientation.  ``owners``: the free owners (gts in phase B); ``sets_of[o]`` = (member,
    I) pairs; ``free_member``: the set of free members; ``need(o)`` the right side of the acceptance test.  -> ``({owner: [its
    members]}, rounds)``; ``free_member`` loses the taken members."""
    free_owner, taken, rounds = set(owners), {}, 0
    while True:
        ready = {}
        for o in free_owner:  # reads the state the previous round left
            S = [(m, I) for m, I in sets_of[o] if m in free_member]
            if len(S) >= 2 and 256 * sum(I for _, I in S) >= need(o):
                ready[o] = [m for m, _ in S]
        if not ready:
            return taken, rounds
        rounds += 1
        keeps = {}
        for o, S in ready.items():
            for m in S:
                keeps[m] = min(keeps.get(m, o), o)
        won = [o for o, S in ready.items() if all(keeps[m] == o for m in S)]
        assert min(ready) in won, 'the lowest ready owner always wins its round'
        for o in won:
            taken[o] = ready[o]
            free_owner.discard(o)
            free_member.difference_update(ready[o])


def line_matching_rounds(gt_kind0, pred_kind0, area_g, area_p, edges, tr_q8: int, tp_q8: int):
    """The same by the rule's rounds, written apart from ``line_matching`` -> its four arrays and ``(rounds_split,
    rounds_merge)``."""
    gk, pk = np.array(gt_kind0, np.uint8), np.array(pred_kind0, np.uint8)
    M, N = len(gk), len(pk)
    gg, pg = np.full((M,), -1, np.int32), np.full((N,), -1, np.int32)
    live = {(g, p): (I, rec, prec) for g, p, I, rec, prec in edges if gk[g] == UNMATCHED and pk[p] == UNMATCHED and I > 0}
    both = [k for k, (_, rec, prec) in live.items() if rec and prec]
    in_row, in_col = Counter(g for g, _ in both), Counter(p for _, p in both)
    for g, p in both:
        if in_row[g] == 1 and in_col[p] == 1:
            gk[g], pk[p], gg[g], pg[p] = ONE_TO_ONE, ONE_TO_ONE, p, g
    free_g = {g for g in range(M) if gk[g] == UNMATCHED}
    free_p = {p for p in range(N) if pk[p] == UNMATCHED}
    sets_g, sets_p = {g: [] for g in free_g}, {p: [] for p in free_p}
    for (g, p), (I, rec, prec) in live.items():
        if prec and g in sets_g:
            sets_g[g].append((p, I))
        if rec and p in sets_p:
            sets_p[p].append((g, I))
    took, rounds_split = _take_rounds(free_g, sets_g, free_p, lambda g: tr_q8 * area_g[g])
    for g, S in took.items():
        gk[g], gg[g] = SPLIT, g
        for p in S:
            pk[p], pg[p] = SPLIT, g
    free_g -= set(took)
    took, rounds_merge = _take_rounds(free_p, sets_p, free_g, lambda p: tp_q8 * area_p[p])
    for p, S in took.items():
        pk[p], pg[p] = MERGE, p
        for g in S:
            gk[g], gg[g] = MERGE, p
    return gk, gg, pk, pg, (rounds_split, rounds_merge)


def line_stats(pairs: LinePairs, gk, pk, rounds=(0, 0)) -> np.ndarray:
    st = np.zeros((STATS,), np.int64)
    g0, p0 = pairs.gt_kind, pairs.pred_kind
    st[:14] = (int((g0 == UNMATCHED).sum()), int((p0 == UNMATCHED).sum()), int((gk == ONE_TO_ONE).sum()),
               int((gk == SPLIT).sum()), int((pk == SPLIT).sum()), int((gk == MERGE).sum()), int((pk == MERGE).sum()),
               int((g0 == APART).sum()), int((p0 == APART).sum()), pairs.pairs, len(pairs.edges), 0, rounds[0], rounds[1])
    return st


def _lines_host(with_rounds, gt_rows, gt_count, gt_care, pred_rows, pred_count, recall_thr, precision_thr, cover_thr, pairs):
    (gt_rows, gt_count, pred_rows, pred_count, gt_care, _), B, M, N = host_tables(gt_rows, gt_count, pred_rows, pred_count,
                                                                                  gt_care)
    tr, tp, cover_thr = check_line_thresholds(recall_thr, precision_thr, cover_thr)
    if pairs is None:
        pairs = line_pairs(gt_rows, gt_count, gt_care, pred_rows, pred_count, recall_thr, precision_thr, cover_thr)
    gt_kind, gt_group = np.zeros((B, M), np.uint8), np.full((B, M), -1, np.int32)
    pred_kind, pred_group = np.zeros((B, N), np.uint8), np.full((B, N), -1, np.int32)
    stats, rounds = np.zeros((B, STATS), np.int64), np.zeros((B, 2), np.int32)
    for b, im in enumerate(pairs):
        args = (im.gt_kind, im.pred_kind, im.area_g, im.area_p, im.edges, tr, tp)
        if with_rounds:
            gt_kind[b], gt_group[b], pred_kind[b], pred_group[b], rounds[b] = line_matching_rounds(*args)
            r = rounds[b]
        else:  # the sequential rule has no rounds: their counts are the rounds form's, which the rule makes part of it
            gt_kind[b], gt_group[b], pred_kind[b], pred_group[b] = line_matching(*args)
            r = line_matching_rounds(*args)[4]
        stats[b] = line_stats(im, gt_kind[b], pred_kind[b], r)
    outs = (gt_kind, gt_group, pred_kind, pred_group, stats)
    return outs + (rounds,) if with_rounds else outs


def match_lines_host(gt_rows, gt_count, gt_care, pred_rows, pred_count, recall_thr=0.8, precision_thr=0.4, cover_thr=0.5,
                     pairs: Optional[List[LinePairs]] = None):
    """The oracle of ``ops.match_lines`` in the sequential form, the definition -> ``(gt_kind (B, M) uint8, gt_group (B, M)
    int32, pred_kind (B, N) uint8, pred_group (B, N) int32, stats (B, 16) int64)``; status is always 0 here: the host has no
    capacity.  The kinds and groups come from the sequential phases; the two round counts in ``stats`` from the rounds
    form, which alone defines them.  Every field of a row is used as it is, as on the device."""
    return _lines_host(False, gt_rows, gt_count, gt_care, pred_rows, pred_count, recall_thr, precision_thr, cover_thr, pairs)


def match_lines_rounds_host(gt_rows, gt_count, gt_care, pred_rows, pred_count, recall_thr=0.8, precision_thr=0.4,
                            cover_thr=0.5, pairs: Optional[List[LinePairs]] = None):
    """The same through the rounds restatement, with ``rounds (B, 2)`` int32 as a sixth result."""
    return _lines_host(True, gt_rows, gt_count, gt_care, pred_rows, pred_count, recall_thr, precision_thr, cover_thr, pairs)


# ---- the score -----------------------------------------------------------------------------------------------------------

@attrs.define
class LineScore:
    """The integer stats over a batch and the credited recall, precision and F1 of the rule; 0 / 0 is 0."""
    split_credit: float = 0.8
    merge_credit: float = 0.8
    n_gt: int = 0
    n_pred: int = 0
    one_to_one: int = 0
    split_gt: int = 0
    split_pred: int = 0
    merged_gt: int = 0
    merge_pred: int = 0
    n_dc: int = 0
    n_ignored: int = 0

    def add(self, stats) -> 'LineScore':
        st = [int(v) for v in np.asarray(stats).reshape(-1)[:9]]
        if len(st) != 9 or min(st) < 0 or st[2] + st[3] + st[5] > st[0] or st[2] + st[4] + st[6] > st[1]:
            raise ValueError(f'LineScore.add: not the stats of an image: {st}')
        for name, v in zip(STAT_NAMES[:9], st):
            setattr(self, name, getattr(self, name) + v)
        return self

    @property
    def recall(self) -> float:
        num = self.one_to_one + self.split_credit * self.split_gt + self.merge_credit * self.merged_gt
        return num / self.n_gt if self.n_gt else 0.0

    @property
    def precision(self) -> float:
        num = self.one_to_one + self.split_credit * self.split_pred + self.merge_credit * self.merge_pred
        return num / self.n_pred if self.n_pred else 0.0

    @property
    def f1(self) -> float:
        p, r = self.precision, self.recall
        return 2.0 * p * r / (p + r) if p + r > 0.0 else 0.0


@attrs.define
class LineMatchResult:
    """One image of ``evaluate_lines``; indices are those of the image's own ``gt`` / ``pred`` arrays."""
    gt_kind: np.ndarray     # (m,) uint8
    gt_group: np.ndarray    # (m,) int32
    pred_kind: np.ndarray   # (n,) uint8
    pred_group: np.ndarray  # (n,) int32
    stats: np.ndarray       # (16,) int64

    def stat(self, name: str) -> int:
        """a word of ``stats`` by its name in ``STAT_NAMES``"""
        return int(self.stats[STAT_NAMES.index(name)])


def _line_results(gt_count, pred_count, outs, split_credit, merge_credit) -> Tuple[List[LineMatchResult], LineScore]:
    gt_kind, gt_group, pred_kind, pred_group, stats = (np.asarray(o) for o in outs[:5])
    score, results = LineScore(float(split_credit), float(merge_credit)), []
    for b in range(len(gt_count)):
        m, n = int(gt_count[b]), int(pred_count[b])
        results.append(LineMatchResult(gt_kind[b, :m].copy(), gt_group[b, :m].copy(), pred_kind[b, :n].copy(),
                                       pred_group[b, :n].copy(), stats[b].copy()))
        score.add(stats[b])
    return results, score


def evaluate_lines_host(pred: Sequence, gt: Sequence, gt_care: Optional[Sequence] = None, recall_thr: float = 0.8,
                        precision_thr: float = 0.4, cover_thr: float = 0.5, split_credit: float = 0.8,
                        merge_credit: float = 0.8) -> Tuple[List[LineMatchResult], LineScore]:
    """What ``evaluate_lines`` returns, through ``match_rows`` and ``match_lines_host``: the slow route, for checks and for
    timing against."""
    check_line_thresholds(recall_thr, precision_thr, cover_thr)
    h_gt, gt_count, care, h_pred, pred_count = padded_sides(pred, gt, gt_care)
    outs = match_lines_host(quad_rows_host(h_gt), gt_count, care, quad_rows_host(h_pred), pred_count, recall_thr,
                            precision_thr, cover_thr)
    return _line_results(gt_count, pred_count, outs, split_credit, merge_credit)


def evaluate_lines(pred: Sequence, gt: Sequence, gt_care: Optional[Sequence] = None, recall_thr: float = 0.8,
                   precision_thr: float = 0.4, cover_thr: float = 0.5, split_credit: float = 0.8, merge_credit: float = 0.8,
                   device='cuda') -> Tuple[List[LineMatchResult], LineScore]:
    """Scores detected text lines against annotated ones on the device.  ``pred`` and ``gt`` are lists with one (n, 4, 2)
    ``(y, x)`` array per image - ``pred`` may be the ``line_polygons`` of ``infer`` / ``infer_batch`` results as they are;
    ``gt_care`` a list of (m,) arrays, 0 = don't care, or None.  The padded quads, care flags and counts go up once, both row
    tables are built on the device (``ops.quad_rows``, one call per side), ``ops.match_lines`` is called once and the results
    are read back; if an image reports ``status`` the call is repeated once with the reported candidate count as capacity.
    Returns ``(per-image LineMatchResult list, LineScore over the batch)``."""
    from .. import ops
    device = require_gpu('evaluate_lines', device, 'evaluate_lines_host')
    check_line_thresholds(recall_thr, precision_thr, cover_thr)
    tables = padded_sides(pred, gt, gt_care)
    if len(tables[1]) == 0:
        return [], LineScore(float(split_credit), float(merge_credit))
    d_gt, d_gt_count, d_care, d_pred, d_pred_count = (torch.from_numpy(t).to(device, non_blocking=True) for t in tables)
    d_gt_rows, d_pred_rows = ops.quad_rows(d_gt), ops.quad_rows(d_pred)
    call = lambda cap: ops.match_lines(d_gt_rows, d_gt_count, d_care, d_pred_rows, d_pred_count, recall_thr, precision_thr,
                                       cover_thr, max_pairs=cap)
    outs, stats = with_capacity('evaluate_lines', call, lambda o: o[4].cpu().numpy(), np.s_[:, 11], np.s_[:, 10])
    return _line_results(tables[1], tables[4], [o.cpu().numpy() for o in outs[:4]] + [stats], split_credit, merge_credit)
