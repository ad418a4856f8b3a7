"""Shared inputs and restatements of the quad-matching tests (test_cpu_quad_match.py, test_gpu_quad_match.py,
test_gpu_quad_match_infer.py): an exact-arithmetic IoU over fractions.Fraction and a mutual-best-rounds matching, both
written apart from inferencing/evaluation.py; the hand cases; random quads; the seeded page."""
from fractions import Fraction
from functools import lru_cache

import numpy as np

from vkit_ocr_model_adaptive_scaling_amd.inferencing import evaluation as E

SQ = lambda y, x, h, w: [[y, x], [y, x + w], [y + h, x + w], [y + h, x]]  # up-left, up-right, down-right, down-left


def rotated(cy, cx, h, w, deg):
    t = np.deg2rad(deg)
    rot = np.array([[np.cos(t), np.sin(t)], [-np.sin(t), np.cos(t)]])  # (y, x): clockwise with y down stays clockwise
    base = np.array([[-h / 2, -w / 2], [-h / 2, w / 2], [h / 2, w / 2], [h / 2, -w / 2]])
    return base @ rot.T + np.array([cy, cx])


# ---- exact arithmetic ------------------------------------------------------------------------------------------------

def _corners(row):
    return [(Fraction(int(row[2 * k])), Fraction(int(row[2 * k + 1]))) for k in range(4)]


def _shoelace(ring):
    s = Fraction(0)
    for k in range(len(ring)):
        (y0, x0), (y1, x1) = ring[k], ring[(k + 1) % len(ring)]
        s += x0 * y1 - x1 * y0
    return s


def exact_inter2(g_row, p_row):
    """twice the area of the intersection of two convex clockwise quads (Q4 corners of the rows), exactly"""
    ring = _corners(p_row)
    gq = _corners(g_row)
    for k in range(4):
        (ay, ax), (by, bx) = gq[k], gq[(k + 1) % 4]
        side = lambda v: (bx - ax) * (v[0] - ay) - (by - ay) * (v[1] - ax)
        out = []
        for i in range(len(ring)):
            v, w = ring[i], ring[(i + 1) % len(ring)]
            dv, dw = side(v), side(w)
            if dv >= 0:
                out.append(v)
            if (dv >= 0) != (dw >= 0):
                t = dv / (dv - dw)
                out.append((v[0] + t * (w[0] - v[0]), v[1] + t * (w[1] - v[1])))
        ring = out
        if not ring:
            return Fraction(0)
    return _shoelace(ring)


def exact_iou(g_row, p_row):
    inter = exact_inter2(g_row, p_row)
    return inter / (_shoelace(_corners(g_row)) + _shoelace(_corners(p_row)) - inter)


# ---- matching, restated as rounds ------------------------------------------------------------------------------------

def mutual_best_rounds(edges, M, N):
    """``edges`` (g, p, w) -> (gt_match, pred_match, rounds that took an edge): in a round g takes p iff p is g's best free
    candidate (highest w, then lowest p) and g is p's best (highest w, then lowest g)"""
    gt_match, pred_match = np.full((M,), -1, np.int32), np.full((N,), -1, np.int32)
    rounds = 0
    while True:
        best_p, best_g = {}, {}
        for g, p, w in edges:
            if gt_match[g] >= 0 or pred_match[p] >= 0:
                continue
            if g not in best_p or (w, -p) > best_p[g]:
                best_p[g] = (w, -p)
            if p not in best_g or (w, -g) > best_g[p]:
                best_g[p] = (w, -g)
        took = [(g, -mp) for g, (w, mp) in best_p.items() if best_g[-mp] == (w, -g)]
        if not took:
            return gt_match, pred_match, rounds
        for g, p in took:
            gt_match[g], pred_match[p] = p, g
        rounds += 1


# ---- hand cases: name -> (gt quads, pred quads, expected IoU of pair (0, 0) as a Fraction or None) --------------------

def _turned_square():
    return rotated(8.0, 8.0, 8.0, 8.0, 45.0)


HAND = {
    'identical': ([SQ(3, 5, 4, 4)], [SQ(3, 5, 4, 4)], Fraction(1)),
    'disjoint': ([SQ(0, 0, 4, 4)], [SQ(0, 9, 4, 4)], Fraction(0)),
    'touching': ([SQ(0, 0, 4, 4)], [SQ(0, 4, 4, 4)], Fraction(0)),
    'half_inside': ([SQ(0, 0, 4, 4)], [SQ(0, 0, 2, 4)], Fraction(1, 2)),
    'diamond': ([SQ(0, 0, 4, 4)], [[[0, 2], [2, 4], [4, 2], [2, 0]]], Fraction(1, 2)),
    'diamond_gt': ([[[0, 2], [2, 4], [4, 2], [2, 0]]], [SQ(0, 0, 4, 4)], Fraction(1, 2)),
    'turned': ([SQ(4, 4, 8, 8)], [_turned_square()], None),
}


def hand_rows(name):
    g, p, want = HAND[name]
    return E.match_rows(np.array(g, dtype=np.float64))[0], E.match_rows(np.array(p, dtype=np.float64))[0], want


def tie_cases():
    """two identical preds on one gt; two identical gts with one pred"""
    a = np.array([SQ(0, 0, 8, 8)], dtype=np.float64)
    two = np.array([SQ(0, 1, 8, 8), SQ(0, 1, 8, 8)], dtype=np.float64)
    return {'two_preds': (a, two), 'two_gts': (two, a)}


def chain_case():
    """64 x 64 squares along x at offsets that shrink along the chain: IoU (64 - d) / (64 + d) rises from g0-p0 to p2-g3, every
    neighbour pair is above 0.5 and every other gt-pred pair far below.  Rounds take g3-p2, then g2-p1, then g1-p0."""
    gt = np.array([SQ(0, x, 64, 64) for x in (0, 41, 78, 111)], dtype=np.float64)
    pred = np.array([SQ(0, x, 64, 64) for x in (21, 60, 95)], dtype=np.float64)
    return gt, pred, np.array([-1, 0, 1, 2], np.int32), 3


# ---- random quads and the seeded page --------------------------------------------------------------------------------

def random_pair(rng):
    """a rotated quad of 4 to 60 px with its centre up to 3000 px away from the origin, and a jittered, shifted copy"""
    h, w = rng.uniform(4, 60, 2)
    cy, cx = rng.uniform(40, 3000, 2)
    g = rotated(cy, cx, h, w, rng.uniform(0, 360)) + rng.uniform(-0.1, 0.1, (4, 2)) * min(h, w)
    shift = rng.uniform(-0.6, 0.6, 2) * np.array([h, w])
    p = rotated(cy + shift[0], cx + shift[1], h * rng.uniform(0.7, 1.3), w * rng.uniform(0.7, 1.3), rng.uniform(0, 360))
    p = p + rng.uniform(-0.1, 0.1, (4, 2)) * min(h, w)
    return g, p


def random_tables(seed, B, M, N, counts_g=None, counts_p=None):
    """(B, M, 16) / (B, N, 16) tables of small rotated quads on a crowded 160 px square, so that boxes overlap often; two
    predictions in three are jittered copies of a gt of their image (in shuffled order), the others are unrelated"""
    rng = np.random.default_rng(seed)
    quad = lambda: rotated(*rng.uniform(10, 150, 2), *rng.uniform(6, 20, 2), rng.uniform(-25, 25))
    gq = np.stack([quad() for _ in range(B * M)]).reshape(B, M, 4, 2)
    pq = np.stack([quad() for _ in range(B * N)]).reshape(B, N, 4, 2)
    for b in range(B):
        src = rng.permutation(M)
        for k in range(min(M, N)):
            if rng.uniform() < 2 / 3:
                pq[b, k] = gq[b, src[k]] + rng.normal(0, 0.5, (4, 2)) + rng.normal(0, 0.7, (1, 2))
    gt, pred = E.match_rows(gq.reshape(-1, 4, 2))[0].reshape(B, M, 16), E.match_rows(pq.reshape(-1, 4, 2))[0].reshape(B, N, 16)
    cg = np.full((B,), M, np.int32) if counts_g is None else np.array(counts_g, np.int32)
    cp = np.full((B,), N, np.int32) if counts_p is None else np.array(counts_p, np.int32)
    return gt, cg, pred, cp


def page(seed, lines=12, per_line=25):
    """An annotated page: ``lines`` x ``per_line`` characters in slightly slanted lines, and predictions of it: jittered,
    10 % missing, 10 % duplicated (a second jitter of the same character), 20 spurious -> (gt (n, 4, 2), pred (m, 4, 2))"""
    rng = np.random.default_rng(seed)
    gt = []
    for li in range(lines):
        x, y0, slope = 20.0, 30.0 + 31.0 * li, rng.uniform(-0.02, 0.02)  # lines close enough for boxes to meet
        for _ in range(per_line):
            h, w = rng.uniform(22, 30), rng.uniform(12, 22)
            gt.append(rotated(y0 + slope * x, x + w / 2, h, w, np.rad2deg(np.arctan(slope)) + rng.uniform(-3, 3)))
            x += w + rng.uniform(1, 4)
    gt = np.stack(gt)
    jitter = lambda q: q + rng.normal(0, 1.2, (4, 2)) + rng.normal(0, 1.5, (1, 2))
    pred = []
    for q in gt:
        u = rng.uniform()
        if u < 0.1:
            continue
        pred.append(jitter(q))
        if u > 0.9:
            pred.append(jitter(q))
    for _ in range(20):
        pred.append(rotated(rng.uniform(20, 400), rng.uniform(20, 550), rng.uniform(10, 30), rng.uniform(10, 30),
                            rng.uniform(-20, 20)))
    pred = np.stack(pred)
    return gt, pred[rng.permutation(len(pred))]


@lru_cache(maxsize=None)
def page_reference(seed):
    """the page's tables and the oracle's answer on them, computed once and shared: do not modify"""
    gt, pred = page(seed)
    tables = E.evaluation_tables([pred], [gt])
    ref = E.match_quads_host(*tables[:4], 0.5)
    g, p = tables[0][0], tables[2][0]
    gi, pi = E.box_pairs(g, p)
    ious = np.array([E.quad_iou_host(g[a], p[c]) for a, c in zip(gi, pi)])
    return tables, ref, ious


def ulp_distance(a, b):
    """distance of two non-negative float64 arrays in representable steps"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return np.abs(a.view(np.int64) - b.view(np.int64))
