"""Shared inputs of the ribbon score tests (test_cpu_ribbon_match.py, test_gpu_ribbon_match.py,
test_gpu_ribbon_match_infer.py): arcs and S-curves as ribbons, straight lines cut into segments, the two concentric arcs,
seeded pages of bent lines whose predictions are whole, split into words, merged in pairs, missing or spurious, and the
hostile tables.  Every point lies on the 1/16 grid, so the rows hold it exactly."""
from functools import lru_cache

import numpy as np

from tests import line_match_cases as Q
from vkit_ocr_model_adaptive_scaling_amd.inferencing import ribbon_evaluation as R

grid = lambda a: np.rint(np.asarray(a, dtype=np.float64) * 16) / 16


def arc(cy, cx, r, h, a0, a1, n):
    """a line of height ``h`` along the circle of radius ``r`` about (cy, cx) from angle ``a0`` to ``a1`` (degrees, counter-
    clockwise from +x with y down: 120 -> 60 runs left to right over the top), n segments -> ribbon (n + 1, 2, 2)"""
    a = np.deg2rad(np.linspace(a0, a1, n + 1))
    rail = lambda rr: np.stack([cy - rr * np.sin(a), cx + rr * np.cos(a)], axis=1)
    return grid(np.stack([rail(r + h / 2), rail(r - h / 2)], axis=1))


def quarter(r, h=12.0, step=10):
    """the quarter arc of the issue: radius r about (300, 300), knots every ``step`` degrees"""
    return arc(300.0, 300.0, r, h, 135.0, 45.0, 90 // step)


def s_curve(n=12, h=10.0):
    """two arcs of opposite bend joined at a common tangent: the top rail is the outer side of the first and the inner side
    of the second"""
    first = arc(200.0, 100.0, 60.0, h, 150.0, 90.0, n // 2)
    second = arc(80.0, 100.0, 60.0, -h, 270.0, 330.0, n // 2)
    return grid(np.concatenate([first, second[1:]]))


def straight(y, x, h, w, cuts=()):
    """an axis-aligned line from (y, x), h high and w long, with knots at x + c for c in ``cuts``"""
    xs = np.array([0.0] + list(cuts) + [w]) + x
    return np.stack([np.stack([np.full_like(xs, y), xs], 1), np.stack([np.full_like(xs, y + h), xs], 1)], axis=1)


def outline_area2_q4(ribbon):
    """the integer shoelace sum of a ribbon's outline in Q4^2 (top rail forwards, bottom rail backwards), in Python ints"""
    q = np.rint(np.asarray(ribbon) * 16).astype(np.int64)
    ring = [(int(y), int(x)) for y, x in q[:, 0]] + [(int(y), int(x)) for y, x in q[::-1, 1]]
    return sum(x0 * y1 - x1 * y0 for (y0, x0), (y1, x1) in zip(ring, ring[1:] + ring[:1]))


def tables(gt, pred, care=None, gt_count=None, pred_count=None):
    """one image of ribbons -> the seven tables of ``match_ribbons_host``, B = 1"""
    g_rows, g_count, g_segs, bad_g = R.ribbon_tables([gt])
    p_rows, p_count, p_segs, bad_p = R.ribbon_tables([pred])
    assert not bad_g and not bad_p, (bad_g, bad_p)
    care = None if care is None else np.array(care, np.uint8)[None]
    cg = g_count if gt_count is None else np.array([gt_count], np.int32)
    cp = p_count if pred_count is None else np.array([pred_count], np.int32)
    return g_rows, cg, care, g_segs, p_rows, cp, p_segs


def from_line_tables(t):
    """the five tables of a line-score case -> the seven of the ribbon score with every row a ribbon of one segment: the
    segment tables are the match rows, the ribbon rows keep box, area and valid and name their own row"""
    gt_rows, gt_count, care, pred_rows, pred_count = t

    def side(rows):
        rows = np.asarray(rows, np.int32)
        rib = np.zeros_like(rows)
        rib[..., 8:15] = rows[..., 8:15]
        rib[..., 0] = np.arange(rows.shape[1], dtype=np.int32)[None]
        rib[..., 1] = 1
        return rib, rows.copy()
    g, gs = side(gt_rows)
    p, ps = side(pred_rows)
    return g, gt_count, care, gs, p, pred_count, ps


# ---- the two concentric arcs -----------------------------------------------------------------------------------------------

def two_arcs(outer=216.0):
    """the two lines of the issue, as ribbons and as the chord rectangles of ``quad_lines_lists_host`` on characters laid
    along them -> (ribbons, rectangles (2, 4, 2))"""
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import quad_lines_lists_host
    ribbons = [quarter(200.0), quarter(outer)]
    rects = []
    for r in (200.0, outer):
        chars = arc(300.0, 300.0, r, 12.0, 135.0, 45.0, 30)  # 30 characters of 3 degrees
        quads = np.stack([chars[:-1, 0], chars[1:, 0], chars[1:, 1], chars[:-1, 1]], axis=1)
        res = quad_lines_lists_host([quads])[0][0]
        assert len(res.polygons) == 1, len(res.polygons)
        rects.append(np.asarray(res.polygons[0], dtype=np.float64))
    return ribbons, np.stack(rects)


# ---- seeded pages of bent lines --------------------------------------------------------------------------------------------

def page(seed, n_lines, dont_care=0.05, spurious=0.05, per_row=3, segs=(6, 13)):
    """``n_lines`` annotated lines bent to a radius of 400 px, ``per_row`` to a text row, about 10 segments each.  Of the
    predictions about a third are split into two words, a sixth merge two neighbours, one in twenty is missing, the others
    are whole and jittered, with knots of their own; a few are spurious; the order is shuffled.
    -> (gt ribbons, care (n,) uint8, pred ribbons)"""
    rng = np.random.default_rng(seed)
    gt, pred = [], []
    row = 0
    nseg = lambda span: max(1, int(rng.integers(*segs) * span / 18.0 + 0.5))
    while len(gt) < n_lines:
        cy, cx, h = 460.0 + 44.0 * row, 500.0, rng.uniform(20, 28)
        row += 1
        a, spans = 120.0, []
        for _ in range(min(per_row, n_lines - len(gt))):
            w = rng.uniform(15, 19)
            spans.append((a, a - w))
            a -= w + rng.uniform(1.0, 2.0)
        gt += [arc(cy, cx, 400.0, h, a0, a1, nseg(a0 - a1)) for a0, a1 in spans]
        jit = lambda a0, a1: arc(cy + rng.normal(0, 0.8), cx + rng.normal(0, 0.8), 400.0, h * rng.uniform(0.9, 1.1),
                                 a0 + rng.normal(0, 0.15), a1 + rng.normal(0, 0.15), nseg(a0 - a1))
        i = 0
        while i < len(spans):
            a0, a1 = spans[i]
            u = rng.uniform()
            if u < 1 / 3 and i + 1 < len(spans):
                pred.append(jit(a0, spans[i + 1][1]))
                i += 2
                continue
            if u < 1 / 2:
                cut = a0 - (a0 - a1) * rng.uniform(0.3, 0.7)
                pred += [jit(a0, cut + 0.3), jit(cut - 0.3, a1)]
            elif u < 0.95:
                pred.append(jit(a0, a1))
            i += 1
    for _ in range(max(1, int(spurious * n_lines))):
        a0 = rng.uniform(70, 120)
        pred.append(arc(rng.uniform(300, 460 + 44 * row), rng.uniform(300, 700), 400.0, rng.uniform(15, 25), a0, a0 - rng.uniform(4, 10), 4))
    care = (rng.uniform(size=len(gt)) >= dont_care).astype(np.uint8)
    return gt, care, [pred[i] for i in rng.permutation(len(pred))]


def straight_page(seed, n_lines):
    """straight lines cut into 1..5 segments, predicted whole, as two words or merged in pairs, as one-image tables"""
    rng = np.random.default_rng(seed)
    gt, pred = [], []
    cuts = lambda w: sorted({float(c) for c in grid(rng.uniform(4, w - 4, rng.integers(0, 5)))})  # 1..5 segments
    k = 0
    while k < n_lines:
        y, x = 30.0 * (k // 4) + 4, 260.0 * (k % 4) + 4
        w = float(grid(rng.uniform(80, 110)))
        u = rng.uniform()
        if u < 0.3 and k % 4 != 3 and k + 1 < n_lines:  # two annotations of w under one detection
            gt += [straight(y, x, 16.0, w, cuts(w)), straight(y, x + w + 8, 16.0, w, cuts(w))]
            pred.append(straight(y + 0.5, x, 16.0, 2 * w + 8, cuts(2 * w + 8)))
            k += 2
            continue
        gt.append(straight(y, x, 16.0, w, cuts(w)))
        if u < 0.65:
            half = float(grid(w / 2))
            pred += [straight(y, x, 16.0, half - 2, cuts(half - 2)), straight(y, x + half + 2, 16.0, w - half - 2, cuts(w - half - 2))]
        else:
            pred.append(straight(y + 0.25, x + 0.5, 16.0, w, cuts(w)))
        k += 1
    return tables(gt, [pred[i] for i in rng.permutation(len(pred))])


def random_tables(seed, B, M, N, counts_g=None, counts_p=None, **kw):
    """(B, M, 16) / (B, N, 16) ribbon tables from ``page``: M annotated lines and the first N of their shuffled predictions
    (filled up with repeats when there are fewer); from 9 rows on a few ribbons are invalid (zero rows: their segments stay
    in the table, unused) -> the seven tables"""
    gts, preds, cares = [], [], []
    for b in range(B):
        g, c, p = page(1000 * seed + b, M, dont_care=0.1, **kw)
        gts.append(g)
        preds.append([p[i % len(p)] for i in range(N)])
        cares.append(c * (1 + 2 * b))
    g_rows, _, g_segs, _ = R.ribbon_tables(gts)
    p_rows, _, p_segs, _ = R.ribbon_tables(preds)
    if N > 8:
        p_rows[:, 5::17] = 0
    if M > 8:
        g_rows[:, 3::13] = 0
    cg = np.full((B,), M, np.int32) if counts_g is None else np.array(counts_g, np.int32)
    cp = np.full((B,), N, np.int32) if counts_p is None else np.array(counts_p, np.int32)
    return g_rows, cg, np.stack(cares).astype(np.uint8), g_segs, p_rows, cp, p_segs


def reference(t, **params):
    """both oracles on one ``ribbon_pairs`` -> (pairs, sequential outputs, rounds outputs)"""
    pairs = R.ribbon_pairs(*t, **params)
    return pairs, R.match_ribbons_host(*t, **params, pairs=pairs), R.match_ribbons_rounds_host(*t, **params, pairs=pairs)


@lru_cache(maxsize=None)
def page_reference(seed, n_lines=200):
    """a page's tables and both oracles' answers at the default thresholds, computed once and shared: do not modify"""
    gt, care, pred = page(seed, n_lines)
    t = tables(gt, pred, care)
    return (t,) + reference(t)


# ---- many segments ---------------------------------------------------------------------------------------------------------

def long_line(n, y=0.0, x=0.0, h=8.0, w=512.0):
    """a straight line of n segments, equal up to the 1/16 grid"""
    return straight(y, x, h, w, [float(grid(w * k / n)) for k in range(1, n)])


def segment_count_case(ng, npred):
    """one gt of ``ng`` segments under one pred of ``npred``, shifted by (1, 3): one to one, I = 2 * (7 * 16) * (509 * 16)
    whatever the two subdivisions; beside them a second pair of lines that is a split, so that the phases run too"""
    gt = [long_line(ng), long_line(ng, 40.0)]
    pred = [long_line(npred, 1.0, 3.0), long_line(max(npred // 2, 1), 40.0, 0.0, 8.0, 250.0),
            long_line(max(npred // 2, 1), 40.0, 262.0, 8.0, 250.0)]
    return tables(gt, pred)


# ---- hostile tables (rule 8) -------------------------------------------------------------------------------------------------

def hostile_cases():
    """name -> (tables, what the oracle must answer: (gt_kind, pred_kind, candidates)).  One gt over one pred, both of 4
    segments and equal: one to one before the table is spoilt."""
    base = lambda: [a.copy() if isinstance(a, np.ndarray) else a for a in tables([long_line(4)], [long_line(4)])]
    c = {}
    t = base(); c['intact'] = (t, ([Q.ONE], [Q.ONE], 1))
    t = base(); t[0][0, 0, 1] = 0; c['seg_count_zero'] = (t, ([Q.FREE], [Q.FREE], 0))
    t = base(); t[4][0, 0, 1] = 257; c['seg_count_257'] = (t, ([Q.FREE], [Q.FREE], 0))
    t = base(); t[0][0, 0, 1] = -3; c['seg_count_negative'] = (t, ([Q.FREE], [Q.FREE], 0))
    t = base(); t[0][0, 0, 0] = -1; c['seg_start_negative'] = (t, ([Q.FREE], [Q.FREE], 0))
    t = base(); t[4][0, 0, 0] = 1; c['run_leaves_the_table'] = (t, ([Q.FREE], [Q.FREE], 0))
    t = base(); t[4][0, 0, 0] = (1 << 31) - 1; t[4][0, 0, 1] = 256; c['start_plus_count_overflows'] = (t, ([Q.FREE], [Q.FREE], 0))
    t = base(); t[0][0, 0, 0] = -(1 << 31); c['seg_start_int_min'] = (t, ([Q.FREE], [Q.FREE], 0))
    # three of the pred's four segments lose their valid word: I = a quarter of the line, below both thresholds' reach
    t = base(); t[6][0, 1:4, 14] = 0; c['invalid_segments'] = (t, ([Q.FREE], [Q.FREE], 0))
    # ... and with one invalid segment three quarters are left: precision holds, recall 0.8 does not
    t = base(); t[6][0, 3, 14] = 0; c['one_invalid_segment'] = (t, ([Q.FREE], [Q.FREE], 1))
    # a segment box that lies: pruned, so that segment contributes nothing although its corners overlap
    t = base(); t[3][0, 0, 8:12] = (100000, 100000, 100100, 100100); c['lying_segment_box'] = (t, ([Q.FREE], [Q.FREE], 1))
    # a ribbon box that lies: the pair is never met
    t = base(); t[0][0, 0, 8:12] = (100000, 100000, 100100, 100100); c['lying_ribbon_box'] = (t, ([Q.FREE], [Q.FREE], 0))
    # a ribbon area that lies (four times the truth): rec fails, prec holds -> a candidate, no match
    t = base(); t[0][0, 0, 12] *= 4; c['lying_ribbon_area'] = (t, ([Q.FREE], [Q.FREE], 1))
    # a segment area of zero: the clamp of the clip takes its pairs to 0
    t = base(); t[3][0, :, 12:14] = 0; c['zero_segment_areas'] = (t, ([Q.FREE], [Q.FREE], 0))
    return c
