"""The text-line rule of inferencing/lines.py on the host: the oracle against a second restatement written differently, the
layout cases against their known truth, each threshold at equality and one Q4 step beyond, the magnitude bounds at the
corner COORD_MAX, ``line_quads`` against Fraction arithmetic, the parameter ranges.  Exact equality throughout."""
from fractions import Fraction

import numpy as np
import pytest

from tests import quad_line_cases as Q
from vkit_ocr_model_adaptive_scaling_amd.inferencing import evaluation as E
from vkit_ocr_model_adaptive_scaling_amd.inferencing import lines as L

DEFAULT = (24, 8, 32)  # gap 1.5, cross 0.5, height_ratio 2.0 as Q4


def assert_truth(quads, truth, **kw):
    rows, count = Q.table_of(quads)
    got = L.quad_lines_host(rows, count, **kw)
    line, order, table, n = Q.truth_outputs(rows, count, truth)
    assert np.array_equal(got[0], line), [np.flatnonzero(got[0][0] == l).tolist() for l in range(int(got[3][0, 3]))]
    assert np.array_equal(got[1], order) and np.array_equal(got[2], table)
    assert got[3][0, [0, 1, 3]].tolist() == [n, n, len(truth)]
    return got


# ---- the oracle against the restatement --------------------------------------------------------------------------------

def random_graph(seed, n):
    """random rows (valid quads, a few rows invalid) and a random link graph over the rows that take part: a few long chains
    in scrambled index order, a few random links, the rest alone"""
    rng = np.random.default_rng(seed)
    quads, _ = Q.layout(1, n, 30.0, 16.0, 19.0, 42.0, angle=rng.uniform(0, 6), seed=seed)
    rows = E.match_rows(quads)[0]
    rows[rng.uniform(size=n) < 0.1] = 0
    if seed % 2:  # exact ties of k: every row the same quad
        rows[rows[:, 14] != 0] = rows[np.flatnonzero(rows[:, 14])[0]]
    part = rows[:, 14] != 0
    idx = rng.permutation(np.flatnonzero(part))
    cuts = sorted(rng.choice(np.arange(1, len(idx)), size=4, replace=False).tolist())
    li, lj = [], []
    for a, b in zip([0] + cuts[:3], cuts[:3] + [cuts[3]]):  # the members behind the last cut stay alone
        chain = idx[a:b]
        for x, y in zip(chain[:-1], chain[1:]):
            li.append(int(min(x, y)))
            lj.append(int(max(x, y)))
    for _ in range(3):
        x, y = rng.choice(idx, 2, replace=False)
        li.append(int(min(x, y)))
        lj.append(int(max(x, y)))
    return rows, part, np.array(li), np.array(lj)


@pytest.mark.parametrize('seed', range(6))
def test_sequential_form_equals_the_rounds_restatement(seed):
    rows, part, li, lj = random_graph(seed, 60)
    line, order, table = L.lines_of_links(rows, part, li, lj)
    rline, rorder, rtable = Q.lines_by_rounds(rows, part, li.tolist(), lj.tolist())
    assert np.array_equal(line, rline) and order == rorder and table == rtable
    sizes = sorted(t[1] for t in table)
    assert sizes[-1] >= 10 and sizes[0] == 1 and (line == -1).sum() == (~part).sum() > 0


def test_hand_cases():
    for name, (rows, count, line, order, table, stats) in Q.hand_cases().items():
        got = L.quad_lines_host(rows[None], [count])
        assert got[0][0].tolist() == line and got[1][0].tolist() == order and got[3][0].tolist() == stats, name
        if table is not None:
            assert got[2][0, :len(table)].tolist() == table and not got[2][0, len(table):].any(), name
        n = min(count, len(rows))
        part, li, lj = L.link_pairs(rows[:n], *DEFAULT)
        rline, rorder, rtable = Q.lines_by_rounds(rows[:n], part, li.tolist(), lj.tolist())
        assert got[0][0, :n].tolist() == rline.tolist() and got[1][0, :len(rorder)].tolist() == rorder, name
        assert got[2][0, :len(rtable)].tolist() == rtable, name


# ---- layouts against their truth -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('angle', Q.ANGLES)
@pytest.mark.parametrize('script', ['cjk', 'latin'])
def test_three_lines_of_fifteen_are_recovered(script, angle):
    if script == 'cjk':
        quads, truth = Q.layout(3, 15, **Q.CJK, angle=angle, seed=3)
    else:
        quads, truth = Q.layout(3, 15, **Q.LATIN, word_space=10.0, angle=angle, seed=4)
    got = assert_truth(quads, truth)
    assert got[3][0, 3] == 3 and sorted(truth[0]) != truth[0]  # the index order is scrambled


@pytest.mark.parametrize('angle', Q.ANGLES)
def test_word_space_20_splits_the_lines_into_their_words(angle):
    # CJK: 33 + 20 = 53 px between the centres at a word space, above gap = 1.5 heights = 45 px
    quads, truth = Q.layout(3, 15, **Q.CJK, word_space=20.0, angle=angle, seed=5)
    assert_truth(quads, Q.split_words(truth))
    # Latin: 19 + 20 = 39 px, which 1.5 heights still bridge; gap = 1.0 height = 30 px splits there and keeps the pitch of 19
    quads, truth = Q.layout(3, 15, **Q.LATIN, word_space=20.0, angle=angle, seed=6)
    assert_truth(quads, truth)
    assert_truth(quads, Q.split_words(truth), gap=1.0)


def test_lists_route_and_line_quads_on_a_layout():
    quads, truth = Q.layout(3, 15, **Q.LATIN, word_space=10.0, angle=0.35, seed=7)
    res, stats = L.quad_lines_lists_host([quads, quads[:0], quads[:7]])
    assert [r.tolist() for r in res[0].lines] == truth and res[0].valid.all() and stats[0] == 45 + 7
    assert res[1].lines == [] and res[1].polygons.shape == (0, 4, 2) and res[1].line.shape == (0,)
    assert res[0].line.dtype == np.int32 and res[0].lines[0].dtype == np.int32
    rows, ok = E.match_rows(res[0].polygons)
    assert ok.all()  # strictly convex and clockwise: fit for evaluate_quads
    assert L.quad_lines_lists_host([]) [0] == []


# ---- thresholds --------------------------------------------------------------------------------------------------------

def linked(rows, q4=DEFAULT):
    part, li, lj = L.link_pairs(rows, *q4)
    assert part.all()
    return len(li) == 1


def test_each_threshold_at_equality_and_one_step_beyond():
    # 32 px boxes: v = (1024, 0), vv = 2^20, d = 4 * (dy, dx): 8 |d.v| = 2^15 dy <= cross * 2^20  <=>  dy <= 32 cross, and
    # likewise dx <= 32 gap
    assert linked(Q.pair_rows(32 * 8, 0)) and not linked(Q.pair_rows(32 * 8 + 1, 0)) and linked(Q.pair_rows(-32 * 8, 0))
    assert not linked(Q.pair_rows(-32 * 8 - 1, 0))
    assert linked(Q.pair_rows(0, 32 * 24)) and not linked(Q.pair_rows(0, 32 * 24 + 1)) and linked(Q.pair_rows(0, -32 * 24))
    assert not linked(Q.pair_rows(0, -32 * 24 - 1))
    assert linked(Q.pair_rows(32 * 8, 32 * 24)) and linked(Q.pair_rows(32 * 8 + 1, 0), (24, 9, 32))
    assert linked(Q.pair_rows(0, 32 * 24 + 1), (25, 8, 32))
    # the smaller box decides: 16 px against 32 px, its own half height is 8 px and its own gap 24 px
    assert linked(Q.pair_rows(16 * 8, 16 * 24, h1=16)) and not linked(Q.pair_rows(16 * 8 + 1, 0, h1=16))
    assert not linked(Q.pair_rows(0, 16 * 24 + 1, h1=16))
    # heights: 256 vv_i <= ratio^2 vv_j  <=>  16 h_i <= ratio h_j: 32 against 16 at ratio 2.0 is equality
    assert linked(Q.pair_rows(0, 160, h0=32, h1=16)) and not linked(Q.pair_rows(0, 160, h0=32.125, h1=16))
    assert linked(Q.pair_rows(0, 160, h0=16, h1=32)) and not linked(Q.pair_rows(0, 160, h0=16, h1=32.125))
    assert not linked(Q.pair_rows(0, 160, h0=32, h1=16), (24, 8, 31)) and linked(Q.pair_rows(0, 160, h0=32.125, h1=16), (24, 8, 33))
    # v_i . v_j = 0: the second square's corners one place on (its v is the first's u), both on one centre
    rows = Q.pair_rows(0, 0, w0=32, w1=32)
    rows[1, 0:8] = rows[1, [6, 7, 0, 1, 2, 3, 4, 5]]
    _, v, _, vv = L.quad_frames(rows)
    assert int((v[0] * v[1]).sum()) == 0 and vv[0] == vv[1] and not linked(rows)
    rows[1, 4] += 1  # P2_y one Q4 step down: v_j,y = 1
    assert int((L.quad_frames(rows)[1][0] * L.quad_frames(rows)[1][1]).sum()) == 1024 and linked(rows)
    rows[1, 4] -= 2
    assert not linked(rows)


# ---- magnitudes ----------------------------------------------------------------------------------------------------------

def test_products_at_the_corner_stay_below_2_to_60_and_equal_python_integers():
    M = E.COORD_MAX
    # the largest frames the coordinate range allows: corners at +-2^19 (raw rows: the valid word set by hand)
    # the whole box; the same turned half round; the top edge in one corner and the bottom edge in the opposite one
    # (v = (2^21, 2^21), vv = 2^43); all four corners in one corner (s = +-2^21: d reaches 2^22); the whole box once more
    big = np.array([[-M, -M, -M, M, M, M, M, -M], [M, M, M, -M, -M, -M, -M, M], [-M, -M, -M, -M, M, M, M, M],
                    [M, M, M, M, M, M, M, M], [-M, -M, -M, -M, -M, -M, -M, -M], [-M, -M, -M, M, M, M, M, -M]], np.int64)
    rows = np.zeros((6, 16), np.int32)
    rows[:, :8], rows[:, 14] = big, 1
    s, v, u, vv = L.quad_frames(rows)
    assert abs(s).max() == 1 << 21 and abs(v).max() == 1 << 21 and abs(u).max() == 1 << 21 and vv.max() == 1 << 43
    worst = 0
    for gap, cross, ratio in ((4096, 4096, 256), (1, 1, 16), (24, 8, 32)):
        want = []
        for i in range(6):
            for j in range(i + 1, 6):
                P = [[(int(big[m, 2 * k]), int(big[m, 2 * k + 1])) for k in range(4)] for m in (i, j)]
                S = [[sum(p[k][c] for k in range(4)) for c in (0, 1)] for p in P]
                V = [[p[3][c] + p[2][c] - p[0][c] - p[1][c] for c in (0, 1)] for p in P]
                VV = [x[0] * x[0] + x[1] * x[1] for x in V]
                d = [S[1][0] - S[0][0], S[1][1] - S[0][1]]
                terms = [8 * abs(d[0] * V[a][0] + d[1] * V[a][1]) for a in (0, 1)]
                terms += [8 * abs(d[0] * V[a][1] - d[1] * V[a][0]) for a in (0, 1)]
                terms += [cross * VV[a] for a in (0, 1)] + [gap * VV[a] for a in (0, 1)]
                terms += [256 * VV[a] for a in (0, 1)] + [ratio * ratio * VV[a] for a in (0, 1)]
                worst = max(worst, max(terms))
                ok = all(terms[a] <= cross * VV[a] and terms[2 + a] <= gap * VV[a] for a in (0, 1))
                ok = ok and 256 * VV[0] <= ratio * ratio * VV[1] and 256 * VV[1] <= ratio * ratio * VV[0]
                ok = ok and V[0][0] * V[1][0] + V[0][1] * V[1][1] > 0
                if ok:
                    want.append((i, j))
        _, li, lj = L.link_pairs(rows, gap, cross, ratio)
        assert list(zip(li.tolist(), lj.tolist())) == want, (gap, cross, ratio)
    assert (1 << 58) <= worst < (1 << 60)
    # a line of 8192 such rows: |U| <= 2^34, keys at or below 2^56, extents at or below 2^54 - inside int64
    U = 8192 * (1 << 21)
    assert 2 * (1 << 21) * U <= 1 << 56 and 2 * M * U <= 1 << 54
    got = L.quad_lines_host(rows[None, [0, 5]], [2])  # two coincident rows: one line
    line, order, table, _ = Q.truth_outputs(rows[None, [0, 5]], [2], [[0, 1]])
    assert got[3][0].tolist() == [2, 2, 1, 1] and np.array_equal(got[2], table) and abs(table).max() == M * (1 << 22)


# ---- line_quads ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('angle', [0.0, 0.35, 3.0])
def test_line_quads_against_fractions_and_every_member_corner_inside(angle):
    quads, truth = Q.layout(3, 15, **Q.LATIN, word_space=10.0, angle=angle, seed=8)
    rows, count = Q.table_of(quads)
    line, order, table, stats = L.quad_lines_host(rows, count)
    t = table[0, :3]
    polys = L.line_quads(t)
    assert polys.shape == (3, 4, 2) and polys.dtype == np.float64
    for l, (start, size, uy, ux, a0, a1, b0, b1) in enumerate(t.tolist()):
        UU = uy * uy + ux * ux
        want = [[float(Fraction(a * uy + b * ux, 16 * UU)), float(Fraction(a * ux - b * uy, 16 * UU))]
                for a, b in ((a0, b0), (a1, b0), (a1, b1), (a0, b1))]
        assert polys[l].tolist() == want
        # in the line's own frame every member corner lies within the extent, exactly; and in pixels within one rounding of
        # the rectangle: its (a, b) against the rounded corners' (a, b), a tolerance of 2^-40 of the line's length in a-units
        U = np.array([uy, ux], np.float64)
        for m in order[0, start:start + size]:
            for k in range(4):
                py, px = int(rows[0, m, 2 * k]), int(rows[0, m, 2 * k + 1])
                assert a0 <= py * uy + px * ux <= a1 and b0 <= py * ux - px * uy <= b1
        ca = polys[l] @ U * 16
        cb = polys[l] @ np.array([ux, -uy], np.float64) * 16
        eps = (a1 - a0) * 2.0 ** -40
        assert abs(ca - [a0, a1, a1, a0]).max() <= eps and abs(cb - [b0, b0, b1, b1]).max() <= eps
    assert L.line_quads(table[0, 3:6]).tolist() == np.zeros((3, 4, 2)).tolist()  # rows without members


# ---- parameters ------------------------------------------------------------------------------------------------------------

def test_parameters_outside_their_ranges_raise():
    assert L.line_params() == DEFAULT and L.line_params(256.0, 1 / 16, 16.0) == (4096, 1, 256)
    assert L.line_params(0.03125 * 3, 0.5, 1.0) == (2, 8, 16)  # rint: 1.5 goes to the even 2
    rows, count = Q.table_of(np.array([Q.SQ(0, 0, 30, 16)], np.float64))
    for bad in (dict(gap=0.0), dict(gap=256.1), dict(cross=0.02), dict(cross=300.0), dict(height_ratio=0.9),
                dict(height_ratio=16.1), dict(gap=float('nan')), dict(cross=float('inf')), dict(gap=-1.5)):
        with pytest.raises(ValueError):
            L.line_params(**bad)
        with pytest.raises(ValueError):
            L.quad_lines_host(rows, count, **bad)
        with pytest.raises(ValueError):
            L.quad_lines_lists_host([np.array([Q.SQ(0, 0, 30, 16)], np.float64)], **bad)
    with pytest.raises(ValueError):
        L.quad_lines_host(rows[0], count)
    with pytest.raises(ValueError):
        L.quad_lines_lists_host([np.zeros((8193, 4, 2))])
