"""The rule from a line's character quads to its spine, the integer rule from knots to columns, the layout and the host oracle
(inferencing/spines.py), on the host: a straight line against its analytic positions (upright, turned, mirrored), a quarter
circle against the circle and against the chord rectangle's strip, the integer rule against a restatement in Python integers
at the extremes and at every bound, and the rule's own decisions.

The straight lines are cut with margin 0 at heights 20 and 40: twelve characters of 16 x 20 px then give 192 and 384 columns
and every knot falls on a whole column (8, 24, 40, ... px along the line), so that the position bound below - which holds
no term for a knot column's rounding - is the rule's own; at other heights a knot sits up to half a column off (the module
docstring's limits)."""
import numpy as np
import pytest

from tests import spine_cases as P
from tests import strip_cases as C
from vkit_ocr_model_adaptive_scaling_amd.inferencing import spines as S
from vkit_ocr_model_adaptive_scaling_amd.inferencing import strips as Q
from vkit_ocr_model_adaptive_scaling_amd.inferencing.packing import warp_host

NONE = -(1 << 63)


def frame(quads):
    """start, unit reading direction, down vector (of the height) and length of a straight line of equal characters."""
    A = ((quads[:, 1] - quads[:, 0]) + (quads[:, 2] - quads[:, 3])) / 2
    D = ((quads[:, 3] - quads[:, 0]) + (quads[:, 2] - quads[:, 1])) / 2
    start = quads[0].mean(axis=0) - A[0] / 2
    return start, A[0] / np.hypot(*A[0]), D[0], float(np.hypot(*A.T).sum())


LINES = {'upright': dict(), '0.35 rad': dict(angle=0.35, at=(40.0, 30.0)), '1.57 rad': dict(angle=1.57, at=(20.0, 60.0)),
         '3.0 rad': dict(angle=3.0, at=(60.0, 230.0)), 'mirrored': dict(mirrored=True), 'mirrored, 0.35 rad': dict(angle=0.35, mirrored=True)}


@pytest.mark.parametrize('h', [20, 40])
@pytest.mark.parametrize('name', list(LINES))
def test_a_straight_line_maps_onto_its_analytic_positions(name, h):
    quads = P.straight(**LINES[name])
    start, along, down, length = frame(quads)
    img = C.picture((240, 260), 5)
    out = S.spine_strips_host([img], [[quads]], h, 2048, 1, 0.0)
    w = 192 * h // 20
    assert out.status.tolist() == [0] and out.widths.tolist() == [w] and not out.squeezed[0]
    assert out.rows[0, 7] == 0 or 'rad' in name  # a turned step of one pixel may round to just above one: log2n 1
    knots = out.knots
    assert knots[:, 0].tolist() == [0] + [(8 + 16 * k) * h // 20 for k in range(12)] + [w], 'every knot on a whole column'
    centres, downs = out.spine(0)[:, 0], out.spine(0)[:, 1]
    off = (centres - start) @ np.array([along[1], -along[0]])
    assert np.abs(off).max() <= 2.0 ** -16, 'the knots are collinear'
    assert np.abs(downs - down).max() <= 2.0 ** -16
    cols = S.spine_columns_host(knots, w, h)
    assert (cols != NONE).all()
    if 'rad' not in name:
        assert (cols[:, [2, 4]] == cols[0, [2, 4]]).all(), 'all columns share myy, mxy'
    assert np.ptp(cols[:, 2]) <= 1 and np.ptp(cols[:, 4]) <= 1
    j = np.arange(w) + 0.5
    bound = (2 + h / 4) * 2.0 ** -16 + 2.0 ** -16  # the floor in C, the knots' and the steps' half units over h/2 rows
    worst = 0.0
    for y, part in ((h / 2, 0.0), (0.0, -0.5), (float(h), 0.5)):
        got = out.remap(0, np.stack([np.full((w,), y), j], axis=1))
        want = start + (j * length / w)[:, None] * along + part * down
        worst = max(worst, float(np.abs(got - want).max()))
    print(f'{name}, h {h}: position error {worst * 65536:.2f} / 65536 px, bound {bound * 65536:.2f} / 65536')
    assert worst <= bound
    # between the column centres the map is affine along the line
    mid = out.remap(0, np.array([[h / 2, 10.0], [h / 2, 10.5], [h / 2, 11.0]]))
    assert np.abs(mid[0] + mid[2] - 2 * mid[1]).max() <= 2.0 ** -15
    # the upright line at its natural height is a numpy slice
    if name == 'upright' and h == 20:
        assert np.array_equal(out.strip(0), img[50:70, 40:232])
    if name == 'mirrored' and h == 20:
        assert np.array_equal(out.strip(0), img[50:70, 40:232][:, ::-1]), 'a mirrored line gives a mirrored strip'


CENTRE, R, SPACING = (20.0, 20.0), 200.0, 15.7


def circle_scene():
    return P.arc(CENTRE, R, 20, 12.0, 20.0, SPACING), P.radial_image((256, 256), CENTRE, R)


def rows_are_level(strip):
    v = strip[:, :, 0].astype(np.int64)
    return int(np.abs(v - np.median(v, axis=1, keepdims=True)).max())


def test_a_quarter_circle_is_cut_along_the_circle_and_its_chord_rectangle_is_not():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import quad_lines_lists_host
    quads, img = circle_scene()
    h = 32
    out = S.spine_strips_host([img], [[quads]], h)
    assert out.status.tolist() == [0] and len(out.knots) == 22
    w, q = int(out.widths[0]), out.knots[:, 0]
    inner = np.arange(q[1], q[-2])  # the columns between the first and the last character
    r = np.hypot(*(out.remap(0, np.stack([np.full(len(inner), h / 2), inner + 0.5], axis=1)) - CENTRE).T)
    low, high = R - SPACING ** 2 / (8 * R) - 2.0 ** -10, R + 2.0 ** -10
    print(f'column centres at {r.min():.5f} .. {r.max():.5f} px from the centre, allowed {low:.5f} .. {high:.5f}')
    assert low <= r.min() and r.max() <= high
    level = rows_are_level(out.strip(0))
    print(f'{w} columns; a row varies by at most {level} levels about its median (allowed 2)')
    assert level <= 2
    assert (np.diff(out.strip(0)[:, w // 2, 0].astype(int)) > 0).all(), 'down the strip is away from the centre'
    # the chord rectangle of the same line: what the straight route cuts
    ref, _ = quad_lines_lists_host([quads])
    assert [m.tolist() for m in ref[0].lines] == [list(range(20))]
    chord = Q.quad_strips_host([img], [ref[0].polygons], h)
    assert chord.status.tolist() == [0]
    print(f'the chord rectangle: {int(chord.widths[0])} columns, a row varies by {rows_are_level(chord.strip(0))} levels')
    assert rows_are_level(chord.strip(0)) > 2, 'the straight strip is not level: the point of the feature'
    # the outline follows the ring
    poly = S.spine_polygon(out.knots)
    assert poly.shape == (44, 2)
    rr = np.hypot(*(poly - CENTRE).T)
    assert np.abs(rr[1:21] - (R - 12.5)).max() < 0.01 and np.abs(rr[23:43] - (R + 12.5)).max() < 0.01


# ---- the integer rule ------------------------------------------------------------------------------------------------
def column_py(knots, j, h):
    """The rule of the module docstring in Python integers -> (record or None, the largest intermediate)."""
    K = len(knots)
    lo, hi = 0, K
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if knots[mid][0] <= j:
            lo = mid
        else:
            hi = mid
    if lo + 1 >= K:
        return None, 0
    e0, e1 = knots[lo], knots[lo + 1]
    if not e0[0] <= j < e1[0] or e1[0] - e0[0] > 8192:
        return None, 0
    for e in (e0, e1):
        if max(abs(e[1]), abs(e[2])) >= 1 << 39 or max(abs(e[3]), abs(e[4])) > 1 << 30:
            return None, 0
    n, a = e1[0] - e0[0], 2 * (j - e0[0]) + 1
    seen = [2 * n]
    mid = []
    for c in range(1, 5):
        seen.append((e1[c] - e0[c]) * a)
        mid.append(e0[c] + seen[-1] // (2 * n))
    Cy, Cx, Vy, Vx = mid
    rdiv = lambda x, d: (seen.append(2 * x + d), (2 * x + d) // (2 * d))[1]
    myy, mxy, myx, mxx = rdiv(Vy, h), rdiv(Vx, h), rdiv(e1[1] - e0[1], n), rdiv(e1[2] - e0[2], n)
    seen += [(h - 1) * myy, (h - 1) * mxy]
    ay, ax = Cy - ((h - 1) * myy) // 2, Cx - ((h - 1) * mxy) // 2
    big = max(abs(v) for v in seen + mid + [ay, ax])
    if max(abs(ay), abs(ax)) >= 1 << 40 or max(abs(myy), abs(myx), abs(mxy), abs(mxx)) > 1 << 22:
        return None, big
    return [ay, ax, myy, myx, mxy, mxx], big


def assert_columns(knots, w, h, what):
    got = S.spine_columns_host(np.array(knots, np.int64), w, h)
    assert got.shape == (w, 6) and got.dtype == np.int64
    biggest, valid = 0, 0
    for j in range(w):
        want, big = column_py(knots, j, h)
        biggest = max(biggest, big)
        valid += want is not None
        assert got[j].tolist() == (want if want is not None else [NONE] * 6), (what, j)
    return valid, biggest


def test_the_integer_rule_equals_its_restatement_at_the_extremes():
    top, step = (1 << 39) - 1, (1 << 22) - 1
    biggest = 0
    for h in (1, 7, 256):
        for n in (1, 8192):
            v = h * step
            for sy, sx in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
                # valid at the extremes: the far knot at |c| = 2^39 - 1, the near one n full steps before it
                knots = [[0, sy * (top - n * step), sx * (top - n * step), sy * v, -sx * v, 0], [n, sy * top, sx * top, -sy * v, sx * v, 0]]
                assert S.knot_status(knots, h) == 0
                valid, big = assert_columns(knots, n, h, ('extreme', h, n))
                assert valid == n
                biggest = max(biggest, big)
            # the largest intermediates: knots from one end of the range to the other (no valid column unless n is large)
            knots = [[0, -top, top, -(1 << 30), 1 << 30, 0], [n, top, -top, 1 << 30, -(1 << 30), 0]]
            valid, big = assert_columns(knots, n, h, ('span', h, n))
            assert valid == 0 and S.knot_status(knots, h) == 2
            biggest = max(biggest, big)
    print(f'the largest intermediate: 2^{np.log2(float(biggest)):.2f}')
    assert (1 << 53) < biggest < (1 << 55)  # |dc| * a < 2^40 * 2^14: far below 2^63
    rng = np.random.default_rng(1)
    for case in range(40):
        h, K = int(rng.integers(1, 257)), int(rng.integers(2, 9))
        q = np.concatenate([[0], np.cumsum(rng.integers(1, 40, K - 1))])
        scale = [1 << 12, 1 << 20, 1 << 24][case % 3]
        c = np.cumsum(rng.integers(-scale, scale + 1, (K, 2)) * np.diff(q, prepend=0)[:, None], axis=0) + int(rng.integers(-1 << 30, 1 << 30))
        v = rng.integers(-h * scale, h * scale + 1, (K, 2))
        knots = np.concatenate([q[:, None], c, v, np.zeros((K, 1), np.int64)], axis=1).tolist()
        valid, _ = assert_columns(knots, int(q[-1]) + 3, h, ('random', case))  # three columns beyond the last knot
        if S.knot_status(knots, h) == 0:
            assert valid == q[-1], 'knots within the host rule\'s bounds give valid columns throughout'


def test_every_bound_at_equality_and_one_step_beyond():
    top, step = (1 << 39) - 1, (1 << 22) - 1
    h, n = 32, 100
    base = [[0, 1000, -2000, h * 65536, 0, 0], [n, 1000 + n * 65536, -2000, h * 65536, 0, 0]]

    def with_(knot, word, value):
        k = [list(e) for e in base]
        k[knot][word] = value
        return k

    for knot in (0, 1):
        for word in (1, 2):
            for sign in (1, -1):
                far = sign * top
                near = [list(e) for e in base]
                near[knot][word], near[1 - knot][word] = far, far - sign * 1000
                assert S.knot_status(near, h) == 0 and assert_columns(near, n, h, 'c at 2^39 - 1')[0] == n
                near[knot][word] = sign * (1 << 39)
                assert S.knot_status(near, h) == 2 and assert_columns(near, n, h, 'c at 2^39')[0] == 0
        for word in (3, 4):
            for sign in (1, -1):
                assert S.knot_status(with_(knot, word, sign * h * step), h) == 0
                assert assert_columns(with_(knot, word, sign * h * step), n, h, 'v at h * (2^22 - 1)')[0] == n
                assert S.knot_status(with_(knot, word, sign * (h * step + 1)), h) == 2
    for word in (1, 2):
        for sign in (1, -1):
            k = with_(1, word, base[0][word] + sign * n * step)
            assert S.knot_status(k, h) == 0 and assert_columns(k, n, h, 'dc at n * (2^22 - 1)')[0] == n
            k = with_(1, word, base[0][word] + sign * (n * step + 1))
            assert S.knot_status(k, h) == 2
            # the column rule's own bound: |m| <= 2^22
            assert assert_columns(with_(1, word, base[0][word] + sign * (n << 22)), n, h, 'm at 2^22')[0] == n
            assert assert_columns(with_(1, word, base[0][word] + sign * ((n << 22) + n)), n, h, 'm beyond 2^22')[0] == 0
    # |v| <= 2^30 for the knots the columns read (h * 2^22 at h = 256), and |m| <= 2^22 of the record
    tall = [[0, 0, 0, 1 << 30, -(1 << 30), 0], [4, 0, 0, 1 << 30, -(1 << 30), 0]]
    assert assert_columns(tall, 4, 256, 'v at 2^30')[0] == 4 and assert_columns(tall, 4, 255, 'v / h beyond 2^22')[0] == 0
    tall[1][3] += 1
    assert assert_columns(tall, 4, 256, 'v beyond 2^30')[0] == 0
    # n <= 8192
    wide = [[0, 0, 0, 65536, 0, 0], [8192, 8192 * 65536, 0, 65536, 0, 0]]
    assert assert_columns(wide, 8192, 1, 'n = 8192')[0] == 8192
    wide[1][0] = 8193
    assert assert_columns(wide, 8192, 1, 'n = 8193')[0] == 0
    # through the float rule: a line whose corners lie beyond the range, and a strip row more than 64 pixels high
    far = C.box(float(1 << 23), 0, 20, 16)[None]
    assert S.spine_knots(far, 32, 2048, 0.0)[0] == 2 and S.spine_knots(far / 2, 32, 2048, 0.0)[0] == 0
    assert S.spine_knots(C.box(0, 0, 64, 64)[None], 1, 2048, 0.0)[0] == 2  # a knot's v = 64 px > h * (2^22 - 1)
    assert S.spine_knots(C.box(0, 0, 63.9, 63.9)[None], 1, 2048, 0.0)[0] == 0
    assert S.spine_knots(C.box(1e300, 0, 1e300, 1e300)[None], 8, 2048, 0.0)[0] == 2


def test_the_defined_search_on_hostile_knots():
    h = 8
    good = [[0, 0, 0, h * 65536, 0, 0], [5, 5 * 65536, 0, h * 65536, 0, 0], [9, 9 * 65536, 0, h * 65536, 0, 0],
            [20, 20 * 65536, 0, h * 65536, 0, 0]]
    assert assert_columns(good, 20, h, 'good')[0] == 20
    swapped = [good[0], good[2], good[1], good[3]]  # q = 0, 9, 5, 20: the search has one answer all the same
    valid, _ = assert_columns(swapped, 20, h, 'swapped')
    got = S.spine_columns_host(swapped, 20, h)
    assert valid == 20 and (got != NONE).all()
    for name, q in (('q_0 above 0', [3, 5, 9, 20]), ('q_last below w', [0, 5, 9, 15]), ('equal', [0, 5, 5, 20]),
                    ('falling', [20, 9, 5, 0]), ('huge', [0, 5, 1 << 62, 20]), ('negative', [-(1 << 62), 5, 9, 1 << 62]),
                    ('all minimum', [NONE] * 4), ('all maximum', [(1 << 63) - 1] * 4)):
        knots = [[v] + e[1:] for v, e in zip(q, good)]
        assert_columns(knots, 20, h, name)
    assert (S.spine_columns_host(good[:1], 5, h) == NONE).all() and (S.spine_columns_host(np.zeros((0, 6)), 5, h) == NONE).all()
    assert S.spine_columns_host(good, 0, h).shape == (0, 6)
    hostile = [[0, NONE, (1 << 63) - 1, NONE, (1 << 63) - 1, 7], [20, (1 << 63) - 1, NONE, 0, 0, 7]]
    assert assert_columns(hostile, 20, h, 'extreme words')[0] == 0


# ---- the rule's own decisions ----------------------------------------------------------------------------------------
def test_point_dropping_and_knot_dropping():
    one = C.box(10, 10, 20, 16)[None]
    st, p, H, sgn = S.spine_points(one, 0.0)
    assert st == 0 and H == 20 and sgn == 1 and p.tolist() == [[20, 10], [20, 18], [20, 26]]
    # a centre at most H/4 from the previously kept point or from the last point is dropped; the ends stay
    assert S.spine_points(C.box(10, 10, 20, 10)[None], 0.0)[1].tolist() == [[20, 10], [20, 20]]           # 5 = H/4 from both
    assert S.spine_points(C.box(10, 10, 20, 10.02)[None], 0.0)[1].tolist() == [[20, 10], [20, 15.01], [20, 20.02]]
    pair = np.stack([C.box(10, 10, 20, 16), C.box(10, 14, 20, 16)])  # centres 4 px apart: the second one goes
    assert S.spine_points(pair, 0.0)[1].tolist() == [[20, 10], [20, 18], [20, 30]]
    near_end = np.stack([C.box(10, 10, 20, 16), C.box(10, 30, 20, 8)])  # the last centre is 4 px from the end
    assert S.spine_points(near_end, 0.0)[1].tolist() == [[20, 10], [20, 18], [20, 38]]
    # the margin pushes the ends along the first and the last segment
    assert S.spine_points(one, 0.25)[1].tolist() == [[20, 5], [20, 18], [20, 31]]
    bent = np.stack([C.box(10, 10, 20, 16), C.rect(40.0, 40.0, 16, 20, -np.pi / 2)])  # the second one reads upwards
    p = S.spine_points(bent, 0.5)[1]
    assert np.allclose(p[0], [20, 0]) and np.allclose(p[-1], [22, 40]) and len(p) == 4
    assert S.spine_points(one[:, [1, 0, 3, 2]], 0.0)[3] == -1
    # knots on one column merge; an interior knot on the last column goes
    st, sq, w, knots, _ = S.spine_knots(P.straight(12), 20, 6, 0.0)
    assert (st, sq, w) == (0, True, 6) and knots[:, 0].tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert S.spine_knots(P.straight(12), 20, 3, 0.0)[0] == 2  # 64 px per column: a step beyond 2^22 - 1
    st, sq, w, knots, _ = S.spine_knots(P.straight(3), 20, 1, 0.0)
    assert (st, sq, w) == (0, True, 1) and knots[:, 0].tolist() == [0, 1]
    assert S.spine_columns_host(knots, 1, 20)[0, 3:6:2].tolist() == [0, 48 * 65536]  # one column: the whole line per step
    # the down vector turns with the line: perpendicular to the neighbours' chord
    st, _, _, knots, _ = S.spine_knots(P.arc(), 32, 2048, 0.125)
    c, v = knots[:, 1:3].astype(float), knots[:, 3:5].astype(float)
    chord = c[2:] - c[:-2]
    assert np.abs((chord * v[1:-1]).sum(axis=1) / np.hypot(*chord.T) / np.hypot(*v[1:-1].T)).max() < 1e-4
    assert np.abs(np.hypot(*v.T) / 65536 - 25).max() < 1e-4


def test_statuses_widths_and_log2n():
    ok = C.box(5, 7, 8, 20)
    bad, inf = ok.copy(), ok.copy()
    bad[2, 1], inf[0, 0] = np.nan, np.inf
    for quads, status in ((ok[None], 0), (bad[None], 1), (inf[None], 1), (np.stack([ok, bad]), 1), (np.zeros((0, 4, 2)), 1),
                          (C.box(5, 7, 0.05, 8)[None], 1), (C.box(5, 7, 1 / 16, 1 / 16)[None], 0), (C.box(5, 7, 8, 0.05)[None], 1),
                          (np.zeros((1, 4, 2)), 1), (np.stack([C.box(5, 7, 8, 0.01), C.box(5, 7.01, 8, 0.01)]), 1)):
        assert S.spine_knots(quads, 8, 2048, 0.0)[0] == status
    line = P.straight(12)
    for width_max, w, squeezed in ((2048, 192, False), (192, 192, False), (191, 191, True), (20, 20, True)):
        st, sq, got, knots, _ = S.spine_knots(line, 20, width_max, 0.0)
        assert (st, sq, got) == (0, squeezed, w) and knots[0, 0] == 0 and knots[-1, 0] == w and (np.diff(knots[:, 0]) > 0).all()
    assert S.spine_knots(C.box(2, 3, 8, 0.2)[None], 8, 2048, 0.0)[1:3] == (False, 1)  # w_nat = 0: one column
    assert S.spine_knots(line, 25, 2048, 0.125)[2] == 197                             # (192 + 2 * 2.5) * 25 / 25
    for height, want in ((8, 0), (16, 1), (32, 2), (33, 3), (100, 3)):
        assert S.spine_knots(C.box(1, 2, height, 3 * height)[None], 8, 2048, 0.0)[4] == want, height
    assert S.spine_knots(line, 20, 48, 0.0)[4] == 2  # squeezed four times along the line
    for scale, want in ((1, 0), (2, 1), (4, 2), (8, 3)):
        assert S.spine_knots(P.arc(scale=scale), 32, 2048, 0.125)[4] == want


def layout_scene():
    lengths = [9, 4, 8, 12, 3, 13]
    return lengths, [C.box(1, 2, 8, n)[None] for n in lengths]


def test_slots_buckets_and_the_table():
    lengths, lines = layout_scene()
    img = C.picture((40, 60), 11)
    layout = S.spine_rows([lines[:4], lines[4:]], 8, 2048, 4, 0.0)
    quads = Q.strip_rows([np.concatenate(lines[:4]), np.concatenate(lines[4:])], 8, 2048, 4, 0.0)
    for name in ('image', 'status', 'squeezed', 'widths', 'bucket', 'index', 'bucket_shapes', 'out_bytes'):
        a, b = getattr(layout, name), getattr(quads, name)
        assert np.array_equal(a, b) and type(a) is type(b), name
    assert np.array_equal(layout.rows[:, :4], quads.rows[:, :4]), 'src, offset, slot_w, w as for the straight strips'
    assert layout.rows[:, 6].tolist() == [0, 9, 13, 21, 33, 36] and layout.columns == sum(lengths)
    assert layout.rows[:, 5].tolist() == [3, 2, 3, 3, 2, 3] and layout.rows[:, 4].tolist() == [0, 3, 5, 8, 11, 13]
    assert len(layout.knots) == 16 and not layout.rows[:, 8:].any()
    sources = [[0, 40, 60, 0], [0, 40, 60, 0]]
    S.check_spine_rows(layout.rows, layout.knots, sources, 8, layout.out_bytes, layout.columns)
    table = S.spine_table(layout.rows, layout.knots, 8)
    assert table[:72].reshape(6, 12).tolist() == layout.rows.tolist() and table[72:79].tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert table[79:].reshape(-1, 6).tolist() == layout.knots.tolist()
    assert np.array_equal(table[:79], Q.strip_table(layout.rows, 8)), 'the rows and tiles of strip_table'
    strips = S.spine_strips_host([img, img], [lines[:4], lines[4:]], 8, 2048, 4, 0.0)
    assert [b.shape for b in strips.buckets] == layout.bucket_shapes and strips.height == 8
    for k, n in enumerate(lengths):
        if n % 2 == 0:  # the middle knot of an odd width sits half a column off: no plain slice
            assert np.array_equal(strips.strip(k), img[1:9, 2:2 + n])
        assert not strips.buckets[strips.bucket[k]][strips.index[k]][:, n:].any(), 'the columns beyond w are zero'
        assert strips.spine(k).shape == (layout.rows[k, 5], 2, 2) and strips.spine(k)[0].tolist() == [[5.0, 2.0], [8.0, 0.0]]
    assert strips.buckets[0].base is strips.buckets[3].base is not None, 'one allocation'
    mixed = S.spine_strips_host([img], [[lines[0][0], np.full((1, 4, 2), np.nan), lines[1][0]]], 8, 2048, 4, 0.0)
    assert mixed.status.tolist() == [0, 1, 0] and np.array_equal(mixed.strip(2), img[1:9, 2:6])
    with pytest.raises(ValueError):
        mixed.strip(1)
    with pytest.raises(ValueError):
        mixed.spine(1)
    empty = S.spine_rows([[]], 8, 2048, 4, 0.0)
    assert empty.rows.shape == (0, 12) and empty.knots.shape == (0, 6) and empty.out_bytes == 0 and empty.columns == 0
    assert S.spine_table(empty.rows, empty.knots, 8).tolist() == [0]
    with pytest.raises(ValueError):
        S.spine_strips_host([img, img], [lines])
    with pytest.raises(ValueError):
        S.spine_rows([lines], 0)


def test_the_pixels_are_warp_hosts_column_by_column():
    quads, img = P.arc(scale=0.5, centre=(8.0, 8.0)), C.picture((130, 130), 3)
    seen = set()
    for h in (32, 8, 5, 3):
        layout = S.spine_rows([[quads]], h, 2048, 16, 0.125)
        want_log2n = int(layout.rows[0, 7])
        seen.add(want_log2n)
        w = int(layout.rows[0, 3])
        cols = S.spine_columns_host(layout.knots, w, h)
        got = S.spine_pixels_host(img, cols, h, want_log2n)
        for j in range(0, w, 7):
            col = warp_host(img, [[0, 0, h, 1] + cols[j].tolist() + [want_log2n, 0]], np.zeros((h, 1, 3), np.uint8))
            assert np.array_equal(got[:, j], col[:, 0]), (h, j)
    assert seen == {0, 1, 2, 3}
    cols[3] = NONE
    assert not S.spine_pixels_host(img, cols, h, 3)[:, 3].any() and S.spine_pixels_host(img, cols, h, 3)[:, 4].any()


def test_check_spine_rows_rejects():
    _, lines = layout_scene()
    layout = S.spine_rows([lines], 8, 2048, 4, 0.0)
    sources, rows, knots, size, columns = [[0, 40, 60, 0]], layout.rows, layout.knots, layout.out_bytes, layout.columns
    assert np.array_equal(S.check_spine_rows(rows, knots, sources, 8, size, columns), rows)

    def bad(col, value, row=0, knot=None, **kw):
        r, t = rows.copy(), knots.copy()
        if knot is None:
            r[row, col] = value
        else:
            t[knot, col] = value
        with pytest.raises(ValueError):
            S.check_spine_rows(r, t, kw.get('sources', sources), kw.get('h', 8), kw.get('size', size), kw.get('columns', columns))

    bad(1, rows[3, 1])             # two rows on one slot
    bad(1, rows[3, 1] - 1)         # overlap by a byte
    bad(1, -1)
    bad(1, size - 10)
    bad(3, 13)                     # w > slot_w
    bad(3, 0)
    bad(3, 10)                     # q_last != w
    bad(2, 8196)
    bad(0, 1)
    bad(0, -1)
    bad(7, 4)
    bad(7, -1)
    bad(4, -1)                     # knot_start / knots outside the knot table
    bad(4, 14)
    bad(5, 1)
    bad(5, 17)
    bad(5, 2)                      # fewer knots: q_last != w
    bad(4, 3, row=2)               # another row's knots: q_last != w
    bad(6, -1)                     # columns outside the workspace, or shared
    bad(6, columns - 8)
    bad(6, 1)
    bad(0, 1, knot=0)              # q_0 != 0
    bad(0, 10, knot=2)             # q_last != w
    bad(0, 9, knot=1)              # not strictly increasing
    bad(0, 0, knot=1)
    for kw in (dict(size=size - 1), dict(h=9), dict(h=0), dict(columns=columns - 1), dict(sources=[[0, 40, 32769, 0]]),
               dict(sources=[[-1, 40, 60, 0]])):
        bad(0, 0, **kw)
    for r, t in ((rows.astype(np.float64), knots), (rows[:, :11], knots), (rows, knots[:, :5]), (rows, knots.astype(np.float32))):
        with pytest.raises(ValueError):
            S.check_spine_rows(r, t, sources, 8, size, columns)
