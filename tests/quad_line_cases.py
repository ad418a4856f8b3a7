"""Shared inputs and restatements of the text-line tests (test_cpu_quad_lines.py, test_gpu_quad_lines.py,
test_gpu_quad_lines_infer.py): straight-line layouts with their true partition and order; raw-row cases for what valid
quads do not reach; the grouping restated as label-minimum rounds with positions by counting, written apart from
inferencing/lines.py."""
from functools import lru_cache

import numpy as np

from vkit_ocr_model_adaptive_scaling_amd.inferencing import evaluation as E
from vkit_ocr_model_adaptive_scaling_amd.inferencing import lines as L

SQ = lambda y, x, h, w: [[y, x], [y, x + w], [y + h, x + w], [y + h, x]]  # up-left, up-right, down-right, down-left

CJK = dict(height=30.0, width=30.0, pitch=33.0, leading=42.0)
LATIN = dict(height=30.0, width=16.0, pitch=19.0, leading=42.0)
ANGLES = (0.0, 0.35, 1.57, 3.0)


# ---- layouts ---------------------------------------------------------------------------------------------------------

def layout(n_lines, n_chars, height, width, pitch, leading, word_space=0.0, word=5, angle=0.0, seed=0, jitter=1.0,
           scramble=True):
    """``n_lines`` straight lines of ``n_chars`` characters: character c of a line stands ``c * pitch + (c // word) *
    word_space`` along it, the lines ``leading`` apart, the page centred on the origin and turned by ``angle`` (rad).  Jitter
    from a seeded generator, in proportion to the height: centres by up to 2 %, sizes by up to 3 %, each character's own
    angle by up to 0.02 rad.  The index order is scrambled.  -> ``(quads (n, 4, 2) float64 (y, x), truth)`` with ``truth`` the
    lines as lists of indices in reading order, ordered by their smallest member as the rule numbers them."""
    rng = np.random.default_rng(seed)
    n = n_lines * n_chars
    c = np.arange(n) % n_chars
    along = c * pitch + (c // word) * word_space
    down = (np.arange(n) // n_chars) * leading
    cy, cx = down - down.mean(), along - along.mean()
    cy = cy + jitter * rng.uniform(-0.02, 0.02, n) * height
    cx = cx + jitter * rng.uniform(-0.02, 0.02, n) * height
    h = height * (1 + jitter * rng.uniform(-0.03, 0.03, n))
    w = width * (1 + jitter * rng.uniform(-0.03, 0.03, n))
    own = jitter * rng.uniform(-0.02, 0.02, n)
    base = np.stack([np.stack([-h / 2, -w / 2], 1), np.stack([-h / 2, w / 2], 1), np.stack([h / 2, w / 2], 1),
                     np.stack([h / 2, -w / 2], 1)], axis=1)                                     # (n, 4, 2)

    def turn(p, t):  # (y, x): clockwise with y down stays clockwise
        t = np.broadcast_to(t, p.shape[:-1])
        return np.stack([p[..., 0] * np.cos(t) + p[..., 1] * np.sin(t), -p[..., 0] * np.sin(t) + p[..., 1] * np.cos(t)], -1)

    quads = turn(base, own[:, None]) + np.stack([cy, cx], 1)[:, None, :]
    quads = turn(quads, angle)
    perm = rng.permutation(n) if scramble else np.arange(n)
    at = np.empty(n, np.int64)
    at[perm] = np.arange(n)              # the character that was o stands at index at[o]
    truth = [[int(at[l * n_chars + k]) for k in range(n_chars)] for l in range(n_lines)]
    return quads[perm], sorted(truth, key=min)


def split_words(truth, word=5):
    """the truth of a layout whose lines fall apart at the word spaces"""
    return sorted([ln[k:k + word] for ln in truth for k in range(0, len(ln), word)], key=min)


def table_of(quads, K=None, count=None):
    """quads of one image -> ``(rows (1, K, 16), count (1,))`` through ``match_rows``, every quad valid"""
    rows, ok = E.match_rows(quads)
    assert ok.all()
    K = len(rows) if K is None else K
    out = np.zeros((1, max(K, 1), 16), np.int32)
    out[0, :len(rows)] = rows
    return out, np.array([len(rows) if count is None else count], np.int32)


def spread(quads, at, K):
    """the quads at the given indices of a (1, K, 16) table, zero (invalid) rows everywhere else, count = K"""
    rows, ok = E.match_rows(quads)
    assert ok.all() and len(set(at)) == len(at) == len(rows)
    out = np.zeros((1, K, 16), np.int32)
    out[0, list(at)] = rows
    return out, np.array([K], np.int32)


def stack_tables(tables):
    """(rows (1, K_b, 16), count (1,)) tables -> one (B, K, 16) table with K the largest"""
    K = max(t[0].shape[1] for t in tables)
    rows = np.zeros((len(tables), K, 16), np.int32)
    for b, (r, _) in enumerate(tables):
        rows[b, :r.shape[1]] = r[0]
    return rows, np.array([int(t[1][0]) for t in tables], np.int32)


def truth_outputs(rows, count, truth):
    """the four outputs that a (1, K, 16) table must give if its lines are ``truth`` (the table rows from the rule's sums,
    restated here on Python integers)"""
    K = rows.shape[1]
    n = min(max(int(count[0]), 0), K)
    line, order = np.full((1, K), -1, np.int32), np.full((1, K), -1, np.int32)
    table = np.zeros((1, K, 8), np.int64)
    at = 0
    for l, mem in enumerate(truth):
        P = [[(int(rows[0, m, 2 * k]), int(rows[0, m, 2 * k + 1])) for k in range(4)] for m in mem]
        U = [sum(p[1][c] + p[2][c] - p[0][c] - p[3][c] for p in P) for c in (0, 1)]
        U = [0, 16] if U == [0, 0] else U
        a = [y * U[0] + x * U[1] for p in P for y, x in p]
        b = [y * U[1] - x * U[0] for p in P for y, x in p]
        line[0, mem] = l
        order[0, at:at + len(mem)] = mem
        table[0, l] = (at, len(mem), U[0], U[1], min(a), max(a), min(b), max(b))
        at += len(mem)
    return line, order, table, n


# ---- the grouping, restated ------------------------------------------------------------------------------------------

def lines_by_rounds(rows, part, li, lj):
    """``lines_of_links`` written differently: every quad starts with its own index as label, a round gives both ends of
    every link the smaller of their labels as the round before left them, until nothing changes; lines are numbered by
    counting the smaller labels that are their own; a member's place is the number of members with a smaller (k, m)."""
    n = len(part)
    r = np.asarray(rows, dtype=np.int64).reshape(-1, 16)
    label = list(range(n))
    while True:
        new = list(label)
        for a, b in zip(li, lj):
            new[a] = min(new[a], label[b])
            new[b] = min(new[b], label[a])
        if new == label:
            break
        label = new
    own = [m for m in range(n) if part[m] and label[m] == m]
    line = np.array([sum(o < label[m] for o in own) if part[m] else -1 for m in range(n)], np.int32)
    order, table = [-1] * int(np.sum(part)), []
    start = 0
    for l in range(len(own)):
        mem = [m for m in range(n) if line[m] == l]
        Uy = sum(int(r[m, 2] + r[m, 4] - r[m, 0] - r[m, 6]) for m in mem)
        Ux = sum(int(r[m, 3] + r[m, 5] - r[m, 1] - r[m, 7]) for m in mem)
        if Uy == 0 and Ux == 0:
            Ux = 16
        k = {m: int(r[m, 0:8:2].sum()) * Uy + int(r[m, 1:8:2].sum()) * Ux for m in mem}
        for m in mem:
            order[start + sum((k[o], o) < (k[m], m) for o in mem)] = m
        a = [int(r[m, 2 * c]) * Uy + int(r[m, 2 * c + 1]) * Ux for m in mem for c in range(4)]
        b = [int(r[m, 2 * c]) * Ux - int(r[m, 2 * c + 1]) * Uy for m in mem for c in range(4)]
        table.append([start, len(mem), Uy, Ux, min(a), max(a), min(b), max(b)])
        start += len(mem)
    return line, order, table


# ---- raw-row cases: name -> (rows (K, 16), count, line, order, table rows, stats) ---------------------------------------

def _rows(quads):
    rows, ok = E.match_rows(np.array(quads, dtype=np.float64))
    assert ok.all()
    return rows


def hand_cases():
    cases = {}
    # 30 x 16 boxes 19 apart: a line of three; the fourth stands 100 px below, alone
    abc = _rows([SQ(0, 0, 30, 16), SQ(0, 19, 30, 16), SQ(0, 38, 30, 16), SQ(100, 0, 30, 16)])
    U3, U1 = 3 * 32 * 16, 32 * 16  # u = (0, 2 w) in Q4
    cases['three_and_one'] = (abc, 4, [0, 0, 0, 1], [0, 1, 2, 3],
                              [[0, 3, 0, U3, 0, 54 * 16 * U3, 0, 30 * 16 * U3], [3, 1, 0, U1, 0, 16 * 16 * U1, 1600 * U1, 2080 * U1]],
                              [4, 4, 3, 2])
    # exact ties of k: 1 and 2 share their centre's x (6 px apart in y, linked), so the index decides; 3 is 1 once more
    ties = _rows([SQ(0, 19, 30, 16), SQ(-3, 0, 30, 16), SQ(3, 0, 30, 16), SQ(-3, 0, 30, 16), SQ(0, -19, 30, 16)])
    cases['ties'] = (ties, 5, [0] * 5, [4, 1, 2, 3, 0], None, [5, 5, 10, 1])
    # a row with valid = 0 inside the count takes no part: its corners would bridge 0 and 2, which are 60 px apart (no link)
    gap = _rows([SQ(0, 0, 30, 16), SQ(0, 30, 30, 16), SQ(0, 60, 30, 16), SQ(100, 0, 30, 16)])
    gap[1, 14] = 0
    cases['invalid_inside'] = (gap, 4, [0, -1, 1, 2], [0, 2, 3, -1], None, [4, 3, 0, 3])
    wide = abc.copy()
    wide[1, 14] = -7  # valid is any non-zero word
    cases['valid_is_any_nonzero_word'] = (wide, 4, [0, 0, 0, 1], [0, 1, 2, 3], None, [4, 4, 3, 2])
    # rows beyond the count would link if they were read
    cases['beyond_the_count'] = (abc, 2, [0, 0, -1, -1], [0, 1, -1, -1], None, [2, 2, 1, 1])
    cases['count_zero'] = (abc, 0, [-1] * 4, [-1] * 4, [], [0, 0, 0, 0])
    # the second row is the first mirrored left to right (ul <-> ur, dl <-> dr): v is the same, u the opposite, so U = (0, 0)
    # becomes (0, 16); no valid quad has this winding, the row's valid word is set by hand
    mirror = _rows([SQ(0, 0, 30, 16), SQ(0, 19, 30, 16)])
    mirror[1, 0:8] = mirror[1, [2, 3, 0, 1, 6, 7, 4, 5]]
    cases['u_cancels'] = (mirror, 2, [0, 0], [0, 1], [[0, 2, 0, 16, 0, 35 * 16 * 16, 0, 30 * 16 * 16]], [2, 2, 1, 1])
    # upside down against its neighbour: v_i . v_j < 0
    flip = _rows([SQ(0, 0, 30, 16), SQ(0, 19, 30, 16)])
    flip[1, 0:8] = flip[1, [4, 5, 6, 7, 0, 1, 2, 3]]
    cases['opposite_v'] = (flip, 2, [0, 1], [0, 1], None, [2, 2, 0, 2])
    return cases


# ---- threshold cases: two axis-aligned boxes at exact Q4 distances ---------------------------------------------------------

def pair_rows(dy_q4, dx_q4, h0=32, w0=16, h1=32, w1=16):
    """two boxes with Q4-exact sizes in pixels (so v = (2 h 16, 0)) whose centres differ by exactly (dy_q4, dx_q4) / 16 px"""
    a = np.array(SQ(-h0 / 2, -w0 / 2, h0, w0), np.float64)
    b = np.array(SQ(-h1 / 2, -w1 / 2, h1, w1), np.float64) + np.array([dy_q4, dx_q4]) / 16.0
    return _rows([a, b])


# ---- shared references -----------------------------------------------------------------------------------------------

@lru_cache(maxsize=None)
def big_reference(kind):
    """the K = 8192 tables and the oracle's answers on them, computed once and shared: do not modify.  ``one_line``: 8192
    characters 6 x 3 px at pitch 4 in one straight line (the page is 32768 px wide, inside the coordinate range);
    ``singles``: 8192 characters on a 20 px grid."""
    if kind == 'one_line':
        quads, truth = layout(1, 8192, 6.0, 3.0, 4.0, 10.0, seed=11)
    else:
        quads, truth = layout(8192, 1, 6.0, 4.0, 0.0, 0.0, seed=12)
        k = np.arange(8192)
        quads = quads + np.stack([20.0 * (k // 91), 20.0 * (k % 91)], 1)[:, None, :] - 900.0
        truth = [[m] for m in range(8192)]
    rows, count = table_of(quads)
    return (rows, count), L.quad_lines_host(rows, count), truth
