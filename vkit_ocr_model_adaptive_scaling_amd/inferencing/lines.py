"""Grouping character quadrilaterals into text lines: the rule, its host oracle, the device route and the step that ``infer`` /
``infer_batch`` apply to a result.

The rule is THIS PROJECT'S OWN, stated in integers on the match rows of inferencing/evaluation.py so that the device kernels
(csrc/quadlines.hip) and the host oracle are held to each other for equality.

Inputs, per image: K match rows (``match_rows`` / ``ops.quad_rows``: 16 int32, corners ``P0..P3`` as Q4 ``(y, x)`` in the order
ul, ur, dr, dl), ``count`` clamped to [0, K], and three parameters as Q4 integers: ``gap_q4`` in 1..4096, ``cross_q4`` in
1..4096, ``ratio_q4`` in 16..256.  The public functions take floats and convert with ``rint(x * 16)``; the defaults are 1.5, 0.5
and 2.0, and a value outside its range raises.  A row TAKES PART iff it lies within the count and its ``valid`` word is set.
Every field is used as it stands in the row.

Per quad (int64): ``s = P0 + P1 + P2 + P3`` (four times the centre); ``v = (P3 + P2) - (P0 + P1)`` (down the character: twice
the vector from the top edge's midpoint to the bottom edge's midpoint); ``u = (P1 + P2) - (P0 + P3)`` (along the reading
direction); ``vv = v.v``.  For a valid row ``vv > 0`` (a strictly convex quad's edge midpoints differ) and every component of
``s``, ``v`` and ``u`` is at most 2^21 in magnitude, since ``|P| <= COORD_MAX = 2^19``.

Link: for i != j, both taking part, with ``d = s_j - s_i``, the quads are linked iff all of

* for a in {i, j}: ``8 * |d.v_a| <= cross_q4 * vv_a`` - the other's centre lies within ``cross_q4 / 16`` heights of a's mid-line
  (``d`` is four centres' difference and ``v`` two heights, so ``|d.v| / vv`` is twice the offset in heights);
* for a in {i, j}: ``8 * |d_y * v_a,x - d_x * v_a,y| <= gap_q4 * vv_a`` - and within ``gap_q4 / 16`` heights along it;
* ``256 * vv_i <= ratio_q4^2 * vv_j`` and the same with i and j swapped - the heights differ by at most ``ratio_q4 / 16``;
* ``v_i.v_j > 0`` - the two point the same way.

The relation is symmetric.  Bounds: ``|d| <= 2^22`` per component, so ``|d.v|`` and the cross product stay below 2^45 and
eight times them below 2^48; ``vv <= 2^43``, so ``cross_q4 * vv`` and ``gap_q4 * vv`` stay at or below 2^55, ``256 * vv`` at or
below 2^51 and ``ratio_q4^2 * vv`` at or below 2^59: every product stays below 2^60 (tests/test_cpu_quad_lines.py checks them
with corners at +-COORD_MAX against Python integers).

Lines: a line is a connected component of the link graph over the quads that take part; lines are numbered from 0 in
ascending order of their smallest member index; a quad that takes part but has no link is a line of one.

Reading order, per line: ``U = sum of u_m`` over its members (int64); if ``U == (0, 0)`` then ``U = (0, 16)``.  ``k_m = s_m.U``
and the members are listed in ascending ``(k_m, m)``.  ``|U| <= 8192 * 2^21 = 2^34`` per component, ``|k| <= 2^56``.

Extent, per line: with ``a(P) = P_y*U_y + P_x*U_x`` and ``b(P) = P_y*U_x - P_x*U_y``, ``a_min, a_max, b_min, b_max`` over all
four corners of all members; magnitudes stay at or below 2^54.

Outputs, per image: ``line`` (K,) int32, the line number, or -1 for a row that takes no part or lies beyond the count;
``order`` (K,) int32, the member indices line after line in reading order, -1 beyond the ``n_part`` entries; ``table`` (K, 8)
int64 rows ``start, size, U_y, U_x, a_min, a_max, b_min, b_max`` for lines 0..L-1 and zero rows after them (K rows is the
exact worst case: there is no overflow path); ``stats`` (4,) int64 = ``n, n_part, links, lines`` with ``links`` counting pairs
i < j.

Line quadrilaterals: ``line_quads(table)`` runs on the host, on the table rows only (as ``region_scales`` does), and gives the
oriented rectangle of each line as (4, 2) float64 ``(y, x)`` in pixels, corners ul, ur, dr, dl = ``(a_min, b_min)``, ``(a_max,
b_min)``, ``(a_max, b_max)``, ``(a_min, b_max)``, the point for ``(a, b)`` being ``((a*U_y + b*U_x) / UU, (a*U_x - b*U_y) / UU) /
16``, computed exactly and rounded once.  Whenever it has area the rectangle is a strictly convex clockwise quad, so it can
go into ``evaluate_quads`` and ``evaluate_quads_ranked`` as it is; line-level scoring itself stays out of scope.

Differences from common practice: the test is mutual - both characters' frames must agree; units are character heights,
not widths, because narrow glyphs have no useful width; the scope is the image, not the rough region (a region merges
touching lines, splits a line at a wide gap and carries no order); words and lines differ only by ``gap``; a curved line
gets the rectangle of its chord direction."""
from typing import List, Sequence, Tuple

import attrs
import numpy as np
import torch

from .evaluation import ROW_VALID, ROW_WORDS, fitting_quads, match_rows
from .quad_tables import capacity, clamped, host_table, pad_quads, pad_rows, quad_lists, require_gpu

GAP_RANGE, CROSS_RANGE, RATIO_RANGE = (1, 4096), (1, 4096), (16, 256)
TABLE_WORDS, STATS_WORDS = 8, 4
_BLOCK = 256  # rows of i per vectorised step of the oracle's pair test


def line_params(gap: float = 1.5, cross: float = 0.5, height_ratio: float = 2.0) -> Tuple[int, int, int]:
    """The three parameters as Q4 integers ``(gap_q4, cross_q4, ratio_q4)``: ``rint(x * 16)``, each within its range or a
    ValueError."""
    out = []
    for name, x, (lo, hi) in (('gap', gap, GAP_RANGE), ('cross', cross, CROSS_RANGE), ('height_ratio', height_ratio, RATIO_RANGE)):
        x = float(x)
        q = np.rint(x * 16.0)
        if not (q >= lo and q <= hi):  # NaN compares false
            raise ValueError(f'{name} = {x} must lie in [{lo / 16}, {hi / 16}] (Q4 {lo}..{hi})')
        out.append(int(q))
    return tuple(out)


def quad_frames(rows) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(n, 16) rows -> ``(s (n, 2), v (n, 2), u (n, 2), vv (n,))`` int64, the per-quad quantities of the rule."""
    p = np.asarray(rows, dtype=np.int64).reshape(-1, ROW_WORDS)[:, :8].reshape(-1, 4, 2)
    s = p[:, 0] + p[:, 1] + p[:, 2] + p[:, 3]
    v = (p[:, 3] + p[:, 2]) - (p[:, 0] + p[:, 1])
    u = (p[:, 1] + p[:, 2]) - (p[:, 0] + p[:, 3])
    return s, v, u, (v * v).sum(axis=1)


def link_pairs(rows, gap_q4: int, cross_q4: int, ratio_q4: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """One image, already cut to its count: ``(part (n,) bool, i, j)`` - the rows that take part and the linked pairs i < j,
    i-major ascending.  All pairs are tested, ``_BLOCK`` rows of i at a time."""
    r = np.asarray(rows, dtype=np.int64).reshape(-1, ROW_WORDS)
    n = len(r)
    part = r[:, ROW_VALID] != 0
    s, v, _, vv = quad_frames(r)
    r2 = int(ratio_q4) * int(ratio_q4)
    li, lj = [], []
    idx = np.arange(n)
    for lo in range(0, n, _BLOCK):
        hi = min(lo + _BLOCK, n)
        c0 = lo + 1                                                             # j > i: the columns from lo + 1 on
        dy, dx = s[None, c0:, 0] - s[lo:hi, None, 0], s[None, c0:, 1] - s[lo:hi, None, 1]  # [i, j] = s_j - s_i
        along_i = np.abs(dy * v[lo:hi, None, 1] - dx * v[lo:hi, None, 0])
        hit = (8 * along_i <= gap_q4 * vv[lo:hi, None]) & part[lo:hi, None] & part[None, c0:] & (idx[None, c0:] > idx[lo:hi, None])
        i, j = np.nonzero(hit)
        i += lo
        j += c0
        dd = s[j] - s[i]
        ok = 8 * np.abs(dd[:, 0] * v[j, 1] - dd[:, 1] * v[j, 0]) <= gap_q4 * vv[j]
        ok &= 8 * np.abs((dd * v[i]).sum(axis=1)) <= cross_q4 * vv[i]
        ok &= 8 * np.abs((dd * v[j]).sum(axis=1)) <= cross_q4 * vv[j]
        ok &= (256 * vv[i] <= r2 * vv[j]) & (256 * vv[j] <= r2 * vv[i])
        ok &= (v[i] * v[j]).sum(axis=1) > 0
        li.append(i[ok])
        lj.append(j[ok])
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros((0,), np.int64)
    return part, cat(li), cat(lj)


def _components(n: int, i: Sequence[int], j: Sequence[int]) -> List[int]:
    """union-find over the links -> the root (smallest member) of every index"""
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b in zip(i, j):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return [find(a) for a in range(n)]


def lines_of_links(rows, part, li, lj):
    """One image cut to its count, its taking-part mask and its links -> ``(line (n,) int32, order list, table rows list)``
    by the sequential form: union-find, lines numbered by their smallest member, members sorted by ``(k, m)``."""
    n = len(part)
    s, _, u, _ = quad_frames(rows)
    p = np.asarray(rows, dtype=np.int64).reshape(-1, ROW_WORDS)[:, :8].reshape(-1, 4, 2)
    root = _components(n, li.tolist(), lj.tolist())
    line = np.full((n,), -1, dtype=np.int32)
    members: List[List[int]] = []
    number = {}
    for m in range(n):
        if not part[m]:
            continue
        if root[m] not in number:  # ascending m: a root is its line's smallest member, so lines come in that order
            number[root[m]] = len(members)
            members.append([])
        line[m] = number[root[m]]
        members[line[m]].append(m)
    order, table = [], []
    for mem in members:
        U = [int(u[mem, 0].sum()), int(u[mem, 1].sum())]
        if U == [0, 0]:
            U = [0, 16]
        key = {m: int(s[m, 0]) * U[0] + int(s[m, 1]) * U[1] for m in mem}
        mem = sorted(mem, key=lambda m: (key[m], m))
        a = [int(c[0]) * U[0] + int(c[1]) * U[1] for m in mem for c in p[m]]
        b = [int(c[0]) * U[1] - int(c[1]) * U[0] for m in mem for c in p[m]]
        table.append([len(order), len(mem), U[0], U[1], min(a), max(a), min(b), max(b)])
        order += mem
    return line, order, table


def quad_lines_host(rows, count, gap: float = 1.5, cross: float = 0.5, height_ratio: float = 2.0):
    """The oracle of ``ops.quad_lines``: ``rows`` (B, K, 16), ``count`` (B,) -> ``(line (B, K) int32, order (B, K) int32, table
    (B, K, 8) int64, stats (B, 4) int64)`` as the rule states them.  Every field of a row is used as it is, as on the
    device."""
    q = line_params(gap, cross, height_ratio)
    (rows, count, _), B, K = host_table(rows, count)
    line = np.full((B, K), -1, dtype=np.int32)
    order = np.full((B, K), -1, dtype=np.int32)
    table = np.zeros((B, K, TABLE_WORDS), dtype=np.int64)
    stats = np.zeros((B, STATS_WORDS), dtype=np.int64)
    for b in range(B):
        n = clamped(count[b], K)
        part, li, lj = link_pairs(rows[b, :n], *q)
        ln, od, tb = lines_of_links(rows[b, :n], part, li, lj)
        line[b, :n] = ln
        order[b, :len(od)] = od
        if tb:
            table[b, :len(tb)] = np.array(tb, dtype=np.int64)
        stats[b] = (n, int(part.sum()), len(li), len(tb))
    return line, order, table, stats


def line_quads(table) -> np.ndarray:
    """Table rows (L, 8) int64 ``start, size, U_y, U_x, a_min, a_max, b_min, b_max`` -> (L, 4, 2) float64 ``(y, x)`` pixels: the
    oriented rectangle of each line, corners ul, ur, dr, dl, each coordinate the exact quotient rounded once (Python
    integers; their true division is correctly rounded).  A row without members (size 0) gives zeros."""
    t = np.asarray(table, dtype=np.int64).reshape(-1, TABLE_WORDS)
    out = np.zeros((len(t), 4, 2), dtype=np.float64)
    for l, (_, size, uy, ux, a0, a1, b0, b1) in enumerate(t.tolist()):
        den = 16 * (uy * uy + ux * ux)
        if size <= 0 or den == 0:
            continue
        for c, (a, b) in enumerate(((a0, b0), (a1, b0), (a1, b1), (a0, b1))):
            out[l, c, 0] = (a * uy + b * ux) / den
            out[l, c, 1] = (a * ux - b * uy) / den
    return out


@attrs.define
class QuadLinesResult:
    """One image of ``quad_lines``; indices are those of the image's own array."""
    line: np.ndarray          # (n,) int32: the line of each quad, -1 for one that takes no part
    lines: List[np.ndarray]   # L int32 index arrays, each in reading order
    polygons: np.ndarray      # (L, 4, 2) float64 (y, x) pixels: ``line_quads``
    valid: np.ndarray         # (n,) bool: the rule's validity


def _line_results(counts, valid, line, order, table, stats):
    results = []
    for b, n in enumerate(int(c) for c in counts):
        L = int(stats[b, 3])
        t = table[b, :L]
        lines = [order[b, int(s):int(s) + int(k)].astype(np.int32) for s, k in t[:, :2].tolist()]
        results.append(QuadLinesResult(line[b, :n].astype(np.int32), lines, line_quads(t), np.asarray(valid[b], dtype=bool)))
    return results, (stats.sum(axis=0) if len(stats) else np.zeros((STATS_WORDS,), np.int64))


def quad_lines_lists_host(quads: Sequence, gap: float = 1.5, cross: float = 0.5, height_ratio: float = 2.0):
    """What ``quad_lines`` returns, through ``match_rows`` and ``quad_lines_host``: the slow route, for checks and for timing
    against."""
    q = quad_lists(quads)
    line_params(gap, cross, height_ratio)
    tabs = [match_rows(a) for a in q]
    rows, count = pad_rows([r for r, _ in tabs])
    if len(q) == 0:
        return [], np.zeros((STATS_WORDS,), np.int64)
    return _line_results(count, [v for _, v in tabs], *quad_lines_host(rows, count, gap, cross, height_ratio))


def quad_lines(quads: Sequence, gap: float = 1.5, cross: float = 0.5, height_ratio: float = 2.0, device='cuda'):
    """Groups character quads into text lines on the device.  ``quads`` is a list with one (n, 4, 2) ``(y, x)`` array per
    image.  The padded quads and the counts go up in one buffer, ``ops.quad_rows`` and ``ops.quad_lines`` are called once and
    their outputs come back in one buffer.  Returns ``(per-image QuadLinesResult list, stats (4,) int64 summed over the
    images: n, n_part, links, lines)``."""
    from .. import ops
    device = require_gpu('quad_lines', device, 'quad_lines_lists_host')
    line_params(gap, cross, height_ratio)
    q = quad_lists(quads)
    B, K = len(q), capacity(q)
    if B == 0:
        return [], np.zeros((STATS_WORDS,), np.int64)
    up = np.zeros((B * K * 64 + B * 4,), np.uint8)  # quads and counts go up in one buffer: the builder fills its two views
    _, count = pad_quads(q, up[:B * K * 64].view(np.float64).reshape(B, K, 4, 2), up[B * K * 64:].view(np.int32))
    d_up = torch.from_numpy(up).to(device, non_blocking=True)
    d_quads, d_count = d_up[:B * K * 64].view(torch.float64).view(B, K, 4, 2), d_up[B * K * 64:].view(torch.int32)
    d_rows = ops.quad_rows(d_quads)
    outs = ops.quad_lines(d_rows, d_count, gap, cross, height_ratio)
    valid = (d_rows[:, :, ROW_VALID] != 0).to(torch.uint8)
    parts = [t.contiguous().view(-1).view(torch.uint8) for t in (outs[2], outs[3], outs[0], outs[1], valid)]  # int64 first
    down = torch.cat(parts).cpu().numpy()
    cuts = np.cumsum([0] + [int(t.numel()) for t in parts])
    piece = lambda k, dtype, shape: down[cuts[k]:cuts[k + 1]].view(dtype).reshape(shape)
    table, stats = piece(0, np.int64, (B, K, TABLE_WORDS)), piece(1, np.int64, (B, STATS_WORDS))
    line, order, ok = piece(2, np.int32, (B, K)), piece(3, np.int32, (B, K)), piece(4, np.uint8, (B, K)) != 0
    return _line_results(count, [ok[b, :count[b]] for b in range(B)], line, order, table, stats)


def group_results(results: Sequence, gap: float = 1.5, cross: float = 0.5, height_ratio: float = 2.0, device='cuda') -> list:
    """The step of ``infer`` / ``infer_batch``: the characters of every result, in ``result_quads`` order with all regions
    together, go through ONE ``quad_lines`` call, each image on its own; the results come back with ``char_lines``,
    ``line_chars`` and ``line_polygons`` filled.  An image with more than ``MAX_QUADS`` characters gets ``lines_status = 2``
    and no lines."""
    tabs, fits = fitting_quads(results)
    out = [attrs.evolve(r, lines_status=2) for r in results]
    res, _ = quad_lines([tabs[i][0] for i in fits], gap, cross, height_ratio, device=device)
    for i, r in zip(fits, res):
        out[i] = attrs.evolve(results[i], char_lines=r.line, line_chars=r.lines, line_polygons=r.polygons, lines_status=0)
    return out
