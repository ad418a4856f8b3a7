"""vkas_spine_columns / vkas_spine_strips_u8 (csrc/spines.hip) through the C ABI, ``ops.spine_columns`` /
``ops.spine_strips_u8`` and ``inferencing.spine_strips`` against inferencing/spines.py on the MI355X: column records word for
word (``spine_columns_host``), strips byte for byte (``spine_strips_host``).  An arena of three images (420 x 430, 33 x 47 with
odd row bytes, 1 x 1); the quarter circle and tight arcs at ``log2n`` 0 .. 3, straight lines of w = 1, 63, 64, 65 and 300 columns,
a line of two knots, hand-made rows with a knot at every column and with 300 knots, lines partly and wholly outside their
image; h = 1, 16, 17, 32; n = 0; slots at odd addresses with canary bytes between them and around the output, guard words
around the workspace, canaries around the arena; hostile rows, knots and tile tables against the rule's defined answer; more
tiles than either kernel's grid takes in one trip; the argument errors; eager = replayed graph = second eager run."""
import ctypes

import numpy as np
import pytest
import torch

from tests import spine_cases as P
from tests import strip_cases as C

pytestmark = pytest.mark.gpu

CANARY = 0x5A
GUARD = 0x5A5A5A5A5A5A5A5A
NONE = -(1 << 63)
IMAGES = [C.picture((420, 430), 11), C.picture((33, 47), 12), C.picture((1, 1), 13)]


def mods():
    from vkit_ocr_model_adaptive_scaling_amd import inferencing, ops
    from vkit_ocr_model_adaptive_scaling_amd._lib import lib
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import spines
    return ops, lib, spines, inferencing


def scene(h, margin=0.125):
    """Lines per image for strips of height h.  A tight arc (six characters on a radius of three heights) at four scales: its
    down vector is 0.7, 1.5, 3 and 4.3 source pixels per strip row (log2n 0 .. 3); the quarter circle of
    tests/test_cpu_spines.py; straight lines of exactly w columns (w = 1 needs margin 0)."""
    grown = 1 + 2 * margin
    tight = lambda f: P.arc((10.0 / f, 10.0 / f), 60.0, 6, 12.0, 20.0, 15.7, 0.1, scale=h * f / (20 * grown))
    first = [P.arc((20.0, 20.0)), P.arc((20.0, 20.0))[::-1, [1, 0, 3, 2]]]  # and read from the other end
    first += [tight(f) for f in (0.7, 1.5, 3.0, 4.3)]

    def line(w, at, angle):  # characters 0.25 * h high: a column is 0.25 * grown px
        count = max(1, w // 4)
        return P.straight(count, (w * 0.25 * grown - 2 * margin * 0.25 * h) / count, 0.25 * h, at, angle)

    second = [line(w, at, angle) for w, at, angle in ((63, (2.0, 2.0), 0.35), (64, (30.0, 3.0), -0.3), (65, (3.0, 40.0), 1.57),
                                                      (300, (16.0, -20.0), 0.1))]
    if margin == 0:
        second.append(line(1, (4.0, 5.0), 0.0))
    second += [C.box(4, 5, 0.25 * h, 0.1 * h)[None], P.straight(3, 4.0, 5.0, (-100.0, -100.0))]  # two knots; wholly outside
    third = [C.box(-2, -3, 5, 9)[None], P.straight(3, 1.0, 1.5, (0.5, -1.0), 0.8)]
    return [first, second, third]


def hand_rows(layout, S, h):
    """Two rows by hand after the layout's: a wavy line of 70 columns with a knot at EVERY column (n = 1 throughout), and one
    of 330 columns with 300 knots.  -> (rows, knots, out_bytes, columns)."""
    rows, knots = [layout.rows], [layout.knots]
    at, knot_at, col_at = layout.out_bytes, len(layout.knots), layout.columns
    for w, q in ((70, np.arange(71)), (330, np.concatenate([np.arange(299), [330]]))):
        t = q / 10.0
        c = np.stack([150 + 30 * np.sin(t / 3), 20 + 7.0 * t], axis=1)
        d = np.stack([10 * np.cos(t / 3), np.full(len(t), 7.0)], axis=1)
        d /= np.hypot(*d.T)[:, None]
        v = np.stack([d[:, 1], -d[:, 0]], axis=1) * 0.9 * h
        k = np.concatenate([q[:, None], np.rint(65536 * (c - 0.5)), np.rint(65536 * v), np.zeros((len(q), 1))], axis=1).astype(np.int64)
        assert S.knot_status(k, h) == 0
        slot_w = -(-w // 16) * 16
        rows.append(np.array([[0, at, slot_w, w, knot_at, len(k), col_at, S.knots_log2n(k, h), 0, 0, 0, 0]], np.int64))
        knots.append(k)
        at, knot_at, col_at = at + 3 * h * slot_w, knot_at + len(k), col_at + w
    return np.concatenate(rows), np.concatenate(knots), at, col_at


def defined_answer(S, rows, knots, h, size, sources, arena_bytes, columns, images=IMAGES, fill=CANARY):
    """What the kernels give for ANY table: ``fill`` everywhere; a row without a defined slot is skipped, a row that fails
    another check gets zeros, every other row the oracle's pixels for whatever its knots hold."""
    out = np.full((size,), fill, np.uint8)
    for r in np.asarray(rows).tolist():
        src, offset, slot_w, w, at, count, col, log2n = r[:8]
        if not (1 <= slot_w <= 8192 and 0 <= offset <= size and 3 * h * slot_w <= size - offset):
            continue
        out[offset:offset + 3 * h * slot_w] = 0
        ok = 1 <= w <= slot_w and 0 <= log2n <= 3 and at >= 0 and count >= 2 and at + count <= len(knots) and col >= 0 and \
            col + w <= columns and 0 <= src < len(sources)
        if ok:
            off, hs, ws, _ = (int(v) for v in sources[src])
            ok = 1 <= hs <= 32768 and 1 <= ws <= 32768 and 0 <= off and off + 3 * hs * ws <= arena_bytes
        if ok:
            S.spine_bytes_host(images, [r], knots, h, out)
    return out


class Device:
    """The arena between canaries, a canary-filled buffer around the output and guard words around the workspace; ``run``
    calls the C ABI."""

    def __init__(self, out_bytes, columns, lead=259):
        ops, lib, spines, _ = mods()
        self.lib, self.S = lib, spines
        arena, self.sources, _ = ops.image_arena(IMAGES, torch.device('cuda'))
        self.total = int(arena.numel())
        self.padded = torch.full((self.total + 512,), CANARY, dtype=torch.uint8, device='cuda')
        self.padded[256:256 + self.total] = arena
        self.arena_copy = arena
        self.lead, self.out_bytes, self.columns = lead, out_bytes, columns  # an odd lead: the output is not 4-byte aligned
        self.buf = torch.full((out_bytes + 2 * lead,), CANARY, dtype=torch.uint8, device='cuda')
        self.ws = torch.full(((columns + 16) * 6,), GUARD, dtype=torch.int64, device='cuda')

    def args(self, rows, knots, h, sources=None, table=None):
        sources = self.sources if sources is None else np.asarray(sources, np.int64)
        table = self.S.spine_table(rows, knots, h) if table is None else np.asarray(table, np.int64)
        self.d_sources, self.d_table = torch.from_numpy(sources).cuda(), torch.from_numpy(table).cuda()
        return sources

    def run(self, rows, knots, h, sources=None, table=None):
        sources = self.args(rows, knots, h, sources, table)
        p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
        err = self.lib.vkas_spine_strips_u8(p(self.padded, 256), self.total, p(self.d_sources), len(sources), p(self.d_table),
                                            len(rows), len(knots), h, p(self.ws, 8 * 48), self.columns * 48,
                                            p(self.buf, self.lead), self.out_bytes,
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return err

    def run_columns(self, rows, knots, h):
        self.args(rows, knots, h)
        p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
        err = self.lib.vkas_spine_columns(p(self.d_table), len(rows), len(knots), h, p(self.ws, 8 * 48), self.columns,
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return err

    def records(self):
        ws = self.ws.cpu().numpy().reshape(-1, 6)
        assert (ws[:8] == np.int64(GUARD)).all() and (ws[8 + self.columns:] == np.int64(GUARD)).all(), 'around the workspace'
        return ws[8:8 + self.columns]

    def check_columns(self, rows, knots, h, what):
        got, want = self.records(), np.full((self.columns, 6), np.int64(GUARD))
        for r in np.asarray(rows).tolist():
            want[r[6]:r[6] + r[3]] = self.S.spine_columns_host(knots[r[4]:r[4] + r[5]], r[3], h)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert len(bad) == 0, f'{what}: {len(bad)} column records differ, first {bad[0]}: {got[bad[0]]} != {want[bad[0]]}'

    def check(self, want_out, what):
        self.records()
        got = self.buf.cpu().numpy()
        assert (got[:self.lead] == CANARY).all() and (got[self.lead + self.out_bytes:] == CANARY).all(), f'{what}: around out'
        inner = got[self.lead:self.lead + self.out_bytes]
        bad = np.flatnonzero(inner != want_out)
        assert len(bad) == 0, f'{what}: {len(bad)} bytes differ, first at {bad[0]}: {inner[bad[0]]} != {want_out[bad[0]]}'
        pad = self.padded.cpu().numpy()
        assert (pad[:256] == CANARY).all() and (pad[256 + self.total:] == CANARY).all(), f'{what}: around the arena'
        assert torch.equal(self.padded[256:256 + self.total], self.arena_copy), f'{what}: the arena'


def spaced(rows, h, columns, gap=5):
    """The rows with their slots laid out afresh in scrambled order, ``gap`` canary bytes before each (odd slot addresses),
    and their column ranges in another scrambled order with a record of room before each."""
    rows = np.array(rows)
    at = gap
    for r in np.random.default_rng(3).permutation(len(rows)).tolist():
        rows[r, 1] = at
        at += h * rows[r, 2] * 3 + gap
    col = 1
    for r in np.random.default_rng(5).permutation(len(rows)).tolist():
        rows[r, 6] = col
        col += rows[r, 3] + 1
    return rows, at, col


def answer(S, rows, knots, h, size):
    return S.spine_bytes_host(IMAGES, rows, knots, h, np.full((size,), CANARY, np.uint8))


@pytest.mark.parametrize('h', [1, 16, 17, 32])
def test_c_abi_equals_the_oracle_between_canaries(h):
    _, _, S, _ = mods()
    margin = 0.0 if h in (1, 17) else 0.125
    layout = S.spine_rows(scene(h, margin), h, 2048, 16, margin)
    assert (layout.status == 0).all() and len(layout.bucket_shapes) >= 2 and {0, 1, 2, 3} <= set(layout.rows[:, 7].tolist())
    assert {63, 64, 65, 300} | ({1} if margin == 0 else set()) <= set(layout.widths.tolist()) and 2 in layout.rows[:, 5].tolist()
    rows, knots, size, columns = hand_rows(layout, S, h)
    assert rows[-1, 5] == 300 and rows[-2, 5] == rows[-2, 3] + 1
    S.check_spine_rows(rows, knots, np.array([[0, 420, 430, 0], [0, 33, 47, 0], [0, 1, 1, 0]]), h, size, columns)
    dev = Device(size, columns, lead=256)
    assert dev.run_columns(rows, knots, h) == 0
    dev.check_columns(rows, knots, h, ('columns alone', h))
    dev.check(np.full((size,), CANARY, np.uint8), ('columns alone', h))
    # the layout of spine_rows: slots back to back
    assert dev.run(rows, knots, h) == 0
    dev.check_columns(rows, knots, h, ('packed', h))
    want = answer(S, rows, knots, h, size)
    assert (want != CANARY).mean() > 0.9
    dev.check(want, ('packed', h))
    # odd addresses, gaps, rows in scrambled source order, columns in another order
    rows, size, columns = spaced(rows, h, columns)
    rows = rows[np.random.default_rng(4).permutation(len(rows))]
    assert (np.diff(rows[:, 0]) < 0).any()
    dev = Device(size, columns)
    assert dev.run(rows, knots, h) == 0
    dev.check_columns(rows, knots, h, ('spaced', h))
    dev.check(answer(S, rows, knots, h, size), ('spaced', h))


def test_tiles_beyond_both_grids_take_a_second_trip():
    """More tiles than the columns kernel has waves (8192) and four times what the strips kernel has workgroups (2048): 65
    hand-made rows of h = 1 and two knots in slots of 8192 pixels, 128 tiles each.  Narrow rows, and wide ones at the end:
    the last row's columns are all written on a wave's second trip, its pixels on a workgroup's fifth."""
    ops, _, S, _ = mods()
    h, slot_w, n = 1, 8192, 65
    widths = [3 + k % 40 for k in range(n - 3)] + [5000, 8191, 8192]
    rows, knots, col_at = [], [], 0
    for k, w in enumerate(widths):
        angle, length = 0.3 * k, min(0.9 * w, 300.0)
        d = np.array([np.sin(angle), np.cos(angle)])                       # along the line, (y, x)
        c = np.array([210.0, 215.0])[None] + np.array([[-0.5], [0.5]]) * length * d[None]
        v = np.array([d[1], -d[0]]) * (0.9 if k % 2 else 2.0)              # down: 0.9 or 2 source pixels per strip row
        t = np.concatenate([[[0], [w]], np.rint(65536 * (c - 0.5)), np.tile(np.rint(65536 * v), (2, 1)), [[0], [0]]], axis=1).astype(np.int64)
        assert S.knot_status(t, h) == 0
        rows.append([0, 0, slot_w, w, 2 * k, 2, col_at, S.knots_log2n(t, h), 0, 0, 0, 0])
        knots.append(t)
        col_at += w
    rows, knots = np.array(rows, np.int64), np.concatenate(knots)
    rows, size, columns = spaced(rows, h, col_at)
    S.check_spine_rows(rows, knots, np.array([[0, 420, 430, 0], [0, 33, 47, 0], [0, 1, 1, 0]]), h, size, columns)
    table = S.spine_table(rows, knots, h)
    assert table[13 * n] == 128 * n > 8192 and table[12 * n + n - 1] == 8192 and {0, 1} <= set(rows[:, 7].tolist())
    want = answer(S, rows, knots, h, size)
    last = rows[-1].tolist()
    assert want[last[1]:last[1] + 3 * slot_w].reshape(-1, 3).any(axis=1).mean() > 0.9
    dev = Device(size, columns)
    assert dev.run(rows, knots, h) == 0
    dev.check_columns(rows, knots, h, 'second trip')
    dev.check(want, 'second trip')
    cols = ops.spine_columns(dev.d_table, n, len(knots), h, columns, validate=False).cpu().numpy()
    for r in rows.tolist():
        assert np.array_equal(cols[r[6]:r[6] + r[3]], S.spine_columns_host(knots[r[4]:r[4] + r[5]], r[3], h)), r[:8]


def test_ops_equal_the_oracle_and_n_0():
    ops, _, S, _ = mods()
    h = 16
    layout = S.spine_rows(scene(h), h, 2048, 16, 0.125)
    arena, sources, d_sources = ops.image_arena(IMAGES, torch.device('cuda'))
    n, T = len(layout.rows), len(layout.knots)
    table = S.spine_table(layout.rows, layout.knots, h)
    want = answer(S, layout.rows, layout.knots, h, layout.out_bytes)
    want_cols = np.concatenate([S.spine_columns_host(layout.knots[r[4]:r[4] + r[5]], r[3], h) for r in layout.rows.tolist()])
    d_table = torch.from_numpy(table).cuda()
    for validate in (True, False):
        out = ops.spine_strips_u8(arena, d_sources, d_table, n, T, h, layout.out_bytes, validate=validate)
        assert out.shape == (layout.out_bytes,) and out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), want), validate
        cols = ops.spine_columns(d_table, n, T, h, layout.columns + 2, validate=validate)
        assert cols.shape == (layout.columns + 2, 6) and cols.dtype == torch.int64
        assert np.array_equal(cols.cpu().numpy()[:-2], want_cols) and (cols.cpu().numpy()[-2:] == NONE).all()
    assert np.array_equal(ops.spine_strips_u8(arena, sources, table, n, T, h, layout.out_bytes).cpu().numpy(), want), 'host tables'
    # n = 0: no launch, an output nobody wrote
    none = torch.from_numpy(S.spine_table(np.zeros((0, 12)), np.zeros((0, 6)), h)).cuda()
    assert ops.spine_strips_u8(arena, d_sources, none, 0, 0, h, 0).shape == (0,)
    assert ops.spine_strips_u8(arena, d_sources, none, 0, 0, h, 96).shape == (96,)
    assert ops.spine_columns(none, 0, 0, h, 0).shape == (0, 6)
    # what the table check refuses: two rows on one slot, shared columns, knots that do not rise
    twice, shared, knots = layout.rows.copy(), layout.rows.copy(), layout.knots.copy()
    twice[1, 1:3] = twice[0, 1:3]
    twice[1, 3] = min(twice[1, 3], twice[0, 2])
    shared[1, 6] = shared[0, 6]
    knots[1, 0] = 0
    for r, t in ((twice, layout.knots), (shared, layout.knots), (layout.rows, knots)):
        with pytest.raises(ValueError):
            ops.spine_strips_u8(arena, d_sources, torch.from_numpy(S.spine_table(r, t, h)).cuda(), n, T, h, layout.out_bytes)
    for call in (lambda: ops.spine_strips_u8(arena, d_sources, d_table, n, T, 0, layout.out_bytes),
                 lambda: ops.spine_strips_u8(arena, d_sources, d_table, n, T, 257, layout.out_bytes),
                 lambda: ops.spine_strips_u8(arena, d_sources, d_table, n, T, h, 1 << 40),
                 lambda: ops.spine_strips_u8(arena, d_sources, d_table, n, T, h, layout.out_bytes - 1),
                 lambda: ops.spine_strips_u8(arena, d_sources, d_table, n, T - 1, h, layout.out_bytes),
                 lambda: ops.spine_strips_u8(arena, d_sources, d_table, n + 1, T, h, layout.out_bytes),
                 lambda: ops.spine_strips_u8(arena, d_sources, d_table, -1, T, h, layout.out_bytes),
                 lambda: ops.spine_strips_u8(arena, d_sources, d_table[:-1], n, T, h, layout.out_bytes),
                 lambda: ops.spine_strips_u8(arena, d_sources, d_table.to(torch.int32), n, T, h, layout.out_bytes),
                 lambda: ops.spine_strips_u8(arena.view(1, -1), d_sources, d_table, n, T, h, layout.out_bytes),
                 lambda: ops.spine_strips_u8(arena[:100], d_sources, d_table, n, T, h, layout.out_bytes),
                 lambda: ops.spine_strips_u8(arena, d_sources[:, :3], d_table, n, T, h, layout.out_bytes),
                 lambda: ops.spine_strips_u8(arena, d_sources, d_table, n, T, h, 3 * h * (n - 1), validate=False),
                 lambda: ops.spine_strips_u8(arena, d_sources, table, n, T, h, layout.out_bytes, validate=False),
                 lambda: ops.spine_columns(d_table, n, T, h, layout.columns - 1),
                 lambda: ops.spine_columns(d_table, n, T, h, n - 1, validate=False),
                 lambda: ops.spine_columns(table, n, T, h, layout.columns)):
        with pytest.raises(ValueError):
            call()


def test_hostile_tables_get_the_defined_answer():
    _, _, S, _ = mods()
    h = 8
    lines = [[P.arc((20.0, 20.0), scale=0.5), P.straight(5, 6.0, 9.0, (200.0, 30.0), 0.35)], [P.straight(4, 6.0, 9.0, (10.0, 5.0), 0.2)],
             [C.box(0, 0, 1, 3)[None]]]
    base = S.spine_rows(lines, h, 2048, 1, 0.0)
    good, good_knots = base.rows, base.knots
    assert len(good) == 4 and good[0, 5] >= 20 and good[0, 3] > 64
    arena_sources = mods()[0].image_arena(IMAGES, torch.device('cuda'))[1]
    arena_bytes = int(arena_sources[-1, 0]) + 16
    sources = np.concatenate([arena_sources, [[1 << 30, 20, 20, 0], [0, 0, 4, 0], [0, 32769, 1, 0], [-16, 4, 4, 0], [0, 4, 32769, 0]]])
    big = 1 << 62
    row_cases = [(0, -1), (0, len(sources)), (0, 3), (0, 4), (0, 5), (0, 6), (0, 7),               # src, the source entry
                 (3, 0), (3, -5), (3, good[0, 2] + 1), (3, big),                                     # w
                 (4, -1), (4, 'end'), (4, big), (4, -big), (5, 1), (5, 0), (5, -3), (5, 'past'), (5, big),  # knot_start, knots
                 (6, -1), (6, 'cap'), (6, big), (6, -big),                                           # col_start
                 (7, 4), (7, -1), (7, 1 << 40)]                                                      # log2n
    knot_cases = [('falling', lambda k: k.__setitem__((slice(None), 0), k[::-1, 0].copy())),
                  ('not rising', lambda k: k.__setitem__((5, 0), k[4, 0])), ('swapped', lambda k: k.__setitem__(([3, 9], 0), k[[9, 3], 0])),
                  ('q_0 above 0', lambda k: k.__setitem__((0, 0), 3)), ('q_0 below 0', lambda k: k.__setitem__((0, 0), -big)),
                  ('q_last below w', lambda k: k.__setitem__((-1, 0), k[-1, 0] - 7)), ('q_last huge', lambda k: k.__setitem__((-1, 0), big)),
                  ('a segment above 8192', lambda k: k.__setitem__((slice(1, None), 0), k[1:, 0] + 9000)),
                  ('c at 2^39', lambda k: k.__setitem__((4, 1), 1 << 39)), ('c minimum', lambda k: k.__setitem__((4, 2), NONE)),
                  ('v beyond 2^30', lambda k: k.__setitem__((6, 3), (1 << 30) + 1)), ('v maximum', lambda k: k.__setitem__((6, 4), (1 << 63) - 1)),
                  ('a step beyond 2^22', lambda k: k.__setitem__((7, 1), k[7, 1] + (100 << 22))),
                  ('v / h beyond 2^22', lambda k: k.__setitem__((8, 3), (h << 22) + h))]
    rows, knots = [good[1]], [good_knots[good[1, 4]:good[1, 4] + good[1, 5]]]
    mine = good_knots[:good[0, 5]]

    def add(row, k):
        row = row.copy()
        row[4] = sum(len(t) for t in knots) if k is not None else row[4]
        rows.append(row)
        knots.append(k if k is not None else np.zeros((0, 6), np.int64))

    pending = []
    for col, value in row_cases:
        r = good[0].copy()
        add(r, mine)
        pending.append((len(rows) - 1, col, value))
        k = len(rows) % 3 + 1
        add(good[k], good_knots[good[k, 4]:good[k, 4] + good[k, 5]])
    for name, change in knot_cases:
        k = mine.copy()
        change(k)
        add(good[0], k)
    rows, knots = np.array(rows), np.concatenate(knots)
    rows, size, columns = spaced(rows, h, 0)
    for at, col, value in pending:
        value = {'end': len(knots) - 1, 'past': len(knots) - rows[at, 4] + 1, 'cap': columns - rows[at, 3] + 1}.get(value, value)
        rows[at, col] = value
    skipped = []
    for col, value in ((1, -1), (1, size - 10), (1, 1 << 41), (2, 0), (2, -64), (2, 8193), (1, -big), (2, big)):
        r = rows[0].copy()
        r[1] = 7  # on top of a valid slot's gap: a write would show
        r[col] = value
        skipped.append(r)
    table_rows = np.concatenate([rows[:5], skipped[:4], rows[5:], skipped[4:]])
    want = defined_answer(S, table_rows, knots, h, size, sources, arena_bytes, columns)
    zeroed = sum(1 for r in rows.tolist() if not want[r[1]:r[1] + 3 * h * r[2]].any())
    assert zeroed >= len(row_cases) and (want != 0).mean() > 0.3
    dev = Device(size, columns)
    assert dev.total == arena_bytes
    assert dev.run(table_rows, knots, h, sources=sources) == 0
    dev.check(want, 'hostile rows and knots')
    for r, t in ((rows[1:2], knots), (skipped[:1], knots), (rows[-1:], knots)):
        with pytest.raises(ValueError):
            S.check_spine_rows(np.array(r), t, sources, h, size, columns)
    # a tile table that lies: a byte is the rule's or untouched, whatever it holds
    valid, T = good.copy(), good_knots
    valid, size, columns = spaced(valid, h, 0)
    honest = S.spine_table(valid, T, h)
    n = len(valid)
    full = answer(S, valid, T, h, size)
    for name, tail in (('huge', np.full((n + 1,), big)), ('negative', np.full((n + 1,), -big)),
                       ('falling', honest[12 * n:13 * n + 1][::-1]), ('zero', np.zeros((n + 1,))),
                       ('shifted', honest[12 * n:13 * n + 1] + 3)):
        dev = Device(size, columns)
        table = np.concatenate([honest[:12 * n], tail, honest[13 * n + 1:]]).astype(np.int64)
        assert dev.run(valid, T, h, table=table) == 0
        got = dev.buf.cpu().numpy()[dev.lead:dev.lead + size]
        assert ((got == full) | (got == CANARY)).all(), name
        dev.check(got, name)


def test_argument_errors_launch_nothing():
    _, _, S, _ = mods()
    h = 8
    layout = S.spine_rows(scene(h), h, 2048, 16, 0.125)
    rows, knots, size, columns = layout.rows, layout.knots, layout.out_bytes, layout.columns
    dev = Device(size, columns, lead=256)
    assert dev.run(rows, knots, h) == 0
    lib, n, T = dev.lib, len(rows), len(knots)
    dev.buf.fill_(CANARY)
    dev.ws.fill_(GUARD)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    arena, src, tab, ws, out = p(dev.padded, 256), p(dev.d_sources), p(dev.d_table), p(dev.ws, 8 * 48), p(dev.buf, 256)
    S_, total, wsb = len(dev.sources), dev.total, columns * 48
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = (arena, total, src, S_, tab, n, T, h, ws, wsb, out, size)
    changes = [(7, 0), (7, 257), (7, -8), (0, None), (2, None), (4, None), (8, None), (10, None), (2, p(dev.d_sources, 4)),
               (4, p(dev.d_table, 4)), (8, p(dev.ws, 8 * 48 + 4)), (5, -1), (6, -1), (11, 1 << 40), (11, -1), (1, 0), (3, 0),
               (9, 48 * n - 1), (9, -48), (9, 0)]
    for k, (at, value) in enumerate(changes):
        args = list(ok)
        args[at] = value
        assert lib.vkas_spine_strips_u8(*args, stream) != 0, k
    ok = (tab, n, T, h, ws, columns)
    for k, (at, value) in enumerate([(0, None), (4, None), (0, p(dev.d_table, 4)), (4, p(dev.ws, 4)), (1, -1), (2, -1), (3, 0), (3, 257),
                                     (5, n - 1), (5, -1), (5, 1 << 40)]):
        args = list(ok)
        args[at] = value
        assert lib.vkas_spine_columns(*args, stream) != 0, k
    assert lib.vkas_spine_strips_u8(arena, total, src, S_, tab, 0, T, h, ws, wsb, out, size, stream) == 0  # n = 0: no launch
    assert lib.vkas_spine_columns(tab, 0, T, h, ws, columns, stream) == 0
    assert lib.vkas_spine_strips_workspace_bytes(0) == 0 and lib.vkas_spine_strips_workspace_bytes(7) == 7 * 48
    assert lib.vkas_spine_strips_workspace_bytes(-1) < 0
    torch.cuda.synchronize()
    dev.check(np.full((size,), CANARY, np.uint8), 'argument errors')
    assert (dev.records() == np.int64(GUARD)).all()


def test_eager_replay_and_second_run_agree():
    ops, _, S, _ = mods()
    h = 32
    layout = S.spine_rows(scene(h), h, 2048, 64, 0.125)
    arena, sources, d_sources = ops.image_arena(IMAGES, torch.device('cuda'))
    d_table = torch.from_numpy(S.spine_table(layout.rows, layout.knots, h)).cuda()
    want = S.spine_bytes_host(IMAGES, layout.rows, layout.knots, h, np.zeros((layout.out_bytes,), np.uint8))
    run = lambda: ops.spine_strips_u8(arena, d_sources, d_table, len(layout.rows), len(layout.knots), h, layout.out_bytes,
                                      validate=False)
    first, second = run(), run()
    torch.cuda.synchronize()
    assert first.data_ptr() != second.data_ptr() and torch.equal(first, second) and np.array_equal(first.cpu().numpy(), want)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = run()
    for k in range(2):
        static.fill_(CANARY)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static, first), f'replay {k}'


def assert_same_strips(got, want):
    assert got.height == want.height and len(got.buckets) == len(want.buckets)
    for name in ('image', 'status', 'squeezed', 'widths', 'bucket', 'index', 'rows', 'knots'):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    for a, b in zip(got.buckets, want.buckets):
        assert a.is_cuda and a.dtype == torch.uint8 and tuple(a.shape) == b.shape and np.array_equal(a.cpu().numpy(), b)
    for k in np.flatnonzero(want.status == 0).tolist():
        assert np.array_equal(got.strip(k).cpu().numpy(), want.strip(k))
        assert np.array_equal(got.spine(k), want.spine(k))


def test_inferencing_spine_strips_equals_the_host_route():
    ops, _, S, inf = mods()
    lines = scene(32)
    lines[1] = lines[1] + [np.full((2, 4, 2), np.nan), C.box(0, 0, 64 * 32 + 1, 64)[None]]  # status 1 and 2
    want = inf.spine_strips_host(IMAGES, lines)
    assert sorted(set(want.status.tolist())) == [0, 1, 2] and len(want.buckets) >= 2 and want.height == 32
    assert_same_strips(inf.spine_strips(IMAGES, lines), want)
    arena, sources, d_sources = ops.image_arena(IMAGES, torch.device('cuda'))
    assert_same_strips(inf.spine_strips((arena, sources), lines), want)
    assert_same_strips(inf.spine_strips((arena, sources, d_sources), lines), want)
    assert_same_strips(inf.spine_strips([torch.from_numpy(m).cuda() for m in IMAGES], lines), want)
    got = inf.spine_strips(IMAGES, lines)
    assert got.buckets[0].untyped_storage().data_ptr() == got.buckets[-1].untyped_storage().data_ptr(), 'one allocation'
    pts = np.array([[0.0, 0.0], [32.0, 5.0], [16.0, 7.5]])
    assert np.array_equal(got.remap(0, pts), want.remap(0, pts))
    # S = 3 sources of which one has no line
    some = [lines[0][:2], [], lines[2]]
    assert_same_strips(inf.spine_strips(IMAGES, some), inf.spine_strips_host(IMAGES, some))
    other = inf.spine_strips(IMAGES, lines, height=8, width_max=24, width_step=8, margin=0.0)
    assert_same_strips(other, inf.spine_strips_host(IMAGES, lines, 8, 24, 8, 0.0))
    assert other.squeezed.any()
    none = inf.spine_strips(IMAGES, [[], [], []])
    assert none.buckets == [] and none.rows.shape == (0, 12) and none.knots.shape == (0, 6)
    with pytest.raises(ValueError):
        inf.spine_strips(IMAGES, lines, device='cpu')
    with pytest.raises(ValueError):
        inf.spine_strips(IMAGES[:2], lines)
