"""vkas_quad_strips_u8 (csrc/strips.hip) through the C ABI, ``ops.quad_strips_u8`` and ``inferencing.quad_strips`` against
inferencing/strips.py::quad_strips_host on the MI355X, byte for byte: an arena of three images (40 x 60, 33 x 47 with odd row
bytes, 1 x 1); exact cuts, slanted quads shrunk by 1, 3 and 10, quads partly and wholly outside their image, w = 1, slot_w
and slot_w - 1, several bucket widths; h = 1, 8, 32, 37; n = 0, 1, 65, 300; rows in scrambled order; slots at odd addresses
with canary bytes between them and around the output and the arena; every kind of invalid row next to valid neighbours;
hostile tile tables; more tiles than the grid has workgroups; the argument errors; eager = replayed graph = second eager run."""
import ctypes

import numpy as np
import pytest
import torch

from tests import strip_cases as C

pytestmark = pytest.mark.gpu

CANARY = 0x5A
IMAGES = [C.picture((40, 60), 11), C.picture((33, 47), 12), C.picture((1, 1), 13)]


def mods():
    from vkit_ocr_model_adaptive_scaling_amd import inferencing, ops
    from vkit_ocr_model_adaptive_scaling_amd._lib import lib
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import strips
    return ops, lib, strips, inferencing


def scene(h):
    """Quads per image for strips of height h: the shrink factors 1, 2, 3, 10 (log2n 0 .. 3) are the quad's height over h."""
    s = float(h)
    first = [C.box(5, 7, 8, 20), C.turned(C.box(5, 7, 8, 20), 2), C.box(5, 7, 8, 20)[[1, 0, 3, 2]],
             np.array([[10, 28], [30, 28], [30, 20], [10, 20]], np.float64),
             C.turned(np.array([[10, 28], [30, 28], [30, 20], [10, 20]], np.float64), 2), C.box(3, 9, 16, 40)]
    first += [C.rect(20, 30, 3.3 * s * k, s * k, a) for a in (0.35, 1.57, 3.0) for k in (1, 2, 3, 10)]
    second = [C.rect(16, 23, 30, 9, a) for a in (0.35, 1.57, 3.0)]
    second += [C.rect(2, 40, 30, 9, 0.6), C.rect(-100, -100, 30, 9, 0.6), C.rect(500, 20, 30, 9, 0.0)]  # partly, wholly outside
    second += [C.box(4, 5, s, 0.3), C.box(4, 5, s, 16), C.box(4, 5, s, 15), C.box(4, 5, s, 32), C.box(4, 5, s, 17)]  # w = 1, slot_w, slot_w - 1
    third = [C.box(0, 0, 1, 1), C.box(-2, -3, 5, 9), C.rect(0.5, 0.5, 3, 1, 0.8)]
    return [np.stack(first), np.stack(second), np.stack(third)]


def host_bytes(strips_mod, rows, h, size, fill=CANARY, images=IMAGES):
    """The output the rule gives for valid rows: ``fill`` everywhere, each slot its strip and zeros beyond w."""
    from vkit_ocr_model_adaptive_scaling_amd.inferencing.packing import warp_host
    out = np.full((size,), fill, np.uint8)
    for src, offset, slot_w, w, *coef in np.asarray(rows).tolist():
        slot = out[offset:offset + h * slot_w * 3].reshape(h, slot_w, 3)
        slot[:] = 0
        slot[:, :w] = warp_host(images[src], [[0, 0, h, w] + coef], np.zeros((h, w, 3), np.uint8))
    return out


class Device:
    """The arena between canaries and a canary-filled buffer around the output; ``run`` calls the C ABI."""

    def __init__(self, out_bytes, lead=259):
        ops, lib, strips, _ = mods()
        self.lib, self.strips = lib, strips
        arena, self.sources, _ = ops.image_arena(IMAGES, torch.device('cuda'))
        self.total = int(arena.numel())
        self.padded = torch.full((self.total + 512,), CANARY, dtype=torch.uint8, device='cuda')
        self.padded[256:256 + self.total] = arena
        self.arena_copy = arena
        self.lead, self.out_bytes = lead, out_bytes  # an odd lead: the output itself is not 4-byte aligned
        self.buf = torch.full((out_bytes + 2 * lead,), CANARY, dtype=torch.uint8, device='cuda')

    def run(self, rows, h, sources=None, table=None, n=None, out_bytes=None):
        sources = self.sources if sources is None else np.asarray(sources, np.int64)
        table = self.strips.strip_table(rows, h) if table is None else np.asarray(table, np.int64)
        self.d_sources, self.d_table = torch.from_numpy(sources).cuda(), torch.from_numpy(table).cuda()
        p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
        err = self.lib.vkas_quad_strips_u8(p(self.padded, 256), self.total, p(self.d_sources), len(sources), p(self.d_table),
                                           len(rows) if n is None else n, h, p(self.buf, self.lead),
                                           self.out_bytes if out_bytes is None else out_bytes,
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return err

    def check(self, want_out, what):
        got = self.buf.cpu().numpy()
        assert (got[:self.lead] == CANARY).all() and (got[self.lead + self.out_bytes:] == CANARY).all(), f'{what}: around out'
        inner = got[self.lead:self.lead + self.out_bytes]
        bad = np.flatnonzero(inner != want_out)
        assert len(bad) == 0, f'{what}: {len(bad)} bytes differ, first at {bad[0]}: {inner[bad[0]]} != {want_out[bad[0]]}'
        pad = self.padded.cpu().numpy()
        assert (pad[:256] == CANARY).all() and (pad[256 + self.total:] == CANARY).all(), f'{what}: around the arena'
        assert torch.equal(self.padded[256:256 + self.total], self.arena_copy), f'{what}: the arena'


def spaced(rows, h, gap=5):
    """The rows with their slots laid out afresh in scrambled order, ``gap`` canary bytes before each: odd slot addresses."""
    rows = np.array(rows)
    at = gap
    for r in np.random.default_rng(3).permutation(len(rows)).tolist():
        rows[r, 1] = at
        at += h * rows[r, 2] * 3 + gap
    return rows, at


@pytest.mark.parametrize('h', [1, 8, 32, 37])
def test_c_abi_equals_the_oracle_between_canaries(h):
    _, _, S, _ = mods()
    layout = S.strip_rows(scene(h), h, 2048, 16, 0.0)
    assert (layout.status == 0).all() and len(layout.bucket_shapes) >= 2 and {0, 1, 2, 3} <= set(layout.rows[:, 10].tolist())
    widths, slots = layout.rows[:, 3], layout.rows[:, 2]
    assert (widths == 1).any() and (widths == slots).any() and (widths == slots - 1).any()
    # the layout of strip_rows: slots back to back (aligned when h * 3 * 16 is)
    dev = Device(layout.out_bytes, lead=256)
    assert dev.run(layout.rows, h) == 0
    dev.check(host_bytes(S, layout.rows, h, layout.out_bytes), ('packed', h))
    # odd addresses, gaps, rows in scrambled source order
    rows, size = spaced(layout.rows, h)
    rows = rows[np.random.default_rng(4).permutation(len(rows))]
    assert (np.diff(rows[:, 0]) < 0).any()
    dev = Device(size)
    assert dev.run(rows, h) == 0
    dev.check(host_bytes(S, rows, h, size), ('spaced', h))


@pytest.mark.parametrize('n', [0, 1, 65, 300])
def test_many_small_strips_through_ops(n):
    ops, _, S, _ = mods()
    rng = np.random.default_rng(n)
    quads = [[], [], []]
    for k in range(n):
        quads[int(rng.integers(0, 3))].append(C.rect(rng.uniform(0, 30), rng.uniform(0, 45), rng.uniform(4, 40), rng.uniform(3, 12),
                                                     rng.uniform(0, 6.3)))
    quads = [np.array(q, np.float64).reshape(-1, 4, 2) for q in quads]
    h = 8
    layout = S.strip_rows(quads, h, 64, 8, 0.125)
    assert len(layout.rows) == n
    arena, sources, d_sources = ops.image_arena(IMAGES, torch.device('cuda'))
    want = host_bytes(S, layout.rows, h, layout.out_bytes)
    out = ops.quad_strips_u8(arena, sources, layout.rows, h, layout.out_bytes)
    assert out.shape == (layout.out_bytes,) and out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), want)
    if n:
        order = rng.permutation(n)
        d_rows = torch.from_numpy(layout.rows[order]).cuda()
        for rows in (d_rows, torch.from_numpy(S.strip_table(layout.rows[order], h)).cuda()):  # device rows, device table
            for validate in (True, False):
                out = ops.quad_strips_u8(arena, d_sources, rows, h, layout.out_bytes, validate=validate)
                assert np.array_equal(out.cpu().numpy(), want), (n, tuple(rows.shape), validate)
        if n > 1:  # two rows on one slot are refused when the table is checked
            twice = layout.rows.copy()
            twice[1, 1:3] = twice[0, 1:3]
            twice[1, 3] = min(twice[1, 3], twice[0, 2])
            with pytest.raises(ValueError):
                ops.quad_strips_u8(arena, d_sources, torch.from_numpy(twice).cuda(), h, layout.out_bytes)


def test_invalid_rows_next_to_valid_neighbours():
    _, _, S, _ = mods()
    h = 8
    quads = [np.stack([C.rect(20, 30, 26, 9, 0.35)]), np.stack([C.rect(16, 23, 30, 9, 1.57)]), np.stack([C.box(0, 0, 1, 3)])]
    good = S.strip_rows(quads, h, 2048, 1, 0.0).rows
    sources = np.concatenate([mods()[0].image_arena(IMAGES, torch.device('cuda'))[1],
                              [[1 << 30, 20, 20, 0], [0, 0, 4, 0], [0, 32769, 1, 0], [-16, 4, 4, 0], [0, 4, 32769, 0]]])
    zeroed = [(0, -1), (0, len(sources)), (0, 3), (0, 4), (0, 5), (0, 6), (0, 7), (3, 0), (3, -5), (3, good[0, 2] + 1),
              (6, (1 << 22) + 1), (7, -(1 << 22) - 1), (8, (1 << 22) + 1), (9, -(1 << 23)), (4, 1 << 40), (5, -(1 << 40)),
              (10, 4), (10, -1), (10, 1 << 40)]
    rows = [good[1]]
    for col, value in zeroed:
        r = good[0].copy()
        r[col] = value
        rows += [r, good[len(rows) % 3]]
    rows, size = spaced(np.array(rows), h)
    skipped = []
    for col, value in ((1, -1), (1, size - 10), (1, 1 << 41), (2, 0), (2, -64), (2, 8193), (1, -(1 << 62)), (2, 1 << 62)):
        r = good[0].copy()
        r[1] = 7  # on top of a valid slot's gap: a write would show
        r[col] = value
        skipped.append(r)
    bad = [k for k in range(1, len(rows), 2)]
    want = host_bytes(S, np.delete(rows, bad, axis=0), h, size)
    for r in rows[bad].tolist():
        want[r[1]:r[1] + h * r[2] * 3] = 0
    table_rows = np.concatenate([rows[:5], skipped[:4], rows[5:], skipped[4:]])
    dev = Device(size)
    assert dev.run(table_rows, h, sources=sources) == 0
    dev.check(want, 'invalid rows')
    for r in (rows[1], skipped[0]):
        with pytest.raises(ValueError):
            S.check_strip_rows(np.array([r]), sources, h, size)
    # a tile table that lies: nothing outside the slots, whatever it holds
    valid = np.delete(rows, bad, axis=0)
    honest = S.strip_table(valid, h)
    n = len(valid)
    for name, tail in (('huge', np.full((n + 1,), 1 << 62)), ('negative', np.full((n + 1,), -(1 << 62))),
                       ('falling', honest[-(n + 1):][::-1]), ('zero', np.zeros((n + 1,))),
                       ('shifted', honest[-(n + 1):] + 3)):
        dev = Device(size)
        table = np.concatenate([honest[:n * 12], tail]).astype(np.int64)
        assert dev.run(valid, h, table=table) == 0
        got = dev.buf.cpu().numpy()[dev.lead:dev.lead + size]
        full = host_bytes(S, valid, h, size)
        assert ((got == full) | (got == CANARY)).all(), name  # a byte is the rule's or untouched
        dev.check(got, name)


def test_tiles_beyond_the_grid_take_a_second_trip():
    """More tiles than the grid has workgroups (2048): 18 hand-made rows of h = 1 in slots of 8192 pixels, 128 tiles each, so
    the rows from the 17th on are cut wholly on a workgroup's second trip over the tiles - narrow rows, and at the end wide
    ones along and across the source's rows, whose tiles carry picture bytes and the zeros beyond w."""
    _, _, S, _ = mods()
    h, slot_w = 1, 8192
    widths = [5 + 3 * k for k in range(14)] + [8192, 4100, 5000, 8191]
    rows = []
    for k, w in enumerate(widths):
        src = k % 2
        Hs, Ws = IMAGES[src].shape[:2]
        along, across = 65536 * (Ws - 1) // w, 65536 * (Hs - 1) // w      # the diagonal of the image in w steps
        if k == len(widths) - 2:                                             # one wide row runs down the image: lanes along i
            rows.append([src, 0, slot_w, w, 0, 65536 * (Ws // 2), 65536, 65536 * (Hs - 1) // w, 0, 7, 0, 0])
        else:
            rows.append([src, 0, slot_w, w, 65536, 0, 65536 if k % 3 else 3 * 65536, across, 0, along, 0 if k % 3 else 2, 0])
    rows, size = spaced(np.array(rows, np.int64), h)
    sources = mods()[0].image_arena(IMAGES, torch.device('cuda'))[1]
    S.check_strip_rows(rows, sources, h, size)
    table = S.strip_table(rows, h)
    assert table[-1] == 128 * len(rows) > 2048 and table[12 * len(rows) + 16] == 2048
    assert (np.abs(rows[:, 9]) < np.abs(rows[:, 7])).any() and {0, 2} <= set(rows[:, 10].tolist())
    want = host_bytes(S, rows, h, size)
    for r in rows[-3:].tolist():  # the second trip writes picture bytes, and zeros beyond w in the narrower row
        assert want[r[1]:r[1] + 3 * r[3]].any() and not want[r[1] + 3 * r[3]:r[1] + 3 * slot_w].any()
    dev = Device(size)
    assert dev.run(rows, h) == 0
    dev.check(want, 'second trip')


def test_argument_errors_launch_nothing():
    _, _, S, _ = mods()
    h = 8
    layout = S.strip_rows(scene(h), h, 2048, 16, 0.0)
    dev = Device(layout.out_bytes, lead=256)
    untouched = np.full((layout.out_bytes,), CANARY, np.uint8)
    assert dev.run(layout.rows, h) == 0
    lib, n = dev.lib, len(layout.rows)
    dev.buf.fill_(CANARY)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    arena, src, tab, out = p(dev.padded, 256), p(dev.d_sources), p(dev.d_table), p(dev.buf, 256)
    size, S_ = layout.out_bytes, len(dev.sources)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    calls = [(arena, dev.total, src, S_, tab, n, 0, out, size), (arena, dev.total, src, S_, tab, n, 257, out, size),
             (arena, dev.total, src, S_, tab, n, -8, out, size), (None, dev.total, src, S_, tab, n, h, out, size),
             (arena, dev.total, None, S_, tab, n, h, out, size), (arena, dev.total, src, S_, None, n, h, out, size),
             (arena, dev.total, src, S_, tab, n, h, None, size), (arena, dev.total, p(dev.d_sources, 4), S_, tab, n, h, out, size),
             (arena, dev.total, src, S_, p(dev.d_table, 4), n, h, out, size), (arena, dev.total, src, S_, tab, -1, h, out, size),
             (arena, dev.total, src, S_, tab, n, h, out, 1 << 40), (arena, dev.total, src, S_, tab, n, h, out, -1),
             (arena, 0, src, S_, tab, n, h, out, size), (arena, dev.total, src, 0, tab, n, h, out, size)]
    for k, args in enumerate(calls):
        assert lib.vkas_quad_strips_u8(*args, stream) != 0, k
    assert lib.vkas_quad_strips_u8(arena, dev.total, src, S_, tab, 0, h, out, size, stream) == 0  # n = 0: no launch
    torch.cuda.synchronize()
    dev.check(untouched, 'argument errors')
    ops = mods()[0]
    a, sources = dev.arena_copy, dev.sources
    for call in (lambda: ops.quad_strips_u8(a, sources, layout.rows, 0, size), lambda: ops.quad_strips_u8(a, sources, layout.rows, 257, size),
                 lambda: ops.quad_strips_u8(a, sources, layout.rows, h, 1 << 40), lambda: ops.quad_strips_u8(a, sources, layout.rows, h, size - 1),
                 lambda: ops.quad_strips_u8(a.view(1, -1), sources, layout.rows, h, size),
                 lambda: ops.quad_strips_u8(a, sources[:, :3], layout.rows, h, size),
                 lambda: ops.quad_strips_u8(a, sources, layout.rows[:, :11], h, size),
                 lambda: ops.quad_strips_u8(a, sources, layout.rows.astype(np.int32), h, size),
                 lambda: ops.quad_strips_u8(a[:100], sources, layout.rows, h, size),
                 lambda: ops.quad_strips_u8(a, sources, torch.from_numpy(S.strip_table(layout.rows, h))[:-1].cuda(), h, size),
                 lambda: ops.quad_strips_u8(a, torch.from_numpy(sources).cuda(), layout.rows, h, size, validate=False)):
        with pytest.raises(ValueError):
            call()


def test_eager_replay_and_second_run_agree():
    ops, _, S, _ = mods()
    h = 32
    layout = S.strip_rows(scene(h), h, 2048, 64, 0.125)
    arena, sources, d_sources = ops.image_arena(IMAGES, torch.device('cuda'))
    d_table = torch.from_numpy(S.strip_table(layout.rows, h)).cuda()
    want = host_bytes(S, layout.rows, h, layout.out_bytes)
    run = lambda: ops.quad_strips_u8(arena, d_sources, d_table, h, layout.out_bytes, validate=False)
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
    for name in ('image', 'status', 'squeezed', 'widths', 'bucket', 'index', 'rows'):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    for a, b in zip(got.buckets, want.buckets):
        assert a.is_cuda and a.dtype == torch.uint8 and tuple(a.shape) == b.shape and np.array_equal(a.cpu().numpy(), b)
    for k in np.flatnonzero(want.status == 0).tolist():
        assert np.array_equal(got.strip(k).cpu().numpy(), want.strip(k))


def test_inferencing_quad_strips_equals_the_host_route():
    ops, _, S, inf = mods()
    quads = scene(32)
    quads[1] = np.concatenate([quads[1], np.full((1, 4, 2), np.nan), C.box(0, 0, 64 * 32 + 1, 64)[None]])  # status 1 and 2
    want = inf.quad_strips_host(IMAGES, quads)
    assert sorted(set(want.status.tolist())) == [0, 1, 2] and len(want.buckets) >= 2 and want.height == 32
    assert_same_strips(inf.quad_strips(IMAGES, quads), want)
    arena, sources, d_sources = ops.image_arena(IMAGES, torch.device('cuda'))
    assert_same_strips(inf.quad_strips((arena, sources), quads), want)
    assert_same_strips(inf.quad_strips((arena, sources, d_sources), quads), want)
    assert_same_strips(inf.quad_strips([torch.from_numpy(m).cuda() for m in IMAGES], quads), want)
    got = inf.quad_strips(IMAGES, quads)
    assert got.buckets[0].untyped_storage().data_ptr() == got.buckets[-1].untyped_storage().data_ptr(), 'one allocation'
    pts = np.array([[0.0, 0.0], [32.0, 5.0]])
    assert np.array_equal(got.remap(0, pts), want.remap(0, pts))
    other = inf.quad_strips(IMAGES, quads, height=8, width_max=24, width_step=8, margin=0.0)
    assert_same_strips(other, inf.quad_strips_host(IMAGES, quads, 8, 24, 8, 0.0))
    assert other.squeezed.any()
    none = inf.quad_strips(IMAGES, [np.zeros((0, 4, 2))] * 3)
    assert none.buckets == [] and none.rows.shape == (0, 12)
    with pytest.raises(ValueError):
        inf.quad_strips(IMAGES, quads, device='cpu')
    with pytest.raises(ValueError):
        inf.quad_strips(IMAGES[:2], quads)
