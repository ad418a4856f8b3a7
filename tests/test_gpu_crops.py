"""ops.crop_warp (csrc/crops.hip) against dataset/crops.py::crop_host on the MI355X, bit for bit (float32 compared as int32
views): the scenes of tests/crop_cases.py - one tile, ragged tiles with plain stores, an unaligned plane, three sources of
different sizes in one arena; every log2n, rotations, crops partly and wholly outside the page, fy == 0 and fx == 0 taps;
photometric off, at the clamps, with noise -, hostile tables behind validate=False with canaries around the output and the
arena, a captured graph replayed over rewritten rows, run-to-run determinism and the argument errors."""
import numpy as np
import pytest
import torch

from tests import crop_cases as C

pytestmark = pytest.mark.gpu

CANARY = 0x5A


def ops_mod():
    from vkit_ocr_model_adaptive_scaling_amd import ops
    return ops


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def assert_bits(got: torch.Tensor, want: np.ndarray, what=''):
    g = got.cpu().numpy()
    assert g.dtype == np.float32 and g.shape == want.shape, what
    bad = np.argwhere(bits(g) != bits(want))
    assert len(bad) == 0, f'{what}: {len(bad)} elements differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]} != {want[tuple(bad[0])]}'


def upload(c):
    arena, table, _ = ops_mod().image_arena(c['sources'], torch.device('cuda'))
    return arena, table


@pytest.mark.parametrize('name', ['one_tile', 'ragged_37x70', 'batch3'])
def test_equals_the_oracle(name):
    c = C.case(name)
    arena, table = upload(c)
    out = ops_mod().crop_warp(arena, table, np.array(c['rows']), c['size'])
    assert_bits(out, c['ref'], name)
    if name == 'batch3':
        assert [int(v) for v in table[:, 1] * table[:, 2]] == [1, 5 * 8192, 300 * 200]
        assert c['rows'][0, 0] == c['rows'][3, 0]  # two rows share a source


def test_unaligned_plane_and_canaries():
    """the output starts 4 bytes into a 16-byte aligned buffer: plain stores; nothing before or after it is written"""
    c = C.case('unaligned_32x128')
    arena, table = upload(c)
    B, (H, W) = len(c['rows']), c['size']
    n = B * 3 * H * W
    buf = torch.full((n + 64,), float('nan'), dtype=torch.float32, device='cuda')
    guard = buf.clone()
    assert buf.data_ptr() % 16 == 0
    out = buf[1:1 + n].view(B, 3, H, W)
    got = ops_mod().crop_warp(arena, table, np.array(c['rows']), c['size'], out=out)
    assert got.data_ptr() == out.data_ptr() and got.data_ptr() % 16 == 4
    assert_bits(got, c['ref'], 'unaligned')
    for part in (slice(0, 1), slice(1 + n, None)):
        assert torch.equal(buf[part].view(torch.int32), guard[part].view(torch.int32))
    aligned = ops_mod().crop_warp(arena, table, np.array(c['rows']), c['size'])  # the same rows through the 16-byte stores
    assert aligned.data_ptr() % 16 == 0
    assert_bits(aligned, c['ref'], 'aligned')


def test_hostile_tables_behind_validate_false():
    """What an unchecked table gives is stated by the rule: a zero image for a source index outside [0, S) and for a source
    entry that leaves the arena or has a side out of range, log2n clamped to [0, 3]; every other image equals the oracle,
    and nothing outside the output is written (canaries around the output and around the arena)."""
    ops = ops_mod()
    c = C.case('batch3')
    dev = torch.device('cuda')
    arena, table = upload(c)
    total = int(arena.numel())
    padded = torch.full((total + 512,), CANARY, dtype=torch.uint8, device=dev)
    padded[256:256 + total] = arena
    inner = padded[256:256 + total]
    S = len(table)
    sources = np.concatenate([table, [[total - 100, 20, 20, 0],      # offset + 3*20*20 exceeds the arena
                                      [0, 8193, 4, 0],               # a side above 8192
                                      [-16, 4, 4, 0]]])              # a negative offset
    base = np.array(c['rows'])
    rows = np.concatenate([base, base[:1], base[:1], base[:1], base[:1], base[:1], base[1:2], base[:1]])
    rows[4, 0], rows[5, 0], rows[6, 0], rows[7, 0], rows[8, 0] = -1, S + 3, S, S + 1, S + 2
    rows[9, 7] = 7                       # log2n = 7: clamped to 3
    rows[10, 3] = (1 << 22) + 1          # a coefficient out of bounds: a zero image
    B, (H, W) = len(rows), c['size']
    want = np.zeros((B, 3, H, W), np.float32)
    want[:4] = c['ref']
    clamped = base[1:2].copy()
    clamped[0, 7] = 3
    want[9] = C.crop_host(c['sources'], clamped, c['size'])[0]
    host_rule = C.crop_host(c['sources'], rows[[0, 1, 2, 3, 4, 5, 9, 10]], c['size'], strict=False)
    assert np.array_equal(bits(host_rule), bits(want[[0, 1, 2, 3, 4, 5, 9, 10]]))  # the host states the same rule
    n = B * 3 * H * W
    buf = torch.full((n + 128,), float('nan'), dtype=torch.float32, device=dev)
    guard = buf.clone()
    out = buf[64:64 + n].view(B, 3, H, W)
    d_sources, d_rows = torch.from_numpy(sources).to(dev), torch.from_numpy(rows).to(dev)
    ops.crop_warp(inner, d_sources, d_rows, c['size'], validate=False, out=out)
    torch.cuda.synchronize()
    assert_bits(out, want, 'hostile')
    for part in (slice(0, 64), slice(64 + n, None)):
        assert torch.equal(buf[part].view(torch.int32), guard[part].view(torch.int32))
    assert bool((padded[:256] == CANARY).all()) and bool((padded[256 + total:] == CANARY).all())
    assert torch.equal(inner, arena)
    with pytest.raises(ValueError):      # the same tables are refused when they are checked
        ops.crop_warp(inner, d_sources, d_rows, c['size'], validate=True)


def test_captured_graph_replays_over_rewritten_rows_and_runs_are_identical():
    ops = ops_mod()
    a, b = C.case('one_tile'), C.case('ragged_37x70')
    dev = torch.device('cuda')
    arena, table = upload(a)
    d_sources = torch.from_numpy(table).to(dev)
    d_rows = torch.from_numpy(np.array(a['rows'])).to(dev)
    run = lambda: ops.crop_warp(arena, d_sources, d_rows, a['size'], validate=False)
    first, second = run(), run()
    torch.cuda.synchronize()
    assert first.data_ptr() != second.data_ptr() and torch.equal(first.view(torch.int32), second.view(torch.int32))
    assert_bits(first, a['ref'], 'eager')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = run()
    graph.replay()
    torch.cuda.synchronize()
    assert_bits(static, a['ref'], 'replay 1')
    # other rows on the same page and size: the maps of the ragged scene's first five rows, the photometric words reversed
    new_rows = np.array(a['rows'])
    new_rows[:, 1:8] = b['rows'][:5, 1:8]
    new_rows[:, 8:] = a['rows'][::-1, 8:]
    want = C.crop_host(a['sources'], new_rows, a['size'])
    assert not np.array_equal(want, a['ref'])
    d_rows.copy_(torch.from_numpy(new_rows))
    for k in (2, 3):
        graph.replay()
        torch.cuda.synchronize()
        assert_bits(static, want, f'replay {k}')


def test_argument_errors_launch_nothing():
    ops = ops_mod()
    c = C.case('one_tile')
    arena, table = upload(c)
    rows, size = np.array(c['rows']), c['size']
    B = len(rows)
    out = torch.full((B, 3) + size, -7.0, dtype=torch.float32, device='cuda')

    def bad_row(word, value):
        r = rows.copy()
        r[1, word] = value
        return r
    big = table.copy()
    big[0, 0] = 16
    calls = [lambda: ops.crop_warp(arena.view(1, -1), table, rows, size, out=out),
             lambda: ops.crop_warp(arena.to(torch.int8), table, rows, size, out=out),
             lambda: ops.crop_warp(arena[::2], table, rows, size, out=out),
             lambda: ops.crop_warp(arena, table[:, :3], rows, size, out=out),
             lambda: ops.crop_warp(arena, table.astype(np.int32), rows, size, out=out),
             lambda: ops.crop_warp(arena, table[:0], rows, size, out=out),
             lambda: ops.crop_warp(arena, big, rows, size, out=out),                 # the source leaves the arena
             lambda: ops.crop_warp(arena, table, rows[:, :12], size, out=out),
             lambda: ops.crop_warp(arena, table, rows.astype(np.int32), size, out=out),
             lambda: ops.crop_warp(arena, table, bad_row(0, 1), size, out=out),
             lambda: ops.crop_warp(arena, table, bad_row(7, 4), size, out=out),
             lambda: ops.crop_warp(arena, table, bad_row(4, 1 << 23), size, out=out),
             lambda: ops.crop_warp(arena, table, bad_row(8, 0x7FC00000), size, out=out),
             lambda: ops.crop_warp(arena, table, rows, (0, 64), out=out),
             lambda: ops.crop_warp(arena, table, rows, (16, 8193), out=out),
             lambda: ops.crop_warp(arena, table, rows, 64, out=out),
             lambda: ops.crop_warp(arena, table, rows, size, out=out[:, :, :, ::2]),
             lambda: ops.crop_warp(arena, table, rows, size, out=out.double()),
             lambda: ops.crop_warp(arena, table, rows, size, out=out[:2]),
             lambda: ops.crop_warp(arena, torch.from_numpy(table).cuda(), rows, size, validate=False, out=out)]
    for k, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f'call {k} did not raise')
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.crop_warp(arena.cpu(), table, rows, size)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())  # nothing was launched
    empty = ops.crop_warp(arena, table, rows[:0], size)
    assert tuple(empty.shape) == (0, 3) + size
