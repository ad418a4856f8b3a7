"""ops.crop_warp_blur (the blur kernels of csrc/crops.hip) against dataset/blur.py::crop_blur_host on the MI355X, bit for bit
(float32 compared as int32 views): the scenes of tests/blur_cases.py - one tile, a halo of 7 across tile borders on every
side, ragged tiles with plain stores, an unaligned plane, radii 0, 1, 3 and 7 over three sources in one batch; every log2n,
rotations, crops partly and wholly outside the page, the three kinds of table; photometric off, at the clamps, with noise -,
radius_max above the table's maximum, all radii 0 against ops.crop_warp, the impulse response, hostile tables behind
validate=False with canaries around the output, the work buffer and the arena, a work buffer that is too small, a captured
graph replayed over rewritten rows and blur rows, and run-to-run determinism."""
import numpy as np
import pytest
import torch

from tests import blur_cases as BC
from tests import crop_cases as C

pytestmark = pytest.mark.gpu

CANARY = 0x5A


@pytest.fixture(scope='module', autouse=True)
def release_device_memory():
    """the canary-filled buffers and work planes of this module go back to the driver: the tests after it allocate as they
    would without it"""
    yield
    torch.cuda.empty_cache()


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


@pytest.mark.parametrize('radius_max', [None, 7])
@pytest.mark.parametrize('name', ['one_tile', 'halo_48x192', 'ragged_37x70', 'batch4'])
def test_equals_the_oracle(name, radius_max):
    c = BC.case(name)
    arena, table = upload(c)
    out = ops_mod().crop_warp_blur(arena, table, np.array(c['rows']), np.array(c['blur']), c['size'], radius_max=radius_max)
    assert_bits(out, c['ref'], name)
    radii = c['blur'][:, 0].tolist()
    if name == 'one_tile':
        assert sorted(c['rows'][:, 7].tolist()) == [0, 0, 1, 2, 3] and max(radii) == 3   # radius_max = 7 is above the table's
    elif name == 'halo_48x192':
        assert radii[:2] == [7, 7]
    elif name == 'batch4':
        assert radii == [0, 1, 3, 7] and c['rows'][0, 0] == c['rows'][3, 0]              # two rows share a source
        assert [int(v) for v in table[:, 1] * table[:, 2]] == [1, 23 * 37, 300 * 200]


def test_unaligned_plane_and_canaries():
    """the output starts 4 bytes into a 16-byte aligned buffer: plain stores; nothing before or after it is written, and
    nothing behind the planes of the work buffer"""
    ops = ops_mod()
    c = BC.case('unaligned_32x128')
    arena, table = upload(c)
    B, (H, W) = len(c['rows']), c['size']
    n = B * 3 * H * W
    buf = torch.full((n + 64,), float('nan'), dtype=torch.float32, device='cuda')
    guard = buf.clone()
    assert buf.data_ptr() % 16 == 0
    out = buf[1:1 + n].view(B, 3, H, W)
    radius_max = int(c['blur'][:, 0].max())
    need = ops.crop_blur_work_bytes(B, c['size'], radius_max)
    work = torch.full((need + 256,), CANARY, dtype=torch.uint8, device='cuda')
    got = ops.crop_warp_blur(arena, table, np.array(c['rows']), np.array(c['blur']), c['size'], out=out, work=work)
    assert got.data_ptr() == out.data_ptr() and got.data_ptr() % 16 == 4
    assert_bits(got, c['ref'], 'unaligned')
    for part in (slice(0, 1), slice(1 + n, None)):
        assert torch.equal(buf[part].view(torch.int32), guard[part].view(torch.int32))
    assert bool((work[need:] == CANARY).all())
    aligned = ops.crop_warp_blur(arena, table, np.array(c['rows']), np.array(c['blur']), c['size'])  # the 16-byte stores
    assert aligned.data_ptr() % 16 == 0
    assert_bits(aligned, c['ref'], 'aligned')


def test_all_radii_zero_on_device_tables_is_crop_warp():
    """device tables are not looked at on the host: the two launches run, and give crop_warp's output bit for bit"""
    ops = ops_mod()
    for name in ('one_tile', 'ragged_37x70'):
        c = C.case(name)
        arena, table = upload(c)
        dev = arena.device
        d_sources, d_rows = torch.from_numpy(table).to(dev), torch.from_numpy(np.array(c['rows'])).to(dev)
        d_blur = torch.from_numpy(np.stack([BC.identity_blur_row()] * len(c['rows']))).to(dev)
        want = ops.crop_warp(arena, d_sources, d_rows, c['size'], validate=False)
        for radius_max in (None, 0, 3):
            got = ops.crop_warp_blur(arena, d_sources, d_rows, d_blur, c['size'], validate=False, radius_max=radius_max)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (name, radius_max)
        assert_bits(want, c['ref'], name)
        # host tables of radius 0 take crop_warp itself: the work buffer is not touched
        work = torch.full((ops.crop_blur_work_bytes(len(c['rows']), c['size'], 7),), CANARY, dtype=torch.uint8, device=dev)
        got = ops.crop_warp_blur(arena, table, np.array(c['rows']), d_blur.cpu().numpy(), c['size'], work=work)
        assert_bits(got, c['ref'], name)
        assert bool((work == CANARY).all())


def test_the_device_impulse_response():
    ops = ops_mod()
    page = np.zeros((40, 50, 3), np.uint8)
    page[20, 30] = 255
    size = (40, 50)
    arena, table, _ = ops.image_arena([page], torch.device('cuda'))
    row = C.affine_row(size, 1.0, 0.0, (20.0, 25.0))
    for blur in (BC.radius_row(7, 11), BC.motion_blur_row(9.0, 0.5), BC.radius_row(3, 12)):
        out = ops.crop_warp_blur(arena, table, row[None], blur[None], size)
        want = np.zeros((1, 3) + size, np.float32)
        want[0, :, 13:28, 23:38] = (255 * blur[1:].astype(np.int64).reshape(15, 15)[::-1, ::-1]).astype(np.float32) * np.float32(2.0 ** -16)
        assert_bits(out, want, 'impulse')


def test_hostile_tables_behind_validate_false():
    """What unchecked tables give is stated by the rule: a zero image for a blur row that is invalid - radius 9 or -1, a sum
    off by one, a weight of 65537 or -1, a weight outside the square - or above radius_max, and for the bad crop rows of
    tests/test_gpu_crops.py; every other image equals the oracle, and nothing outside the output, the planes of the work
    buffer and - read only - the arena is touched (canaries around all three)."""
    ops = ops_mod()
    c = BC.case('batch4')
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
    good = BC.radius_row(3, 14)
    centre = 1 + 7 * 15 + 7

    def edit(word, value, fix=None):
        r = good.copy()
        r[word] = value
        if fix is not None:
            r[fix] -= value - good[word]
        return r
    hostile = [edit(0, 9), edit(0, -1), edit(centre, good[centre] + 1), edit(centre, good[centre] - 1),
               edit(centre, 65537, centre + 1), edit(centre + 1, -1, centre), edit(centre + 4, 5, centre),
               BC.radius_row(6, 15)]                                 # valid, but above radius_max = 5
    base_rows, base_blur = np.array(c['rows']), np.array(c['blur'])
    base_blur[3] = BC.radius_row(5, 16)                              # the scene's radius 7 would be above radius_max too
    rows = np.concatenate([base_rows, np.repeat(base_rows[:1], len(hostile) + 7, axis=0)])
    blur = np.concatenate([base_blur, np.stack(hostile), np.repeat(good[None], 7, axis=0)])
    k = 4 + len(hostile)                                             # bad crop rows under a good blur row
    rows[k, 0], rows[k + 1, 0], rows[k + 2, 0], rows[k + 3, 0], rows[k + 4, 0] = -1, S + 3, S, S + 1, S + 2
    rows[k + 5, 7] = 7                                               # log2n = 7: clamped to 3
    rows[k + 6, 3] = (1 << 22) + 1                                   # a coefficient out of bounds: a zero image
    B, (H, W) = len(rows), c['size']
    want = np.zeros((B, 3, H, W), np.float32)
    want[:4] = BC.crop_blur_host(c['sources'], base_rows, base_blur, c['size'])
    clamped = base_rows[:1].copy()
    clamped[0, 7] = 3
    want[k + 5] = BC.crop_blur_host(c['sources'], clamped, good[None], c['size'])[0]
    told = [i for i in range(B) if i not in (k + 2, k + 3, k + 4, 4 + len(hostile) - 1)]   # source entries, radius_max: the op's
    host_rule = BC.crop_blur_host(c['sources'], rows[told], blur[told], c['size'], strict=False)
    assert np.array_equal(bits(host_rule), bits(want[told]))         # the host states the same rule
    assert want[:4].any(axis=(1, 2, 3)).all() and want[k + 5].any()
    n = B * 3 * H * W
    buf = torch.full((n + 128,), float('nan'), dtype=torch.float32, device=dev)
    guard = buf.clone()
    out = buf[64:64 + n].view(B, 3, H, W)
    need = ops.crop_blur_work_bytes(B, c['size'], 5)
    work_buf = torch.full((need + 512,), CANARY, dtype=torch.uint8, device=dev)
    work = work_buf[256:256 + need]
    assert work.data_ptr() % 16 == 0
    d_sources, d_rows, d_blur = (torch.from_numpy(a).to(dev) for a in (sources, rows, blur))
    ops.crop_warp_blur(inner, d_sources, d_rows, d_blur, c['size'], validate=False, out=out, work=work, radius_max=5)
    torch.cuda.synchronize()
    assert_bits(out, want, 'hostile')
    for part in (slice(0, 64), slice(64 + n, None)):
        assert torch.equal(buf[part].view(torch.int32), guard[part].view(torch.int32))
    assert bool((work_buf[:256] == CANARY).all()) and bool((work_buf[256 + need:] == CANARY).all())
    assert bool((padded[:256] == CANARY).all()) and bool((padded[256 + total:] == CANARY).all())
    assert torch.equal(inner, arena)
    with pytest.raises(ValueError):      # the same tables are refused when they are checked
        ops.crop_warp_blur(inner, d_sources, d_rows, d_blur, c['size'], validate=True, radius_max=5)


def test_a_small_work_buffer_raises_before_any_launch():
    ops = ops_mod()
    from vkit_ocr_model_adaptive_scaling_amd import _lib
    c = BC.case('one_tile')
    arena, table = upload(c)
    dev = arena.device
    B, size = len(c['rows']), c['size']
    d_sources, d_rows, d_blur = (torch.from_numpy(np.array(a)).to(dev) for a in (table, c['rows'], c['blur']))
    out = torch.full((B, 3) + size, -7.0, dtype=torch.float32, device=dev)
    need = ops.crop_blur_work_bytes(B, size, 7)
    work = torch.full((need,), CANARY, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match='work'):
        ops.crop_warp_blur(arena, d_sources, d_rows, d_blur, size, validate=False, out=out, work=work[:need - 16])
    with pytest.raises(ValueError, match='work'):
        ops.crop_warp_blur(arena, d_sources, d_rows, d_blur, size, validate=False, out=out, work=work[4:])   # not 16-byte aligned
    p = lambda t: t.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    rc = _lib.lib.vkas_crop_warp_blur_f32(p(arena), int(arena.numel()), p(d_sources), 1, p(d_rows), p(d_blur), B, 7, p(work),
                                          need - 1, p(out), size[0], size[1], stream)
    assert rc == -1 and b'work' in _lib.lib.vkas_last_error()
    rc = _lib.lib.vkas_crop_warp_blur_f32(p(arena), int(arena.numel()), p(d_sources), 1, p(d_rows), p(d_blur), B, 8, p(work),
                                          need, p(out), size[0], size[1], stream)
    assert rc == -1 and b'radius_max' in _lib.lib.vkas_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((work == CANARY).all())   # nothing was launched
    empty = ops.crop_warp_blur(arena, table, np.array(c['rows'])[:0], np.array(c['blur'])[:0], size)
    assert tuple(empty.shape) == (0, 3) + size


def test_captured_graph_replays_over_rewritten_tables_and_runs_are_identical():
    ops = ops_mod()
    a, b = BC.case('one_tile'), BC.case('ragged_37x70')
    dev = torch.device('cuda')
    arena, table = upload(a)
    B, size = len(a['rows']), a['size']
    d_sources = torch.from_numpy(table).to(dev)
    d_rows = torch.from_numpy(np.array(a['rows'])).to(dev)
    d_blur = torch.from_numpy(np.array(a['blur'])).to(dev)
    work = torch.empty((ops.crop_blur_work_bytes(B, size, 7),), dtype=torch.uint8, device=dev)
    run = lambda: ops.crop_warp_blur(arena, d_sources, d_rows, d_blur, size, validate=False, work=work)
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
    # other rows on the same page and size: the maps and the blur rows of the ragged scene, the photometric words reversed
    new_rows = np.array(a['rows'])
    new_rows[:, 1:8] = b['rows'][:5, 1:8]
    new_rows[:, 8:] = a['rows'][::-1, 8:]
    new_blur = np.array(b['blur'])
    assert int(new_blur[:, 0].max()) > int(a['blur'][:, 0].max())    # the replay meets radii the capture did not
    want = BC.crop_blur_host(a['sources'], new_rows, new_blur, size)
    assert not np.array_equal(want, a['ref'])
    d_rows.copy_(torch.from_numpy(new_rows))
    d_blur.copy_(torch.from_numpy(new_blur))
    for k in (2, 3):
        graph.replay()
        torch.cuda.synchronize()
        assert_bits(static, want, f'replay {k}')
