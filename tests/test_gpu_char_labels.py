"""csrc/labels.hip on the MI355X, through ops.char_label_maps and through the raw C ABI, against the host oracle
dataset/labels.py::char_label_maps_host (itself held to an independent fill in tests/test_cpu_char_labels.py).

owner, mask and height are exact quantities (integers, and float32 arithmetic without contraction in a fixed order): they
are compared with torch.equal.  score is zero exactly where the oracle's is; elsewhere it is expf of the same float32
argument and may differ from the oracle's correctly rounded float64 exp by SCORE_ULPS float32 steps.  Every output buffer of
the raw calls starts as a canary with guard words behind it.  The scenes are tests/char_label_cases.py's: the smallest maps
that reach every branch (one tile; ragged tiles with scalar stores; a crop with 16-byte stores; B = 3 with counts (5, 0,
K); two table chunks) with exact ties, pixel centres on edges and corners, sub-pixel quads, quads outside map and crop, and
rotations in every one of them."""
import ctypes

import numpy as np
import pytest
import torch

from tests import char_label_cases as C

pytestmark = pytest.mark.gpu

# The bound on |device score - oracle score| in float32 steps, where the oracle's score is not zero: twice the largest
# distance to the float64 host oracle measured over this file's inputs on an MI355X, which is 1 step (every case, 8961 cells
# in the largest).  ROCm's documented expf accuracy (1 ulp) plus the oracle's own rounding gives the same 2.
SCORE_ULPS = 2
G = 64  # guard words behind every buffer the kernel writes
INT_CANARY, F_CANARY = -7777, -7777.0


def _lib():
    from vkit_ocr_model_adaptive_scaling_amd import _lib as L
    return L.lib, L.check


def ops_mod():
    from vkit_ocr_model_adaptive_scaling_amd import ops
    return ops


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def guarded(shape, fill, dtype):
    n = int(np.prod(shape))
    buf = torch.full((n + G,), fill, dtype=dtype, device='cuda')
    return buf[:n].view(shape), buf[n:]


def raw_call(c, rows=None, count=None, want=(True, True, True, True), K=None):
    """the C ABI on canary-filled, guarded buffers -> ([owner, mask, height, score] or None each, guards_ok)"""
    lib, check = _lib()
    rows = torch.from_numpy(np.array(c['rows'] if rows is None else rows)).cuda()
    count = torch.from_numpy(np.array(c['count'] if count is None else count, dtype=np.int32)).cuda()
    B, K = rows.shape[0], (rows.shape[1] if K is None else K)
    up, down, left, right = c['box']
    CH, CW = down - up + 1, right - left + 1
    bufs = [guarded((B, CH, CW), INT_CANARY if i == 0 else F_CANARY, torch.int32 if i == 0 else torch.float32) if w
            else (None, None) for i, w in enumerate(want)]
    check(lib.vkas_char_label_maps(p(rows), p(count), B, K, c['h'], c['w'], up, left, CH, CW, 2.0, *[p(b[0]) for b in bufs],
                                   st()), 'char_label_maps')
    torch.cuda.synchronize()
    ok = all(bool((g == (INT_CANARY if i == 0 else F_CANARY)).all()) for i, (_, g) in enumerate(bufs) if g is not None)
    return [None if b[0] is None else b[0].cpu().numpy() for b in bufs], ok


def assert_matches(got, ref, what=''):
    """got / ref: (owner, mask, height, score); None entries of got are skipped"""
    for name, g, r in zip(('owner', 'mask', 'height'), got, ref):
        if g is not None:
            assert np.array_equal(g, r), (what, name, int((g != r).sum()))
    if got[3] is not None:
        zero = ref[3] == 0
        assert np.array_equal(got[3] == 0, zero), (what, 'score zeros')
        d = C.ulp_distance(got[3][~zero], ref[3][~zero])
        worst = int(d.max()) if d.size else 0
        print(f'{what}: largest score distance {worst} float32 steps over {d.size} cells')
        assert worst <= SCORE_ULPS, (what, 'score', worst)


@pytest.mark.parametrize('name', C.CASES)
def test_raw_call_matches_the_oracle(name):
    c = C.case(name)
    got, guards = raw_call(c)
    assert guards, 'guard words overwritten'
    assert_matches(got, c['ref'], name)
    again, _ = raw_call(c)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), 'two calls differ'


@pytest.mark.parametrize('name', C.CASES)
def test_ops_call_matches_the_oracle(name):
    c = C.case(name)
    rows, count = torch.from_numpy(np.array(c['rows'])).cuda(), torch.from_numpy(np.array(c['count'])).cuda()
    out = ops_mod().char_label_maps(rows, count, c['h'], c['w'], c['box'], with_owner=True)
    assert out[0].dtype == torch.int32 and all(o.dtype == torch.float32 for o in out[1:])
    assert_matches([o.cpu().numpy() for o in out], c['ref'], name)
    part = ops_mod().char_label_maps(rows, count, c['h'], c['w'], c['box'], with_height=False)
    assert part[0] is None and part[2] is None and torch.equal(part[1], out[1]) and torch.equal(part[3], out[3])


def test_second_chunk_beats_first_and_ties_go_to_the_lower_index():
    got, _ = raw_call(C.case('two_chunks'))
    assert got[0][0, 5, 7] == 281
    got, _ = raw_call(C.case('one_tile'))
    assert (got[0][0, 2:8, 2:11] == 1).all() and got[0][0, 12, 8] == 3


@pytest.mark.parametrize('name', ['ragged_33x130', 'crop_3_5'])
def test_bad_rows_are_skipped_or_clipped(name):
    """valid = 0 rows, boxes that lie (too large, negative), counts outside [0, K]: guards intact, and the result is the
    oracle's on the cleaned table"""
    c = C.case(name)
    B, K, _ = c['rows'].shape
    oracle = lambda rows, count: C.char_label_maps_host(rows, count, c['h'], c['w'], c['box'])
    # rows marked invalid, wherever they sit, equal their removal
    dead = np.array(c['rows'])
    kill = [0, 4, K // 2, K - 1]
    dead[0, kill, 19] = 0
    clean = np.zeros_like(dead)
    keep = [i for i in range(K) if i not in kill]
    clean[0, :len(keep)] = c['rows'][0, keep]
    ref = oracle(clean, [len(keep)])
    renumber = np.concatenate([[0], np.array(keep) + 1])  # owner of the cleaned table -> owner of the original one
    got, guards = raw_call(c, rows=dead)
    assert guards
    assert_matches(got, (renumber[ref[0]].astype(np.int32),) + ref[1:], name + ' valid=0')
    # lying boxes: the inside test decides, the box is clipped to the tile
    lie = np.array(c['rows'])
    lie[0, 0::3, 8:12] = (0, 0, c['h'] + 100, c['w'] + 100)
    lie[0, 1::3, 8:12] = (-50, -(1 << 30), 1 << 30, (1 << 31) - 1)
    got, guards = raw_call(c, rows=lie)
    assert guards
    assert_matches(got, c['ref'], name + ' lying boxes')
    assert_matches(got, oracle(lie, c['count']), name + ' lying boxes, oracle on the same table')
    # count above K and below 0
    got, guards = raw_call(c, count=[K + 1000])
    assert guards
    assert_matches(got, c['ref'], name + ' count > K')
    got, guards = raw_call(c, count=[-5])
    assert guards and all(not g.any() for g in got)
    got, guards = raw_call(c, K=0)  # an empty table: zero maps
    assert guards and all(not g.any() for g in got)


def test_null_outputs_in_every_combination():
    c = C.case('ragged_17x65')
    full, _ = raw_call(c)
    for bits in range(1, 15):
        want = tuple(bool(bits >> i & 1) for i in range(4))
        got, guards = raw_call(c, want=want)
        assert guards, want
        for w, g, f in zip(want, got, full):
            assert (g is None) == (not w) and (g is None or g.tobytes() == f.tobytes()), want
    lib, _ = _lib()
    rows, count = torch.from_numpy(np.array(c['rows'])).cuda(), torch.from_numpy(np.array(c['count'])).cuda()
    assert lib.vkas_char_label_maps(p(rows), p(count), 1, rows.shape[1], 17, 65, 0, 0, 17, 65, 2.0, None, None, None, None,
                                    st()) == -1


def test_unaligned_outputs_take_the_scalar_stores():
    """CW % 4 == 0 but a mask that starts 4 bytes off a 16-byte boundary"""
    lib, check = _lib()
    c = C.case('crop_3_5')
    rows, count = torch.from_numpy(np.array(c['rows'])).cuda(), torch.from_numpy(np.array(c['count'])).cuda()
    up, down, left, right = c['box']
    CH, CW = down - up + 1, right - left + 1
    buf = torch.full((1 + CH * CW + G,), F_CANARY, dtype=torch.float32, device='cuda')
    mask = buf[1:1 + CH * CW]
    assert mask.data_ptr() % 16 == 4
    check(lib.vkas_char_label_maps(p(rows), p(count), 1, rows.shape[1], c['h'], c['w'], up, left, CH, CW, 2.0, None, p(mask),
                                   None, None, st()), 'char_label_maps')
    torch.cuda.synchronize()
    assert float(buf[0]) == F_CANARY and bool((buf[1 + CH * CW:] == F_CANARY).all())
    assert np.array_equal(mask.cpu().numpy().reshape(1, CH, CW), c['ref'][1])


def test_sigma_sets_k():
    c = C.case('one_tile')
    rows, count = torch.from_numpy(np.array(c['rows'])).cuda(), torch.from_numpy(np.array(c['count'])).cuda()
    for sigma in (0.35, 1.0):
        out = ops_mod().char_label_maps(rows, count, c['h'], c['w'], c['box'], sigma=sigma, with_owner=True)
        ref = C.char_label_maps_host(c['rows'], c['count'], c['h'], c['w'], c['box'], sigma=sigma)
        assert_matches([o.cpu().numpy() for o in out], ref, f'sigma {sigma}')


def test_captured_graph_replays_with_a_new_table():
    """capture-safe: a replay after the table was overwritten in place equals the eager result for the new table"""
    ops = ops_mod()
    a, b = C.case('ragged_33x130'), C.case('one_tile')
    K = a['rows'].shape[1]
    new_rows = np.zeros_like(a['rows'])
    new_rows[0, :b['rows'].shape[1]] = b['rows'][0][::-1]  # other quads, other order, on the same map
    new_count = np.array([b['rows'].shape[1]], dtype=np.int32)
    rows, count = torch.from_numpy(np.array(a['rows'])).cuda(), torch.from_numpy(np.array(a['count'])).cuda()
    run = lambda: ops.char_label_maps(rows, count, a['h'], a['w'], a['box'], with_owner=True)
    eager_a = [o.clone() for o in run()]
    torch.cuda.synchronize()
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
    assert all(torch.equal(s, e) for s, e in zip(static, eager_a))
    rows.copy_(torch.from_numpy(new_rows))
    count.copy_(torch.from_numpy(new_count))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [s.clone() for s in static]
    eager_b = run()
    torch.cuda.synchronize()
    assert all(torch.equal(r, e) for r, e in zip(replayed, eager_b))
    assert_matches([r.cpu().numpy() for r in replayed],
                   C.char_label_maps_host(new_rows, new_count, a['h'], a['w'], a['box']), 'replayed')
    assert not torch.equal(replayed[0], eager_a[0])
