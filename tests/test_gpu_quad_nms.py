"""The suppression kernels of csrc/quadmatch.hip on the MI355X, through the raw C ABI, ops.quad_rows / ops.nms_quads and
inferencing.nms_quads, against the host oracles inferencing.match_rows and inferencing/nms.py::nms_quads_host (itself held
to a rounds restatement in tests/test_cpu_quad_nms.py).

Everything is compared for equality: rows, keep, suppressor, the six statistics and the rounds.  Every output of the raw
calls and the workspace start as canaries between guard words.  Shapes are the smallest that reach each path: one tile,
ragged tiles, several tiles, B = 3 with counts (5, 0, K), the 8192 limit."""
import ctypes

import numpy as np
import pytest
import torch

from tests import quad_match_cases as C
from tests import quad_nms_cases as Q
from vkit_ocr_model_adaptive_scaling_amd.inferencing import evaluation as E
from vkit_ocr_model_adaptive_scaling_amd.inferencing import nms as N

pytestmark = pytest.mark.gpu

G = 64  # guard elements in front of and behind every buffer the kernels write
CANARY = 0x5B


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


def guarded(shape, dtype):
    """a canary-filled buffer (every byte CANARY) with G guard elements on either side -> (view, bytes of the whole)"""
    n = int(np.prod(shape))
    size = torch.empty((), dtype=dtype).element_size()
    raw = torch.full(((n + 2 * G) * size,), CANARY, dtype=torch.uint8, device='cuda')
    return raw[G * size:(G + n) * size].view(dtype).view(shape), raw, G * size, n * size


def intact(g):
    _, raw, lead, body = g
    return bool((raw[:lead] == CANARY).all()) and bool((raw[lead + body:] == CANARY).all())


def untouched(g):
    _, raw, _, _ = g
    return bool((raw == CANARY).all())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw_nms(rows, count, probs, thr=0.5, max_pairs=None, expect_rc=0, **over):
    """the C ABI on canary-filled buffers between guards -> ((keep, suppressor, stats, rounds), guards_ok, outputs untouched)"""
    lib, _ = _lib()
    rows, probs = dev(np.asarray(rows, np.int32)), dev(np.asarray(probs, np.float32))
    count = dev(np.asarray(count, dtype=np.int32))
    B, K = rows.shape[0], rows.shape[1]
    max_pairs = 4 * K if max_pairs is None else max_pairs
    nbytes = lib.vkas_quad_nms_workspace_bytes(B, K, max(max_pairs, 0))
    assert nbytes >= 0
    ws = torch.full((nbytes + 512,), 0x5A, dtype=torch.uint8, device='cuda')
    outs = [guarded((B, K), torch.uint8), guarded((B, K), torch.int32), guarded((B, 6), torch.int64),
            guarded((B,), torch.int32)]
    a = dict(B=B, K=K, thr=thr, cap=max_pairs, nbytes=nbytes)
    a.update(over)
    rc = lib.vkas_quad_nms(p(rows), p(count), p(probs), a['B'], a['K'], a['thr'], a['cap'], p(ws[256:]), a['nbytes'],
                           *[p(o[0]) for o in outs], st())
    torch.cuda.synchronize()
    assert rc == expect_rc, lib.vkas_last_error()
    ok = all(intact(o) for o in outs) and bool((ws[:256] == 0x5A).all()) and bool((ws[256 + nbytes:] == 0x5A).all())
    return [o[0].cpu().numpy() for o in outs], ok, all(untouched(o) for o in outs)


def assert_equal(got, ref, what=''):
    for name, g, r in zip(('keep', 'suppressor', 'stats'), got, ref):
        assert g.dtype == r.dtype and np.array_equal(g, r), (what, name, g.tolist() if g.size < 40 else int((g != r).sum()),
                                                              r.tolist() if r.size < 40 else '')


def check_table(table, what, thr=0.5, **kw):
    ref = N.nms_quads_host(*table, thr)
    got, guards, _ = raw_nms(*table, thr=thr, **kw)
    assert guards, 'guard words overwritten'
    assert_equal(got, ref, what)
    for b in range(len(table[1])):
        assert got[3][b] == Q.rounds_of(table[0][b], table[1][b], table[2][b], thr), (what, 'rounds', b)
    return got, ref


# ---- vkas_quad_rows ------------------------------------------------------------------------------------------------------

def rows_inputs():
    """seeded quads with everything the rule distinguishes -> (quads (2, K, 4, 2), valid (2, K) uint8)"""
    rng = np.random.default_rng(8)
    quads = [C.rotated(*rng.uniform(-3000, 3000, 2), *rng.uniform(2, 80, 2), rng.uniform(0, 360)) for _ in range(300)]
    quads += [C.random_pair(rng)[0] for _ in range(60)]
    sq = lambda y, x, h, w: np.array(C.SQ(y, x, h, w), np.float64)
    edge = 2.0 ** 15
    quads += [sq(-edge, -edge, 2 * edge, 2 * edge), sq(-edge, -edge, 2 * edge + 1 / 16, 2 * edge),  # +-2^19 and a step beyond
              sq(-edge - 1 / 16, 0, 8, 8), sq(0, edge - 8, 8, 8), sq(0, edge - 8, 8, 8 + 1 / 32), sq(0, edge - 8, 8, 8 + 3 / 32)]
    ties = sq(0, 0, 9, 9) + np.array([0.5, 1.5, 2.5, -0.5, -1.5, 3.5, 0.25, 0.75]).reshape(4, 2) / 16  # .5 / 16 ties
    quads += [ties, ties + 1 / 32, -ties[::-1] + 40, sq(1 / 32, 3 / 32, 5 + 1 / 32, 7 + 3 / 32)]
    quads += [q[::-1] for q in quads[:20]]                                     # anticlockwise
    quads += [sq(5, 5, 0, 8), sq(5, 5, 8, 0), sq(5, 5, 0, 0), np.array([[0, 0], [0, 8], [8, 8], [4, 4.0]]),  # degenerate, reflex
              np.array([[0, 0], [0, 8], [0, 16], [8, 0.0]]), np.array([[0, 0], [8, 8], [0, 8], [8, 0.0]])]   # collinear, crossed
    for bad in (np.nan, np.inf, -np.inf, 1e300, -1e300, 1e-320):
        q = sq(3, 4, 10, 12)
        q[int(rng.integers(0, 4)), int(rng.integers(0, 2))] = bad
        quads.append(q)
    quads.append(np.full((4, 2), np.nan))
    quads = np.stack(quads)
    K = (len(quads) + 1) // 2
    quads = np.concatenate([quads, np.zeros((2 * K - len(quads), 4, 2))]).reshape(2, K, 4, 2)
    valid = (rng.uniform(size=(2, K)) < 0.85).astype(np.uint8) * rng.integers(1, 256, (2, K)).astype(np.uint8)
    return quads, valid


def test_quad_rows_equals_match_rows():
    lib, _ = _lib()
    quads, valid = rows_inputs()
    B, K = valid.shape
    for v in (valid, None):
        ref, ok = E.match_rows(quads.reshape(-1, 4, 2), None if v is None else v.reshape(-1))
        out = guarded((B, K, 16), torch.int32)
        d_quads, d_valid = dev(quads), None if v is None else dev(v)  # held until the call has run
        rc = lib.vkas_quad_rows(p(d_quads), p(d_valid), B, K, p(out[0]), st())
        torch.cuda.synchronize()
        assert rc == 0 and intact(out)
        got = out[0].cpu().numpy().reshape(-1, 16)
        assert np.array_equal(got, ref), np.flatnonzero((got != ref).any(axis=1))[:10]
        through_ops = ops_mod().quad_rows(dev(quads), None if v is None else dev(v))
        assert through_ops.dtype == torch.int32 and np.array_equal(through_ops.cpu().numpy().reshape(-1, 16), ref)
    # on the oracle: the inputs reach both sides of every test
    ref, ok = E.match_rows(quads.reshape(-1, 4, 2))
    assert 300 < ok.sum() < len(ok) - 30 and abs(ref[:, :8]).max() == 1 << 19
    assert (valid == 0).sum() > 20 and (valid > 1).sum() > 100
    empty = ops_mod().quad_rows(torch.zeros((0, 5, 4, 2), dtype=torch.float64, device='cuda'))
    assert tuple(empty.shape) == (0, 5, 16)


# ---- vkas_quad_nms -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(Q.hand_cases()))
def test_hand_cases_through_the_c_abi(name):
    rows, count, probs, thr, keep, suppressor, rounds = Q.hand_cases()[name]
    got, _ = check_table((rows[None], [count], probs[None]), name, thr=thr)
    assert got[0][0].tolist() == keep and got[1][0].tolist() == suppressor and got[2][0].tolist() == Q.hand_stats(name)
    assert got[3][0] == rounds


@pytest.mark.parametrize('K', [1, 63, 64, 65, 129])
def test_sizes(K):
    got, ref = check_table(Q.random_table(200 + K, 1, K), f'K = {K}')
    assert K == 1 or (ref[2][0, 3] > ref[2][0, 4] > 0 and 0 < ref[2][0, 0] < K)


def test_batch_with_an_empty_image_and_counts_outside_the_table():
    K = 70
    got, ref = check_table(Q.random_table(5, 3, K, (5, 0, K)), 'batch')
    assert ref[2][1].tolist() == [0] * 6 and ref[2][2, 0] < K and (got[0][1] == 0).all() and (got[0][0, 5:] == 0).all()
    check_table(Q.random_table(6, 3, K, (-4, K + 50, 1 << 30)), 'counts outside [0, K]')


def test_bad_tables_stay_inside_the_buffers():
    rows, count, probs = Q.random_table(9, 2, 66)
    lie = rows.copy()
    lie[:, 0::4, 8:12] = (0, 0, 4000, 4000)                        # covers everything: clipped against every quad
    lie[:, 1::4, 8:12] = (100000, 100000, 100100, 100100)          # far away: pruned
    lie[:, 2::4, 8:12] = (50, 50, 10, 10)                          # empty
    lie[0, 3, 8:12] = (-(1 << 30), -(1 << 30), 1 << 30, 1 << 30)   # the origin moves 2^30 away
    lie[0, 7, 12:14] = (-5, -1)                                    # a negative area
    lie[:, 0::5, 12:14] = (0, 0)                                   # zero areas
    lie[:, 9, 14] = -3                                             # valid is any non-zero word
    got, ref = check_table((lie, count, probs), 'lying boxes and areas', thr=0.25, max_pairs=66 * 66)
    assert ref[2][:, 3].min() > 16 * 16


def test_chain_of_forty_needs_forty_rounds():
    rows, probs, keep, suppressor, rounds = Q.chain_case()
    got, _ = check_table((rows[None], [40], probs[None]), 'chain')
    assert np.array_equal(got[0][0], keep) and np.array_equal(got[1][0], suppressor) and got[3][0] == rounds == 40


def test_seeded_page():
    table, ref = Q.page_reference(2)
    # on the oracle alone, never skipped
    assert table[1][0] == 330 and 330 - ref[2][0, 0] >= 20 and ref[2][0, 0] >= 250
    got, guards, _ = raw_nms(*table)
    assert guards
    assert_equal(got, ref, 'page')
    assert got[3][0] == Q.rounds_of(table[0][0], 330, table[2][0])
    print(f'page: stats {ref[2][0].tolist()}, {got[3][0]} rounds')


def test_capacity():
    table = Q.random_table(21, 3, 48, (20, 48, 30))
    ref = N.nms_quads_host(*table)
    cand = ref[2][:, 4]
    assert cand[1] > cand[0] and cand[1] > cand[2] and cand.min() > 0
    got, guards, _ = raw_nms(*table, max_pairs=int(cand[1]) - 1)
    assert guards
    assert got[2][1].tolist() == [48, 48, ref[2][1, 2], ref[2][1, 3], cand[1], 1] and got[3][1] == 0
    assert (got[0][1] == 1).all() and (got[1][1] == -1).all()
    for b in (0, 2):  # the other images are unaffected
        assert_equal([o[b:b + 1] for o in got], [o[b:b + 1] for o in ref], f'beside an overflow, image {b}')
    got, guards, _ = raw_nms(*table, max_pairs=int(cand[1]))
    assert guards
    assert_equal(got, ref, 'capacity = candidates')
    got, guards, _ = raw_nms(*table, max_pairs=0)
    assert guards and got[2][:, 5].tolist() == [1, 1, 1] and np.array_equal(got[2][:, 1:5], ref[2][:, 1:5])
    assert np.array_equal(got[0], np.arange(48)[None] < np.array([20, 48, 30])[:, None]) and (got[1] == -1).all()


def test_nms_quads_retries_and_equals_the_host_route():
    rng = np.random.default_rng(4)
    heap = np.stack([np.array(C.SQ(10, 10, 20, 20), float) + rng.uniform(-1, 1, (4, 2)) for _ in range(30)])
    quads, probs = Q.page(3)
    quads, probs = quads[:40], probs[:40]
    args = ([heap, quads, quads[:0]], [rng.uniform(0.5, 1, 30).astype(np.float32), probs, probs[:0]])
    ref, ref_stats = N.nms_quads_lists_host(*args, iou_thr=0.3, score_thr=0.55)
    present = int((args[1][0] >= 0.55).sum())
    assert ref_stats[4] - 0 >= present * (present - 1) // 2 > 4 * 40, 'the default capacity must overflow: a retry'
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import nms_quads
    res, stats = nms_quads(*args, iou_thr=0.3, score_thr=0.55)
    assert np.array_equal(stats, ref_stats) and len(res) == 3 and stats[5] == 0
    for a, b in zip(res, ref):
        assert np.array_equal(a.keep, b.keep) and np.array_equal(a.suppressor, b.suppressor) and np.array_equal(a.valid, b.valid)
        assert a.keep.dtype == np.bool_ and a.suppressor.dtype == np.int32
    assert res[0].keep.sum() == 1 and res[2].keep.shape == (0,)
    empty = nms_quads([], [])
    assert empty[0] == [] and empty[1].tolist() == [0] * 6


def test_ops_call_graph_replay_and_determinism():
    ops = ops_mod()
    a, b = Q.random_table(31, 2, 70), Q.random_table(32, 2, 70, (70, 3))
    d = [dev(t) for t in a]
    rounds = torch.full((2,), -7777, dtype=torch.int32, device='cuda')
    run = lambda: ops.nms_quads(*d, rounds=rounds)
    first = run()
    assert [o.dtype for o in first] == [torch.uint8, torch.int32, torch.int64] and first[2].shape == (2, 6)
    ref_a, ref_b = N.nms_quads_host(*a), N.nms_quads_host(*b)
    assert_equal([o.cpu().numpy() for o in first], ref_a, 'ops, eager')
    assert rounds.cpu().tolist() == [Q.rounds_of(a[0][k], a[1][k], a[2][k]) for k in range(2)]
    again = run()
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(first, again)), 'two eager runs differ'
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    graph.replay()
    assert_equal([o.cpu().numpy() for o in outs], ref_a, 'replayed')
    for dst, t in zip(d, b):  # rewritten tables, the same buffers
        dst.copy_(torch.from_numpy(np.ascontiguousarray(t)))
    graph.replay()
    assert_equal([o.cpu().numpy() for o in outs], ref_b, 'replayed over rewritten tables')
    assert rounds.cpu().tolist() == [Q.rounds_of(b[0][k], b[1][k], b[2][k]) for k in range(2)]
    assert ref_b[2][1, 1] == 3 and ref_a[2][:, 0].min() > 3 and not np.array_equal(ref_a[0], ref_b[0])


def test_the_limit_of_8192_quads():
    K = 8192
    small_rows, _, small_probs = Q.random_table(41, 1, 40)
    at = np.r_[0:20, K - 20:K]  # duplicates in the first and the last tile only; monotone, so the ranks carry over
    rows, probs = np.zeros((2, K, 16), np.int32), np.zeros((2, K), np.float32)
    rows[:, at], probs[:, at] = small_rows[0], small_probs[0]
    small = N.nms_quads_host(small_rows, [40], small_probs)
    got, guards, _ = raw_nms(rows, [K, K], probs, max_pairs=256)
    assert guards and all(np.array_equal(o[0], o[1]) for o in got)
    want_keep = np.ones((K,), np.uint8)  # the zero rows between them take no part: kept
    want_keep[at] = small[0][0]
    want_sup = np.full((K,), -1, np.int32)
    want_sup[at] = np.where(small[1][0] >= 0, at[small[1][0]], -1)
    want_stats = small[2].copy()
    want_stats[0, 0] += K - 40
    want_stats[0, 1] = K
    assert_equal([o[:1] for o in got[:3]], (want_keep[None], want_sup[None], want_stats), 'K = 8192')
    assert got[3][0] == Q.rounds_of(small_rows[0], 40, small_probs[0]) and 40 - small[2][0, 0] > 3
    assert (small[1][0][20:] >= 0).any() and (small[1][0][:20] >= 0).any()


def test_argument_errors_launch_nothing():
    lib, _ = _lib()
    rows, count, probs = Q.random_table(51, 1, 8)
    for over, word in (({'K': 8193}, b'1..8192'), ({'K': 0}, b'1..8192'), ({'B': -1}, b'bad B'), ({'thr': 0.0}, b'iou_thr'),
                       ({'thr': 1.5}, b'iou_thr'), ({'cap': -2}, b'max_pairs'), ({'nbytes': 16}, b'needed')):
        got, guards, clean = raw_nms(rows, count, probs, expect_rc=-1, **over)
        assert word in lib.vkas_last_error(), (over, lib.vkas_last_error())
        assert guards and clean, (over, 'an output was written')
    assert lib.vkas_quad_nms_workspace_bytes(1, 8193, 8) == -1 and lib.vkas_quad_nms_workspace_bytes(1, 8, -1) == -1
    out = guarded((1, 8, 16), torch.int32)
    assert lib.vkas_quad_rows(p(dev(np.zeros((1, 8, 4, 2)))), None, -1, 8, p(out[0]), st()) == -1 and untouched(out)
    assert lib.vkas_quad_rows(None, None, 1, 8, p(out[0]), st()) == -1 and untouched(out)
    ops = ops_mod()
    d = [dev(rows), dev(count), dev(probs)]
    big = torch.zeros((1, 8193, 16), dtype=torch.int32, device='cuda')
    for bad in (lambda: ops.nms_quads(big, d[1], torch.zeros((1, 8193), device='cuda')),
                lambda: ops.nms_quads(d[0], d[1], d[2], iou_thr=0.0),
                lambda: ops.nms_quads(d[0], d[1], d[2].double()),
                lambda: ops.nms_quads(d[0], d[1], d[2][:, :4]),
                lambda: ops.nms_quads(d[0], d[1], d[2], max_pairs=-1),
                lambda: ops.nms_quads(d[0].cpu(), d[1], d[2]),
                lambda: ops.quad_rows(torch.zeros((1, 8, 4, 2), device='cuda')),
                lambda: ops.quad_rows(torch.zeros((1, 8, 4, 2), dtype=torch.float64, device='cuda'),
                                      torch.zeros((1, 7), dtype=torch.uint8, device='cuda'))):
        with pytest.raises((ValueError, RuntimeError)):
            bad()


def test_quad_match_is_unchanged_on_a_seeded_page():
    """vkas_quad_match shares its tile body with the suppression: its answer on the seeded page of test_gpu_quad_match.py is
    still the oracle's, gt_iou bit for bit."""
    ops = ops_mod()
    tables, ref, _ = C.page_reference(2)
    outs = ops.match_quads(*[dev(t) for t in tables[:4]])
    got = [o.cpu().numpy() for o in outs]
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[3], ref[3])
    assert got[2].tobytes() == ref[2].tobytes() and ref[3][0, 0] > 200
