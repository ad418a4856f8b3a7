"""The ranked matching of csrc/quadmatch.hip on the MI355X, through the raw C ABI, ops.match_quads_ranked and
inferencing.evaluate_quads_ranked, against the host oracles of inferencing/ranking.py: match_quads_ranked_host (the sorted
sequential form) and match_quads_ranked_rounds_host (the rounds, with their count), themselves held to each other in
tests/test_cpu_quad_rank.py.

Everything is compared for equality: matches, states, the IoUs bit for bit, coverage, both statistics tables and the
rounds.  Every output of the raw calls and the workspace start as canaries between guard words.  Shapes are the smallest
that reach each path: one tile, ragged tiles, several tiles, T = 1, 3 and 16, B = 3 with counts (5, 0, K), the 8192 limit."""
import ctypes

import numpy as np
import pytest
import torch

from tests import quad_match_cases as C
from tests import quad_rank_cases as Q
from vkit_ocr_model_adaptive_scaling_amd.inferencing import ranking as R

pytestmark = pytest.mark.gpu

G = 64  # guard elements in front of and behind every buffer the kernels write
CANARY = 0x5B
NAMES = ('pred_match', 'pred_state', 'gt_match', 'pred_iou', 'covered', 'stats', 'dc_stats', 'rounds')
THR3 = (0.3, 0.5, 0.7)
THR16 = tuple(0.2 + 0.05 * i for i in range(16))


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
    """a canary-filled buffer (every byte CANARY) with G guard elements on either side -> (view, raw, lead bytes, body bytes)"""
    n = int(np.prod(shape))
    size = torch.empty((), dtype=dtype).element_size()
    raw = torch.full(((n + 2 * G) * size,), CANARY, dtype=torch.uint8, device='cuda')
    return raw[G * size:(G + n) * size].view(dtype).view(shape), raw, G * size, n * size


def intact(g):
    _, raw, lead, body = g
    return bool((raw[:lead] == CANARY).all()) and bool((raw[lead + body:] == CANARY).all())


def untouched(g):
    return bool((g[1] == CANARY).all())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw_ranked(gt_rows, gt_count, gt_care, pred_rows, pred_count, probs, thrs, cover_thr=0.5, max_pairs=None, expect_rc=0,
               **over):
    """the C ABI on canary-filled buffers between guards -> (the eight outputs, guards_ok, outputs untouched)"""
    lib, _ = _lib()
    d = [dev(np.asarray(gt_rows, np.int32)), dev(np.asarray(gt_count, np.int32)),
         None if gt_care is None else dev(np.asarray(gt_care, np.uint8)), dev(np.asarray(pred_rows, np.int32)),
         dev(np.asarray(pred_count, np.int32)), dev(np.asarray(probs, np.float32))]
    B, M, N, T = d[0].shape[0], d[0].shape[1], d[3].shape[1], len(thrs)
    max_pairs = 4 * max(M, N) if max_pairs is None else max_pairs
    nbytes = lib.vkas_quad_match_ranked_workspace_bytes(B, M, N, min(max(T, 1), 16), max(max_pairs, 0))
    assert nbytes >= 0
    ws = torch.full((nbytes + 512,), 0x5A, dtype=torch.uint8, device='cuda')
    Ts = max(T, 1)
    outs = [guarded((B, Ts, N), torch.int32), guarded((B, Ts, N), torch.uint8), guarded((B, Ts, M), torch.int32),
            guarded((B, Ts, N), torch.float64), guarded((B, N), torch.uint8), guarded((B, Ts, 8), torch.int64),
            guarded((B, 3), torch.int64), guarded((B, Ts), torch.int32)]
    a = dict(B=B, M=M, N=N, T=T, cover=cover_thr, cap=max_pairs, nbytes=nbytes)
    a.update(over)
    host_thrs = (ctypes.c_double * max(len(thrs), 1))(*thrs)
    rc = lib.vkas_quad_match_ranked(p(d[0]), p(d[1]), p(d[2]), p(d[3]), p(d[4]), p(d[5]), a['B'], a['M'], a['N'],
                                    ctypes.cast(host_thrs, ctypes.c_void_p), a['T'], a['cover'], a['cap'], p(ws[256:]),
                                    a['nbytes'], *[p(o[0]) for o in outs], st())
    torch.cuda.synchronize()
    assert rc == expect_rc, lib.vkas_last_error()
    ok = all(intact(o) for o in outs) and bool((ws[:256] == 0x5A).all()) and bool((ws[256 + nbytes:] == 0x5A).all())
    return [o[0].cpu().numpy() for o in outs], ok, all(untouched(o) for o in outs)


def assert_equal(got, ref, what=''):
    for name, g, r in zip(NAMES, got, ref):
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name, g.dtype, r.dtype, g.shape, r.shape)
        same = g.tobytes() == r.tobytes() if name == 'pred_iou' else np.array_equal(g, r)
        assert same, (what, name, g.tolist() if g.size < 40 else int((g != r).sum()), r.tolist() if r.size < 40 else '')


def check_table(table, thrs, what, cover_thr=0.5, **kw):
    """device == rounds oracle (all eight outputs) == sorted oracle (the first seven), guards intact"""
    pairs = R.ranked_pairs(*table, thrs, cover_thr)
    ref = R.match_quads_ranked_rounds_host(*table, thrs, cover_thr, pairs=pairs)
    seq = R.match_quads_ranked_host(*table, thrs, cover_thr, pairs=pairs)
    got, guards, _ = raw_ranked(*table, thrs, cover_thr, **kw)
    assert guards, 'guard words overwritten'
    assert_equal(got, ref, what)
    assert_equal(got[:7], seq, what + ' (sorted form)')
    return got, ref


@pytest.mark.parametrize('name', list(Q.hand_cases()))
def test_hand_cases_through_the_c_abi(name):
    table, thrs, cover, states, match, covered, n_gt, dc_stats, rounds = Q.hand_cases()[name]
    got, _ = check_table(table, thrs, name, cover)
    assert got[1][0].tolist() == states and got[0][0].tolist() == match and got[4][0].tolist() == covered
    assert got[5][0, :, 3].tolist() == [n_gt] * len(thrs) and got[6][0].tolist() == dc_stats and got[7][0].tolist() == rounds


@pytest.mark.parametrize('K', [1, 63, 64, 65, 129])
def test_sizes(K):
    got, ref = check_table(Q.random_tables(300 + K, 1, K, K), THR3, f'M = N = {K}')
    assert K == 1 or (ref[5][0, 0, 5] > ref[5][0, 0, 6] > ref[5][0, 2, 6] > 0 and ref[6][0, 2] > 0 and ref[5][0, 0, 0] > 0)


def test_sizes_differ_between_the_sides_and_sixteen_thresholds():
    got, ref = check_table(Q.random_tables(11, 1, 65, 129), THR16, 'M = 65, N = 129, T = 16')
    cand = ref[5][0, :, 6]
    assert (np.diff(cand) <= 0).all() and cand[0] > cand[-1] and len(set(ref[5][0, :, 0].tolist())) > 3
    check_table(Q.random_tables(12, 1, 129, 63), (0.5,), 'M = 129, N = 63, T = 1')
    table = Q.random_tables(13, 2, 40, 40)
    check_table((table[0], table[1], None) + table[3:], THR3, 'gt_care = NULL')


def test_batch_with_an_empty_image_and_counts_outside_the_table():
    K = 70
    got, ref = check_table(Q.random_tables(5, 3, K, K, (5, 0, K), (5, 0, K)), THR3, 'batch')
    assert not ref[5][1].any() and not ref[6][1].any() and (got[1][1] == 0).all() and (got[1][0, :, 5:] == 0).all()
    assert (got[7][1] == 0).all() and ref[5][2, 0, 0] > 10
    check_table(Q.random_tables(6, 3, K, K, (-4, K + 50, 1 << 30), (K + 1, -1, 1 << 30)), THR3, 'counts outside [0, K]')
    check_table(Q.random_tables(7, 2, K, K, (K, 0), (0, K)), THR3, 'one side empty')


def test_bad_tables_stay_inside_the_buffers():
    gt, cg, care, pred, cp, probs = Q.random_tables(9, 2, 66, 66)
    for lie in (gt, pred):
        lie[:, 0::4, 8:12] = (0, 0, 4000, 4000)                        # covers everything: clipped against every quad
        lie[:, 1::4, 8:12] = (100000, 100000, 100100, 100100)          # far away: pruned
        lie[:, 2::4, 8:12] = (50, 50, 10, 10)                          # empty
        lie[0, 3, 8:12] = (-(1 << 30), -(1 << 30), 1 << 30, 1 << 30)   # the origin moves 2^30 away
        lie[0, 7, 12:14] = (-5, -1)                                    # a negative area
        lie[:, 0::5, 12:14] = (0, 0)                                   # zero areas
        lie[:, 9, 14] = -3                                             # valid is any non-zero word
    got, ref = check_table((gt, cg, care, pred, cp, probs), (0.25, 0.5), 'lying boxes and areas', max_pairs=66 * 66)
    assert ref[5][:, 0, 5].min() > 16 * 16 and ref[6][:, 1].min() > 16


def test_chain_of_forty_needs_forty_rounds():
    table, thrs, states, match, rounds = Q.chain_case()
    got, _ = check_table(table, thrs, 'chain')
    assert np.array_equal(got[1][0], states) and np.array_equal(got[0][0], match) and got[7][0].tolist() == rounds == [40, 1]


def test_seeded_page():
    table, pairs, ref = Q.page_reference(2)
    thrs = Q.PAGE_THRS
    # on the oracle alone, never skipped: no IoU within 1e-10 of a threshold, no coverage within 1e-10 of cover_thr
    ious = pairs[0].ious
    assert min(np.abs(ious - t).min() for t in thrs) > 1e-10 and pairs[0].cover_margin > 1e-10
    stats, dc = ref[5][0], ref[6][0]
    assert table[1][0] == 270 and dc[0] == 15 and dc[2] >= 25 and stats[0, 3] == 255
    assert stats[0, 0] > 200 and stats[-1, 0] < stats[0, 0] // 2 and stats[0, 2] >= 20 and stats[0, 1] >= 20
    got, guards, _ = raw_ranked(*table, thrs)
    assert guards
    assert_equal(got, ref, 'page')
    print(f'page: stats at 0.50 {stats[0].tolist()}, at 0.95 {stats[-1].tolist()}, dc {dc.tolist()}, rounds {got[7][0].tolist()}')


def test_capacity():
    table = Q.random_tables(21, 3, 48, 48, (20, 48, 30), (48, 48, 25))
    ref = R.match_quads_ranked_rounds_host(*table, THR3)
    cand = ref[5][:, 0, 6]
    assert cand[1] > cand[0] and cand[1] > cand[2] and cand.min() > 0
    got, guards, _ = raw_ranked(*table, THR3, max_pairs=int(cand[1]) - 1)
    assert guards
    want = ref[5][1].copy()  # the true counts at every threshold; no result
    want[:, :3], want[:, 7] = 0, 1
    assert np.array_equal(got[5][1], want) and (got[7][1] == 0).all()
    assert (got[1][1] == 0).all() and (got[0][1] == -1).all() and (got[2][1] == -1).all() and (got[3][1] == 0).all()
    assert np.array_equal(got[4], ref[4]) and np.array_equal(got[6], ref[6])  # coverage does not depend on the capacity
    for b in (0, 2):  # the other images are unaffected
        assert_equal([o[b:b + 1] for o in got], [o[b:b + 1] for o in ref], f'beside an overflow, image {b}')
    got, guards, _ = raw_ranked(*table, THR3, max_pairs=int(cand[1]))
    assert guards
    assert_equal(got, ref, 'capacity = candidates')
    got, guards, _ = raw_ranked(*table, THR3, max_pairs=0)
    assert guards and (got[5][:, :, 7] == 1).all() and np.array_equal(got[5][:, :, 3:7], ref[5][:, :, 3:7])
    assert (got[1] == 0).all() and (got[0] == -1).all() and not got[5][:, :, :3].any()


def test_evaluate_quads_ranked_retries_and_equals_the_host_route():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import evaluate_quads_ranked, evaluate_quads_ranked_host
    rng = np.random.default_rng(4)
    heap = np.stack([np.array(C.SQ(10, 10, 20, 20), float) + rng.uniform(-1, 1, (4, 2)) for _ in range(30)])
    gt, care, pred, probs = Q.page(3)
    gt, care, pred, probs = gt[:40], care[:40], pred[:50], probs[:50]
    args = ([heap, pred, pred[:0]], [heap[:12], gt, gt[:0]], [rng.uniform(0.5, 1, 30).astype(np.float32), probs, probs[:0]],
            [np.ones(12, np.uint8), care, care[:0]])
    thrs = (0.3, 0.6)
    ref, ref_score = evaluate_quads_ranked_host(*args, iou_thrs=thrs)
    assert ref[0].stats[0, 6] > 4 * 50, 'the default capacity must overflow: a retry'
    res, score = evaluate_quads_ranked(*args, iou_thrs=thrs)
    assert len(res) == 3 and score.iou_thrs == thrs and res[2].pred_state.shape == (2, 0)
    for a, b in zip(res, ref):
        for f in ('pred_state', 'pred_match', 'gt_match', 'covered', 'gt_valid', 'gt_care', 'pred_valid', 'stats', 'dc_stats'):
            assert np.array_equal(getattr(a, f), getattr(b, f)) and getattr(a, f).dtype == getattr(b, f).dtype, f
        assert a.pred_iou.tobytes() == b.pred_iou.tobytes() and not a.stats[:, 7].any()
    assert np.array_equal(score.ap, ref_score.ap) and score.map == ref_score.map and score.n_gt == ref_score.n_gt == 12 + int(
        sum(r.stats[0, 3] for r in ref[1:]))
    assert np.array_equal(score.tp, ref_score.tp) and score.best == ref_score.best and 0 < score.map < 1
    assert res[0].stats[0, 0] == 12 and res[0].stats[0, 1] == 18
    empty = evaluate_quads_ranked([], [], [])
    assert empty[0] == [] and empty[1].map == 0.0 and empty[1].n_gt == 0


def test_ops_call_graph_replay_and_determinism():
    ops = ops_mod()
    a, b = Q.random_tables(31, 2, 70, 70), Q.random_tables(32, 2, 70, 70, (70, 3), (4, 70))
    d = [dev(t) for t in a]
    rounds = torch.full((2, 3), -7777, dtype=torch.int32, device='cuda')
    run = lambda: ops.match_quads_ranked(*d, THR3, rounds=rounds)
    first = run()
    assert [o.dtype for o in first] == [torch.int32, torch.uint8, torch.int32, torch.float64, torch.uint8, torch.int64,
                                        torch.int64]
    assert first[5].shape == (2, 3, 8) and first[0].shape == (2, 3, 70) and first[6].shape == (2, 3)
    ref_a, ref_b = R.match_quads_ranked_rounds_host(*a, THR3), R.match_quads_ranked_rounds_host(*b, THR3)
    assert_equal([o.cpu().numpy() for o in first] + [rounds.cpu().numpy()], ref_a, 'ops, eager')
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
    assert_equal([o.cpu().numpy() for o in outs] + [rounds.cpu().numpy()], ref_a, 'replayed')
    for dst, t in zip(d, b):  # rewritten tables, the same buffers
        dst.copy_(torch.from_numpy(np.ascontiguousarray(t)))
    graph.replay()
    assert_equal([o.cpu().numpy() for o in outs] + [rounds.cpu().numpy()], ref_b, 'replayed over rewritten tables')
    assert ref_b[5][1, 0, 3] <= 3 and ref_a[5][:, 0, 0].min() > 3 and not np.array_equal(ref_a[1], ref_b[1])


def test_the_limit_of_8192_quads():
    K = 8192
    small = Q.random_tables(41, 1, 40, 40)
    at = np.r_[0:20, K - 20:K]  # quads in the first and the last tile only; monotone, so the ranks carry over
    gt, pred = np.zeros((2, K, 16), np.int32), np.zeros((2, K, 16), np.int32)
    care, probs = np.ones((2, K), np.uint8), np.zeros((2, K), np.float32)
    gt[:, at], pred[:, at], care[:, at], probs[:, at] = small[0][0], small[3][0], small[2][0], small[5][0]
    ref = R.match_quads_ranked_rounds_host(*small, THR3)
    got, guards, _ = raw_ranked(gt, [K, K], care, pred, [K, K], probs, THR3, max_pairs=256)
    assert guards and all(np.array_equal(o[0], o[1]) for o in got)
    back = np.full((K,), -1, np.int32)
    want_state, want_pm = np.zeros((3, K), np.uint8), np.full((3, K), -1, np.int32)
    want_gm, want_iou, want_cov = np.full((3, K), -1, np.int32), np.zeros((3, K)), np.zeros((K,), np.uint8)
    want_state[:, at], want_iou[:, at], want_cov[at] = ref[1][0], ref[3][0], ref[4][0]
    want_pm[:, at] = np.where(ref[0][0] >= 0, at[ref[0][0]], -1)
    want_gm[:, at] = np.where(ref[2][0] >= 0, at[ref[2][0]], -1)
    assert_equal([o[:1] for o in got], (want_pm[None], want_state[None], want_gm[None], want_iou[None], want_cov[None],
                                        ref[5], ref[6], ref[7]), 'K = 8192')
    assert (ref[0][0][:, 20:] >= 0).any() and (ref[0][0][:, :20] >= 0).any() and ref[6][0, 2] > 0 and ref[7][0].max() > 1


def test_argument_errors_launch_nothing():
    lib, _ = _lib()
    table = Q.random_tables(51, 1, 8, 8)
    cases = (({'N': 8193}, (0.5,), b'1..8192'), ({'M': 0}, (0.5,), b'1..8192'), ({'B': -1}, (0.5,), b'bad B'),
             ({}, (0.0, 0.5), b'(0, 1]'), ({}, (0.5, 1.5), b'(0, 1]'), ({}, (0.5, 0.5), b'ascend'), ({}, (0.6, 0.5), b'ascend'),
             ({'T': 0}, (0.5,), b'1..16'), ({'T': 17}, tuple(0.1 + 0.05 * i for i in range(17)), b'1..16'),
             ({'cover': 0.0}, (0.5,), b'cover_thr'), ({'cover': 1.25}, (0.5,), b'cover_thr'), ({'cap': -2}, (0.5,), b'max_pairs'),
             ({'nbytes': 16}, (0.5,), b'needed'), ({'B': 4096}, THR16, b'65535'))
    for over, thrs, word in cases:
        got, guards, clean = raw_ranked(*table, thrs, expect_rc=-1, **over)
        assert word in lib.vkas_last_error(), (over, lib.vkas_last_error())
        assert guards and clean, (over, 'an output was written')
    assert lib.vkas_quad_match_ranked_workspace_bytes(1, 8193, 8, 1, 8) == -1
    assert lib.vkas_quad_match_ranked_workspace_bytes(1, 8, 8, 17, 8) == -1
    assert lib.vkas_quad_match_ranked_workspace_bytes(4096, 8, 8, 16, 8) == -1
    ops = ops_mod()
    d = [dev(t) for t in table]
    for bad in (lambda: ops.match_quads_ranked(*d, (0.5, 0.5)), lambda: ops.match_quads_ranked(*d, ()),
                lambda: ops.match_quads_ranked(*d, (0.5,), cover_thr=0.0),
                lambda: ops.match_quads_ranked(*d[:5], d[5].double(), (0.5,)),
                lambda: ops.match_quads_ranked(d[0], d[1], d[2][:, :4], d[3], d[4], d[5], (0.5,)),
                lambda: ops.match_quads_ranked(*d, (0.5,), max_pairs=-1),
                lambda: ops.match_quads_ranked(d[0].cpu(), *d[1:], (0.5,)),
                lambda: ops.match_quads_ranked(*d, (0.5,), rounds=torch.zeros((1,), dtype=torch.int32, device='cuda'))):
        with pytest.raises((ValueError, RuntimeError)):
            bad()


def test_quad_match_is_unchanged_on_a_seeded_page():
    """vkas_quad_match shares its tile body with the ranked matching: its answer on the seeded page of
    test_gpu_quad_match.py is still the oracle's, gt_iou bit for bit."""
    ops = ops_mod()
    tables, ref, _ = C.page_reference(2)
    outs = ops.match_quads(*[dev(t) for t in tables[:4]])
    got = [o.cpu().numpy() for o in outs]
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[3], ref[3])
    assert got[2].tobytes() == ref[2].tobytes() and ref[3][0, 0] > 200
