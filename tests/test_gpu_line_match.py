"""csrc/linematch.hip on the MI355X, through the raw C ABI, ops.match_lines and inferencing.evaluate_lines, against the host
oracles of inferencing/line_evaluation.py: match_lines_host (the sequential form, the definition) and
match_lines_rounds_host (the rounds, with their counts), themselves held to each other in tests/test_cpu_line_match.py.

Everything is compared for equality: kinds, groups, the statistics and the rounds.  Every output of the raw calls and the
workspace start as canaries between guard words.  Shapes are the smallest that reach each path: one tile, ragged tiles,
several tiles, B = 3 with counts (5, 0, K), the 8192 limit."""
import ctypes

import numpy as np
import pytest
import torch

from tests import line_match_cases as Q
from vkit_ocr_model_adaptive_scaling_amd.inferencing import evaluation as E
from vkit_ocr_model_adaptive_scaling_amd.inferencing import line_evaluation as L

pytestmark = pytest.mark.gpu

G = 64  # guard elements in front of and behind every buffer the kernels write
CANARY = 0x5B
NAMES = ('gt_kind', 'gt_group', 'pred_kind', 'pred_group', 'stats', 'rounds')


def _lib():
    from vkit_ocr_model_adaptive_scaling_amd import _lib as lib_mod
    return lib_mod.lib, lib_mod.check


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
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw_lines(gt_rows, gt_count, gt_care, pred_rows, pred_count, recall_thr=0.8, precision_thr=0.4, cover_thr=0.5,
              max_pairs=None, expect_rc=0, **over):
    """the C ABI on canary-filled buffers between guards -> (the six outputs, guards_ok, outputs untouched)"""
    lib, _ = _lib()
    d = [dev(np.asarray(gt_rows, np.int32)), dev(np.asarray(gt_count, np.int32)),
         None if gt_care is None else dev(np.asarray(gt_care, np.uint8)), dev(np.asarray(pred_rows, np.int32)),
         dev(np.asarray(pred_count, np.int32))]
    B, M, N = d[0].shape[0], d[0].shape[1], d[3].shape[1]
    max_pairs = 4 * max(M, N) if max_pairs is None else max_pairs
    nbytes = lib.vkas_line_match_workspace_bytes(B, M, N, max(max_pairs, 0))
    assert nbytes >= 0
    ws = torch.full((nbytes + 512,), 0x5A, dtype=torch.uint8, device='cuda')
    outs = [guarded((B, M), torch.uint8), guarded((B, M), torch.int32), guarded((B, N), torch.uint8),
            guarded((B, N), torch.int32), guarded((B, 16), torch.int64), guarded((B, 2), torch.int32)]
    a = dict(B=B, M=M, N=N, tr=int(np.rint(recall_thr * 256)), tp=int(np.rint(precision_thr * 256)), cover=cover_thr,
             cap=max_pairs, nbytes=nbytes)
    a.update(over)
    rc = lib.vkas_line_match(p(d[0]), p(d[1]), p(d[2]), p(d[3]), p(d[4]), a['B'], a['M'], a['N'], a['tr'], a['tp'], a['cover'],
                             a['cap'], p(ws[256:]), a['nbytes'], *[p(o[0]) for o in outs], st())
    torch.cuda.synchronize()
    assert rc == expect_rc, lib.vkas_last_error()
    ok = all(intact(o) for o in outs) and bool((ws[:256] == 0x5A).all()) and bool((ws[256 + nbytes:] == 0x5A).all())
    return [o[0].cpu().numpy() for o in outs], ok, all(untouched(o) for o in outs)


def assert_equal(got, ref, what=''):
    for name, g, r in zip(NAMES, got, ref):
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name, g.dtype, r.dtype, g.shape, r.shape)
        assert np.array_equal(g, r), (what, name, g.tolist() if g.size < 40 else int((g != r).sum()),
                                      r.tolist() if r.size < 40 else '')


def check_table(t, what, params=None, **kw):
    """device == sequential oracle (five outputs) == rounds oracle (all six), guards intact"""
    params = params or {}
    pairs = L.line_pairs(*t, **params)
    seq = L.match_lines_host(*t, **params, pairs=pairs)
    ref = L.match_lines_rounds_host(*t, **params, pairs=pairs)
    got, guards, _ = raw_lines(*t, **params, **kw)
    assert guards, 'guard words overwritten'
    assert_equal(got[:5], seq, what + ' (sequential form)')
    assert_equal(got, ref, what)
    return got, ref


@pytest.mark.parametrize('name', list(Q.hand_cases()))
def test_hand_cases_through_the_c_abi(name):
    t, params, gk, gg, pk, pg, stats = Q.hand_cases()[name]
    got, _ = check_table(t, name, params)
    assert got[0][0].tolist() == gk and got[1][0].tolist() == gg and got[2][0].tolist() == pk and got[3][0].tolist() == pg
    for key, value in stats.items():
        assert got[4][0, L.STAT_NAMES.index(key)] == value, key


@pytest.mark.parametrize('name', list(Q.equality_cases()))
def test_comparisons_at_equality_through_the_c_abi(name):
    t, params, gk, pk = Q.equality_cases()[name]
    got, _ = check_table(t, name, params)
    assert got[0][0].tolist() == gk and got[2][0].tolist() == pk


@pytest.mark.parametrize('K', [1, 3, 64, 65, 130])
def test_sizes(K):
    got, ref = check_table(Q.random_tables(300 + K, 1, K, K), f'M = N = {K}')
    st_ = ref[4][0]
    assert K < 64 or (st_[2] > 3 and st_[3] > 3 and st_[5] >= 2 and st_[7] > 0 and st_[9] > st_[10] > 0), st_.tolist()


def test_sizes_differ_between_the_sides_and_gt_care_null():
    check_table(Q.random_tables(11, 1, 65, 130), 'M = 65, N = 130')
    check_table(Q.random_tables(12, 1, 130, 63), 'M = 130, N = 63')
    t = Q.random_tables(13, 2, 40, 40)
    got, ref = check_table((t[0], t[1], None) + t[3:], 'gt_care = NULL')
    assert not ref[4][:, 7].any() and not ref[4][:, 8].any()


def test_split_and_merge_across_tiles():
    """a split whose parts lie in two different pred tiles and a merge whose parts lie in two different gt tiles"""
    line, words = Q.BAR(0, 100), [Q.BAR(0, 45), Q.BAR(55, 45)]
    far = lambda k: Q.BAR(1000 + 40 * k, 30, y=500)  # fillers that meet nothing else
    pred = [far(k) for k in range(130)]
    pred[3], pred[100] = words
    got, _ = check_table(Q.table([line], pred), 'split over two pred tiles')
    assert got[0][0].tolist() == [3] and np.flatnonzero(got[2][0] == 3).tolist() == [3, 100] and got[4][0, 12] == 1
    gts = [far(k) for k in range(130)]
    gts[60], gts[70] = Q.BAR(0, 40), Q.BAR(50, 40)
    got, _ = check_table(Q.table(gts, [Q.BAR(0, 90)]), 'merge over two gt tiles')
    assert got[2][0].tolist() == [4] and np.flatnonzero(got[0][0] == 4).tolist() == [60, 70] and got[4][0, 13] == 1


def test_batch_with_an_empty_image_and_counts_outside_the_table():
    K = 70
    got, ref = check_table(Q.random_tables(5, 3, K, K, (5, 0, K), (5, 0, K)), 'batch')
    assert not ref[4][1].any() and (got[0][1] == 0).all() and (got[2][1] == 0).all() and (got[0][0, 5:] == 0).all()
    assert (got[5][1] == 0).all() and ref[4][2, 2] > 5
    check_table(Q.random_tables(6, 3, K, K, (-4, K + 50, 1 << 30), (K + 1, -1, 1 << 30)), 'counts outside [0, K]')
    check_table(Q.random_tables(7, 2, K, K, (K, 0), (0, K)), 'one side empty')


def test_bad_tables_stay_inside_the_buffers():
    gt, cg, care, pred, cp = Q.random_tables(9, 2, 66, 66)
    for lie in (gt, pred):
        lie[:, 0::4, 8:12] = (0, 0, 40000, 40000)                      # covers everything: clipped against every quad
        lie[:, 1::4, 8:12] = (1000000, 1000000, 1000100, 1000100)      # far away: pruned
        lie[:, 2::4, 8:12] = (50, 50, 10, 10)                          # empty
        lie[0, 3, 8:12] = (-(1 << 30), -(1 << 30), 1 << 30, 1 << 30)   # the origin moves 2^30 away
        lie[0, 7, 12:14] = (-5, -1)                                    # a negative area
        lie[:, 0::5, 12:14] = (0, 0)                                   # zero areas
        lie[0, 9, 12:14] = (0, 1 << 30)                                # an area of 2^62
        lie[:, 11, 14] = -3                                            # valid is any non-zero word
    got, ref = check_table((gt, cg, care, pred, cp), 'lying boxes and areas', max_pairs=66 * 66)
    assert ref[4][:, 9].min() > 16 * 16


def test_chains_need_one_round_per_link():
    for case in (Q.split_chain(40), Q.merge_chain(5)):
        t, params, gk, gg, pk, pg, rounds = case
        got, _ = check_table(t, 'chain', params)
        assert np.array_equal(got[0][0], gk) and np.array_equal(got[3][0], pg) and got[5][0].tolist() == rounds
        assert got[4][0, 12:14].tolist() == rounds


def test_seeded_page():
    t, pairs, seq, ref = Q.page_reference(2)
    # on the oracle alone, never skipped: no comparison within one unit of each summed intersection of equality, no coverage
    # within 1e-10 of cover_thr
    margins = Q.comparison_margins(t, pairs, seq)
    assert min(abs(m) - 256 * n for m, n in margins) > 0 and pairs[0].cover_margin > 1e-10
    stats = ref[4][0]
    assert t[1][0] == 200 and stats[0] + stats[7] == 200 and stats[7] >= 5 and stats[8] >= 3
    assert stats[2] > 40 and stats[3] > 30 and stats[5] >= 20 and stats[4] >= 2 * stats[3] and stats[5] >= 2 * stats[6] > 0
    got, guards, _ = raw_lines(*t)
    assert guards
    assert_equal(got[:5], seq, 'page (sequential form)')
    assert_equal(got, ref, 'page')
    print(f'page: stats {stats.tolist()}')


def test_capacity():
    t = Q.random_tables(21, 3, 48, 48, (20, 48, 30), (48, 48, 25))
    ref = L.match_lines_rounds_host(*t)
    cand = ref[4][:, 10]
    assert cand[1] > cand[0] and cand[1] > cand[2] and cand.min() > 0
    got, guards, _ = raw_lines(*t, max_pairs=int(cand[1]) - 1)
    assert guards
    want = ref[4][1].copy()  # the true counts; no match
    want[2:7], want[11], want[12:14] = 0, 1, 0
    assert np.array_equal(got[4][1], want) and (got[5][1] == 0).all()
    assert (got[1][1] == -1).all() and (got[3][1] == -1).all()
    assert set(got[0][1].tolist()) <= {0, 1, 5} and set(got[2][1].tolist()) <= {0, 1, 5}
    assert np.array_equal(got[0][1] == 5, ref[0][1] == 5) and np.array_equal(got[2][1] == 5, ref[2][1] == 5)
    assert np.array_equal(got[0][1] == 0, ref[0][1] == 0) and np.array_equal(got[2][1] == 0, ref[2][1] == 0)
    for b in (0, 2):  # the other images are unaffected
        assert_equal([o[b:b + 1] for o in got], [o[b:b + 1] for o in ref], f'beside an overflow, image {b}')
    got, guards, _ = raw_lines(*t, max_pairs=int(cand[1]))
    assert guards
    assert_equal(got, ref, 'capacity = candidates')
    got, guards, _ = raw_lines(*t, max_pairs=0)
    assert guards and (got[4][:, 11] == 1).all() and np.array_equal(got[4][:, 7:11], ref[4][:, 7:11])
    assert (got[1] == -1).all() and (got[3] == -1).all() and not got[4][:, 2:7].any()


def test_evaluate_lines_retries_and_equals_the_host_route():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import evaluate_lines, evaluate_lines_host
    rng = np.random.default_rng(4)
    heap = np.stack([np.array(Q.BAR(10, 60), float) + np.rint(rng.uniform(-1, 1, (1, 2)) * 16) / 16 for _ in range(30)])
    gt, care, pred = Q.page(3, 40)
    args = ([heap, pred, pred[:0]], [heap[:12], gt, gt[:0]], [np.ones(12, np.uint8), care, care[:0]])
    ref, ref_score = evaluate_lines_host(*args)
    assert ref[0].stats[10] > 4 * max(len(pred), 40), 'the default capacity must overflow: a retry'
    res, score = evaluate_lines(*args)
    assert len(res) == 3 and res[2].pred_kind.shape == (0,)
    for a, b in zip(res, ref):
        for f in ('gt_kind', 'gt_group', 'pred_kind', 'pred_group', 'stats'):
            assert np.array_equal(getattr(a, f), getattr(b, f)) and getattr(a, f).dtype == getattr(b, f).dtype, f
        assert a.stats[11] == 0
    assert score == ref_score and 0 < score.recall < 1 and 0 < score.precision < 1 and 0 < score.f1 < 1
    assert res[1].stat('split_gt') > 3 and res[1].stat('merged_gt') >= 2 and res[1].stat('one_to_one') > 3
    empty = evaluate_lines([], [])
    assert empty[0] == [] and empty[1].f1 == 0.0 and empty[1].n_gt == 0


def test_ops_call_graph_replay_and_determinism():
    ops = ops_mod()
    a, b = Q.random_tables(31, 2, 70, 70), Q.random_tables(32, 2, 70, 70, (70, 3), (4, 70))
    d = [dev(t) for t in a]
    rounds = torch.full((2, 2), -7777, dtype=torch.int32, device='cuda')
    run = lambda: ops.match_lines(*d, rounds=rounds)
    first = run()
    assert [o.dtype for o in first] == [torch.uint8, torch.int32, torch.uint8, torch.int32, torch.int64]
    assert first[4].shape == (2, 16) and first[0].shape == (2, 70) and first[3].shape == (2, 70)
    ref_a, ref_b = L.match_lines_rounds_host(*a), L.match_lines_rounds_host(*b)
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
    assert not np.array_equal(ref_a[0], ref_b[0]) and ref_a[4][:, 2].min() > 3
    after = run()
    assert_equal([o.cpu().numpy() for o in after] + [rounds.cpu().numpy()], ref_b, 'second eager run')


def test_the_limit_of_8192_quads():
    K = 8192
    small = Q.random_tables(41, 1, 40, 40)
    at = np.r_[0:20, K - 20:K]  # quads in the first and the last tile only; monotone, so the index orders carry over
    gt, pred = np.zeros((2, K, 16), np.int32), np.zeros((2, K, 16), np.int32)
    care = np.ones((2, K), np.uint8)
    gt[:, at], pred[:, at], care[:, at] = small[0][0], small[3][0], small[2][0]
    ref = L.match_lines_rounds_host(*small)
    got, guards, _ = raw_lines(gt, [K, K], care, pred, [K, K], max_pairs=256)
    assert guards and all(np.array_equal(o[0], o[1]) for o in got)
    want_gk, want_pk = np.zeros((K,), np.uint8), np.zeros((K,), np.uint8)
    want_gg, want_pg = np.full((K,), -1, np.int32), np.full((K,), -1, np.int32)
    want_gk[at], want_pk[at] = ref[0][0], ref[2][0]
    want_gg[at] = np.where(ref[1][0] >= 0, at[ref[1][0]], -1)
    want_pg[at] = np.where(ref[3][0] >= 0, at[ref[3][0]], -1)
    assert_equal([o[:1] for o in got], (want_gk[None], want_gg[None], want_pk[None], want_pg[None], ref[4], ref[5]), 'K = 8192')
    kinds = ref[0][0]
    assert ((kinds[:20] >= 2) & (kinds[:20] <= 4)).any() and ((kinds[20:] >= 2) & (kinds[20:] <= 4)).any() and ref[5].max() >= 1


def test_argument_errors_launch_nothing():
    lib, _ = _lib()
    t = Q.random_tables(51, 1, 8, 8)
    cases = (({'N': 8193}, b'1..8192'), ({'M': 0}, b'1..8192'), ({'B': -1}, b'bad B'), ({'tr': 0}, b'recall'),
             ({'tr': 257}, b'recall'), ({'tp': 0}, b'precision'), ({'tp': 300}, b'precision'), ({'cover': 0.0}, b'cover_thr'),
             ({'cover': 1.25}, b'cover_thr'), ({'cap': -2}, b'max_pairs'), ({'nbytes': 16}, b'needed'))
    for over, word in cases:
        got, guards, clean = raw_lines(*t, expect_rc=-1, **over)
        assert word in lib.vkas_last_error(), (over, lib.vkas_last_error())
        assert guards and clean, (over, 'an output was written')
    assert lib.vkas_line_match_workspace_bytes(1, 8193, 8, 8) == -1 and lib.vkas_line_match_workspace_bytes(1, 8, 0, 8) == -1
    assert lib.vkas_line_match_workspace_bytes(1, 8, 8, -1) == -1
    ops = ops_mod()
    d = [dev(x) for x in t]
    for bad in (lambda: ops.match_lines(*d, recall_thr=0.0), lambda: ops.match_lines(*d, precision_thr=1.5),
                lambda: ops.match_lines(*d, cover_thr=0.0), lambda: ops.match_lines(d[0], d[1], d[2][:, :4], d[3], d[4]),
                lambda: ops.match_lines(d[0], d[1], d[2].int(), d[3], d[4]), lambda: ops.match_lines(*d, max_pairs=-1),
                lambda: ops.match_lines(d[0].cpu(), *d[1:]),
                lambda: ops.match_lines(*d, rounds=torch.zeros((1,), dtype=torch.int32, device='cuda'))):
        with pytest.raises((ValueError, RuntimeError)):
            bad()


def test_ops_and_evaluate_lines_against_the_host_route():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import evaluate_lines, evaluate_lines_host
    ops = ops_mod()
    gt, care, pred = Q.page(9, 50)
    quads_g, quads_p = torch.from_numpy(gt[None]).cuda(), torch.from_numpy(pred[None]).cuda()
    rows_g, rows_p = ops.quad_rows(quads_g), ops.quad_rows(quads_p)
    assert np.array_equal(rows_g.cpu().numpy()[0], E.match_rows(gt)[0])
    count = lambda n: torch.tensor([n], dtype=torch.int32, device='cuda')
    params = dict(recall_thr=0.7, precision_thr=0.5, cover_thr=0.6)
    outs = ops.match_lines(rows_g, count(len(gt)), dev(care[None]), rows_p, count(len(pred)), **params)
    ref = L.match_lines_host(E.match_rows(gt)[0][None], [len(gt)], care[None], E.match_rows(pred)[0][None], [len(pred)], **params)
    assert_equal([o.cpu().numpy() for o in outs], ref, 'ops.match_lines')
    res, score = evaluate_lines([pred], [gt], [care], **params, split_credit=0.5, merge_credit=1.0)
    want, want_score = evaluate_lines_host([pred], [gt], [care], **params, split_credit=0.5, merge_credit=1.0)
    assert np.array_equal(res[0].stats, want[0].stats) and np.array_equal(res[0].pred_group, want[0].pred_group)
    assert score == want_score and score.split_credit == 0.5 and np.array_equal(res[0].stats, ref[4][0])
