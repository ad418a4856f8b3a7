"""csrc/ribbonmatch.hip on the MI355X, through the raw C ABI, ops.match_ribbons and inferencing.evaluate_ribbons, against the
host oracles of inferencing/ribbon_evaluation.py: match_ribbons_host (the sequential form, the definition) and
match_ribbons_rounds_host (the rounds, with their counts), themselves held to each other in tests/test_cpu_ribbon_match.py.

Everything is compared for equality: kinds, groups, the statistics and the rounds.  Every output of the raw calls and the
workspace start as canaries between guard words.  Shapes are the smallest that reach each path: one tile, ragged tiles,
several tiles, 1 to 256 segments a side, B = 3 with counts (5, 0, K)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import line_match_cases as Q
from tests import ribbon_cases as C
from vkit_ocr_model_adaptive_scaling_amd.inferencing import ribbon_evaluation as R

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


def dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def raw_ribbons(gt_rows, gt_count, gt_care, gt_segs, pred_rows, pred_count, pred_segs, recall_thr=0.8, precision_thr=0.4,
                cover_thr=0.5, max_pairs=None, expect_rc=0, null=None, shift=None, **over):
    """the C ABI on canary-filled buffers between guards -> (the six outputs, guards_ok, outputs untouched).  ``null``
    names an argument passed as NULL, ``shift`` one whose table is passed 4 bytes off its alignment."""
    lib, _ = _lib()
    d = dict(gt_rows=dev(gt_rows, np.int32), gt_count=dev(gt_count, np.int32), gt_care=dev(gt_care, np.uint8),
             gt_segs=dev(gt_segs, np.int32), pred_rows=dev(pred_rows, np.int32), pred_count=dev(pred_count, np.int32),
             pred_segs=dev(pred_segs, np.int32))
    B, M, N = d['gt_rows'].shape[0], d['gt_rows'].shape[1], d['pred_rows'].shape[1]
    max_pairs = 4 * max(M, N) if max_pairs is None else max_pairs
    nbytes = lib.vkas_ribbon_match_workspace_bytes(B, M, N, max(max_pairs, 0))
    assert nbytes >= 0
    ws = torch.full((nbytes + 512,), 0x5A, dtype=torch.uint8, device='cuda')
    outs = [guarded((B, M), torch.uint8), guarded((B, M), torch.int32), guarded((B, N), torch.uint8),
            guarded((B, N), torch.int32), guarded((B, 16), torch.int64), guarded((B, 2), torch.int32)]
    a = dict(B=B, M=M, N=N, Sg=d['gt_segs'].shape[1], Sp=d['pred_segs'].shape[1], tr=int(np.rint(recall_thr * 256)),
             tp=int(np.rint(precision_thr * 256)), cover=cover_thr, cap=max_pairs, nbytes=nbytes)
    a.update(over)
    if shift:  # the same words one int32 further on: a copy with one word in front
        flat = d[shift].reshape(-1)
        d[shift] = torch.cat([flat[:1], flat])[1:]
        assert d[shift].data_ptr() % 16 == 4
    ptr = {k: (None if k == null else p(v)) for k, v in d.items()}
    rc = lib.vkas_ribbon_match(ptr['gt_rows'], ptr['gt_count'], ptr['gt_care'], ptr['gt_segs'], a['Sg'], ptr['pred_rows'],
                               ptr['pred_count'], ptr['pred_segs'], a['Sp'], a['B'], a['M'], a['N'], a['tr'], a['tp'], a['cover'],
                               a['cap'], None if null == 'workspace' else p(ws[256:]), a['nbytes'],
                               *[None if null == name else p(o[0]) for name, o in zip(NAMES[:5], outs[:5])], p(outs[5][0]), st())
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
    _, seq, ref = C.reference(t, **params)
    got, guards, _ = raw_ribbons(*t, **params, **kw)
    assert guards, 'guard words overwritten'
    assert_equal(got[:5], seq, what + ' (sequential form)')
    assert_equal(got, ref, what)
    return got, ref


@pytest.mark.parametrize('K', [1, 3, 64, 65, 130])
def test_sizes(K):
    got, ref = check_table(C.random_tables(300 + K, 1, K, K), f'M = N = {K}')
    st_ = ref[4][0]
    assert K < 64 or (st_[2] > 3 and st_[3] > 3 and st_[5] >= 2 and st_[7] > 0 and st_[9] > st_[10] > 0), st_.tolist()


def test_sizes_differ_between_the_sides_and_gt_care_null():
    check_table(C.random_tables(11, 1, 65, 130), 'M = 65, N = 130')
    check_table(C.random_tables(12, 1, 130, 63), 'M = 130, N = 63')
    t = C.random_tables(13, 2, 40, 40)
    got, ref = check_table(t[:2] + (None,) + t[3:], 'gt_care = NULL')
    assert not ref[4][:, 7].any() and not ref[4][:, 8].any()
    got, ref = check_table(t, 'with don\'t-care ribbons')
    assert ref[4][:, 7].min() > 0 and ref[4][:, 8].sum() > 0


@pytest.mark.parametrize('counts', [(1, 1), (1, 256), (8, 9), (63, 65), (64, 64), (256, 256)])
def test_segment_counts(counts):
    t = C.segment_count_case(*counts)
    assert t[0][0, 0, 1] == counts[0] and t[4][0, 0, 1] == counts[1]
    got, ref = check_table(t, f'segments {counts}')
    assert got[0][0].tolist() == [Q.ONE, Q.SPLIT] and got[2][0].tolist() == [Q.ONE, Q.SPLIT, Q.SPLIT]
    pairs = R.ribbon_pairs(*t)[0]
    assert pairs.edges[0][2] == 2 * (7 * 16) * (509 * 16)


FAR = lambda k: C.straight(500.0, 1000.0 + 40 * k, 16.0, 30.0, [15.0])  # fillers that meet nothing else


def test_the_only_candidate_in_a_diagonal_and_in_an_off_diagonal_tile():
    line = C.arc(460.0, 500.0, 400.0, 20.0, 110.0, 95.0, 7)
    for g, q in ((70, 70), (3, 100)):
        gts, preds = [FAR(k) for k in range(130)], [FAR(200 + k) for k in range(130)]
        gts[g], preds[q] = line, C.arc(460.5, 500.25, 400.0, 20.0, 110.0, 95.0, 5)
        got, ref = check_table(C.tables(gts, preds), f'the one candidate at ({g}, {q})')
        assert got[4][0, 9:11].tolist() == [1, 1] and got[4][0, 2] == 1 and got[1][0, g] == q and got[3][0, q] == g


def test_split_and_merge_across_tiles():
    """a split whose parts lie in two different pred tiles and a merge whose parts lie in two different gt tiles"""
    bent = lambda a0, a1, n: C.arc(460.0, 500.0, 400.0, 20.0, a0, a1, n)
    line, words = bent(115.0, 95.0, 9), [bent(115.0, 106.0, 4), bent(104.0, 95.0, 5)]
    pred = [FAR(k) for k in range(130)]
    pred[3], pred[100] = words
    got, _ = check_table(C.tables([line], pred), 'split over two pred tiles')
    assert got[0][0].tolist() == [3] and np.flatnonzero(got[2][0] == 3).tolist() == [3, 100] and got[4][0, 12] == 1
    gts = [FAR(k) for k in range(130)]
    gts[60], gts[70] = words
    got, _ = check_table(C.tables(gts, [line]), 'merge over two gt tiles')
    assert got[2][0].tolist() == [4] and np.flatnonzero(got[0][0] == 4).tolist() == [60, 70] and got[4][0, 13] == 1


def test_batch_with_an_empty_image_and_counts_outside_the_table():
    K = 70
    got, ref = check_table(C.random_tables(5, 3, K, K, (5, 0, K), (5, 0, K)), 'batch')
    assert not ref[4][1].any() and (got[0][1] == 0).all() and (got[2][1] == 0).all() and (got[0][0, 5:] == 0).all()
    assert (got[5][1] == 0).all() and ref[4][2, 2] > 5
    check_table(C.random_tables(6, 3, K, K, (-4, K + 50, 1 << 30), (K + 1, -1, 1 << 30)), 'counts outside [0, K]')
    check_table(C.random_tables(7, 2, K, K, (K, 0), (0, K)), 'one side empty')


@pytest.mark.parametrize('name', list(C.hostile_cases()))
def test_hostile_tables(name):
    t, (gk, pk, cand) = C.hostile_cases()[name]
    got, _ = check_table(t, name)
    assert got[0][0].tolist() == gk and got[2][0].tolist() == pk and got[4][0, 10] == cand


def test_hostile_rows_in_a_full_page_stay_inside_the_buffers():
    t = [a.copy() if isinstance(a, np.ndarray) else a for a in C.random_tables(9, 2, 66, 66)]
    for rows, segs in ((t[0], t[3]), (t[4], t[6])):
        S = segs.shape[1]
        rows[:, 0::7, 0] = S - 1                       # the run leaves the table
        rows[:, 1::14, 1] = 257                        # too many segments
        rows[:, 8::14, 1] = 0                          # none
        rows[0, 2, 0:2] = ((1 << 31) - 1, 256)         # start + count overflows an int
        rows[0, 9, 0] = -(1 << 31)
        rows[1, 2, 1] = -(1 << 31)
        rows[:, 3::7, 8:12] = (0, 0, 40000, 40000)     # covers everything: every pair is met
        rows[0, 4, 12:14] = (-5, -1)                   # a negative ribbon area
        rows[:, 11, 14] = -3                           # valid is any non-zero word
        segs[:, 0::9, 14] = 0                          # invalid segments
        segs[:, 1::9, 8:12] = (0, 0, 40000, 40000)     # segment boxes that lie
        segs[:, 2::9, 12:14] = (0, 1 << 30)            # a segment area of 2^62
    got, ref = check_table(tuple(t), 'hostile rows', max_pairs=66 * 66)
    assert ref[4][:, 9].min() > 16 * 16


def test_chains_need_one_round_per_link():
    for case in (Q.split_chain(40), Q.merge_chain(5)):
        t, params, gk, gg, pk, pg, rounds = case
        got, _ = check_table(C.from_line_tables(t), 'chain', params)
        assert np.array_equal(got[0][0], gk) and np.array_equal(got[3][0], pg) and got[5][0].tolist() == rounds


def test_capacity():
    t = C.random_tables(21, 3, 48, 48, (20, 48, 30), (48, 48, 25))
    _, _, ref = C.reference(t)
    cand = ref[4][:, 10]
    assert cand[1] > cand[0] and cand[1] > cand[2] and cand.min() > 0
    got, guards, _ = raw_ribbons(*t, max_pairs=int(cand[1]) - 1)
    assert guards
    want = ref[4][1].copy()  # the true counts; no match
    want[2:7], want[11], want[12:14] = 0, 1, 0
    assert np.array_equal(got[4][1], want) and (got[5][1] == 0).all()
    assert (got[1][1] == -1).all() and (got[3][1] == -1).all()
    assert np.array_equal(got[0][1] == 5, ref[0][1] == 5) and np.array_equal(got[2][1] == 5, ref[2][1] == 5)
    assert np.array_equal(got[0][1] == 0, ref[0][1] == 0) and np.array_equal(got[2][1] == 0, ref[2][1] == 0)
    assert set(got[0][1].tolist()) <= {0, 1, 5} and set(got[2][1].tolist()) <= {0, 1, 5}
    for b in (0, 2):  # the other images are unaffected
        assert_equal([o[b:b + 1] for o in got], [o[b:b + 1] for o in ref], f'beside an overflow, image {b}')
    got, guards, _ = raw_ribbons(*t, max_pairs=int(cand[1]))  # the retry
    assert guards
    assert_equal(got, ref, 'capacity = candidates')


def test_ops_call_graph_replay_and_determinism():
    ops = ops_mod()
    a, b = C.random_tables(31, 2, 70, 70), C.random_tables(32, 2, 70, 70, (70, 3), (4, 70))
    S = max(a[3].shape[1], b[3].shape[1], a[6].shape[1], b[6].shape[1])  # one size of segment table for both
    grow = lambda t: tuple(np.concatenate([x, np.zeros((2, S - x.shape[1], 16), np.int32)], 1) if i in (3, 6) else x
                           for i, x in enumerate(t))
    a, b = grow(a), grow(b)
    d = [dev(t) for t in a]
    rounds = torch.full((2, 2), -7777, dtype=torch.int32, device='cuda')
    run = lambda: ops.match_ribbons(*d, rounds=rounds)
    first = run()
    assert [o.dtype for o in first] == [torch.uint8, torch.int32, torch.uint8, torch.int32, torch.int64]
    assert first[4].shape == (2, 16) and first[0].shape == (2, 70) and first[3].shape == (2, 70)
    ref_a, ref_b = C.reference(a)[2], C.reference(b)[2]
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


def test_argument_errors_launch_nothing():
    lib, _ = _lib()
    t = C.random_tables(51, 1, 8, 8)
    cases = (({'N': 8193}, b'1..8192'), ({'M': 0}, b'1..8192'), ({'B': -1}, b'bad B'), ({'Sg': 0}, b'Sg=0'),
             ({'Sp': (1 << 21) + 1}, b'Sp='), ({'tr': 0}, b'recall'), ({'tr': 257}, b'recall'), ({'tp': 0}, b'precision'),
             ({'tp': 300}, b'precision'), ({'cover': 0.0}, b'cover_thr'), ({'cover': 1.25}, b'cover_thr'),
             ({'cap': -2}, b'max_pairs'), ({'nbytes': 16}, b'needed'), ({'null': 'gt_rows'}, b'null'),
             ({'null': 'pred_segs'}, b'null'), ({'null': 'gt_segs'}, b'null'), ({'null': 'pred_count'}, b'null'),
             ({'null': 'workspace'}, b'null'), ({'null': 'stats'}, b'null'), ({'shift': 'gt_rows'}, b'aligned'),
             ({'shift': 'pred_rows'}, b'aligned'), ({'shift': 'gt_segs'}, b'aligned'), ({'shift': 'pred_segs'}, b'aligned'))
    for over, word in cases:
        got, guards, clean = raw_ribbons(*t, expect_rc=-1, **over)
        assert word in lib.vkas_last_error(), (over, lib.vkas_last_error())
        assert guards and clean, (over, 'an output was written')
    assert lib.vkas_ribbon_match_workspace_bytes(1, 8193, 8, 8) == -1 and lib.vkas_ribbon_match_workspace_bytes(1, 8, 0, 8) == -1
    assert lib.vkas_ribbon_match_workspace_bytes(1, 8, 8, -1) == -1
    ops = ops_mod()
    d = [dev(x) for x in t]
    for bad in (lambda: ops.match_ribbons(*d, recall_thr=0.0), lambda: ops.match_ribbons(*d, precision_thr=1.5),
                lambda: ops.match_ribbons(*d, cover_thr=0.0), lambda: ops.match_ribbons(*d[:2], d[2][:, :4], *d[3:]),
                lambda: ops.match_ribbons(*d[:3], d[3][:, :0], *d[4:]), lambda: ops.match_ribbons(*d[:6], d[6].long()),
                lambda: ops.match_ribbons(*d[:6], d[6][:, :, :8]), lambda: ops.match_ribbons(*d, max_pairs=-1),
                lambda: ops.match_ribbons(d[0].cpu(), *d[1:]), lambda: ops.match_ribbons(*d[:3], d[3].cpu(), *d[4:]),
                lambda: ops.match_ribbons(*d, rounds=torch.zeros((1,), dtype=torch.int32, device='cuda'))):
        with pytest.raises((ValueError, RuntimeError)):
            bad()


def test_ops_and_evaluate_ribbons_on_a_seeded_page():
    """200 bent lines: the C ABI, ops.match_ribbons and evaluate_ribbons against the host route"""
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import evaluate_ribbons, evaluate_ribbons_host
    ops = ops_mod()
    t, pairs, seq, ref = C.page_reference(2)
    stats = ref[4][0]
    assert t[1][0] == 200 and stats[0] + stats[7] == 200 and stats[7] >= 5 and stats[8] >= 3
    assert stats[2] > 40 and stats[3] > 30 and stats[5] >= 20 and stats[4] >= 2 * stats[3] and stats[5] >= 2 * stats[6] > 0
    assert 6 <= t[0][0, :, 1].mean() <= 14 and pairs[0].cover_margin > 1e-10
    got, guards, _ = raw_ribbons(*t)
    assert guards
    assert_equal(got[:5], seq, 'page (sequential form)')
    assert_equal(got, ref, 'page')
    outs = ops.match_ribbons(*[dev(x) for x in t])
    assert_equal([o.cpu().numpy() for o in outs], seq, 'ops.match_ribbons')
    gt, care, pred = C.page(2, 200)
    heap = [C.arc(460.0 + dy, 500.0, 400.0, 20.0, 110.0, 100.0, 5) for dy in np.arange(40) / 16]  # 1200 candidates: a retry
    args = ([pred, heap, []], [gt, heap[:30], []], [care, np.ones(30, np.uint8), []])
    want, want_score = evaluate_ribbons_host(*args, split_credit=0.5, merge_credit=1.0)
    assert want[1].stats[10] > 4 * 200, 'the default capacity must overflow: a retry'
    res, score = evaluate_ribbons(*args, split_credit=0.5, merge_credit=1.0)
    assert len(res) == 3 and res[2].pred_kind.shape == (0,)
    for a, b in zip(res, want):
        for f in ('gt_kind', 'gt_group', 'pred_kind', 'pred_group', 'stats'):
            assert np.array_equal(getattr(a, f), getattr(b, f)) and getattr(a, f).dtype == getattr(b, f).dtype, f
        assert a.stats[11] == 0
    assert np.array_equal(res[0].stats, ref[4][0])
    assert score == want_score and score.split_credit == 0.5 and 0 < score.recall < 1 and 0 < score.precision < 1
    empty = evaluate_ribbons([], [])
    assert empty[0] == [] and empty[1].f1 == 0.0
