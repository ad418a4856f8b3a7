"""csrc/quadmatch.hip on the MI355X, through the raw C ABI, ops.match_quads and inferencing.evaluate_quads, against the host
oracle inferencing/evaluation.py::match_quads_host (itself held to exact arithmetic and to a rounds restatement in
tests/test_cpu_quad_match.py).

gt_match, pred_match, tp, n_gt, n_pred, pairs, candidates and status are compared exactly.  gt_iou is binary64 arithmetic
without contraction in the oracle's order, so bit equality is the aim; IOU_ULPS pins the distance.  Every output of the raw
calls and the workspace start as canaries between guard words.  Shapes are the smallest that reach each path: one tile,
ragged tiles on either side, several tiles, B = 3 with counts (5, 0, K), the 8192 limit (more than 64 KB of LDS in the
matching pass)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import quad_match_cases as C
from vkit_ocr_model_adaptive_scaling_amd.inferencing import evaluation as E

pytestmark = pytest.mark.gpu

# The bound on |device gt_iou - oracle gt_iou| in binary64 steps: twice the largest distance measured over this file's inputs
# on an MI355X, which is 0: the same IEEE operations in the same order on both sides.
IOU_ULPS = 0
G = 64  # guard elements in front of and behind every buffer the kernels write
CANARY = -7777


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
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * G,), CANARY, dtype=dtype, device='cuda')
    return buf[G:G + n].view(shape), buf


def intact(view_buf):
    view, buf = view_buf
    return bool((buf[:G] == CANARY).all()) and bool((buf[G + view.numel():] == CANARY).all())


def raw_call(gt, cg, pred, cp, thr=0.5, max_pairs=None, expect_rc=0, **over):
    """the C ABI on canary-filled buffers between guards -> ((gt_match, pred_match, gt_iou, stats, rounds), guards_ok, rc)"""
    lib, _ = _lib()
    gt, pred = torch.from_numpy(np.ascontiguousarray(gt)).cuda(), torch.from_numpy(np.ascontiguousarray(pred)).cuda()
    cg, cp = (torch.from_numpy(np.asarray(c, dtype=np.int32)).cuda() for c in (cg, cp))
    B, M, N = gt.shape[0], gt.shape[1], pred.shape[1]
    max_pairs = 4 * max(M, N) if max_pairs is None else max_pairs
    nbytes = lib.vkas_quad_match_workspace_bytes(B, M, N, max(max_pairs, 0))
    assert nbytes >= 0
    ws = torch.full((nbytes + 512,), 0x5A, dtype=torch.uint8, device='cuda')
    outs = [guarded((B, M), torch.int32), guarded((B, N), torch.int32), guarded((B, M), torch.float64),
            guarded((B, 6), torch.int64), guarded((B,), torch.int32)]
    a = dict(B=B, M=M, N=N, thr=thr, cap=max_pairs, nbytes=nbytes)
    a.update(over)
    rc = lib.vkas_quad_match(p(gt), p(cg), p(pred), p(cp), a['B'], a['M'], a['N'], a['thr'], a['cap'], p(ws[256:]), a['nbytes'],
                             *[p(o[0]) for o in outs], st())
    torch.cuda.synchronize()
    assert rc == expect_rc, lib.vkas_last_error()
    ok = all(intact(o) for o in outs) and bool((ws[:256] == 0x5A).all()) and bool((ws[256 + nbytes:] == 0x5A).all())
    return [o[0].cpu().numpy() for o in outs], ok, rc


WORST = [0]


def assert_matches(got, ref, what=''):
    """got: (gt_match, pred_match, gt_iou, stats[, rounds]); ref: the oracle's four"""
    for name, g, r in zip(('gt_match', 'pred_match'), got, ref):
        assert np.array_equal(g, r), (what, name, int((g != r).sum()))
    assert np.array_equal(got[3], ref[3]), (what, 'stats', got[3].tolist(), ref[3].tolist())
    assert np.array_equal(got[2] == 0, ref[2] == 0), (what, 'gt_iou zeros')
    d = C.ulp_distance(got[2], ref[2])
    worst = int(d.max()) if d.size else 0
    WORST[0] = max(WORST[0], worst)
    print(f'{what}: largest gt_iou distance {worst} binary64 steps over {int((ref[2] != 0).sum())} matches '
          f'(this run so far: {WORST[0]})')
    assert worst <= IOU_ULPS, (what, 'gt_iou', worst)


def check_tables(tables, what, thr=0.5, **kw):
    ref = E.match_quads_host(*tables, thr)
    got, guards, _ = raw_call(*tables, thr=thr, **kw)
    assert guards, 'guard words overwritten'
    assert_matches(got, ref, what)
    return got, ref


@pytest.mark.parametrize('name', list(C.HAND))
def test_hand_cases_through_the_c_abi(name):
    g, q, want = C.hand_rows(name)
    got, ref = check_tables((g[None], [1], q[None], [1]), name)
    if want is not None:
        matched = want >= 0.5
        assert got[0][0, 0] == (0 if matched else -1) and got[2][0, 0] == (float(want) if matched else 0.0)
    assert got[3][0, 3] == (0 if name == 'disjoint' else 1)


@pytest.mark.parametrize('M,N', [(1, 1), (63, 65), (64, 64), (65, 63), (257, 130)])
def test_sizes(M, N):
    got, ref = check_tables(C.random_tables(100 + M, 1, M, N), f'{M}x{N}')
    assert M == 1 or (ref[3][0, 0] > 0 and ref[3][0, 3] > ref[3][0, 4] > 0)


def test_batch_with_an_empty_image():
    K = 70
    got, ref = check_tables(C.random_tables(5, 3, K, K, (5, 0, K), (5, 0, K)), 'batch')
    assert ref[3][1].tolist() == [0] * 6 and ref[3][2, 0] > 0
    mixed = C.random_tables(6, 3, K, K, (K, 5, 0), (0, K, 5))
    check_tables(mixed, 'batch, mixed counts')


def test_bad_tables_stay_inside_the_buffers():
    gt, cg, pred, cp = C.random_tables(9, 3, 66, 40)
    check_tables((gt, [-4, 66 + 50, 1 << 30], pred, [40 + 1, -1, 1 << 30]), 'counts outside [0, K]')
    dead = gt.copy()
    dead[:, ::3, 14] = 0
    dpred = pred.copy()
    dpred[:, 1::2, 14] = 0
    got, ref = check_tables((dead, cg, dpred, cp), 'valid = 0 rows')
    assert ref[3][0, 1] == 44 and ref[3][0, 2] == 20 and (got[0][:, ::3] == -1).all()
    lie = gt.copy()
    lie[:, 0::4, 8:12] = (0, 0, 4000, 4000)                        # covers everything: clipped against every pred
    lie[:, 1::4, 8:12] = (100000, 100000, 100100, 100100)          # far away: pruned
    lie[:, 2::4, 8:12] = (50, 50, 10, 10)                          # empty
    lie[0, 3, 8:12] = (-(1 << 30), -(1 << 30), 1 << 30, 1 << 30)   # the origin moves 2^30 away
    lie[0, 7, 12:14] = (-5, -1)                                    # a negative area
    lie[0, 11, 12:14] = (0, 0)
    plie = pred.copy()
    plie[:, 0::5, 12:14] = (0, 0)                                   # zero areas on both sides: den = 0
    got, ref = check_tables((lie, cg, plie, cp), 'lying boxes and areas', thr=0.25)
    assert ref[3][:, 3].min() > 40 * 16


def test_extremes():
    big = np.array(C.SQ(-2.0 ** 15, -2.0 ** 15, 2.0 ** 16, 2.0 ** 16))
    half = np.array(C.SQ(-2.0 ** 15, -2.0 ** 15, 2.0 ** 16, 2.0 ** 15))
    turned = C.rotated(0.0, 0.0, 2.0 ** 15.4, 2.0 ** 15.4, 45.0)
    gt, ok = E.match_rows(np.stack([big, half]))
    pred, okp = E.match_rows(np.stack([half, big, turned]))
    assert ok.all() and okp.all() and abs(pred[2, :8]).max() > 1 << 18
    got, ref = check_tables((gt[None], [2], pred[None], [3]), 'corners at +-2^19')
    assert got[0][0].tolist() == [1, 0] and got[2][0].tolist() == [1.0, 1.0]


SEEDS = (2, 6)  # checked on the CPU: the two assertions below hold with a wide margin


@pytest.mark.parametrize('seed', SEEDS)
def test_seeded_page(seed):
    tables, ref, ious = C.page_reference(seed)
    # on the oracle alone, never skipped: no IoU within 1e-10 of the threshold, no two distinct IoUs within 1e-10 of each
    # other, so that a last-bit difference could not change a decision
    assert np.abs(ious - 0.5).min() >= 1e-10
    distinct = np.unique(ious)
    assert np.diff(distinct).min() >= 1e-10
    assert tables[1][0] == 300 and 300 <= tables[3][0] <= 345
    print(f'page {seed}: {tables[3][0]} predictions, stats {ref[3][0].tolist()}, closest IoU to the threshold '
          f'{np.abs(ious - 0.5).min():.1e}, closest two IoUs {np.diff(distinct).min():.1e}')
    assert ref[3][0, 3] > 600 and 235 <= ref[3][0, 0] <= 280
    got, guards, _ = raw_call(*tables[:4])
    assert guards
    assert_matches(got, ref, f'page {seed}')


def _rounds_of(tables, thr=0.5):
    g, q = tables[0][0], tables[2][0]
    gi, pi = E.box_pairs(g[:tables[1][0]], q[:tables[3][0]])
    edges = [(a, c, E.quad_iou_host(g[a], q[c])) for a, c in zip(gi.tolist(), pi.tolist())]
    return C.mutual_best_rounds([e for e in edges if e[2] >= thr], g.shape[0], q.shape[0])[2]


def test_ties_and_chain():
    for name, (gt, pred) in C.tie_cases().items():
        t = E.evaluation_tables([pred], [gt])[:4]
        got, ref = check_tables(t, name)
        assert got[0][0, 0] == 0 and got[1][0, 0] == 0 and got[3][0, 0] == 1 and got[4][0] == 1
    gt, pred, want, rounds = C.chain_case()
    t = E.evaluation_tables([pred], [gt])[:4]
    got, ref = check_tables(t, 'chain')
    assert got[0][0].tolist() == want.tolist() and got[4][0] == rounds == _rounds_of(t) and rounds > 1
    for seed in SEEDS:  # and the rounds of a page
        tables = C.page_reference(seed)[0]
        assert raw_call(*tables[:4])[0][4][0] == _rounds_of(tables)


def test_capacity():
    tables = C.random_tables(21, 3, 48, 48, (20, 48, 30), (20, 48, 30))
    ref = E.match_quads_host(*tables)
    cand = ref[3][:, 4]
    assert cand[1] > cand[0] and cand[1] > cand[2] and cand.min() > 0
    got, guards, _ = raw_call(*tables, max_pairs=int(cand[1]) - 1)
    assert guards
    assert got[3][1].tolist() == [0, ref[3][1, 1], ref[3][1, 2], ref[3][1, 3], cand[1], 1] and got[4][1] == 0
    assert (got[0][1] == -1).all() and (got[1][1] == -1).all() and (got[2][1] == 0).all()
    for b in (0, 2):  # the other images are unaffected
        assert_matches([o[b:b + 1] for o in got], [o[b:b + 1] for o in ref], f'beside an overflow, image {b}')
    got, guards, _ = raw_call(*tables, max_pairs=int(cand[1]))
    assert guards
    assert_matches(got, ref, 'capacity = candidates')
    got, guards, _ = raw_call(*tables, max_pairs=0)
    assert guards and got[3][:, 5].tolist() == [1, 1, 1] and (got[0] == -1).all() and np.array_equal(got[3][:, 1:5], ref[3][:, 1:5])


def test_evaluate_quads_retries_and_equals_the_host_route():
    rng = np.random.default_rng(4)
    gt = np.stack([np.array(C.SQ(10, 10, 20, 20), float) + rng.uniform(-2, 2, (4, 2)) for _ in range(14)])
    pred = np.stack([np.array(C.SQ(10, 10, 20, 20), float) + rng.uniform(-2, 2, (4, 2)) for _ in range(14)])
    small_gt, small_pred = C.page(3, lines=2, per_line=6)
    args = ([pred, small_pred, small_pred[:0]], [gt, small_gt, small_gt])
    ref, ref_score = E.evaluate_quads_host(*args, iou_thr=0.3)
    t = E.evaluation_tables(*args)
    assert ref[0].candidates == 196 > 4 * max(t[0].shape[1], t[2].shape[1]), 'the default capacity must overflow: a retry'
    res, score = E.evaluate_quads(*args, iou_thr=0.3)
    assert score == ref_score and score.tp == 14 + ref[1].tp and len(res) == 3
    for a, b in zip(res, ref):
        assert np.array_equal(a.gt_match, b.gt_match) and np.array_equal(a.pred_match, b.pred_match)
        assert C.ulp_distance(a.gt_iou, b.gt_iou).max() <= IOU_ULPS
        assert (a.tp, a.n_gt, a.n_pred, a.pairs, a.candidates) == (b.tp, b.n_gt, b.n_pred, b.pairs, b.candidates)
    assert E.evaluate_quads([], []) == ([], E.DetectionScore())


def test_ops_call_graph_replay_and_determinism():
    ops = ops_mod()
    a, b = C.random_tables(31, 2, 70, 66), C.random_tables(32, 2, 70, 66, (70, 3), (0, 66))
    dev = [torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in a]
    rounds = torch.full((2,), CANARY, dtype=torch.int32, device='cuda')
    run = lambda: ops.match_quads(*dev, rounds=rounds)
    first = run()
    assert [o.dtype for o in first] == [torch.int32, torch.int32, torch.float64, torch.int64] and first[3].shape == (2, 6)
    ref_a, ref_b = E.match_quads_host(*a), E.match_quads_host(*b)
    assert_matches([o.cpu().numpy() for o in first], ref_a, 'ops, eager')
    assert (rounds.cpu().numpy() >= 1).all()
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
    assert_matches([o.cpu().numpy() for o in outs], ref_a, 'replayed')
    for d, t in zip(dev, b):  # rewritten tables, the same buffers
        d.copy_(torch.from_numpy(np.ascontiguousarray(t)))
    graph.replay()
    assert_matches([o.cpu().numpy() for o in outs], ref_b, 'replayed over rewritten tables')
    assert ref_b[3][0, 0] == 0 and 0 < ref_b[3][1, 0] <= 3 and ref_a[3][:, 0].min() > 3


def test_the_limit_of_8192_quads_per_side():
    K = 8192
    gt_small, _, pred_small, _ = C.random_tables(41, 1, 40, 44)
    gi = np.r_[0:20, K - 20:K]
    pi = np.r_[0:22, K - 22:K]
    gt, pred = np.zeros((2, K, 16), np.int32), np.zeros((2, K, 16), np.int32)  # 2 x 128 x 128 tiles
    gt[:, gi], pred[:, pi] = gt_small[0], pred_small[0]
    small = E.match_quads_host(gt_small, [40], pred_small, [44])
    got, guards, _ = raw_call(gt, [K, K], pred, [K, K], max_pairs=256)
    assert guards and all(np.array_equal(o[0], o[1]) for o in got)
    got = [o[:1] for o in got]
    want_g = np.full((K,), -1, np.int32)
    want_g[gi] = np.where(small[0][0] >= 0, pi[small[0][0]], -1)
    want_p = np.full((K,), -1, np.int32)
    want_p[pi] = np.where(small[1][0] >= 0, gi[small[1][0]], -1)
    want_iou = np.zeros((K,))
    want_iou[gi] = small[2][0]
    assert_matches(got, (want_g[None], want_p[None], want_iou[None], small[3]), 'K = 8192')
    assert small[3][0, 0] > 5


def test_argument_errors_launch_nothing():
    lib, _ = _lib()
    tables = C.random_tables(51, 1, 8, 8)
    for over, word in (({'M': 8193}, b'1..8192'), ({'N': 0}, b'1..8192'), ({'B': -1}, b'bad B'), ({'thr': 0.0}, b'iou_thr'),
                       ({'thr': 1.5}, b'iou_thr'), ({'cap': -2}, b'max_pairs'), ({'nbytes': 16}, b'needed')):
        got, guards, rc = raw_call(*tables, expect_rc=-1, **over)
        assert word in lib.vkas_last_error(), (over, lib.vkas_last_error())
        assert guards and all((o == CANARY).all() for o in got), (over, 'an output was written')
