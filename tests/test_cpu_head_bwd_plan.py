"""ops._head_bwd_plan: which heads of a fused pass take which backward path (compact label-point rows, convolution kernels at
the upsampled resolution, matrix products at the neck's resolution).  The function is pure, so it is compiled here from its
source text in ops.py on its own: importing ops would load the HIP library."""
import ast
import itertools
import os

import pytest

OPS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'vkit_ocr_model_adaptive_scaling_amd', 'ops.py')


def _load_plan():
    tree = ast.parse(open(OPS).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == '_head_bwd_plan']
    assert len(fn) == 1
    ns = {}
    exec(compile(ast.Module(body=fn, type_ignores=[]), OPS, 'exec'), ns)
    return ns['_head_bwd_plan']


plan = _load_plan()


def sp_ranges(n):
    """what _point_sparse_run can return for n heads: None, or a non-empty prefix or suffix run (the whole set included)"""
    return [None] + sorted({(0, b) for b in range(1, n + 1)} | {(a, n) for a in range(0, n)})


def cases():
    for n in range(1, 5):
        for low in (False, True):
            for sp in sp_ranges(n):
                dense = [h for h in range(n) if sp is None or not sp[0] <= h < sp[1]]
                for bits in itertools.product((False, True), repeat=len(dense)):
                    marked = [True] * n  # compact heads are marked
                    for h, m in zip(dense, bits):
                        marked[h] = m
                    yield n, sp, marked, low


CASES = list(cases())


def heads_of(r):
    return list(range(r[0], r[1]))


def test_enumeration_is_not_vacuous():
    # per n: 2^n vectors without a compact run, and 2^(dense heads) for each prefix and suffix run: 3 + 9 + 21 + 45, times low
    assert len(CASES) == 2 * (3 + 9 + 21 + 45)
    assert any(sp is None and all(m) for _, sp, m, _ in CASES) and any(sp == (0, 4) for _, sp, _, _ in CASES)


@pytest.mark.parametrize('low', [False, True])
def test_plan_properties_hold_for_every_case(low):
    for n, sp, marked, lw in CASES:
        if lw != low:
            continue
        what = (n, sp, marked, low)
        compact, upres, lowres = plan(n, sp, marked, low)
        for r in (compact, upres, lowres):
            assert 0 <= r[0] <= r[1] <= n, what           # each a contiguous run inside [0, n)
        hs = [heads_of(r) for r in (compact, upres, lowres)]
        assert sorted(hs[0] + hs[1] + hs[2]) == list(range(n)), what  # disjoint, and together every head
        assert hs[0] == (heads_of(sp) if sp is not None else []), what
        if sp is not None:
            assert tuple(compact) == sp, what
        dense = [h for h in range(n) if h not in hs[0]]
        plain = [h for h in dense if not marked[h]]
        if not low:
            assert hs[2] == [], what
            continue
        assert all(not marked[h] for h in hs[2]), what
        is_run = bool(plain) and plain == list(range(plain[0], plain[-1] + 1))
        at_end = is_run and (plain[0] == dense[0] or plain[-1] == dense[-1])
        if at_end:
            assert hs[2] == plain and hs[1] == [h for h in dense if marked[h]], what
        else:  # the unmarked dense heads are no prefix or suffix of the dense run: everything on the convolution kernels
            assert hs[2] == [] and hs[1] == dense, what


F, T = False, True
# (n_heads, sp_range, marked, low) -> (compact, upres, lowres), written out from HeadsFused.backward as it stood before the plan
# function existed: d = dense run, e = its unmarked heads if they are one run at either end of d, u = the rest of d
TABLE = [
    ((4, (1, 4), [F, T, T, T], False), ((1, 4), (0, 1), (0, 0))),  # heads 1-3 compact, head 0 on the convolution kernels
    ((4, (1, 4), [F, T, T, T], True), ((1, 4), (1, 1), (0, 1))),   # ... head 0 at the neck's resolution
    ((4, None, [F, F, F, F], True), ((0, 0), (4, 4), (0, 4))),     # nothing marked: all four at the neck's resolution
    ((4, None, [F, F, F, F], False), ((0, 0), (0, 4), (0, 0))),
    ((4, None, [F, T, T, T], True), ((0, 0), (1, 4), (0, 1))),     # compact path off: marked heads keep the convolution kernels
    ((3, None, [F, T, F], True), ((0, 0), (0, 3), (0, 0))),        # unmarked heads are not one run: all on the convolution kernels
    ((4, (0, 3), [T, T, T, F], True), ((0, 3), (4, 4), (3, 4))),   # compact prefix, the last head at the neck's resolution
    ((4, (0, 2), [T, T, T, F], True), ((0, 2), (2, 3), (3, 4))),   # a marked head left dense next to an unmarked one
    ((4, (0, 2), [T, T, F, T], True), ((0, 2), (3, 4), (2, 3))),
    ((4, None, [T, T, T, T], True), ((0, 0), (0, 4), (0, 0))),     # all marked, no compact run (e.g. different label points)
    ((4, (0, 4), [T, T, T, T], True), ((0, 4), (4, 4), (4, 4))),   # every head compact
    ((1, None, [F], True), ((0, 0), (1, 1), (0, 1))),
]


@pytest.mark.parametrize('args,expected', TABLE, ids=lambda v: None)
def test_plan_literal_cases(args, expected):
    assert tuple(map(tuple, plan(*args))) == expected
