"""The table checkers of ops.py that the five wrappers over match rows share (match_quads, match_quads_ranked, match_lines,
nms_quads, quad_lines), driven through the wrappers with host tensors: every malformed table raises a ValueError that names
the wrapper, and only a well-formed call gets as far as the device check.  Every tensor is a zero-stride view of one
element, so B = 65536 costs nothing.  No GPU."""
import pytest
import torch

from vkit_ocr_model_adaptive_scaling_amd import ops


def z(shape, dtype=torch.int32):
    return torch.zeros((1,) * len(shape), dtype=dtype).expand(shape)


def two_sided(care, probs, rounds_tail):
    def good(B=2, M=4, N=5):
        kw = dict(gt_rows=z((B, M, 16)), gt_count=z((B,)), pred_rows=z((B, N, 16)), pred_count=z((B,)))
        if care:
            kw['gt_care'] = z((B, M), torch.uint8)
        if probs:
            kw.update(probs=z((B, N), torch.float32), iou_thrs=(0.5, 0.75))
        return kw
    return good, ('gt_rows', 'pred_rows'), ('gt_count', 'pred_count'), rounds_tail


def one_sided(probs, rounds_tail):
    def good(B=2, M=4, N=None):
        kw = dict(rows=z((B, M, 16)), count=z((B,)))
        if probs:
            kw['probs'] = z((B, M), torch.float32)
        return kw
    return good, ('rows',), ('count',), rounds_tail


WRAPPERS = {
    'match_quads': two_sided(False, False, ()),
    'match_quads_ranked': two_sided(True, True, (2,)),
    'match_lines': two_sided(True, False, (2,)),
    'nms_quads': one_sided(True, ()),
    'quad_lines': one_sided(False, None),  # no candidate capacity, no rounds
}


def bad_calls(name):
    good, rows_keys, count_keys, rounds_tail = WRAPPERS[name]
    ok = good()
    for k in rows_keys:
        B, K, _ = ok[k].shape
        yield f'{k} of rank 2', {**ok, k: z((K, 16))}
        yield f'{k} with 15 words', {**ok, k: z((B, K, 15))}
        yield f'{k} int64', {**ok, k: z((B, K, 16), torch.int64)}
    for k in count_keys:
        yield f'{k} of the wrong length', {**ok, k: z((3,))}
        yield f'{k} int64', {**ok, k: z((2,), torch.int64)}
    if 'gt_care' in ok:
        yield 'gt_care of the wrong shape', {**ok, 'gt_care': z((2, 5), torch.uint8)}
        yield 'gt_care int32', {**ok, 'gt_care': z((2, 4))}
    if 'probs' in ok:
        yield 'probs float64', {**ok, 'probs': z(tuple(ok['probs'].shape), torch.float64)}
        yield 'probs of the wrong shape', {**ok, 'probs': z((2, 9), torch.float32)}
    for k in (0, 8193):
        yield f'M = {k}', good(M=k)
        if len(rows_keys) == 2:
            yield f'N = {k}', good(N=k)
    yield 'B = 65536', good(B=65536)
    if rounds_tail is not None:
        yield 'max_pairs = -1', {**ok, 'max_pairs': -1}
        yield 'max_pairs beyond 2^31 / B', {**ok, 'max_pairs': 1 << 30}
        yield 'rounds of the wrong shape', {**ok, 'rounds': torch.zeros((3,) + rounds_tail, dtype=torch.int32)}
        yield 'rounds int64', {**ok, 'rounds': torch.zeros((2,) + rounds_tail, dtype=torch.int64)}


CASES = [(name, label, kw) for name in WRAPPERS for label, kw in bad_calls(name)]


@pytest.mark.parametrize('name,label,kw', CASES, ids=[f'{n}-{l}' for n, l, _ in CASES])
def test_bad_table_names_the_wrapper(name, label, kw):
    with pytest.raises(ValueError, match=f'^{name}: '):
        getattr(ops, name)(**kw)


@pytest.mark.parametrize('name', WRAPPERS)
def test_well_formed_host_tables_reach_the_device_check(name):
    good, _, _, rounds_tail = WRAPPERS[name]
    calls = [good(), good(B=0)]
    if rounds_tail is not None:
        calls += [{**good(), 'max_pairs': 0, 'rounds': torch.zeros((2,) + rounds_tail, dtype=torch.int32)}]
    if 'gt_care' in good():
        calls += [{**good(), 'gt_care': None}]
    for kw in calls:
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            getattr(ops, name)(**kw)


def test_workspace_rejects_a_refused_size():
    with pytest.raises(RuntimeError, match='^match_quads'):
        ops._workspace('match_quads', ops.lib.vkas_quad_match_workspace_bytes(1, 0, 1, 0), torch.device('cpu'))
    assert ops._workspace('match_quads', 0, torch.device('cpu')).numel() == 256
