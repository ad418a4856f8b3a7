"""Text regions on the MI355X (csrc/regions.hip, ops.text_regions, rough_infer_text_regions) against the host restatement
``text_regions_host`` (checked against scipy and np.median in test_cpu_text_regions.py): counts, label maps, boxes, areas,
valid counts and medians for exact equality.  The maps are the smallest that cross the 64 x 16 tile seams of the labelling
pass in both directions with ragged edges.  Masks: empty; full (one region over every tile); checkerboard (one region under
8-connectivity only); dots on every other row and column (the most regions a map can hold; with a small table, the overflow
contract); a one-pixel serpentine over the whole map (the longest union-find chains across every seam); a comb and a U whose
arms meet only in the last row (provisional labels that merge late); diagonal and anti-diagonal lines through tile corners;
random masks; batches whose images differ.  Then determinism, replay from a captured graph with the inputs overwritten in
place, and the inference API end to end, eager and replayed."""
import ctypes

import numpy as np
import pytest
import torch

from tests import test_cpu_text_regions as C
from tests.test_gpu_inferencing import build

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 7, 5), (3, 33, 65), (2, 70, 93), (1, 160, 256)]
_ORACLE = {}


def oracle(mask, height):
    """text_regions_host, computed once per distinct (mask, height) and left unchanged."""
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import text_regions_host
    key = (mask.shape, mask.tobytes(), height.tobytes())
    if key not in _ORACLE:
        _ORACLE[key] = text_regions_host(mask, height)
    return _ORACLE[key]


def batch(kind, B, H, W):
    """Image b takes the mask kind b places after ``kind`` and its own heights: the images of a batch differ."""
    k = C.KINDS.index(kind)
    masks = np.stack([C.make_mask(C.KINDS[(k + 5 * b) % len(C.KINDS)], H, W) for b in range(B)])
    heights = np.stack([C.make_height(H, W, 31 * k + b) for b in range(B)])
    return masks, heights


def run_device(masks, heights, max_regions):
    from vkit_ocr_model_adaptive_scaling_amd import ops
    out = ops.text_regions(torch.from_numpy(masks).cuda(), torch.from_numpy(heights).cuda(), max_regions)
    return [t.cpu().numpy() for t in out]


def assert_equals_oracle(out, masks, heights, max_regions):
    count, labels, boxes, areas, valid, medians = out
    B, H, W = masks.shape
    assert count.shape == (B,) and labels.shape == (B, H, W) and boxes.shape == (B, max_regions, 4)
    assert areas.shape == valid.shape == medians.shape == (B, max_regions)
    assert count.dtype == labels.dtype == boxes.dtype == areas.dtype == valid.dtype == np.int32 and medians.dtype == np.float32
    for b in range(B):
        rl, rb, ra, rv, rm = oracle(masks[b], heights[b])
        n = min(len(rb), max_regions)
        assert count[b] == len(rb), (b, int(count[b]), len(rb))
        assert np.array_equal(labels[b], rl), (b, 'labels')
        assert np.array_equal(boxes[b, :n], rb[:n]), (b, 'boxes')
        assert np.array_equal(areas[b, :n], ra[:n]), (b, 'areas')
        assert np.array_equal(valid[b, :n], rv[:n]), (b, 'valid')
        assert medians[b, :n].tobytes() == rm[:n].tobytes(), (b, 'medians')
        assert not boxes[b, n:].any() and not areas[b, n:].any() and not valid[b, n:].any() and not medians[b, n:].any()


@pytest.mark.parametrize('kind', C.KINDS)
@pytest.mark.parametrize('B,H,W', SHAPES)
def test_text_regions_match_host(B, H, W, kind):
    masks, heights = batch(kind, B, H, W)
    cap = (H + 1) // 2 * ((W + 1) // 2)  # the most regions a map can hold
    assert_equals_oracle(run_device(masks, heights, cap), masks, heights, cap)


@pytest.mark.parametrize('B,H,W', SHAPES[2:])
def test_overflow_keeps_true_count_and_labels_and_writes_no_further(B, H, W):
    """More regions than table rows, through the C ABI with guard words behind every output."""
    from vkit_ocr_model_adaptive_scaling_amd import ops
    from vkit_ocr_model_adaptive_scaling_amd._lib import lib, check
    R, G = 7, 64
    masks = np.stack([C.make_mask('dots' if b % 2 == 0 else 'random3_0', H, W) for b in range(B)])
    heights = np.stack([C.make_height(H, W, 5 + b) for b in range(B)])
    assert all(len(oracle(masks[b], heights[b])[1]) > R for b in range(B))
    d_mask, d_height = torch.from_numpy(masks).cuda(), torch.from_numpy(heights).cuda()
    nbytes = lib.vkas_text_regions_workspace_bytes(B, H, W, R)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device='cuda')
    guarded = lambda n, dtype=torch.int32: torch.full((n + G,), -7, dtype=dtype, device='cuda')
    count, labels, boxes = guarded(B), guarded(B * H * W), guarded(B * R * 4)
    areas, valid, medians = guarded(B * R), guarded(B * R), guarded(B * R, torch.float32)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    check(lib.vkas_text_regions(p(d_mask), p(d_height), B, H, W, R, p(ws), nbytes, p(count), p(labels), p(boxes), p(areas),
                                p(valid), p(medians), ops._stream()), 'text_regions')
    torch.cuda.synchronize()
    for t, n in ((count, B), (labels, B * H * W), (boxes, B * R * 4), (areas, B * R), (valid, B * R), (medians, B * R)):
        assert (t[n:] == -7).all(), 'guard words behind an output were overwritten'
    out = [t[:n].reshape(s).cpu().numpy() for t, n, s in (
        (count, B, (B,)), (labels, B * H * W, (B, H, W)), (boxes, B * R * 4, (B, R, 4)), (areas, B * R, (B, R)),
        (valid, B * R, (B, R)), (medians, B * R, (B, R)))]
    assert out[1].max() > R
    assert_equals_oracle(out, masks, heights, R)


def blocks_case(odd: bool):
    """(1, 70, 93): six 8 x 13 blocks with 0, 1, 2, 3, 104 and 103 valid heights and one 50 x 93 band over several tiles
    with an even (4650) or an odd (4649) number."""
    H, W = 70, 93
    g = np.random.default_rng(17)
    mask = np.zeros((H, W), np.uint8)
    height = (np.floor(g.uniform(3, 60, (H, W)) * 2) / 2).astype(np.float32)
    for i, keep in enumerate((0, 1, 2, 3, 104, 103)):
        block = (slice(0, 8), slice(15 * i, 15 * i + 13))
        mask[block] = 1
        zero = np.zeros(104, bool)
        zero[g.permutation(104)[:104 - keep]] = True
        height[block] = np.where(zero.reshape(8, 13), 0, height[block])
    mask[20:70] = 1
    if odd:
        height[41, 57] = 0
    return mask[None], height[None]


@pytest.mark.parametrize('odd', [False, True], ids=['even', 'odd'])
def test_medians_of_small_and_large_regions(odd):
    masks, heights = blocks_case(odd)
    rv = oracle(masks[0], heights[0])[3]
    assert rv.tolist() == [0, 1, 2, 3, 104, 103, 4649 if odd else 4650]
    assert_equals_oracle(run_device(masks, heights, 16), masks, heights, 16)


def test_one_repeated_height_and_invalid_heights():
    B, H, W = 2, 70, 93
    masks = np.stack([C.make_mask('random5_1', H, W), C.make_mask('comb', H, W)])
    heights = np.full((B, H, W), 12.5, np.float32)
    heights[1, ::3] = -4.0  # not > 0: not valid
    heights[1, 1::3] = 0.0
    out = run_device(masks, heights, 512)
    assert_equals_oracle(out, masks, heights, 512)
    assert set(np.unique(out[5]).tolist()) <= {0.0, 12.5}


def test_same_call_twice_is_bit_equal():
    masks, heights = batch('random5_0', 2, 70, 93)
    a, b = run_device(masks, heights, 256), run_device(masks, heights, 256)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


def test_captured_graph_replays_with_inputs_overwritten_in_place():
    from vkit_ocr_model_adaptive_scaling_amd import ops
    B, H, W, R = 2, 70, 93, 700
    cases = [batch(kind, B, H, W) for kind in ('full', 'empty', 'random5_2', 'dots', 'serpentine')]
    d_mask = torch.from_numpy(cases[0][0]).cuda()
    d_height = torch.from_numpy(cases[0][1]).cuda()
    ops.text_regions(d_mask, d_height, R)  # eager first
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.text_regions(d_mask, d_height, R)
    for masks, heights in cases + cases[:1]:
        d_mask.copy_(torch.from_numpy(masks))
        d_height.copy_(torch.from_numpy(heights))
        graph.replay()
        torch.cuda.synchronize()
        assert_equals_oracle([t.cpu().numpy() for t in out], masks, heights, R)


def test_rough_infer_text_regions_matches_host_on_rough_infer_maps():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import region_scales, text_regions_host
    inf, _ = build(torch.float16)
    img = np.random.default_rng(5).integers(0, 256, (100, 150, 3), dtype=np.uint8)  # pads to 128 x 160
    maps = inf.rough_infer(img)
    labels, boxes, areas, valid, medians = text_regions_host(maps.rough_char_mask, maps.rough_char_height_score_map)
    assert len(boxes) >= 2 and (maps.rough_char_mask == 0).any() and (medians > 0).any(), 'a degenerate page shows nothing'
    scales, resized, keep = region_scales(boxes, medians, (100, 150), maps.resized_shape, 35, 0.25)
    captures = inf.graphs.captures
    calls = [inf.rough_infer_text_regions(img), inf.rough_infer_text_regions(img),  # eager, captured + replayed
             inf.rough_infer_text_regions(img, return_labels=False)]                # replayed
    assert inf.graphs.captures == captures + 1
    for k, r in enumerate(calls):
        assert r.resized_shape == (50, 75) and r.padded_image.shape == (128, 160, 3) and r.num_regions == len(boxes)
        if k < 2:
            assert r.labels.dtype == np.int32 and np.array_equal(r.labels, labels)
        else:
            assert r.labels is None
        assert np.array_equal(r.boxes, boxes) and np.array_equal(r.areas, areas) and np.array_equal(r.valid, valid)
        assert r.char_height_medians.tobytes() == medians.tobytes()
        assert np.array_equal(r.scales, scales) and np.array_equal(r.resized_shapes, resized)
        assert np.array_equal(r.keep, keep)
    # a table smaller than the page's regions: the true count, the first rows
    inf.config.rough_text_regions_max = 1
    r = inf.rough_infer_text_regions(img)
    assert r.num_regions == len(boxes) and np.array_equal(r.boxes, boxes[:1]) and np.array_equal(r.labels, labels)
    assert r.char_height_medians.tobytes() == medians[:1].tobytes() and np.array_equal(r.keep, keep[:1])
