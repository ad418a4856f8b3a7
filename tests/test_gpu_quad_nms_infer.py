"""The suppression inside ``infer`` / ``infer_batch`` on the MI355X, on the small untrained model and the images of
tests/test_gpu_infer_batch.py.

Off (the default), the results carry the new fields at their defaults.  On, a result equals - field by field, bit for bit -
the off result filtered by the host oracle (``nms_quads_lists_host`` on ``result_quads``).  What the oracle suppresses on
this model's output is printed, not asserted: the untrained model reports no character twice (measured: no two boxes
of valid quads overlap on any of the three images, so no pair at either threshold).  The suppression path is therefore covered HERE BY
THE SECOND ROUTE: the filter function on device output for a hand-made duplicate set - the regions, points and probs of
an ``infer`` result with hand-made boxes, every one a second time (``test_hand_made_duplicates_in_a_result``) -, where the
oracle is asserted to suppress every duplicate."""
import attrs
import numpy as np
import pytest
import torch

from tests.test_gpu_infer_batch import assert_results_equal, picture
from tests.test_gpu_inferencing import build
from tests.test_gpu_infer_oriented import configure

pytestmark = pytest.mark.gpu

THRS = (0.5, 0.05)  # the usual threshold, and one at which loosely overlapping quads of the untrained model already count


def filtered_by_the_oracle(result, thr):
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import filter_result, nms_quads_lists_host, result_quads
    quads, probs = result_quads(result)
    res, stats = nms_quads_lists_host([quads], [probs], thr)
    return filter_result(result, res[0].keep), stats


def assert_same(a, b, what):
    assert_results_equal(a, b, what)
    assert (a.num_suppressed, a.nms_status) == (b.num_suppressed, b.nms_status), what
    for name in ('oriented', 'warps', 'warp_regions', 'placement_pages'):
        assert np.array_equal(getattr(a, name), getattr(b, name)), (what, name)


def test_infer_and_infer_batch_equal_their_off_results_filtered_by_the_oracle():
    inf, _ = build(torch.float16)
    configure(inf, False)
    imgs = [np.random.default_rng(5).integers(0, 256, (100, 150, 3), dtype=np.uint8), picture((120, 90), 3), picture((64, 200), 4)]
    assert inf.config.precise_char_nms_iou_thr == 0.0
    off = [inf.infer(img) for img in imgs]
    off_batch = inf.infer_batch(imgs).results
    for r in off + list(off_batch):
        assert (r.num_suppressed, r.nms_status) == (0, 0)
    assert sum(len(p) for p in off[0].probs) > 0
    for thr in THRS:
        inf.config.precise_char_nms_iou_thr = thr
        on = [inf.infer(img) for img in imgs]
        on_batch = inf.infer_batch(imgs).results
        for k, (a, b, ob, oo) in enumerate(zip(on, on_batch, off_batch, off)):
            want, stats = filtered_by_the_oracle(oo, thr)
            want_batch, _ = filtered_by_the_oracle(ob, thr)
            print(f'thr {thr}, image {k}: {stats[1]} characters, {stats[3]} box pairs, {stats[4]} candidates, '
                  f'{want.num_suppressed} suppressed')
            assert_same(a, want, ('infer', thr, k))
            assert_same(b, want_batch, ('infer_batch', thr, k))
            assert a.num_suppressed == stats[1] - stats[0] and a.nms_status == 0
    inf.config.precise_char_nms_iou_thr = 0.0
    again = inf.infer(imgs[0])
    assert_same(again, off[0], 'off again')


def test_hand_made_duplicates_in_a_result():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import (filter_result, match_rows, nms_quads, nms_quads_lists_host,
                                                                 result_quads, suppress_results)
    inf, _ = build(torch.float16)
    configure(inf, False)
    base = inf.infer(np.random.default_rng(5).integers(0, 256, (100, 150, 3), dtype=np.uint8))
    # the untrained model's quads are small and apart from one another (measured: 339 of 359 valid, no two boxes overlap): the
    # result keeps its regions, points and probs, and every character gets a 9 x 7 box in a grid cell of its own
    print(f'{int(match_rows(result_quads(base)[0])[1].sum())} of the model\'s quads are valid')
    sizes = [len(p) for p in base.probs]
    n = sum(sizes)
    assert n >= 20 and sum(k > 0 for k in sizes) >= 2
    k = np.arange(n)
    corner = np.stack([20.0 * (k // 25), 20.0 * (k % 25)], axis=1)[:, None, :]
    boxes = corner + np.array([[0, 0], [0, 7], [9, 7], [9, 0]], np.float64)
    cuts = np.cumsum([0] + sizes)
    base = attrs.evolve(base, polygons=[boxes[a:b] for a, b in zip(cuts[:-1], cuts[1:])])
    # every character a second time, a tenth of a pixel away and a shade weaker: appended to its own region, and those of the
    # first region to the last region instead (a character inside two regions' boxes)
    points, probs, polygons = (list(v) for v in (base.points, base.probs, base.polygons))
    regions = [r for r in range(len(probs)) if len(probs[r])]
    for r in regions:
        to = regions[-1] if r == regions[0] else r
        points[to] = np.concatenate([points[to], base.points[r]])
        probs[to] = np.concatenate([probs[to], base.probs[r] * np.float32(0.99)])
        polygons[to] = np.concatenate([polygons[to], base.polygons[r] + 0.1])
    doubled = attrs.evolve(base, points=points, probs=probs, polygons=polygons)
    quads, pr = result_quads(doubled)
    ref, ref_stats = nms_quads_lists_host([quads], [pr], 0.5)
    assert ref_stats[0] == n and ref_stats[1] == 2 * n and ref_stats[4] >= n  # the oracle suppresses every duplicate
    got, stats = nms_quads([quads], [pr], 0.5)
    assert np.array_equal(stats, ref_stats) and np.array_equal(got[0].keep, ref[0].keep)
    assert np.array_equal(got[0].suppressor, ref[0].suppressor)
    out = suppress_results([doubled], 0.5)[0]
    assert_results_equal(out, base, 'duplicates removed')
    assert out.num_suppressed == n and out.nms_status == 0
    assert_results_equal(filter_result(doubled, got[0].keep), base, 'filter on device output')
    oq, op = result_quads(out)
    bq, bp = result_quads(base)
    assert np.array_equal(oq, bq) and np.array_equal(op, bp)


def test_an_image_with_too_many_characters_is_left_alone():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import AdaptiveScalingInferencingResult, suppress_results
    n = 8193
    sq = np.array([[0, 0], [0, 4], [4, 4], [4, 0]], np.float64)
    big = AdaptiveScalingInferencingResult(
        image_shape=(10, 10), regions=None, packed=np.ones((1,), bool), too_large=np.zeros((1,), bool),
        placements=np.zeros((1, 8), np.int32), placement_regions=np.ones((1,), np.int32), page_shape=(256, 256), page=None,
        region_labels=None, points=[np.zeros((n, 2), np.int32)], probs=[np.full((n,), 0.9, np.float32)],
        polygons=[np.broadcast_to(sq, (n, 4, 2)).copy()])
    small = attrs.evolve(big, points=[big.points[0][:3]], probs=[big.probs[0][:3]], polygons=[big.polygons[0][:3]])
    out = suppress_results([big, small], 0.5)
    assert out[0].nms_status == 2 and out[0].num_suppressed == 0 and len(out[0].probs[0]) == n
    assert out[1].nms_status == 0 and out[1].num_suppressed == 2 and len(out[1].probs[0]) == 1
