"""The ribbon score on what the inference path emits, on the MI355X.

The two concentric arcs go through ``evaluate_ribbons``.  A hand-made arc of characters, spread over a result's regions,
becomes a line and a spine by ``group_results`` and ``spine_strips_for_results`` (the steps of ``infer``) and is scored
through ``result_ribbons`` against its own outline: one to one.  Then ``result_ribbons`` of ``infer`` on the small
untrained model, with the curved flag on and off, go through ``evaluate_ribbons`` and equal the host route; with the flag
off every line is a quad and the score is that of ``evaluate_lines`` on ``line_polygons``."""
import attrs
import numpy as np
import pytest
import torch

from tests import ribbon_cases as C
from tests import spine_cases as P

pytestmark = pytest.mark.gpu

FIELDS = ('gt_kind', 'gt_group', 'pred_kind', 'pred_group', 'stats')


def assert_same(got, ref, what):
    assert len(got) == len(ref), what
    for k, (a, b) in enumerate(zip(got, ref)):
        for f in FIELDS:
            assert np.array_equal(getattr(a, f), getattr(b, f)) and getattr(a, f).dtype == getattr(b, f).dtype, (what, k, f)


def test_the_two_arcs_on_the_device():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import evaluate_lines, evaluate_ribbons, evaluate_ribbons_host
    ribbons, rects = C.two_arcs()
    res, score = evaluate_ribbons([ribbons], [ribbons])
    ref, ref_score = evaluate_ribbons_host([ribbons], [ribbons])
    assert_same(res, ref, 'two arcs')
    assert score == ref_score and res[0].gt_kind.tolist() == [2, 2] and res[0].gt_group.tolist() == [0, 1]
    assert res[0].stat('pairs') == 4 and res[0].stat('candidates') == 2 and score.f1 == 1.0
    flat, flat_score = evaluate_lines([rects], [rects])  # the chord rectangles of the same two lines
    assert flat[0].stat('one_to_one') < 2 and flat_score.f1 < 1.0


def test_a_hand_made_arc_against_its_own_outline():
    from tests.test_gpu_inferencing import build
    from tests.test_gpu_infer_oriented import configure
    from tests.test_gpu_quad_lines_infer import images
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import (evaluate_ribbons, evaluate_ribbons_host, group_results,
                                                                  result_ribbons, spine_strips_for_results)
    inf, _ = build(torch.float16)
    configure(inf, False)
    centre, radius = (20.0, 20.0), 200.0
    imgs = [P.radial_image((256, 256), centre, radius)]
    base = inf.infer(images()[0])
    sizes = [len(p) for p in base.probs]
    n = sum(sizes)
    assert n >= 45 and sum(k > 0 for k in sizes) >= 2
    arc = P.arc(centre, radius)
    order = np.random.default_rng(9).permutation(len(arc))
    spare = np.array([[[240.0 - 3 * k, 2.0], [240.0 - 3 * k, 4.0], [242.0 - 3 * k, 4.0], [242.0 - 3 * k, 2.0]]
                      for k in range(n - len(arc))]).reshape(-1, 4, 2)
    quads = np.concatenate([arc[order], spare])
    cuts = np.cumsum([0] + sizes)
    made = attrs.evolve(base, polygons=[quads[a:b] for a, b in zip(cuts[:-1], cuts[1:])])
    out, _ = spine_strips_for_results(group_results([made]), imgs)
    s = [m.tolist() for m in out[0].line_chars].index(np.argsort(order).tolist())
    ribbons = result_ribbons(out[0])
    assert len(ribbons) == len(out[0].line_polygons) and len(ribbons[s]) == len(out[0].line_spines[s]) == 22
    # the annotation: the outline of the characters, top corners along the line, then bottom corners back
    outline = np.rint(np.concatenate([arc[:, :2].reshape(-1, 2), arc[::-1, 2:].reshape(-1, 2)]) * 16) / 16
    assert outline.shape == (80, 2)
    res, score = evaluate_ribbons([ribbons], [[outline]])
    ref, ref_score = evaluate_ribbons_host([ribbons], [[outline]])
    assert_same(res, ref, 'hand-made arc')
    assert score == ref_score and res[0].gt_kind.tolist() == [2] and res[0].gt_group.tolist() == [s]
    assert res[0].pred_kind[s] == 2 and score.one_to_one == 1 and score.recall == 1.0


def test_result_ribbons_of_infer_with_the_curved_flag_on_and_off():
    from tests.test_gpu_inferencing import build
    from tests.test_gpu_infer_oriented import configure
    from tests.test_gpu_quad_lines_infer import images
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import (evaluate_lines, evaluate_ribbons, evaluate_ribbons_host,
                                                                  result_ribbons)
    inf, _ = build(torch.float16)
    configure(inf, False)
    c = inf.config
    c.precise_char_lines = c.precise_line_strips = True
    imgs = images()
    rng = np.random.default_rng(8)
    for curved in (False, True):
        c.precise_line_strip_curved = curved
        results = [inf.infer(imgs[0])] + list(inf.infer_batch(imgs[1:]).results)
        pred = [result_ribbons(r) for r in results]
        quads = [np.asarray(r.line_polygons, np.float64).reshape(-1, 4, 2) for r in results]
        assert sum(len(p) for p in pred) > 10 and [len(p) for p in pred] == [len(q) for q in quads]
        if curved:
            assert any(len(s) >= 2 for r in results for s in r.line_spines)
        else:
            assert all(r.line_spines == [] for r in results) and all(len(a) == 2 for p in pred for a in p)
        # annotations made from the detections' quads: every third one missing, the others grown by a twentieth about
        # their centres; of those every fourth cut into a left and a right half (a merge)
        gt = []
        for q in quads:
            g = q[np.arange(len(q)) % 3 != 2]
            g = g.mean(axis=1, keepdims=True) + 1.05 * (g - g.mean(axis=1, keepdims=True))
            left, right = g[1::4].copy(), g[1::4].copy()
            mid = (left[:, [0, 3]] + left[:, [1, 2]]) / 2
            left[:, [1, 2]], right[:, [0, 3]] = mid, mid
            gt.append(np.concatenate([np.delete(g, np.s_[1::4], axis=0), left, right]))
        got, score = evaluate_ribbons(pred, gt)
        ref, ref_score = evaluate_ribbons_host(pred, gt)
        assert_same(got, ref, f'curved = {curved}')
        assert score == ref_score and score.n_gt > 5 and score.one_to_one + score.merged_gt > 3
        if not curved:  # every line a quad and no don't-care annotation: the line score
            flat, flat_score = evaluate_lines(quads, gt)
            assert_same(got, flat, 'ribbons of one segment against evaluate_lines')
            assert score == flat_score and score.merge_pred > 0
        print(f'curved = {curved}: {score}')
    c.precise_line_strip_curved = False
