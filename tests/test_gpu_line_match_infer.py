"""The text-line score on what the inference path emits, on the MI355X.

Three lines of characters from the hand-made layout of tests/test_gpu_quad_lines_infer.py go through ``group_results`` (the
step of ``infer``), and their ``line_polygons`` are scored against rectangles drawn round the same characters: as
annotated they match one to one; with ``precise_char_line_gap`` lowered so that the lines break into words the same
annotations score as splits - where ``evaluate_quads``, the one-to-one IoU route, reports misses: what the feature adds;
with the annotations given as words and the lines whole they score as merges.  Then the ``line_polygons`` of an ``infer``
call on the small untrained model go through ``evaluate_lines`` and equal the host route."""
import numpy as np
import pytest
import torch

from tests import quad_line_cases as Q

pytestmark = pytest.mark.gpu

ANGLE = 0.35


def rectangle_round(quads, pad=1.0):
    """the rectangle along the page's direction round all corners of ``quads``, ``pad`` px wider on every side, on the 1/16 grid"""
    pts = np.asarray(quads, np.float64).reshape(-1, 2) - 400.0
    c, s = np.cos(ANGLE), np.sin(ANGLE)
    v, u = pts[:, 0] * c - pts[:, 1] * s, pts[:, 0] * s + pts[:, 1] * c  # the page turned back: v down, u along
    v0, v1, u0, u1 = v.min() - pad, v.max() + pad, u.min() - pad, u.max() + pad
    box = np.array([[v0, u0], [v0, u1], [v1, u1], [v1, u0]])
    back = np.stack([box[:, 0] * c + box[:, 1] * s, -box[:, 0] * s + box[:, 1] * c], 1) + 400.0
    return np.rint(back * 16) / 16


def made_result(quads):
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import AdaptiveScalingInferencingResult
    n = len(quads)
    return AdaptiveScalingInferencingResult(
        image_shape=(900, 900), regions=None, packed=np.ones((1,), bool), too_large=np.zeros((1,), bool),
        placements=np.zeros((1, 8), np.int32), placement_regions=np.ones((1,), np.int32), page_shape=(256, 256), page=None,
        region_labels=None, points=[np.zeros((n, 2), np.int32)], probs=[np.full((n,), 0.9, np.float32)], polygons=[quads])


def test_lines_words_and_annotations_of_either_kind():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import (evaluate_lines, evaluate_lines_host, evaluate_quads,
                                                                 group_results)
    quads, truth = Q.layout(3, 15, **Q.LATIN, word_space=10.0, angle=ANGLE, seed=9)
    quads = quads + 400.0
    made = made_result(quads)
    line_gt = np.stack([rectangle_round(quads[line]) for line in truth])
    word_gt = np.stack([rectangle_round(quads[line[k:k + 5]]) for line in truth for k in (0, 5, 10)])
    whole = group_results([made])[0]                 # the default gap of 1.5 character heights
    words = group_results([made], gap=0.75)[0]       # lowered: a word space of 10 px breaks a line
    assert [m.tolist() for m in whole.line_chars] == truth and len(words.line_chars) == 9
    assert all(len(m) == 5 for m in words.line_chars)

    # as annotated: all one to one
    res, score = evaluate_lines([whole.line_polygons], [line_gt])
    assert res[0].gt_kind.tolist() == [2, 2, 2] and res[0].pred_kind.tolist() == [2, 2, 2]
    assert score.precision == 1.0 and score.recall == 1.0 and score.f1 == 1.0 and score.one_to_one == 3

    # the lines broken into words: every annotated line is found as a split of three, worth 0.8 ...
    res, score = evaluate_lines([words.line_polygons], [line_gt])
    assert res[0].gt_kind.tolist() == [3, 3, 3] and res[0].pred_kind.tolist() == [3] * 9
    assert sorted(res[0].pred_group.tolist()) == [0, 0, 0, 1, 1, 1, 2, 2, 2] and res[0].stat('rounds_split') == 1
    assert (score.one_to_one, score.split_gt, score.split_pred, score.merged_gt) == (0, 3, 9, 0)
    assert score.recall == pytest.approx(0.8, abs=1e-12) and score.precision == pytest.approx(0.8, abs=1e-12)
    # ... where the one-to-one IoU matching sees three misses and nine false detections
    _, plain = evaluate_quads([words.line_polygons], [line_gt])
    assert (plain.tp, plain.fn, plain.fp) == (0, 3, 9) and plain.recall == 0.0
    # any other credit can be applied to the same counts
    _, full = evaluate_lines([words.line_polygons], [line_gt], split_credit=1.0)
    assert full.recall == 1.0 and full.precision == 1.0

    # the annotations given as words, the lines whole: merges
    res, score = evaluate_lines([whole.line_polygons], [word_gt])
    assert res[0].gt_kind.tolist() == [4] * 9 and res[0].pred_kind.tolist() == [4, 4, 4]
    assert res[0].gt_group.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2] and res[0].stat('rounds_merge') == 1
    assert (score.one_to_one, score.split_gt, score.merged_gt, score.merge_pred) == (0, 0, 9, 3)
    assert score.recall == pytest.approx(0.8, abs=1e-12) and score.precision == pytest.approx(0.8, abs=1e-12)
    _, plain = evaluate_quads([whole.line_polygons], [word_gt])
    assert plain.tp == 0

    # all of it equals the host route
    for pred, gt in ((whole.line_polygons, line_gt), (words.line_polygons, line_gt), (whole.line_polygons, word_gt)):
        got, got_score = evaluate_lines([pred], [gt])
        ref, ref_score = evaluate_lines_host([pred], [gt])
        assert got_score == ref_score and np.array_equal(got[0].stats, ref[0].stats)
        assert np.array_equal(got[0].gt_group, ref[0].gt_group) and np.array_equal(got[0].pred_group, ref[0].pred_group)


def test_line_polygons_of_infer_through_evaluate_lines():
    from tests.test_gpu_inferencing import build
    from tests.test_gpu_infer_oriented import configure
    from tests.test_gpu_quad_lines_infer import images
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import evaluate_lines, evaluate_lines_host
    inf, _ = build(torch.float16)
    configure(inf, False)
    inf.config.precise_char_lines = True
    imgs = images()
    results = [inf.infer(imgs[0])] + list(inf.infer_batch(imgs[1:]).results)
    pred = [r.line_polygons for r in results]
    assert sum(len(p) for p in pred) > 10
    rng = np.random.default_rng(8)
    # annotations made from the detections: every third one missing, the others grown by a twentieth about their centres;
    # of those every fourth stretched to twice its width (no match) and every fourth cut into a left and a right half (a
    # merge)
    gt, care = [], []
    for p in pred:
        g = p[np.arange(len(p)) % 3 != 2]
        g = g.mean(axis=1, keepdims=True) + 1.05 * (g - g.mean(axis=1, keepdims=True))
        g[::4, 1:3] += (g[::4, 1:3] - g[::4, [0, 3]])
        left, right = g[1::4].copy(), g[1::4].copy()
        mid = (left[:, [0, 3]] + left[:, [1, 2]]) / 2
        left[:, [1, 2]], right[:, [0, 3]] = mid, mid
        g = np.concatenate([np.delete(g, np.s_[1::4], axis=0), left, right])
        gt.append(g)
        care.append((rng.uniform(size=len(g)) > 0.2).astype(np.uint8))
    got, score = evaluate_lines(pred, gt, care)
    ref, ref_score = evaluate_lines_host(pred, gt, care)
    assert score == ref_score and score.n_gt > 5 and score.one_to_one > 3 and score.merge_pred > 0
    for a, b in zip(got, ref):
        for f in ('gt_kind', 'gt_group', 'pred_kind', 'pred_group', 'stats'):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
    print(f'infer: {score}')
