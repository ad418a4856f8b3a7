"""Scoring meets the rest of the project on the MI355X: quads taken through ``label_points`` and the float64 restatement of
precise_build_polygon (the round trip of tests/test_cpu_char_labels.py) score precision = recall = 1 against themselves; a
dropped prediction and a far-away quad move fn and fp by exactly one each; ``result_quads`` of an ``infer`` call goes
through ``evaluate_quads`` and its counts equal the host route's on the same quads."""
import numpy as np
import pytest
import torch

from tests.test_cpu_char_labels import build_polygon, seeded_quads
from tests.test_gpu_inferencing import build
from tests.test_gpu_infer_oriented import configure

pytestmark = pytest.mark.gpu


def round_tripped(n=40):
    """n annotated quads on a grid of 150 px cells and what the precise head's outputs would rebuild for each from its first
    label point -> (gt (n, 4, 2), pred (n, 4, 2)) in image pixels"""
    from vkit_ocr_model_adaptive_scaling_amd.dataset import label_points, quad_rows
    h, w, f, box = 120, 160, 2, (10, 109, 10, 149)
    gt, pred = [], []
    for i, q in enumerate(seeded_quads(n)):
        rows, ok = quad_rows(q[None] * f, h, w, f)
        assert ok[0]
        lp = label_points(q[None] * f, ok, h, w, f, box, 1, rng_seed=11, rng_stream=i)
        p = np.array([lp['downsampled_label_point_y'][0], lp['downsampled_label_point_x'][0]], dtype=np.float64) * f
        built = build_polygon(p, lp['up_left_offsets'][0].astype(np.float64), lp['corner_angles'][0], lp['corner_distances'][0])
        cell = np.array([(i // 8) * 300.0, (i % 8) * 300.0])
        gt.append(q * f + cell)
        pred.append(built + cell)
    return np.stack(gt), np.stack(pred)


def test_round_trip_scores_one_and_misses_count():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import evaluate_quads, evaluate_quads_host
    gt, pred = round_tripped()
    res, score = evaluate_quads([pred], [gt])
    assert (score.tp, score.fp, score.fn) == (40, 0, 0) and score.precision == score.recall == score.f1 == 1.0
    assert res[0].gt_match.tolist() == list(range(40)) and res[0].gt_iou.min() > 0.8 and score.mean_iou > 0.9
    far = np.array([[[5000.0, 5000.0], [5000, 5040], [5030, 5040], [5030, 5000]]])
    res, score = evaluate_quads([np.concatenate([pred[:17], pred[18:], far])], [gt])
    assert (score.tp, score.fp, score.fn) == (39, 1, 1) and res[0].gt_match[17] == -1 and res[0].pred_match[-1] == -1
    assert score.precision == score.recall == 39 / 40
    host, host_score = evaluate_quads_host([np.concatenate([pred[:17], pred[18:], far])], [gt])
    assert host_score == score and np.array_equal(host[0].gt_match, res[0].gt_match)


def test_infer_output_goes_through_evaluate_quads():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import evaluate_quads, evaluate_quads_host, result_quads
    inf, _ = build(torch.float16)
    configure(inf, False)
    img = np.random.default_rng(5).integers(0, 256, (100, 150, 3), dtype=np.uint8)
    quads, probs = result_quads(inf.infer(img))
    assert quads.shape == (len(probs), 4, 2) and len(probs) > 0
    # every other quad of the untrained model, grown by a tenth about its centroid (IoU 1 / 1.21 with its source, whatever
    # its size), as the annotations; a score threshold on the predictions
    centre = quads[::2].mean(axis=1, keepdims=True)
    gt = centre + 1.1 * (quads[::2] - centre)
    thr = float(np.median(probs))
    res, score = evaluate_quads([quads], [gt], pred_scores=[probs], score_thr=thr)
    host, host_score = evaluate_quads_host([quads], [gt], pred_scores=[probs], score_thr=thr)
    print(f'{len(quads)} quads from infer, {res[0].n_pred} at or above the median score, {res[0].n_gt} valid annotations, '
          f'tp {res[0].tp}, pairs {res[0].pairs}')
    assert score == host_score and res[0].pairs >= res[0].tp > 0
    for name in ('tp', 'n_gt', 'n_pred', 'pairs', 'candidates'):
        assert getattr(res[0], name) == getattr(host[0], name), name
    assert np.array_equal(res[0].gt_match, host[0].gt_match) and np.array_equal(res[0].pred_match, host[0].pred_match)
    assert res[0].n_pred == int(((probs >= thr) & res[0].pred_valid).sum()) <= len(quads)
