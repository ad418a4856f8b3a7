"""Average precision meets the rest of the project on the MI355X: the round trip of tests/test_gpu_quad_match_infer.py
scores AP = 1 at 0.5; marking one annotation don't-care turns its prediction from TP to IGNORED and lowers n_gt by one;
``result_quads`` of an ``infer`` call goes through ``evaluate_quads_ranked`` and equals the host route on the same quads."""
import numpy as np
import pytest
import torch

from tests.test_gpu_inferencing import build
from tests.test_gpu_infer_oriented import configure
from tests.test_gpu_quad_match_infer import round_tripped

pytestmark = pytest.mark.gpu

TP, IGNORED = 1, 3


def test_round_trip_scores_ap_one_and_a_dont_care_annotation_ignores_its_prediction():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import evaluate_quads_ranked
    gt, pred = round_tripped()
    probs = np.random.default_rng(3).uniform(0.5, 1.0, len(pred)).astype(np.float32)
    res, score = evaluate_quads_ranked([pred], [gt], [probs], iou_thrs=(0.5, 0.75))
    assert score.ap[0] == 1.0 and score.n_gt == 40 and score.tp[0] == 40 and score.fp[0] == 0 and score.ignored[0] == 0
    assert (res[0].pred_state[0] == TP).all() and res[0].pred_match[0].tolist() == list(range(40))
    assert score.best[0].f1 == 1.0 and score.best[0].score_thr == float(probs.min()) and 0 < score.map <= 1.0
    care = np.ones(40, np.uint8)
    care[17] = 0
    res2, score2 = evaluate_quads_ranked([pred], [gt], [probs], [care], iou_thrs=(0.5, 0.75))
    assert res2[0].pred_state[0, 17] == IGNORED and res2[0].pred_match[0, 17] == -1 and res2[0].covered[17]
    assert score2.n_gt == 39 and score2.tp[0] == 39 and score2.ignored[0] == 1 and score2.fp[0] == 0 and score2.ap[0] == 1.0
    others = np.arange(40) != 17
    assert np.array_equal(res2[0].pred_state[0, others], res[0].pred_state[0, others])
    assert res2[0].gt_match[0, 17] == -1 and res2[0].dc_stats.tolist()[0] == 1


def test_infer_output_goes_through_evaluate_quads_ranked():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import evaluate_quads_ranked, evaluate_quads_ranked_host, result_quads
    inf, _ = build(torch.float16)
    configure(inf, False)
    img = np.random.default_rng(5).integers(0, 256, (100, 150, 3), dtype=np.uint8)
    quads, probs = result_quads(inf.infer(img))
    assert quads.shape == (len(probs), 4, 2) and len(probs) > 0
    # every other quad of the untrained model, grown by a tenth about its centroid (IoU 1 / 1.21 with its source), as the
    # annotations; every fifth of those a don't-care one
    centre = quads[::2].mean(axis=1, keepdims=True)
    gt = centre + 1.1 * (quads[::2] - centre)
    care = (np.arange(len(gt)) % 5 != 0).astype(np.uint8)
    thrs = (0.5, 0.8, 0.9)
    res, score = evaluate_quads_ranked([quads], [gt], [probs], [care], iou_thrs=thrs)
    host, host_score = evaluate_quads_ranked_host([quads], [gt], [probs], [care], iou_thrs=thrs)
    print(f'{len(quads)} quads from infer, stats at 0.5 {res[0].stats[0].tolist()}, dc {res[0].dc_stats.tolist()}, AP '
          f'{score.ap.tolist()}')
    for f in ('pred_state', 'pred_match', 'gt_match', 'covered', 'gt_valid', 'gt_care', 'pred_valid', 'stats', 'dc_stats'):
        assert np.array_equal(getattr(res[0], f), getattr(host[0], f)), f
    assert res[0].pred_iou.tobytes() == host[0].pred_iou.tobytes()
    assert np.array_equal(score.ap, host_score.ap) and score.map == host_score.map and score.best == host_score.best
    assert res[0].stats[0, 0] > 0 and score.n_gt == int((res[0].gt_valid & res[0].gt_care).sum())
