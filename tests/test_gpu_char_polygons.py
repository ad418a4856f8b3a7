"""Character quadrilaterals on the MI355X (csrc/charpoly.hip, ops.char_polygons, precise_infer_char_polygons) against the
numpy restatement of the reference's peak finding and polygon building in test_cpu_char_polygons.py: points, their order
and their probabilities exactly, the quadrilaterals to float32 rounding; end to end through the inference API, eager and
from a replayed HIP graph.  No scipy here (the oracle is plain numpy)."""
import numpy as np
import pytest
import torch

from tests import test_cpu_char_polygons as C
from tests.test_gpu_inferencing import build

pytestmark = pytest.mark.gpu

THR = 0.7


def synthetic_maps(B, H, W, seed):
    """Probabilities in multiples of 1/16 (plateaus and ties), pixels at exactly (float)0.7, a saturated block of 1.0 and
    zeroed padding rows / columns; offsets, softmaxed angles and distances at random."""
    g = np.random.default_rng(seed)
    prob = (np.floor(g.random((B, H, W)) * 16) / 16).astype(np.float32)
    prob[g.random((B, H, W)) < 0.05] = np.float32(THR)
    prob[:, H // 3:H // 3 + max(1, H // 5), W // 4:W // 4 + max(1, W // 6)] = 1.0
    if H > 8:
        prob[:, H - 3:] = 0
    if W > 8:
        prob[:, :, W - 5:] = 0
    offset = (g.standard_normal((B, H, W, 2)) * 6).astype(np.float32)
    logits = g.standard_normal((B, H, W, 4)).astype(np.float32)
    angle = (np.exp(logits) / np.exp(logits).sum(-1, keepdims=True)).astype(np.float32)
    dist = (g.random((B, H, W, 4)) * 12).astype(np.float32)
    return prob, offset, angle, dist


def run_device(prob, offset, angle, dist, thr, size, sy, sx):
    from vkit_ocr_model_adaptive_scaling_amd import ops
    dev = [torch.from_numpy(a).cuda() for a in (prob, offset, angle, dist)]
    count, points, probs, quads = ops.char_polygons(*dev, thr, size, sy, sx)
    n = int(count.item())
    return n, points[:n].cpu().numpy(), probs[:n].cpu().numpy(), quads[:n].cpu().numpy()


@pytest.mark.parametrize('size', [1, 4, 5, 7])
@pytest.mark.parametrize('B,H,W', [(1, 1, 9), (3, 1, 9), (1, 37, 53), (3, 37, 53), (1, 256, 384), (3, 256, 384)])
def test_char_polygons_match_oracle(B, H, W, size):
    maps = synthetic_maps(B, H, W, seed=H * 1000 + W + B + size)
    n, pts, prs, qds = run_device(*maps, THR, size, 2.0, 2.0)
    rp, rr, rq = C.char_polygons(*maps, THR, size, 2.0, 2.0)
    assert n == len(rp) and n > 0
    assert np.array_equal(pts, rp), 'points and their order'
    assert np.array_equal(prs, rr)
    assert np.allclose(qds, rq, atol=1e-3, rtol=1e-5), float(np.abs(qds - rq).max())


def test_char_polygons_plateau_and_empty():
    B, H, W = 2, 37, 53
    prob, offset, angle, dist = synthetic_maps(B, H, W, seed=1)
    full = np.full((B, H, W), 0.9, np.float32)  # one plateau: every pixel is a peak, the exact capacity
    n, pts, prs, qds = run_device(full, offset, angle, dist, THR, 5, 4.0, 4.0)
    assert n == B * H * W
    assert np.array_equal(pts, np.stack(np.nonzero(np.ones((B, H, W))), axis=1))
    assert (prs == np.float32(0.9)).all()
    rq = C.char_polygons(full, offset, angle, dist, THR, 5, 4.0, 4.0)[2]
    assert np.allclose(qds, rq, atol=1e-3, rtol=1e-5)
    low = np.full((B, H, W), 0.5, np.float32)  # below the threshold everywhere
    assert run_device(low, offset, angle, dist, THR, 5, 4.0, 4.0)[0] == 0


def _oracle_on(result, thr, size, fdf):
    return C.char_polygons(result.precise_char_prob_score_map[None], result.precise_np_char_up_left_corner_offset[None],
                           result.precise_np_char_corner_angle_distribution[None],
                           result.precise_np_char_corner_distance[None], thr, size, float(fdf), float(fdf))


def _same(a, b):
    return (np.array_equal(a.points, b.points) and np.array_equal(a.probs, b.probs)
            and np.array_equal(a.polygons, b.polygons))


def _threshold_for(inf, img):
    """A threshold that leaves a good number of peaks on this untrained model's maps (its probabilities sit near 0.5)."""
    p = inf.precise_infer(img).precise_char_prob_score_map
    return float(np.quantile(p[p > 0], 0.6))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16], ids=['f32', 'f16'])
def test_precise_infer_char_polygons_matches_oracle_on_precise_maps(dtype):
    inf, _ = build(dtype)
    img = np.random.default_rng(5).integers(0, 256, (100, 150, 3), dtype=np.uint8)
    inf.config.precise_build_polygons_positive_char_prob_thr = thr = _threshold_for(inf, img)
    q = inf.precise_infer(img)
    r = inf.precise_infer_char_polygons(img)
    rp, rr, rq = _oracle_on(q, thr, 5, 2)
    assert r.points.dtype == np.int32 and r.points.shape == (len(rp), 2) and len(rp) > 10
    assert r.probs.dtype == np.float32 and r.polygons.dtype == np.float32 and r.polygons.shape == (len(rp), 4, 2)
    assert np.array_equal(r.points, rp[:, 1:]), 'same peaks: the device prob values equal precise_infer\'s bit for bit'
    assert np.array_equal(r.probs, rr)
    assert np.allclose(r.polygons, rq, atol=1e-3, rtol=1e-5)
    assert r.padded_image.shape == (128, 160, 3)
    # grouping by a region label map at the map's resolution: the reference's per-region np.nonzero split
    labels = np.zeros((64, 80), np.int32)
    labels[4:30, 5:60] = 1
    labels[35:50, 10:75] = 2
    groups = inf.precise_group_char_polygons(r, labels)
    m = np.zeros((64, 80), bool)
    m[rp[:, 1], rp[:, 2]] = True
    assert len(groups) == 2
    for lab, grp in zip((1, 2), groups):
        expect = np.stack(np.nonzero(m & (labels == lab)), axis=1)
        assert np.array_equal(grp.points, expect)
        keep = labels[r.points[:, 0], r.points[:, 1]] == lab
        assert np.array_equal(grp.polygons, r.polygons[keep]) and np.array_equal(grp.probs, r.probs[keep])


def test_char_polygons_batch_and_graph_replay():
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import AdaptiveScalingInferencing, AdaptiveScalingInferencingConfig
    inf, _ = build(torch.float16)
    g = np.random.default_rng(6)
    imgs = [g.integers(0, 256, s, dtype=np.uint8) for s in ((60, 90, 3), (64, 96, 3), (40, 200, 3))]
    thr = _threshold_for(inf, imgs[0])
    inf.config.precise_build_polygons_positive_char_prob_thr = thr
    inf.config.precise_build_polygons_maximum_filter_size = 4.5
    eager = AdaptiveScalingInferencing(AdaptiveScalingInferencingConfig(
        model_jit=inf.model, compute_dtype=torch.float16, use_hip_graphs=False,
        precise_build_polygons_positive_char_prob_thr=thr, precise_build_polygons_maximum_filter_size=4.5))
    # a batch with two padded shapes (64 x 96 twice, 64 x 224): per page, the oracle on precise_infer_batch's maps
    res = inf.precise_infer_char_polygons_batch(imgs)
    maps = inf.precise_infer_batch(imgs)
    assert [r.padded_image.shape[:2] for r in res] == [(64, 96), (64, 96), (64, 224)]
    assert sum(len(r.points) for r in res) > 10
    for r, q in zip(res, maps):
        rp, rr, rq = _oracle_on(q, thr, 4.5, 2)
        assert np.array_equal(r.points, rp[:, 1:]) and np.array_equal(r.probs, rr)
        assert np.allclose(r.polygons, rq, atol=1e-3, rtol=1e-5)
    # eager first call, captured second call, replayed third call: bit for bit, and equal to use_hip_graphs=False
    img = imgs[2]
    calls = [inf.precise_infer_char_polygons(img) for _ in range(3)]
    assert inf.graphs.captures >= 1 and inf.graphs.replays >= 2
    ref = eager.precise_infer_char_polygons(img)
    for c in calls:
        assert _same(c, calls[0]) and _same(c, ref)
    assert _same(calls[0], res[2]), 'a page alone or in a batch'
    again = inf.precise_infer_char_polygons_batch(imgs)  # replays of both shapes
    for a, b in zip(again, res):
        assert _same(a, b)
