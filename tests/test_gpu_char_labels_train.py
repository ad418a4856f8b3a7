"""Labels from character quadrilaterals through the whole training path on the MI355X - QuadSample pairs ->
adaptive_scaling_quads_collate_fn -> CharLabelRasterizer -> batch_to_device -> TwoPassStep with the loss functions and a
backward pass on the tiny model - and "labels meet inference": the rasterised score map of well-separated quads, fed to
ops.char_polygons at the config defaults, yields exactly one peak per quad at its centroid pixel (the same check runs on
the host oracles in tests/test_cpu_char_labels.py)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import char_label_cases as C
from tests.test_gpu_char_labels import SCORE_ULPS

pytestmark = pytest.mark.gpu


def quad_pairs():
    """B = 2, 64 x 128 images (32 x 64 maps at f = 2), 12 quads in map pixels: six per pass and image, one of them
    outside the core box and one invalid"""
    line = lambda y, n: [C.rot(y + 0.5 * (i % 2), 9.5 + 11 * i, 4, 4.5, 6 * i - 9) for i in range(n)]
    sets = [line(10, 5) + [C.rect(27, 40, 31, 50)], line(20, 4) + [C.rect(5, 50, 14, 60), C.rect(5, 5, 9, 9)[::-1]],
            line(11, 3) + line(22, 3), line(21, 5) + [C.rect(6, 20, 14, 30)]]
    img = lambda i: np.random.default_rng(i).integers(0, 256, (64, 128, 3), dtype=np.uint8)
    q = [np.array(s, dtype=np.float64) * 2 for s in sets]
    from vkit_ocr_model_adaptive_scaling_amd.dataset import QuadSample
    return [(QuadSample(img(0), q[0], index=0), QuadSample(img(1), q[1], index=0)),
            (QuadSample(img(2), q[2], index=1), QuadSample(img(3), q[3], index=1))]


def test_quad_batch_through_two_pass_step():
    from vkit_ocr_model_adaptive_scaling_amd import _lib
    from vkit_ocr_model_adaptive_scaling_amd.dataset import (adaptive_scaling_quads_collate_fn, CharLabelRasterizer,
                                                             char_labels_host, SyntheticAdaptiveScalingIterableDataset,
                                                             adaptive_scaling_dataset_collate_fn)
    from vkit_ocr_model_adaptive_scaling_amd.model import (AdaptiveScaling, AdaptiveScalingConfig, AdaptiveScalingSize,
                                                           AdaptiveScalingNeckHeadType)
    from vkit_ocr_model_adaptive_scaling_amd.loss_function import (
        AdaptiveScalingRoughLossFunction, AdaptiveScalingRoughLossFunctionConifg,
        AdaptiveScalingPreciseLossFunction, AdaptiveScalingPreciseLossFunctionConifg)
    from vkit_ocr_model_adaptive_scaling_amd.training import TwoPassStep, batch_to_device
    dev = torch.device('cuda')
    P = 8
    collated = adaptive_scaling_quads_collate_fn(quad_pairs(), P=P, f=2, margin=4, rng_seed=7)
    batch = CharLabelRasterizer(dev)(collated)
    # the schema of the synthetic source, key for key, and the maps of the host route
    ds = SyntheticAdaptiveScalingIterableDataset(2, (64, 128), margin=4, num_label_points=P)
    want = adaptive_scaling_dataset_collate_fn(ds.sample(i) for i in range(2))
    host = char_labels_host(collated)
    for part in ('rough', 'precise'):
        assert set(batch[part]) == set(want[part])
        for k, v in want[part].items():
            if torch.is_tensor(v):
                assert batch[part][k].dtype == v.dtype and batch[part][k].shape == v.shape, (part, k)
        for k in ('downsampled_mask', 'downsampled_score_map'):
            assert batch[part][k].is_cuda
        assert torch.equal(batch[part]['downsampled_mask'].cpu(), host[part]['downsampled_mask'])
    assert torch.equal(batch['rough']['downsampled_score_map'].cpu(), host['rough']['downsampled_score_map'])
    d = C.ulp_distance(batch['precise']['downsampled_score_map'].cpu().numpy(), host['precise']['downsampled_score_map'].numpy())
    assert int(d.max()) <= SCORE_ULPS
    rough, precise = batch_to_device(batch['rough'], dev), batch_to_device(batch['precise'], dev)
    assert float(rough['downsampled_mask'].sum()) > 0 and float(precise['downsampled_score_map'].max()) > 0.9

    # the label points lie inside the map
    py, px = precise['downsampled_label_point_y'].reshape(-1), precise['downsampled_label_point_x'].reshape(-1)
    margin = torch.full((1,), -99, dtype=torch.int64, device=dev)
    h, w = precise['downsampled_shape']
    _lib.check(_lib.lib.vkas_points_margin(ctypes.c_void_p(py.data_ptr()), ctypes.c_void_p(px.data_ptr()), py.numel(), h, w,
                                           ctypes.c_void_p(margin.data_ptr()),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'points_margin')
    assert int(margin.item()) >= 0

    torch.manual_seed(3)
    model = AdaptiveScaling(AdaptiveScalingConfig(AdaptiveScalingSize.TINY, AdaptiveScalingNeckHeadType.FPN)).to(dev).train()
    rcfg = AdaptiveScalingRoughLossFunctionConifg()
    # the rough l1_mask (loss_function/adaptive_scaling.py:112-114) is not empty
    with torch.no_grad():
        height = model.forward_rough(rough['image'])[1]
    box = rough['downsampled_core_box']
    hc = height[:, 0, box.up:box.down + 1, box.left:box.right + 1].float()
    l1_mask = ((hc > rcfg.char_height_feature_min) & (rough['downsampled_score_map'] > rcfg.downsampled_score_map_min)
               & rough['downsampled_mask'].bool())
    assert int(l1_mask.sum()) > 0

    class KeepGrads:  # TwoPassStep's optimizer slot: no parameter update
        def step(self, lr=None):
            pass

        def zero_grad(self):
            pass

    rough_loss, precise_loss = TwoPassStep(model, AdaptiveScalingRoughLossFunction(rcfg),
                                           AdaptiveScalingPreciseLossFunction(AdaptiveScalingPreciseLossFunctionConifg()),
                                           KeepGrads())(rough, precise)
    for loss in (rough_loss, precise_loss):
        assert np.isfinite(float(loss)) and float(loss) != 0.0
    grads = [q.grad for q in model.parameters() if q.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads) and any(bool(g.any()) for g in grads)


def test_labels_meet_inference():
    from vkit_ocr_model_adaptive_scaling_amd import ops
    from vkit_ocr_model_adaptive_scaling_amd.dataset import quad_rows
    m = C.MEET
    quads = np.array(m['quads'], dtype=np.float64) * m['f']
    rows, ok = quad_rows(quads, m['h'], m['w'], m['f'])
    assert ok.all()
    d_rows = torch.from_numpy(rows[None]).cuda()
    count = torch.tensor([len(rows)], dtype=torch.int32, device='cuda')
    score = ops.char_label_maps(d_rows, count, m['h'], m['w'], m['box'], with_height=False)[3]
    B, H, W = score.shape
    zeros = lambda c: torch.zeros((B, H, W, c), device='cuda')
    n, points, probs, _ = ops.char_polygons(score, zeros(2), zeros(4), zeros(4), 0.7, 5, float(m['f']), float(m['f']))
    n = int(n.item())
    want = np.floor(quads.mean(1) / m['f']).astype(np.int64) - (m['box'][0], m['box'][2])
    got = points[:n].cpu().numpy()
    assert n == len(quads) and (got[:, 0] == 0).all()
    assert sorted(map(tuple, got[:, 1:])) == sorted(map(tuple, want))
    assert float(probs[:n].min()) > 0.9
