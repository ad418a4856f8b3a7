"""Annotated pages through the whole training path on the MI355X - AnnotatedPage pairs -> adaptive_scaling_pages_collate_fn
-> PageCropWarper -> CharLabelRasterizer -> batch_to_device -> TwoPassStep on the tiny model - with the warped images equal to
the host route's bit for bit, and "labels meet inference" through a crop: the rasterised precise score of the transformed
quads, fed to ops.char_polygons, has a peak at the centroid pixel of every quad whose centroid lies in the core box (where
that pixel is the nearest one in the quad's own frame; on it or next to it otherwise)."""
import functools

import numpy as np
import pytest
import torch

from tests import crop_cases as C

pytestmark = pytest.mark.gpu

SIZE, F, MARGIN, P = (128, 128), 2, 4, 8


def pages():
    """four pages of 150 x 220 to 900 x 700 with characters of 12 to 80 px"""
    return [C.synthetic_page(31, 150, 220, 12, 0), C.synthetic_page(32, 400, 380, 30, 1),
            C.synthetic_page(33, 640, 520, 52, 2), C.synthetic_page(34, 900, 700, 80, 3)]


@functools.lru_cache(maxsize=None)
def collated():
    from vkit_ocr_model_adaptive_scaling_amd.dataset import CropConfig, adaptive_scaling_pages_collate_fn
    cfg = CropConfig(size=SIZE, core_margin=F * MARGIN)
    return adaptive_scaling_pages_collate_fn([(p, p) for p in pages()], cfg, P=P, f=F, margin=MARGIN, rng_seed=17)


def test_pages_through_two_pass_step():
    from vkit_ocr_model_adaptive_scaling_amd.dataset import (PageCropWarper, CharLabelRasterizer, crops_host,
                                                             SyntheticAdaptiveScalingIterableDataset,
                                                             adaptive_scaling_dataset_collate_fn)
    from vkit_ocr_model_adaptive_scaling_amd.model import (AdaptiveScaling, AdaptiveScalingConfig, AdaptiveScalingSize,
                                                           AdaptiveScalingNeckHeadType)
    from vkit_ocr_model_adaptive_scaling_amd.loss_function import (
        AdaptiveScalingRoughLossFunction, AdaptiveScalingRoughLossFunctionConifg,
        AdaptiveScalingPreciseLossFunction, AdaptiveScalingPreciseLossFunctionConifg)
    from vkit_ocr_model_adaptive_scaling_amd.training import TwoPassStep, batch_to_device
    dev = torch.device('cuda')
    warped = PageCropWarper(dev)(collated())
    host = crops_host(collated())
    for part in ('rough', 'precise'):
        assert set(warped[part]) == set(host[part]) and 'crop_rows' not in warped[part]
        image = warped[part]['image']
        assert image.is_cuda and image.dtype == torch.float32 and tuple(image.shape) == (4, 3) + SIZE
        assert torch.equal(image.cpu().view(torch.int32), host[part]['image'].view(torch.int32)), part
        assert float(image.min()) >= 0.0 and float(image.max()) <= 255.0 and float(image.std()) > 10.0
    batch = CharLabelRasterizer(dev)(warped)
    ds = SyntheticAdaptiveScalingIterableDataset(4, SIZE, margin=MARGIN, num_label_points=P)
    want = adaptive_scaling_dataset_collate_fn(ds.sample(i) for i in range(4))
    for part in ('rough', 'precise'):  # the schema of the synthetic source, key for key
        assert set(batch[part]) == set(want[part])
        for k, v in want[part].items():
            if torch.is_tensor(v):
                assert batch[part][k].dtype == v.dtype and batch[part][k].shape == v.shape, (part, k)
    rough, precise = batch_to_device(batch['rough'], dev), batch_to_device(batch['precise'], dev)
    assert float(precise['downsampled_mask'].sum()) > 0 and float(precise['downsampled_score_map'].max()) > 0.9

    class KeepGrads:  # TwoPassStep's optimizer slot: no parameter update
        def step(self, lr=None):
            pass

        def zero_grad(self):
            pass

    torch.manual_seed(3)
    model = AdaptiveScaling(AdaptiveScalingConfig(AdaptiveScalingSize.TINY, AdaptiveScalingNeckHeadType.FPN)).to(dev).train()
    rough_loss, precise_loss = TwoPassStep(model, AdaptiveScalingRoughLossFunction(AdaptiveScalingRoughLossFunctionConifg()),
                                           AdaptiveScalingPreciseLossFunction(AdaptiveScalingPreciseLossFunctionConifg()),
                                           KeepGrads())(rough, precise)
    for loss in (rough_loss, precise_loss):
        assert np.isfinite(float(loss))
    grads = [q.grad for q in model.parameters() if q.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads) and any(bool(g.any()) for g in grads)


def centroid_pixel_is_nearest(q):
    """The score of a quad (map pixels) falls with a = |M (p - c)|^2 in its own frame (dataset/labels.py), which is neither
    round nor upright: the pixel that holds the centroid has the highest score only if its centre is the nearest of its 3 x 3
    neighbourhood IN THAT FRAME.  float64, with G = M^T M; a neighbour at step e must be farther by more than what the
    rule's Q4 corners can move the centre - 1/32 px per axis, i.e. 2 |G e|_1 / 32 of a - plus 1e-4 for the float32 rounding
    of a (a is 1 at a side mid-point)."""
    c = q.mean(axis=0)
    frame = np.stack([((q[1] + q[2]) - (q[0] + q[3])) / 4, ((q[3] + q[2]) - (q[0] + q[1])) / 4], axis=1)
    inv = np.linalg.inv(frame)
    G = inv.T @ inv
    a = lambda p: float(((inv @ (p + 0.5 - c)) ** 2).sum())
    pixel = np.floor(c)
    steps = [np.array((i, j), dtype=np.float64) for i in (-1, 0, 1) for j in (-1, 0, 1) if (i, j) != (0, 0)]
    return all(a(pixel + e) - a(pixel) > np.abs(G @ e).sum() / 16 + 1e-4 for e in steps)


def test_labels_meet_inference_through_a_crop():
    from vkit_ocr_model_adaptive_scaling_amd import ops
    from vkit_ocr_model_adaptive_scaling_amd.dataset import crop_quads
    part = collated()['precise']
    h, w = part['downsampled_shape']
    box = part['downsampled_core_box']
    score = ops.char_label_maps(part['char_quad_rows'].cuda(), part['char_quad_count'].cuda(), h, w, box,
                                with_height=False)[3]
    B, CH, CW = score.shape
    zeros = lambda c: torch.zeros((B, CH, CW, c), device='cuda')
    n, points, probs, _ = ops.char_polygons(score, zeros(2), zeros(4), zeros(4), 0.7, 5, float(F), float(F))
    got = {tuple(p) for p in points[:int(n.item())].cpu().numpy().tolist()}
    strict = near = 0
    for b, (page, row) in enumerate(zip(pages(), part['crop_rows'].numpy())):
        for q in crop_quads(page.quads, row) / F:
            cy, cx = np.floor(q.mean(axis=0)).astype(np.int64).tolist()
            if not (box.up <= cy <= box.down and box.left <= cx <= box.right):
                continue
            if centroid_pixel_is_nearest(q):
                assert (b, cy - box.up, cx - box.left) in got, (b, cy, cx)
                strict += 1
            else:
                assert any((b, cy - box.up + i, cx - box.left + j) in got for i in (-1, 0, 1) for j in (-1, 0, 1)), (b, cy, cx)
                near += 1
    assert strict >= 8 and strict > 2 * near
