"""Blurred crops through the whole training path on the MI355X: the four pages of tests/test_gpu_crops_train.py ->
adaptive_scaling_pages_collate_fn with BlurConfig(prob=1.0) -> PageCropWarper -> CharLabelRasterizer -> batch_to_device ->
TwoPassStep on the tiny model, at the sizes used there.  The warped images equal the host route's bit for bit, the losses and
gradients are finite, and the label tensors are those of the same batch collated without blur: the blur changes no geometry."""
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_crops_train import F, MARGIN, P, SIZE, pages

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def release_device_memory():
    """the model, the batches and the work planes of this module go back to the driver: the tests after it allocate as they
    would without it"""
    yield
    import gc
    gc.collect()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def collated(blur: bool):
    from vkit_ocr_model_adaptive_scaling_amd.dataset import BlurConfig, CropConfig, adaptive_scaling_pages_collate_fn
    cfg = CropConfig(size=SIZE, core_margin=F * MARGIN, blur=BlurConfig(prob=1.0) if blur else None)
    return adaptive_scaling_pages_collate_fn([(p, p) for p in pages()], cfg, P=P, f=F, margin=MARGIN, rng_seed=17)


def test_blurred_pages_through_two_pass_step():
    from vkit_ocr_model_adaptive_scaling_amd.dataset import PageCropWarper, CharLabelRasterizer, crops_host
    from vkit_ocr_model_adaptive_scaling_amd.model import (AdaptiveScaling, AdaptiveScalingConfig, AdaptiveScalingSize,
                                                           AdaptiveScalingNeckHeadType)
    from vkit_ocr_model_adaptive_scaling_amd.loss_function import (
        AdaptiveScalingRoughLossFunction, AdaptiveScalingRoughLossFunctionConifg,
        AdaptiveScalingPreciseLossFunction, AdaptiveScalingPreciseLossFunctionConifg)
    from vkit_ocr_model_adaptive_scaling_amd.training import TwoPassStep, batch_to_device
    dev = torch.device('cuda')
    got, plain = collated(True), collated(False)
    for part in ('rough', 'precise'):
        assert set(got[part]) == set(plain[part]) | {'crop_blur'}
        assert int(got[part]['crop_blur'][:, 0].min()) >= 1            # prob = 1: every crop is blurred
    warped, host = PageCropWarper(dev)(got), crops_host(got)
    sharp = PageCropWarper(dev)(plain)
    for part in ('rough', 'precise'):
        assert set(warped[part]) == set(host[part]) == set(sharp[part]) and 'crop_blur' not in warped[part]
        image = warped[part]['image']
        assert image.is_cuda and image.dtype == torch.float32 and tuple(image.shape) == (4, 3) + SIZE
        assert torch.equal(image.cpu().view(torch.int32), host[part]['image'].view(torch.int32)), part
        assert float(image.min()) >= 0.0 and float(image.max()) <= 255.0 and float(image.std()) > 10.0
        assert not torch.equal(image, sharp[part]['image'])
    batch, batch_sharp = CharLabelRasterizer(dev)(warped), CharLabelRasterizer(dev)(sharp)
    for part in ('rough', 'precise'):  # the labels never see the blur
        assert set(batch[part]) == set(batch_sharp[part])
        for k, v in batch_sharp[part].items():
            if torch.is_tensor(v) and k != 'image':
                assert torch.equal(batch[part][k], v), (part, k)
    rough, precise = batch_to_device(batch['rough'], dev), batch_to_device(batch['precise'], dev)

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
