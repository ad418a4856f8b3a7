"""The precise loss's default-off terms (loss_function/adaptive_scaling.py:154-158,272-307 of the reference: mask focal,
prob smooth-L1, weight-adaptive heatmap regression) and the WAHR primitive, on the host: the callables construct with the
reference's knobs, weighted BCE keeps raising, the argument checks that run before any kernel, and an fp64 torch
restatement of the terms (the oracle the GPU tests use) reproduces the reference's golden."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import torch_oracle as O
from tests.golden import recipe_precise_terms as R
from tests.helpers import golden, rel_err


@dataclasses.dataclass
class Knobs:
    """AdaptiveScalingPreciseLossFunctionConifg's factors plus the fixed parameters of the term objects (:154-165)."""
    char_mask_focal_factor: float = 0.0
    char_prob_l1_factor: float = 0.0
    char_prob_pos_l2_factor: float = 2.0
    char_prob_neg_l2_factor: float = 1.0
    char_prob_wahr_factor: float = 0.0
    char_up_left_offset_l1_factor: float = 1.0
    char_up_left_distance_regulation_l1_factor: float = 1.0
    char_corner_angle_cross_entropy_factor: float = 5.0
    char_corner_distance_l1_factor: float = 1.0
    loss_factor: float = 0.15
    prob_smooth_beta: float = 0.25
    focal_alpha: float = 0.25
    focal_gamma: float = 2.0
    wahr_gamma: float = 0.01


def wahr(p, gt, gamma=0.01):
    """weight_adaptive_heatmap_regression.py:29-32: mean of (s (1 - p) + (1 - s) p) (p - gt)^2, s = gt ** gamma."""
    s = gt ** gamma
    return ((s * (1 - p) + (1 - s) * p) * (p - gt) ** 2).mean()


def precise_loss_oracle(k: Knobs, mask_feat, prob, offset, angle, dist, gt_score, gt_mask, core_box, py, px, gt_offsets,
                        gt_angles, gt_dists, scale=1.0):
    """AdaptiveScalingPreciseLossFunction.__call__ with every term (fp64 when the inputs are): the default-active terms
    from oracle.torch_oracle.precise_loss, the three default-off terms restated here."""
    up, down, left, right = core_box
    loss = O.precise_loss(prob, offset, angle, dist, gt_score, gt_mask, core_box, py, px, gt_offsets, gt_angles, gt_dists,
                          k.char_prob_pos_l2_factor, k.char_prob_neg_l2_factor, k.char_up_left_offset_l1_factor,
                          k.char_up_left_distance_regulation_l1_factor, k.char_corner_angle_cross_entropy_factor,
                          k.char_corner_distance_l1_factor, loss_factor=1.0)
    p = torch.sigmoid(prob[:, 0, up:down + 1, left:right + 1])
    if k.char_mask_focal_factor > 0:  # :272-277
        x = mask_feat[:, 0, up:down + 1, left:right + 1]
        loss = loss + k.char_mask_focal_factor * O.sigmoid_focal_mean(x, gt_mask, k.focal_alpha, k.focal_gamma)
    if k.char_prob_l1_factor > 0:  # :284-289
        loss = loss + k.char_prob_l1_factor * O.smooth_l1(p, gt_score, k.prob_smooth_beta, gt_mask)
    if k.char_prob_wahr_factor > 0:  # :303-307
        loss = loss + k.char_prob_wahr_factor * wahr(p, gt_score, k.wahr_gamma)
    return loss * k.loss_factor * scale


def oracle_on_inputs(t, k: Knobs, to=lambda a: torch.from_numpy(a).double()):
    """(loss, {name: input tensor with .grad}) of the oracle on a recipe_precise_terms input dict."""
    preds = {n: to(t[n]).requires_grad_(True) for n in ('mask_feat', 'prob', 'offset', 'angle', 'dist')}
    loss = precise_loss_oracle(k, preds['mask_feat'], preds['prob'], preds['offset'], preds['angle'], preds['dist'],
                               to(t['gt_score_precise']), to(t['gt_mask']), R.L['core_box'], torch.from_numpy(t['py']),
                               torch.from_numpy(t['px']), to(t['gt_offsets']), to(t['gt_angles']), to(t['gt_dists']))
    loss.backward()
    return loss, preds


def test_precise_loss_constructs_with_each_default_off_term():
    from vkit_ocr_model_adaptive_scaling_amd.loss_function import (AdaptiveScalingPreciseLossFunction,
                                                                   AdaptiveScalingPreciseLossFunctionConifg)
    for over in ({'char_mask_focal_factor': 1.0}, {'char_prob_l1_factor': 1.0}, {'char_prob_wahr_factor': 1.0},
                 R.CONFIGS['all']):
        f = AdaptiveScalingPreciseLossFunction(AdaptiveScalingPreciseLossFunctionConifg(**over))
        assert (f.smooth_beta, f.prob_smooth_beta, f.focal_alpha, f.focal_gamma, f.wahr_gamma) == (2.5, 0.25, 0.25, 2.0, 0.01)
    f = AdaptiveScalingPreciseLossFunction(AdaptiveScalingPreciseLossFunctionConifg(char_prob_l1_factor=1.0),
                                           prob_smooth_beta=0.5, focal_alpha=-1.0, focal_gamma=1.5, wahr_gamma=0.1)
    assert (f.prob_smooth_beta, f.focal_alpha, f.focal_gamma, f.wahr_gamma) == (0.5, -1.0, 1.5, 0.1)


def test_wahr_primitive_constructs_and_bce_still_raises():
    from vkit_ocr_model_adaptive_scaling_amd import loss_function as L
    from vkit_ocr_model_adaptive_scaling_amd import _lib
    assert L.WeightAdaptiveHeatmapRegressionLossFunction().gamma == 0.01
    assert L.WeightAdaptiveHeatmapRegressionLossFunction(gamma=0.5).gamma == 0.5
    assert (_lib.LOSS_FOCAL, _lib.LOSS_DICE, _lib.LOSS_L1, _lib.LOSS_SMOOTH_L1, _lib.LOSS_L2, _lib.LOSS_WAHR) == tuple(range(6))
    with pytest.raises(RuntimeError, match='MI355X'):
        L.WeightAdaptiveHeatmapRegressionLossFunction()(torch.zeros(5), torch.zeros(5))  # no CPU fallback
    with pytest.raises(NotImplementedError):
        L.WeightedBceWithLogitsLossFunction()
    with pytest.raises(NotImplementedError):
        L.AdaptiveScalingRoughLossFunction(L.AdaptiveScalingRoughLossFunctionConifg(bce_factor=1.0))


def _cpu_call(over, mask_feat, B=2, H=12, W=14, P=3):
    from vkit_ocr_model_adaptive_scaling_amd.loss_function import (Box, AdaptiveScalingPreciseLossFunction,
                                                                   AdaptiveScalingPreciseLossFunctionConifg)
    z = torch.zeros
    f = AdaptiveScalingPreciseLossFunction(AdaptiveScalingPreciseLossFunctionConifg(**over))
    return f(mask_feat, z(B, 1, H, W), z(B, 2, H, W), z(B, 4, H, W), z(B, 4, H, W), z(B, 8, 9), z(B, 8, 9), (H, W),
             Box(2, 9, 3, 11), z(B, P, dtype=torch.long), z(B, P, dtype=torch.long), z(B, P, 2), z(B, P, 4), z(B, P, 3))


def test_mask_feature_host_checks():
    """The checks run on the host before any kernel (CPU tensors): a missing mask feature with the focal term on is the
    reference's assert (:273), a misshapen one a ValueError; with the term off a passed mask feature is ignored."""
    z = torch.zeros
    with pytest.raises(AssertionError):
        _cpu_call({'char_mask_focal_factor': 1.0}, None)
    for bad in (z(2, 1, 12, 13), z(2, 2, 12, 14), z(1, 1, 12, 14)):
        with pytest.raises(ValueError):
            _cpu_call({'char_mask_focal_factor': 1.0}, bad)
    # valid arguments get as far as the device requirement (no CPU fallback), with and without the extra terms
    for over, mf in (({'char_mask_focal_factor': 1.0}, z(2, 1, 12, 14)), ({'char_prob_l1_factor': 1.0}, None),
                     ({'char_prob_wahr_factor': 1.0}, z(3, 3)), ({}, z(3, 3))):
        with pytest.raises(RuntimeError, match='MI355X'):
            _cpu_call(over, mf)


@pytest.mark.parametrize('variant', R.VARIANTS)
@pytest.mark.parametrize('config', list(R.CONFIGS))
def test_oracle_reproduces_reference_golden(variant, config):
    g = golden('losses_precise_terms')
    loss, preds = oracle_on_inputs(R.loss_inputs(variant), Knobs(**R.CONFIGS[config]))
    ref = float(g[f'{variant}/{config}/loss'])
    assert abs(float(loss.detach()) - ref) <= 1e-12 * abs(ref)
    for n, v in preds.items():
        key = f'{variant}/{config}/g_{n}'
        if key in g.files:
            assert rel_err(v.grad, g[key]) < 1e-6, n
        else:
            assert n == 'mask_feat' and 'char_mask_focal_factor' not in R.CONFIGS[config] and v.grad is None


@pytest.mark.parametrize('variant', R.VARIANTS)
@pytest.mark.parametrize('gamma', R.WAHR_GAMMAS)
def test_wahr_oracle_reproduces_reference_golden(variant, gamma):
    g = golden('losses_precise_terms')
    pred, gt = (torch.from_numpy(a) for a in R.wahr_inputs(variant))
    assert bool((gt == 0).any()) and bool((gt == 1).any())
    pred.requires_grad_(True)
    loss = wahr(pred, gt, gamma)
    loss.backward()
    ref = float(g[f'{variant}/wahr_g{gamma}/loss'])
    assert abs(float(loss.detach()) - ref) <= 1e-12 * abs(ref)
    assert rel_err(pred.grad, g[f'{variant}/wahr_g{gamma}/g_pred']) < 1e-6


def test_c_abi_argument_checks_without_gpu():
    """The precise-loss entry points refuse inconsistent arguments before anything is launched (VKAS_E_ARG + message)."""
    import ctypes
    from vkit_ocr_model_adaptive_scaling_amd import _lib
    a = lambda: ctypes.c_void_p(256)  # any aligned non-null address: the checks run before anything is dereferenced
    cfg = _lib.PreciseLossCfg(2.0, 1.0, 1.0, 1.0, 5.0, 1.0, 0.15, 2.5, 1.0)
    dims = (2, 12, 14, 2, 3, 8, 9, 3)
    fwd, bwd = _lib.lib.vkas_precise_loss_fwd, _lib.lib.vkas_precise_loss_bwd
    ex = _lib.PreciseLossExtraCfg(1.0, 0.0, 0.0, 0.25, 0.01, 0.25, 2.0)
    assert fwd(*[a() for _ in range(11)], *dims, ctypes.byref(cfg), None, ctypes.byref(ex), a(), a(), None) == -1
    assert b'mask feature' in _lib.lib.vkas_last_error()
    assert bwd(*[a() for _ in range(11)], *dims, ctypes.byref(cfg), a(), ctypes.byref(ex), *[a() for _ in range(6)], None,
               None) == -1
    assert b'd_mask_feat' in _lib.lib.vkas_last_error()
    assert fwd(*[a() for _ in range(11)], *dims, ctypes.byref(cfg), a(), None, a(), a(), None) == -1  # no extra cfg
    bad_beta = _lib.PreciseLossExtraCfg(0.0, 1.0, 0.0, 0.0, 0.01, 0.25, 2.0)
    assert fwd(*[a() for _ in range(11)], *dims, ctypes.byref(cfg), None, ctypes.byref(bad_beta), a(), a(), None) == -1
    assert b'prob_l1_beta' in _lib.lib.vkas_last_error()
    crop_out = (2, 12, 14, 5, 3, 8, 9, 3)  # 5 + 8 > 12
    assert fwd(*[a() for _ in range(11)], *crop_out, ctypes.byref(cfg), a(), ctypes.byref(ex), a(), a(), None) == -1
    # the WAHR primitive takes no mask (weight_adaptive_heatmap_regression.py:23-28)
    assert _lib.lib.vkas_elementwise_loss_fwd(_lib.LOSS_WAHR, a(), a(), a(), 8, 0.01, 0.0, 0.0, a(), a(), None) == -1
    assert b'no mask' in _lib.lib.vkas_last_error()
    assert _lib.lib.vkas_elementwise_loss_bwd(_lib.LOSS_WAHR, a(), a(), a(), 8, 0.01, 0.0, 0.0, a(), a(), a(), None) == -1
