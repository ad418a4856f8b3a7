#!/usr/bin/env python3
"""The precise loss's default-off terms (mask focal, prob smooth-L1, weight-adaptive heatmap regression) and the WAHR
primitive, generated from the *imported reference* on the CPU like make_golden.py (same rules: run in the build container
only, the same in-memory stand-ins for ``torchvision.ops.sigmoid_focal_loss`` and ``vkit.element.Box``, inputs regenerated
from the portable seeds of recipe_precise_terms.py, no reference source stored anywhere):

    python tests/golden/make_golden_precise_terms.py

``losses_precise_terms.npz``, for each variant V in recipe_precise_terms.VARIANTS:
  * ``V/C/loss`` (fp64) and ``V/C/g_{prob,offset,angle,dist}`` (fp32) of ``AdaptiveScalingPreciseLossFunction`` under each
    config C of recipe_precise_terms.CONFIGS, plus ``V/C/g_mask_feat`` where the mask focal term is on;
  * ``V/wahr_gG/loss`` and ``V/wahr_gG/g_pred`` of ``WeightAdaptiveHeatmapRegressionLossFunction(gamma=G)``.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, '/root/reference')
sys.path.insert(0, ROOT)

from tests.golden import recipe_precise_terms as R  # noqa: E402
from tests.golden.make_golden import install_stand_ins, save  # noqa: E402


def main():
    Box = install_stand_ins()
    torch.set_default_dtype(torch.float64)
    from vkit_open_model.loss_function import (AdaptiveScalingPreciseLossFunction, AdaptiveScalingPreciseLossFunctionConifg,
                                               WeightAdaptiveHeatmapRegressionLossFunction)
    L = R.L
    arrs = {}
    for variant in R.VARIANTS:
        t = {k: torch.from_numpy(v) for k, v in R.loss_inputs(variant).items()}
        box = Box(*L['core_box'])
        for name, over in R.CONFIGS.items():
            preds = {k: t[k].clone().requires_grad_(True) for k in ('mask_feat', 'prob', 'offset', 'angle', 'dist')}
            loss = AdaptiveScalingPreciseLossFunction(AdaptiveScalingPreciseLossFunctionConifg(**over))(
                precise_char_mask_feature=preds['mask_feat'], precise_char_prob_feature=preds['prob'],
                precise_char_up_left_corner_offset_feature=preds['offset'],
                precise_char_corner_angle_feature=preds['angle'], precise_char_corner_distance_feature=preds['dist'],
                downsampled_char_prob_score_map=t['gt_score_precise'].clone(),
                downsampled_char_mask=t['gt_mask'].clone(), downsampled_shape=L['shape'], downsampled_core_box=box,
                downsampled_label_point_y=t['py'], downsampled_label_point_x=t['px'],
                char_up_left_offsets=t['gt_offsets'], char_corner_angles=t['gt_angles'],
                char_corner_distances=t['gt_dists'])
            loss.backward()
            arrs[f'{variant}/{name}/loss'] = loss.detach().numpy()
            for k, v in preds.items():
                if v.grad is not None:
                    arrs[f'{variant}/{name}/g_{k}'] = v.grad.numpy().astype(np.float32)
        pred, gt = (torch.from_numpy(a) for a in R.wahr_inputs(variant))
        for gamma in R.WAHR_GAMMAS:
            p = pred.clone().requires_grad_(True)
            loss = WeightAdaptiveHeatmapRegressionLossFunction(gamma=gamma)(pred=p, gt=gt.clone())
            loss.backward()
            arrs[f'{variant}/wahr_g{gamma}/loss'] = loss.detach().numpy()
            arrs[f'{variant}/wahr_g{gamma}/g_pred'] = p.grad.numpy().astype(np.float32)
    save('losses_precise_terms', **arrs)


if __name__ == '__main__':
    main()
