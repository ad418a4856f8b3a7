#!/usr/bin/env python3
"""FPN heads at upsampling factors 3 and 4 (the 5x5 smoothing block, fpn.py:41-48,170-174 of the reference), generated from
the *imported reference* on the CPU like make_golden.py / make_golden_r04.py (same rules: run in the build container only,
inputs regenerated from the portable seeds of recipe_fpn5x5.py, no reference source stored anywhere):

    python tests/golden/make_golden_fpn5x5.py

``fpn5x5.npz``:
  * ``FpnHead(in, oc, f)`` for every case of recipe_fpn5x5.HEAD5_CASES (f in {3, 4}, oc in {1, 2, 4}, in in {64, 100},
    odd neck sizes, a batch of 3): output, input gradient and the parameter-gradient summaries under the portable
    cotangent (make_golden.backprop), fp64.
  * a TINY FPN ``AdaptiveScaling`` with rough factor 4 and precise factor 3 on 96 x 96 images: the forward_rough /
    forward_precise outputs and the flat-gradient summary (norm, sum, strided samples) of <outputs, cotangents> for each
    pass, fp64.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, '/root/reference')
sys.path.insert(0, ROOT)

from tests.golden import recipe, recipe_fpn5x5 as R  # noqa: E402
from tests.golden.make_golden import install_stand_ins, load_params, grad_summary, backprop, save  # noqa: E402


def flat_summary(model, prefix):
    g = torch.cat([p.grad.detach().double().reshape(-1) for _, p in model.named_parameters() if p.grad is not None])
    return {prefix + 'flat_norm': np.array(float(g.norm())), prefix + 'flat_sum': np.array(float(g.sum())),
            prefix + 'flat_samp': g[recipe.sample_indices(g.numel(), 256)].numpy()}


def main():
    install_stand_ins()
    torch.set_num_threads(8)
    torch.set_default_dtype(torch.float64)
    from vkit_open_model.model import FpnHead, AdaptiveScaling, AdaptiveScalingConfig, AdaptiveScalingSize

    arrs = {}
    for case in R.HEAD5_CASES:
        f, oc, c, b, hw = case
        head = load_params(FpnHead(c, oc, f), R.head5_seed(case), R.HEAD5['std']).eval()
        assert head.step1_conv[0].kernel_size == (5, 5)
        x = torch.from_numpy(R.head5_input(case)).requires_grad_(True)
        y = head(x)
        assert y.shape == (b, oc, f * hw[0], f * hw[1])
        backprop([y], R.head5_seed(case) + 1)
        tag = R.head5_tag(case)
        arrs[tag + '/out'] = y.detach().numpy().astype(np.float32)
        arrs[tag + '/gx'] = x.grad.numpy().astype(np.float32)
        arrs.update({tag + '/' + k: v for k, v in grad_summary(head).items()})

    Mo = R.MODEL5
    model = AdaptiveScaling(AdaptiveScalingConfig(AdaptiveScalingSize.TINY, rough_upsampling_factor=Mo['rough_factor'],
                                                  precise_upsampling_factor=Mo['precise_factor']))
    load_params(model, Mo['seed'], Mo['std'])
    model.eval()
    img_r, img_p = (torch.from_numpy(a).double() for a in R.model5_images())
    for which, img, seed in (('rough', img_r, Mo['seed'] + 2), ('precise', img_p, Mo['seed'] + 3)):
        model.zero_grad(set_to_none=True)
        outs = model.forward_rough(img) if which == 'rough' else model.forward_precise(img)
        backprop(list(outs), seed)
        for i, o in enumerate(outs):
            arrs[f'model/{which}/out{i}'] = o.detach().numpy().astype(np.float32)
        arrs.update(flat_summary(model, f'model/{which}/'))
    save('fpn5x5', **arrs)


if __name__ == '__main__':
    main()
