"""Input recipes of the FPN 5x5-smoothing fixture (``fpn5x5.npz``, make_golden_fpn5x5.py): FpnHead at upsampling factors
3 and 4 on odd-sized neck maps, and a TINY FPN AdaptiveScaling with rough factor 4 / precise factor 3.  Portable seeds only."""
import numpy as np

from tests.golden import recipe

# (upsampling factor, out_channels, in_channels, batch, neck (H, W))
HEAD5_CASES = ((3, 1, 64, 2, (13, 18)), (3, 2, 100, 1, (9, 14)), (3, 4, 64, 3, (7, 10)),
               (4, 1, 100, 2, (13, 18)), (4, 2, 64, 3, (9, 14)), (4, 4, 100, 1, (11, 7)))
HEAD5 = dict(seed=71, std=0.08, in_std=1.0)
MODEL5 = dict(seed=81, std=0.05, image=(1, 3, 96, 96), rough_factor=4, precise_factor=3)


def head5_tag(case) -> str:
    f, oc, c, b, (h, w) = case
    return f'head_f{f}_oc{oc}_c{c}_b{b}_{h}x{w}'


def head5_seed(case) -> int:
    f, oc, c, b, (h, w) = case
    return HEAD5['seed'] + 100 * f + 10 * oc + c


def head5_input(case) -> np.ndarray:
    f, oc, c, b, hw = case
    return HEAD5['in_std'] * recipe.plain_tensor(head5_seed(case), (b, c, *hw), 'head5_in')


def model5_images():
    seed = MODEL5['seed']
    return recipe.image(seed, MODEL5['image']).astype(np.float32), recipe.image(seed + 1, MODEL5['image']).astype(np.float32)
