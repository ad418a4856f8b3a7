"""Input recipes of the default-off precise-loss terms fixture (``losses_precise_terms.npz``,
make_golden_precise_terms.py): the loss toy of recipe.LOSS_TOY with score-map values forced to exactly 0 and 1, and the
reference configs that switch on the mask focal, prob smooth-L1 and WAHR terms.  Portable seeds only."""
import numpy as np

from tests.golden import recipe

L = recipe.LOSS_TOY
VARIANTS = ('plain', 'edge')
# AdaptiveScalingPreciseLossFunctionConifg overrides (loss_function/adaptive_scaling.py:134-145 of the reference)
CONFIGS = {
    'focal': dict(char_mask_focal_factor=1.0),
    'l1': dict(char_prob_l1_factor=1.0),
    'wahr': dict(char_prob_wahr_factor=1.0),
    'all': dict(char_mask_focal_factor=1.5, char_prob_l1_factor=0.7, char_prob_wahr_factor=3.0,
                char_prob_pos_l2_factor=0.5, char_corner_angle_cross_entropy_factor=2.0, loss_factor=0.3),
}
WAHR_GAMMAS = (0.01, 0.5)  # WeightAdaptiveHeatmapRegressionLossFunction(gamma) on its own


def loss_inputs(variant: str) -> dict:
    """recipe.loss_inputs (``mask_feat`` doubles as the precise mask logits; ``edge`` keeps its all-zero mask image) with
    every 7th precise score-map value set to exactly 0 and every 11th to exactly 1 (0 ** gamma and 1 ** gamma in WAHR)."""
    t = recipe.loss_inputs(L, variant)
    gs = t['gt_score_precise'].reshape(-1).copy()
    idx = np.arange(gs.size)
    gs[idx % 7 == 0] = 0.0
    gs[idx % 11 == 0] = 1.0
    t['gt_score_precise'] = gs.reshape(t['gt_score_precise'].shape)
    return t


def wahr_inputs(variant: str):
    """(pred probabilities, gt) of the WAHR primitive: sigmoid of the cropped prob logits against the forced score map."""
    t = loss_inputs(variant)
    up, down, left, right = L['core_box']
    pred = 1.0 / (1.0 + np.exp(-t['prob'][:, 0, up:down + 1, left:right + 1]))
    return pred, t['gt_score_precise']
