"""The precise loss with and without its default-off terms on the GPU (vkas_precise_loss_fwd/bwd, ops.PreciseLoss) and the
WAHR primitive (VKAS_LOSS_WAHR): against the reference's golden, against the fp64 oracle of
tests/test_cpu_precise_loss_terms.py on a larger case and, through the C ABI, on one whose grid-stride loops take a second
trip, a HIP-graph replay of the default configuration and of every term on, and one TwoPassStep."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.golden import recipe_precise_terms as R
from tests.helpers import golden, rel_err
from tests.test_cpu_precise_loss_terms import Knobs, oracle_on_inputs, precise_loss_oracle, wahr

pytestmark = pytest.mark.gpu

PREDS = ('mask_feat', 'prob', 'offset', 'angle', 'dist')


def _loss_fn(over, **kw):
    from vkit_ocr_model_adaptive_scaling_amd.loss_function import (AdaptiveScalingPreciseLossFunction,
                                                                   AdaptiveScalingPreciseLossFunctionConifg)
    return AdaptiveScalingPreciseLossFunction(AdaptiveScalingPreciseLossFunctionConifg(**over), **kw)


def _call(fn, t, box, shape, preds, scale=1.0):
    return fn(preds['mask_feat'], preds['prob'], preds['offset'], preds['angle'], preds['dist'], t['gt_score_precise'],
              t['gt_mask'], shape, box, t['py'], t['px'], t['gt_offsets'], t['gt_angles'], t['gt_dists'], scale=scale)


def _on_gpu(t):
    return {k: (torch.from_numpy(v).float().cuda() if v.dtype == np.float64 else torch.from_numpy(v).cuda())
            for k, v in t.items()}


@pytest.mark.parametrize('variant', R.VARIANTS)
@pytest.mark.parametrize('config', list(R.CONFIGS))
def test_precise_terms_vs_reference_golden(variant, config):
    from vkit_ocr_model_adaptive_scaling_amd.loss_function import Box
    g = golden('losses_precise_terms')
    c = _on_gpu(R.loss_inputs(variant))
    preds = {k: c[k].requires_grad_(True) for k in PREDS}
    loss = _call(_loss_fn(R.CONFIGS[config]), c, Box(*R.L['core_box']), R.L['shape'], preds)
    loss.backward()
    ref = float(g[f'{variant}/{config}/loss'])
    assert abs(float(loss) - ref) < 2e-5 * abs(ref)
    for k, v in preds.items():
        key = f'{variant}/{config}/g_{k}'
        if key in g.files:
            assert rel_err(v.grad, g[key]) < 1e-4, k
        else:
            assert k == 'mask_feat' and v.grad is None  # the focal term is off: the mask feature is not read


@pytest.mark.parametrize('variant', R.VARIANTS)
@pytest.mark.parametrize('gamma', R.WAHR_GAMMAS)
def test_wahr_primitive_vs_reference_golden(variant, gamma):
    from vkit_ocr_model_adaptive_scaling_amd.loss_function import WeightAdaptiveHeatmapRegressionLossFunction
    g = golden('losses_precise_terms')
    pred, gt = (torch.from_numpy(a).float().cuda() for a in R.wahr_inputs(variant))
    pred.requires_grad_(True)
    loss = WeightAdaptiveHeatmapRegressionLossFunction(gamma=gamma)(pred, gt)
    loss.backward()
    ref = float(g[f'{variant}/wahr_g{gamma}/loss'])
    assert abs(float(loss) - ref) < 2e-5 * abs(ref)
    assert rel_err(pred.grad, g[f'{variant}/wahr_g{gamma}/g_pred']) < 1e-4


def _large_case(seed=7, B=4, H=256, W=256, box=(30, 229, 41, 220), P=200):
    """B=4, 256x256 maps, a 200x180 crop, 200 label points; score map with exact 0 and 1 values (numpy, fp64)."""
    g = torch.Generator().manual_seed(seed)
    up, down, left, right = box
    CH, CW = down - up + 1, right - left + 1
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    gs = torch.rand(B, CH, CW, generator=g, dtype=torch.float64)
    gs.view(-1)[::5] = 0.0
    gs.view(-1)[::13] = 1.0
    t = dict(mask_feat=3.0 * rn(B, 1, H, W), prob=2.0 * rn(B, 1, H, W), offset=6.0 * rn(B, 2, H, W),
             angle=2.0 * rn(B, 4, H, W), dist=(3.0 * rn(B, 4, H, W)).abs() + 0.01, gt_score_precise=gs,
             gt_mask=(torch.rand(B, CH, CW, generator=g) > 0.5).double(),
             py=torch.randint(0, H, (B, P), generator=g), px=torch.randint(0, W, (B, P), generator=g),
             gt_offsets=torch.randint(-20, 21, (B, P, 2), generator=g).double(),
             gt_angles=torch.softmax(rn(B, P, 4), -1), gt_dists=torch.rand(B, P, 3, generator=g, dtype=torch.float64))
    t = {k: v.numpy() for k, v in t.items()}
    return t, box, (H, W)


def test_precise_terms_vs_oracle_large():
    from vkit_ocr_model_adaptive_scaling_amd.loss_function import Box
    t, box, shape = _large_case()
    over = ALL_ON
    kw = dict(prob_smooth_beta=0.3, focal_alpha=0.4, focal_gamma=1.5, wahr_gamma=0.05)
    scale = 0.25
    k = Knobs(**over, prob_smooth_beta=0.3, focal_alpha=0.4, focal_gamma=1.5, wahr_gamma=0.05)
    to = lambda a: torch.from_numpy(a).double()
    ref_in = {n: to(t[n]).requires_grad_(True) for n in PREDS}
    ref = precise_loss_oracle(k, *(ref_in[n] for n in PREDS), to(t['gt_score_precise']), to(t['gt_mask']), box,
                              torch.from_numpy(t['py']), torch.from_numpy(t['px']), to(t['gt_offsets']),
                              to(t['gt_angles']), to(t['gt_dists']), scale=scale)
    ref.backward()
    c = _on_gpu(t)
    preds = {n: c[n].requires_grad_(True) for n in PREDS}
    loss = _call(_loss_fn(over, **kw), c, Box(*box), shape, preds, scale=scale)
    loss.backward()
    assert abs(float(loss) - float(ref)) < 2e-5 * abs(float(ref))
    for n in PREDS:
        assert rel_err(preds[n].grad, ref_in[n].grad) < 1e-4, n
    up, down, left, right = box
    outside = torch.ones(shape, dtype=torch.bool)
    outside[up:down + 1, left:right + 1] = False
    dm = preds['mask_feat'].grad[:, 0].cpu()
    assert bool((dm[:, outside] == 0).all()) and bool((dm[:, ~outside] != 0).any())


def _ops_args(t, box, shape, over, scale=1.0):
    from vkit_ocr_model_adaptive_scaling_amd._lib import PreciseLossCfg, PreciseLossExtraCfg
    k = Knobs(**over)
    cfg = PreciseLossCfg(k.char_prob_pos_l2_factor, k.char_prob_neg_l2_factor, k.char_up_left_offset_l1_factor,
                         k.char_up_left_distance_regulation_l1_factor, k.char_corner_angle_cross_entropy_factor,
                         k.char_corner_distance_l1_factor, k.loss_factor, 2.5, scale)
    ex = PreciseLossExtraCfg(k.char_mask_focal_factor, k.char_prob_l1_factor, k.char_prob_wahr_factor, k.prob_smooth_beta,
                             k.wahr_gamma, k.focal_alpha, k.focal_gamma)
    return cfg, ex


ALL_ON = dict(char_mask_focal_factor=1.5, char_prob_l1_factor=0.7, char_prob_wahr_factor=3.0)


def _abi_case(B=3, H=423, W=419, box=(2, 421, 1, 417), P=37):
    """B*H*W = 531,711 and B*CH*CW = 525,420 both exceed the 2048 * 256 threads a launch is capped at, so the grid-stride
    loops of the dense forward and backward take a second trip; H*W is no multiple of 256; the crop leaves a margin on
    all four sides.  The label points include both corners of the map, pixels outside the crop and one duplicate."""
    t, _, _ = _large_case(seed=11, B=B, H=H, W=W, box=box, P=P)
    up, down, left, right = box
    fixed = [(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0), (1, 200), (422, 7), (100, 0), (300, 418), (57, 91), (57, 91)]
    for b in range(B):
        for i, (y, x) in enumerate(fixed):
            t['py'][b, i], t['px'][b, i] = y, x
    inside = (t['py'] >= up) & (t['py'] <= down) & (t['px'] >= left) & (t['px'] <= right)
    assert (~inside).sum() >= 8 * B and inside.any()
    return t, box, (H, W)


@pytest.fixture(scope='module')
def abi_case():
    return _abi_case()


@pytest.mark.parametrize('terms', ['off', 'on'])
def test_c_abi_vs_oracle_second_grid_trip(abi_case, terms):
    """vkas_precise_loss_fwd/bwd called directly, every output and the sums workspace prefilled with NaN, against the fp64
    oracle; the zero pattern of the gradients is held exactly."""
    from vkit_ocr_model_adaptive_scaling_amd import _lib as L
    t, box, (H, W) = abi_case
    up, down, left, right = box
    on = terms == 'on'
    over = ALL_ON if on else {}
    scale, dl = 0.5, 0.75
    cfg, ex = _ops_args(t, box, (H, W), over, scale=scale)
    to = lambda a: torch.from_numpy(a).double()
    ref_in = {n: to(t[n]).requires_grad_(True) for n in PREDS}
    ref = precise_loss_oracle(Knobs(**over), *(ref_in[n] for n in PREDS), to(t['gt_score_precise']), to(t['gt_mask']), box,
                              torch.from_numpy(t['py']), torch.from_numpy(t['px']), to(t['gt_offsets']),
                              to(t['gt_angles']), to(t['gt_dists']), scale=scale)
    ref.backward(torch.tensor(dl, dtype=torch.float64))
    c = _on_gpu(t)
    B, P = c['py'].shape
    CH, CW = down - up + 1, right - left + 1
    assert B * H * W > 2048 * 256 and B * CH * CW > 2048 * 256 and (H * W) % 256
    nan = lambda *shape, dtype=torch.float32: torch.full(shape, float('nan'), dtype=dtype, device='cuda')
    sums, loss = nan(L.PRECISE_LOSS_SUMS, dtype=torch.float64), nan(1)
    grads = {n: nan(*c[n].shape) for n in PREDS if on or n != 'mask_feat'}
    dloss = torch.full((1,), dl, device='cuda')
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    common = (p(c['prob']), p(c['offset']), p(c['angle']), p(c['dist']), p(c['gt_score_precise']), p(c['gt_mask']),
              p(c['py']), p(c['px']), p(c['gt_offsets']), p(c['gt_angles']), p(c['gt_dists']), B, H, W, up, left, CH, CW, P,
              ctypes.byref(cfg), p(c['mask_feat']) if on else None, ctypes.byref(ex), p(sums))
    L.check(L.lib.vkas_precise_loss_fwd(*common, p(loss), st), 'precise_loss_fwd')
    L.check(L.lib.vkas_precise_loss_bwd(*common, p(dloss), p(grads['prob']), p(grads['offset']), p(grads['angle']),
                                        p(grads['dist']), p(grads.get('mask_feat')), st), 'precise_loss_bwd')
    torch.cuda.synchronize()
    print(f'loss {float(loss):.9g} oracle {float(ref):.9g} rel {abs(float(loss) - float(ref)) / abs(float(ref)):.3g}')
    for n, g in grads.items():
        print(f'{n}: rel_err {rel_err(g, ref_in[n].grad):.3g}')
    assert not bool(torch.isnan(sums).any()) and not bool(torch.isnan(loss).any())
    assert abs(float(loss) - float(ref)) < 2e-5 * abs(float(ref))
    outside = torch.ones((H, W), dtype=torch.bool)
    outside[up:down + 1, left:right + 1] = False
    at_point = torch.zeros((B, H, W), dtype=torch.bool)
    at_point[torch.arange(B)[:, None], torch.from_numpy(t['py']), torch.from_numpy(t['px'])] = True
    for n, g in grads.items():
        g = g.cpu()
        assert not bool(torch.isnan(g).any()), n
        assert rel_err(g, ref_in[n].grad) < 1e-4, n
        if n in ('prob', 'mask_feat'):
            assert bool((g[:, 0][:, outside] == 0).all()), n
        else:
            assert bool((g.permute(0, 2, 3, 1)[~at_point] == 0).all()), n


def _graph_worker(rank, out_dir, terms):
    """Child process of test_precise_terms_graph_replay: capture, replay, compare; raises on a mismatch."""
    from vkit_ocr_model_adaptive_scaling_amd import ops
    torch.cuda.set_device(0)
    t, box, shape = _large_case(seed=9, B=2)
    c = _on_gpu(t)
    # 'default': the three extra factors 0, no mask feature, gradients for the four maps only
    names = PREDS if terms == 'on' else PREDS[1:]
    cfg, ex = _ops_args(t, box, shape, ALL_ON if terms == 'on' else {})
    ins = [c[n].clone().requires_grad_(True) for n in names]
    maps = ins[-4:]

    def run():
        loss = ops.PreciseLoss.apply(maps[0], ins[0] if terms == 'on' else None, maps[1], maps[2], maps[3],
                                     c['gt_score_precise'], c['gt_mask'], c['py'], c['px'], c['gt_offsets'],
                                     c['gt_angles'], c['gt_dists'], box[0], box[2], cfg, ex)
        return (loss,) + torch.autograd.grad(loss, ins)

    def compare(static, eager, what):
        assert abs(float(static[0]) - float(eager[0])) <= 1e-6 * abs(float(eager[0])), what
        for n, s_, e_ in zip(names, static[1:], eager[1:]):
            assert rel_err(s_, e_) < 1e-6, (what, n)

    eager = [x.detach().clone() for x in run()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    ops.check_deferred(wait=True)
    pending = len(ops._DEFERRED)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = run()
    assert len(ops._DEFERRED) == pending  # nothing host-side was recorded inside the capture
    graph.replay()
    torch.cuda.synchronize()
    compare(static, eager, 'replay')
    # new values in the captured inputs: the replay follows them
    with torch.no_grad():
        for x in ins:
            x.mul_(0.75).add_(0.1)
    graph.replay()
    torch.cuda.synchronize()
    compare(static, [x.detach().clone() for x in run()], 'replay after an input update')
    ops.check_deferred(wait=True)
    open(os.path.join(out_dir, 'graph_ok'), 'w').write('ok')


@pytest.mark.parametrize('terms', ['on', 'default'])
def test_precise_terms_graph_replay(tmp_path, terms):
    """Forward + backward of the precise loss, with every term on and in the default configuration, captured in one HIP
    graph (torch.cuda.graph, the backward through torch.autograd.grad) and replayed, equals the eager run: nothing on the
    path waits for the host or allocates host-side state.  Runs in a child process so that a failed capture fails this
    test only."""
    import torch.multiprocessing as mp
    mp.spawn(_graph_worker, args=(str(tmp_path), terms), nprocs=1, join=True)
    assert (tmp_path / 'graph_ok').read_text() == 'ok'


@pytest.mark.parametrize('n', [1, 255, 100_003])
def test_wahr_primitive_vs_oracle(n):
    from vkit_ocr_model_adaptive_scaling_amd.loss_function import WeightAdaptiveHeatmapRegressionLossFunction
    g = torch.Generator().manual_seed(n)
    pred = torch.rand(n, generator=g, dtype=torch.float64)
    gt = torch.rand(n, generator=g, dtype=torch.float64)
    gt[::3] = 0.0
    gt[1::7] = 1.0
    pred[2::11] = 1.0
    for gamma in (0.01, 0.3):
        p64 = pred.clone().requires_grad_(True)
        ref = wahr(p64, gt, gamma)
        ref.backward()
        p = pred.float().cuda().requires_grad_(True)
        loss = WeightAdaptiveHeatmapRegressionLossFunction(gamma)(p, gt.float().cuda())
        loss.backward()
        assert abs(float(loss) - float(ref)) < 2e-5 * abs(float(ref)) + 1e-12
        assert rel_err(p.grad, p64.grad) < 1e-4


def test_two_pass_step_with_prob_terms():
    """One TwoPassStep on a tiny model with the prob smooth-L1 and WAHR terms on: its precise loss equals the oracle on the
    maps forward_precise returns for the same image (TwoPassStep passes no mask feature, train.py:434,532)."""
    import bench
    from vkit_ocr_model_adaptive_scaling_amd.model import (AdaptiveScaling, AdaptiveScalingConfig, AdaptiveScalingSize,
                                                           AdaptiveScalingNeckHeadType)
    from vkit_ocr_model_adaptive_scaling_amd.loss_function import (AdaptiveScalingRoughLossFunction,
                                                                   AdaptiveScalingRoughLossFunctionConifg)
    from vkit_ocr_model_adaptive_scaling_amd.training import TwoPassStep
    dev = torch.device('cuda')
    torch.manual_seed(3)
    model = AdaptiveScaling(AdaptiveScalingConfig(AdaptiveScalingSize.TINY, AdaptiveScalingNeckHeadType.FPN)).to(dev).eval()
    rough, precise = bench.synthetic_batches(1, (128, 128), dev, 17)
    over = dict(char_prob_l1_factor=0.7, char_prob_wahr_factor=3.0)
    with torch.no_grad():
        maps = [m.detach().double().cpu() for m in model.forward_precise(precise['image'])]
    box = precise['downsampled_core_box']
    cpu = lambda k: precise[k].cpu()
    ref = precise_loss_oracle(Knobs(**over), None, *maps, cpu('downsampled_score_map').double(),
                              cpu('downsampled_mask').double(), (box.up, box.down, box.left, box.right),
                              cpu('downsampled_label_point_y'), cpu('downsampled_label_point_x'),
                              cpu('up_left_offsets').double(), cpu('corner_angles').double(),
                              cpu('corner_distances').double(), scale=0.5)

    class KeepGrads:  # TwoPassStep's optimizer slot: no parameter update
        def step(self, lr=None):
            pass

        def zero_grad(self):
            pass

    _, precise_loss = TwoPassStep(model, AdaptiveScalingRoughLossFunction(AdaptiveScalingRoughLossFunctionConifg()),
                                  _loss_fn(over), KeepGrads())(rough, precise)
    assert abs(float(precise_loss) - float(ref)) < 2e-5 * abs(float(ref))
    g = [p.grad for p in model.parameters() if p.grad is not None]
    assert g and all(bool(torch.isfinite(x).all()) for x in g)
