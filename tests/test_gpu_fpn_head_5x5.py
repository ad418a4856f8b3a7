"""FPN heads at upsampling factors 3 and 4 on the MI355X: nearest x f followed by the 5x5 smoothing convolution
(fpn.py:41-48,170-174 of the reference), run as folded per-phase convolutions of the neck feature (ops.UpConv5,
csrc/upconv5.hip) without materialising the upsample.

Checked against (a) the reference fixture tests/golden/fpn5x5.npz (make_golden_fpn5x5.py) to the suite's bounds, (b) the
materialised composite (ops.Resize nearest + ops.Conv 5x5) and (c) a CPU fp64 F.interpolate + F.conv2d restatement, per
phase and on every phase's border rows / columns; plus point-sparse dy, the state-dict round trip, torch.jit.script, a
TwoPassStep at factor 4 and the peak memory of a head's forward + backward."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.golden import recipe, recipe_fpn5x5 as R
from tests.helpers import golden, rel_err, check_grad_summary
from tests.test_gpu_model import FWD_TOL, GRAD_TOL, seed_module, cot, named_params
from vkit_ocr_model_adaptive_scaling_amd.utils import portable_rng as prng

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ['f32', 'bf16', 'f16']
MFMA = [torch.bfloat16, torch.float16]


@pytest.fixture(scope='module')
def g5():
    return golden('fpn5x5')


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('case', R.HEAD5_CASES, ids=[R.head5_tag(c) for c in R.HEAD5_CASES])
def test_head5_reference(g5, case, dtype):
    from vkit_ocr_model_adaptive_scaling_amd.model import FpnHead, set_compute_dtype
    f, oc, c, b, hw = case
    tag = R.head5_tag(case)
    m = set_compute_dtype(seed_module(FpnHead(c, oc, f), R.head5_seed(case), R.HEAD5['std']).cuda().eval(), dtype)
    x = torch.from_numpy(R.head5_input(case)).float().cuda().requires_grad_(True)
    out = m(x)
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(g5[tag + '/out'].shape)
    assert rel_err(out, g5[tag + '/out']) < FWD_TOL[dtype]
    (out * cot(R.head5_seed(case) + 1, 0, out.shape)).sum().backward()
    assert rel_err(x.grad, g5[tag + '/gx']) < GRAD_TOL[dtype]
    check_grad_summary(named_params(m), g5, tol=GRAD_TOL[dtype], prefix=tag + '/')


def _model5(dtype):
    from vkit_ocr_model_adaptive_scaling_amd.model import AdaptiveScaling, AdaptiveScalingConfig, AdaptiveScalingSize
    Mo = R.MODEL5
    model = AdaptiveScaling(AdaptiveScalingConfig(AdaptiveScalingSize.TINY, rough_upsampling_factor=Mo['rough_factor'],
                                                  precise_upsampling_factor=Mo['precise_factor']), compute_dtype=dtype)
    return seed_module(model, Mo['seed'], Mo['std']).cuda().eval()


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_model5_reference(g5, dtype):
    """TINY FPN AdaptiveScaling with rough factor 4 / precise factor 3: outputs and the flat gradient of each pass."""
    Mo = R.MODEL5
    model = _model5(dtype)
    imgs = R.model5_images()
    for which, img, seed in (('rough', imgs[0], Mo['seed'] + 2), ('precise', imgs[1], Mo['seed'] + 3)):
        model.zero_grad(set_to_none=True)
        x = torch.from_numpy(img).cuda()
        outs = model.forward_rough(x) if which == 'rough' else model.forward_precise(x)
        for i, o in enumerate(outs):
            assert rel_err(o, g5[f'model/{which}/out{i}']) < FWD_TOL[dtype], (which, i)
        sum((o * cot(seed, i, o.shape)).sum() for i, o in enumerate(outs)).backward()
        gr = torch.cat([p.grad.double().reshape(-1) for _, p in model.named_parameters() if p.grad is not None]).cpu()
        ref_norm = float(g5[f'model/{which}/flat_norm'])
        assert abs(float(gr.norm()) - ref_norm) < (1e-3 if dtype == torch.float32 else 1e-2) * ref_norm, which
        samp = gr[recipe.sample_indices(gr.numel(), 256)].numpy()
        assert np.linalg.norm(samp - g5[f'model/{which}/flat_samp']) < GRAD_TOL[dtype] * np.linalg.norm(
            g5[f'model/{which}/flat_samp']), which


def _case_tensors(B, H, W, C, N, seed, dtype):
    x = torch.from_numpy(prng.normal_like(seed, 1, B * H * W * C).reshape(B, H, W, C)).float()
    w = 0.2 * torch.from_numpy(prng.normal_like(seed, 2, N * C * 25).reshape(N, C, 5, 5)).float()
    b = torch.from_numpy(prng.normal_like(seed, 3, N)).float()
    return x.to(dtype).float(), w, b  # x holds values the storage type represents exactly


def _fp64_ref(x, w, b, f, dy):
    """F.interpolate (nearest) + F.conv2d (pad 2) in fp64 on the CPU; x (B, H, W, C), dy (B, fH, fW, N)."""
    xd = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
    y = F.conv2d(F.interpolate(xd, scale_factor=f, mode='nearest'), wd, bd, padding=2)
    y.backward(dy.double().permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1), xd.grad.permute(0, 2, 3, 1), wd.grad, bd.grad


def _run(op, x, w, b, dy, dtype):
    from vkit_ocr_model_adaptive_scaling_amd import ops
    C, N = x.shape[3], w.shape[0]
    Cp, Np = ops.rup8(C), ops.rup8(N)
    xa = F.pad(x, (0, Cp - C)).to(dtype).cuda().requires_grad_(True)
    wg, bg = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = op(xa, wg, bg)
    y.backward(F.pad(dy, (0, Np - N)).to(dtype).cuda())
    return y[..., :N].float().cpu(), xa.grad[..., :C].float().cpu(), wg.grad.cpu(), bg.grad.cpu()


def _phase_checks(y, ref, f, tol, what):
    """every output phase on its own, and the border rows / columns of every phase (the zero-padding taps)"""
    for r in range(f):
        for s in range(f):
            ph, rp = y[:, r::f, s::f], ref[:, r::f, s::f]
            assert rel_err(ph, rp) < tol, (what, r, s)
            for sl in ((slice(None), 0), (slice(None), -1), (slice(None), slice(None), 0), (slice(None), slice(None), -1)):
                assert rel_err(ph[sl], rp[sl]) < tol, (what, r, s, sl)


# (B, H, W, C, N): 8-wide and odd widths; C = 100 / N = 200: K tiles that straddle folded taps, two N tiles per phase
SHAPES = ((2, 11, 13, 40, 20), (3, 7, 5, 100, 200), (1, 17, 9, 64, 130))


@pytest.mark.parametrize('dtype', MFMA, ids=['bf16', 'f16'])
@pytest.mark.parametrize('f', [3, 4])
@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_upconv5_folded_vs_composite_and_fp64(shape, f, dtype):
    from vkit_ocr_model_adaptive_scaling_amd import ops
    B, H, W, C, N = shape
    x, w, b = _case_tensors(B, H, W, C, N, 500 + f + C, dtype)
    dy = torch.from_numpy(prng.normal_like(600 + f, 4, B * f * H * f * W * N).reshape(B, f * H, f * W, N)).float().to(dtype).float()
    folded = _run(lambda xa, wg, bg: ops.UpConv5.apply(xa, wg, bg, f), x, w, b, dy, dtype)
    composite = _run(lambda xa, wg, bg: ops.Conv.apply(ops.Resize.apply(xa, (f * H, f * W), 1), wg, bg, 1, 2), x, w, b, dy,
                     dtype)
    ref = _fp64_ref(x, w, b, f, dy)
    tol = 1e-2 if dtype == torch.bfloat16 else 2e-3
    for name, a, c, r in zip(('y', 'dx', 'dW', 'db'), folded, composite, ref):
        assert rel_err(a, r) < tol, (name, rel_err(a, r))
        assert rel_err(c, r) < tol, (name, 'composite', rel_err(c, r))
        assert rel_err(a, c) < 2 * tol, (name, rel_err(a, c))
    _phase_checks(folded[0], ref[0], f, tol, 'y')
    # the low-res border (the rows / columns the folded taps reach through the zero padding)
    for sl in ((slice(None), 0), (slice(None), -1), (slice(None), slice(None), 0), (slice(None), slice(None), -1)):
        assert rel_err(folded[1][sl], ref[1][sl]) < tol, ('dx', sl)


@pytest.mark.parametrize('f', [3, 4])
def test_upconv5_point_sparse_dy(f):
    """dy zero everywhere but at a few label points (what PreciseLoss hands back to the precise heads)."""
    from vkit_ocr_model_adaptive_scaling_amd import ops
    B, H, W, C, N = 2, 9, 12, 64, 24
    x, w, b = _case_tensors(B, H, W, C, N, 700 + f, torch.bfloat16)
    dy = torch.zeros(B, f * H, f * W, N)
    g = torch.Generator().manual_seed(f)
    py, px = torch.randint(0, f * H, (B, 7), generator=g), torch.randint(0, f * W, (B, 7), generator=g)
    py[:, 0], px[:, 0] = 0, f * W - 1  # corners: the zero-padding taps
    for i in range(B):
        dy[i, py[i], px[i]] = torch.randn(7, N, generator=g).to(torch.bfloat16).float()
    _, dx, dw, db = _run(lambda xa, wg, bg: ops.UpConv5.apply(xa, wg, bg, f), x, w, b, dy, torch.bfloat16)
    _, rdx, rdw, rdb = _fp64_ref(x, w, b, f, dy)
    assert rel_err(dx, rdx) < 1e-2 and rel_err(dw, rdw) < 1e-2 and rel_err(db, rdb) < 1e-5


def test_upconv5_dgrad_is_deterministic():
    from vkit_ocr_model_adaptive_scaling_amd import ops
    x, w, b = _case_tensors(2, 13, 11, 96, 48, 900, torch.bfloat16)
    dy = torch.from_numpy(prng.normal_like(901, 4, 2 * 52 * 44 * 48).reshape(2, 52, 44, 48)).float()
    r1 = _run(lambda xa, wg, bg: ops.UpConv5.apply(xa, wg, bg, 4), x, w, b, dy, torch.bfloat16)
    r2 = _run(lambda xa, wg, bg: ops.UpConv5.apply(xa, wg, bg, 4), x, w, b, dy, torch.bfloat16)
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])


@pytest.mark.parametrize('factor', [3, 4])
def test_head5_state_dict_round_trip(g5, factor):
    """reference names and shapes (the fixture's gradient summaries are keyed by them); load -> state_dict is the identity
    and a second head loaded from it computes the same maps"""
    from vkit_ocr_model_adaptive_scaling_amd.model import FpnHead, set_compute_dtype
    case = next(c for c in R.HEAD5_CASES if c[0] == factor)
    f, oc, c, b, hw = case
    names = sorted(k[len(R.head5_tag(case)) + 7:] for k in g5.files if k.startswith(R.head5_tag(case) + '/gnorm/'))
    h1 = seed_module(FpnHead(c, oc, f), R.head5_seed(case), R.HEAD5['std'])
    assert sorted(h1.state_dict()) == names
    sd = {k: v.clone() for k, v in h1.state_dict().items()}
    h2 = FpnHead(c, oc, f)
    h2.load_state_dict(sd)
    assert all(torch.equal(sd[k], v) for k, v in h2.state_dict().items())
    x = torch.from_numpy(R.head5_input(case)).float().cuda()
    y1 = set_compute_dtype(h1.cuda().eval(), torch.bfloat16)(x)
    y2 = set_compute_dtype(h2.cuda().eval(), torch.bfloat16)(x)
    assert torch.equal(y1, y2)


def test_model5_script(g5):
    model = _model5(torch.bfloat16)
    scripted = torch.jit.script(model)
    x = torch.from_numpy(R.model5_images()[0]).cuda()
    with torch.no_grad():
        eager = model.forward_rough(x)
        got = scripted.forward_rough(x)
        assert all(torch.equal(a, b) for a, b in zip(eager, got))
        prec = scripted.forward_precise(torch.from_numpy(R.model5_images()[1]).cuda())
    assert [tuple(p.shape) for p in prec] == [tuple(g5[f'model/precise/out{i}'].shape) for i in range(4)]
    assert rel_err(prec[0], g5['model/precise/out0']) < FWD_TOL[torch.bfloat16]


def test_two_pass_step_factor4():
    import bench
    from vkit_ocr_model_adaptive_scaling_amd.model import AdaptiveScaling, AdaptiveScalingConfig, AdaptiveScalingSize
    from vkit_ocr_model_adaptive_scaling_amd.loss_function import (
        AdaptiveScalingRoughLossFunction, AdaptiveScalingRoughLossFunctionConifg,
        AdaptiveScalingPreciseLossFunction, AdaptiveScalingPreciseLossFunctionConifg)
    from vkit_ocr_model_adaptive_scaling_amd.training import FlatBuffers, FlatAdamW, TwoPassStep
    dev = torch.device('cuda', 0)
    torch.manual_seed(3)
    model = AdaptiveScaling(AdaptiveScalingConfig(AdaptiveScalingSize.TINY, rough_upsampling_factor=4,
                                                  precise_upsampling_factor=4)).to(dev).eval()
    # maps at factor 4 have the image's size: take the targets of a twice larger image (bench's maps are at half size)
    rough, precise = bench.synthetic_batches(2, (256, 256), dev, 11)
    for bt in (rough, precise):
        bt['image'] = bt['image'][:, :, ::2, ::2].contiguous()
    flat = FlatBuffers(model.named_parameters())
    opt = FlatAdamW(None, lr=1e-4, flat=flat)
    before = [p.detach().clone() for p in model.parameters()]
    rl, pl = TwoPassStep(model, AdaptiveScalingRoughLossFunction(AdaptiveScalingRoughLossFunctionConifg()),
                         AdaptiveScalingPreciseLossFunction(AdaptiveScalingPreciseLossFunctionConifg()), opt)(rough, precise)
    assert torch.isfinite(rl) and torch.isfinite(pl) and float(rl) > 0 and float(pl) > 0
    head_w = model.rough_char_mask_head.step1_conv[0].weight
    assert head_w.shape[2:] == (5, 5)
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    assert all(torch.isfinite(p).all() for p in model.parameters())


@pytest.mark.parametrize('f', [3, 4])
def test_head5_peak_memory_below_upsample(f):
    """forward + backward of a head allocate less than the f^2-upsampled neck feature alone would take"""
    from vkit_ocr_model_adaptive_scaling_amd.model import FpnHead, set_compute_dtype
    from vkit_ocr_model_adaptive_scaling_amd.model import helper
    # large enough a map that the pixel-sized tensors (z: half the upsample's channels; dx) outweigh the weight-sized ones
    # (the folded images and the per-phase weight gradient)
    B, C, H, W = 2, 256, 160, 160
    head = set_compute_dtype(FpnHead(C, 1, f).cuda(), torch.bfloat16)
    x = torch.randn(B, C, H, W, device='cuda')
    act = helper.nchw_to_act(x, torch.bfloat16).requires_grad_(True)
    conv, norm = head.step1_conv[0], head.step1_conv[2]
    from vkit_ocr_model_adaptive_scaling_amd import ops
    dz = torch.randn(B, f * H, f * W, ops.rup8(conv.out_channels), device='cuda', dtype=torch.bfloat16)
    up_bytes = B * (f * H) * (f * W) * C * 2
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    z = ops.upconv5(act, conv.weight, conv.bias, f)
    z.backward(dz)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert act.grad is not None and conv.weight.grad is not None
    assert peak < up_bytes, (peak, up_bytes)
