"""ops.PpmBranchesCat (csrc/ppm.hip): the pooled branches of the pyramid-pooling block in three forward and four backward
launches, against the fp64 restatement of tests/ppm_reference.py and against the unfused route (VKAS_PPM_UNFUSED: the pooling,
1x1 block and resize ops the block used before), measured in the same test on the same stored inputs.

Parity condition: norm-wise, error(fused) <= 1.25 * error(unfused) + half an ulp of the storage type (2^-9 bf16, 2^-12 fp16).
The two routes round at the same points or the fused one at fewer, so the margin covers summation order only."""
import pytest
import torch

from tests import parity_log
from tests import ppm_reference as R

pytestmark = pytest.mark.gpu

HALF_ULP = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}
DTYPES = [torch.bfloat16, torch.float16]
# (H, W, C, Cb, scales) at B = 2: every map, width and scale set of the kernels' index paths - odd and non-square maps, H < s
# (5 x 4 under 6 and 5), one and several row groups per branch, partial last groups, 1 .. 12 channel vectors, the full 32 x 32
CASES = [
    (7, 9, 8, 8, (1, 2, 3, 6)),
    (7, 9, 72, 24, (2, 5)),
    (7, 9, 72, 96, (1,)),
    (5, 4, 8, 24, (1, 2, 3, 6)),
    (5, 4, 72, 8, (2, 5)),
    (5, 4, 72, 96, (1, 2, 3, 6)),
    (12, 16, 72, 96, (1, 2, 3, 6)),
    (12, 16, 8, 8, (1,)),
    (12, 16, 72, 24, (2, 5)),
    (32, 32, 72, 96, (1, 2, 3, 6)),
]
B = 2


def _ids(c):
    return '%dx%d-C%d-Cb%d-s%s' % (c[0], c[1], c[2], c[3], ''.join(str(s) for s in c[4]))


def _block(case, dtype, params64, dev):
    from vkit_ocr_model_adaptive_scaling_amd.model.upernext import PpmBlock
    from vkit_ocr_model_adaptive_scaling_amd.model import set_compute_dtype
    H, W, C, Cb, scales = case
    blk = PpmBlock(scales, C, Cb)
    with torch.no_grad():
        for k, branch in enumerate(blk.ap_conv_blocks):
            for p, v in zip((branch[1][1].weight, branch[1][1].bias, branch[1][2].weight, branch[1][2].bias),
                            params64[4 * k:4 * k + 4]):
                p.copy_(v.float())
    set_compute_dtype(blk, dtype)
    return blk.to(dev)


def _branch_params(blk):
    out = []
    for branch in blk.ap_conv_blocks:
        out.extend([branch[1][1].weight, branch[1][1].bias, branch[1][2].weight, branch[1][2].bias])
    return out


def _run(blk, x, dcat, unfused, monkeypatch, x_grad=True):
    """-> cat, dx (or None), the branch parameters' gradients; fresh gradients every call."""
    if unfused:
        monkeypatch.setenv('VKAS_PPM_UNFUSED', '1')
    else:
        monkeypatch.delenv('VKAS_PPM_UNFUSED', raising=False)
    ps = _branch_params(blk)
    for p in ps:
        p.grad = None
    xin = x.clone().requires_grad_(x_grad)
    cat = blk.branches_cat(xin)
    want = 'ResizeCatBackward' if unfused else 'PpmBranchesCatBackward'
    assert type(cat.grad_fn).__name__ == want, type(cat.grad_fn).__name__
    cat.backward(dcat)
    torch.cuda.synchronize()
    monkeypatch.delenv('VKAS_PPM_UNFUSED', raising=False)
    return cat.detach(), (xin.grad if x_grad else None), [p.grad.clone() for p in ps]


def _stored(case, dtype, dev, seed=0):
    """The case's inputs as the device stores them (x and dcat in the storage type, parameters fp32) and their fp64 images."""
    H, W, C, Cb, scales = case
    x64, p64, d64 = R.make_case(1000 * H + 10 * W + C + Cb + seed, B, H, W, C, Cb, scales)
    x = x64.to(dtype).to(dev)
    dcat = d64.to(dtype).to(dev)
    p32 = [p.float() for p in p64]
    return x, dcat, p32, x.double().cpu(), dcat.double().cpu(), [p.double() for p in p32]


def _err(a, ref):
    return float((a.double().cpu() - ref).norm() / ref.norm().clamp_min(1e-300))


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_parity_against_fp64_and_unfused(case, dtype, monkeypatch):
    H, W, C, Cb, scales = case
    dev = torch.device('cuda:0')
    x, dcat, p32, x64, d64, p64 = _stored(case, dtype, dev)
    blk = _block(case, dtype, p32, dev)
    cat_ref, saved = R.forward(x64, p64, scales)
    dx_ref, g_ref = R.backward(d64, p64, scales, saved, C)
    refs = [('cat', cat_ref), ('dx', dx_ref)]
    for k in range(len(scales)):
        refs.extend(zip(('dW%d' % k, 'db%d' % k, 'dgamma%d' % k, 'dbeta%d' % k), g_ref[4 * k:4 * k + 4]))
    cat_f, dx_f, g_f = _run(blk, x, dcat, False, monkeypatch)
    cat_u, dx_u, g_u = _run(blk, x, dcat, True, monkeypatch)
    assert cat_f.shape == cat_u.shape == (B, H, W, C + len(scales) * Cb)
    assert torch.equal(cat_f[..., :C], x)
    name = 'ppm_fused[%s-%s]' % (_ids(case), 'bf16' if dtype == torch.bfloat16 else 'fp16')
    failures = []
    for (q, ref), f, u in zip(refs, [cat_f, dx_f] + g_f, [cat_u, dx_u] + g_u):
        ef, eu = _err(f, ref), _err(u, ref)
        bound = 1.25 * eu + HALF_ULP[dtype]
        print('%s %-8s fused %.3e unfused %.3e bound %.3e' % (name, q, ef, eu, bound))
        parity_log.record(name, q + ' fused', ef, bound, 'unfused %.3e' % eu)
        if not ef <= bound:
            failures.append((q, ef, eu, bound))
    assert not failures, failures


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'fp16'])
def test_strided_dcat_no_input_grad_determinism(dtype, monkeypatch):
    """dcat as a channel slice of a wider buffer gives the bits of the dense one; so does a second run; without an input
    gradient the parameter gradients are the same bits and no dx comes back."""
    case = (7, 9, 72, 24, (1, 2, 3, 6))
    dev = torch.device('cuda:0')
    x, dcat, p32, *_ = _stored(case, dtype, dev, seed=3)
    blk = _block(case, dtype, p32, dev)
    cat0, dx0, g0 = _run(blk, x, dcat, False, monkeypatch)
    cat1, dx1, g1 = _run(blk, x, dcat, False, monkeypatch)
    assert torch.equal(cat0, cat1) and torch.equal(dx0, dx1) and all(torch.equal(a, b) for a, b in zip(g0, g1))
    wide = torch.randn((B, 7, 9, dcat.shape[3] + 16), device=dev).to(dtype)
    view = wide[..., 8:8 + dcat.shape[3]]
    view.copy_(dcat)
    assert not view.is_contiguous()
    cat2, dx2, g2 = _run(blk, x, view, False, monkeypatch)
    assert torch.equal(cat0, cat2) and torch.equal(dx0, dx2) and all(torch.equal(a, b) for a, b in zip(g0, g2))
    cat3, dx3, g3 = _run(blk, x, dcat, False, monkeypatch, x_grad=False)
    assert dx3 is None and torch.equal(cat0, cat3) and all(torch.equal(a, b) for a, b in zip(g0, g3))


def test_gradients_accumulate_onto_flat_views(monkeypatch):
    """With flat gradient views the kernel adds onto what they hold and reports the delivery; the sums are the tensors the
    node returns without sinks."""
    from vkit_ocr_model_adaptive_scaling_amd.training import FlatBuffers
    monkeypatch.delenv('VKAS_PPM_UNFUSED', raising=False)
    case = (5, 4, 72, 24, (1, 2, 3, 6))
    dtype, dev = torch.bfloat16, torch.device('cuda:0')
    x, dcat, p32, *_ = _stored(case, dtype, dev, seed=5)
    plain = _block(case, dtype, p32, dev)
    _, dx_plain, g_plain = _run(plain, x, dcat, False, monkeypatch)
    blk = _block(case, dtype, p32, dev)
    fb = FlatBuffers(blk.named_parameters())
    fb.flat_grad.fill_(0.5)
    names = {id(p): i for i, p in enumerate(fb.params)}
    ps = _branch_params(blk)
    assert all(fb.touched[names[id(p)]] == 0 for p in ps)
    xin = x.clone().requires_grad_(True)
    blk.branches_cat(xin).backward(dcat)
    torch.cuda.synchronize()
    assert torch.equal(xin.grad, dx_plain)
    for p, g in zip(ps, g_plain):
        assert fb.touched[names[id(p)]] == 1 and fb.grad_view_ok(names[id(p)])
        got = p.grad - 0.5
        tol = 2.0 ** -23 * (0.5 + float(g.abs().max()))  # one fp32 rounding of 0.5 + g
        assert float((got - g).abs().max()) <= tol, (float((got - g).abs().max()), tol)
    final = blk.final_conv_block[0].weight
    assert fb.touched[names[id(final)]] == 0 and float((final.grad - 0.5).abs().max()) == 0.0


def test_keep_false_saves_nothing_and_graph_replay(monkeypatch):
    from vkit_ocr_model_adaptive_scaling_amd import ops
    monkeypatch.delenv('VKAS_PPM_UNFUSED', raising=False)
    case = (12, 16, 72, 96, (1, 2, 3, 6))
    dtype, dev = torch.float16, torch.device('cuda:0')
    x, dcat, p32, *_ = _stored(case, dtype, dev, seed=7)
    blk = _block(case, dtype, p32, dev)
    cat_keep, _, _ = _run(blk, x, dcat, False, monkeypatch)
    node = ops.PpmBranchesCat.apply(x.clone().requires_grad_(True), False, case[4], *_branch_params(blk))
    assert len(node.grad_fn.saved_tensors) == 0 and torch.equal(node.detach(), cat_keep)
    with torch.no_grad():
        eager = blk.branches_cat(x)
        torch.cuda.synchronize()
        assert eager.grad_fn is None and torch.equal(eager, cat_keep)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            blk.branches_cat(x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static = blk.branches_cat(x)
        static.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static, eager)


def test_ineligible_block_takes_the_unfused_ops(monkeypatch):
    """PpmBlock((1, 2, 3, 6), 72, 20): 20 branch channels are not their own padded width - the block keeps the old ops."""
    from vkit_ocr_model_adaptive_scaling_amd import ops
    monkeypatch.delenv('VKAS_PPM_UNFUSED', raising=False)
    case = (7, 9, 72, 20, (1, 2, 3, 6))
    dev = torch.device('cuda:0')
    assert not ops.ppm_fused_eligible(torch.bfloat16, 72, 20, case[4])
    x64, p64, _ = R.make_case(11, B, 7, 9, 72, 20, case[4])
    blk = _block(case, torch.bfloat16, [p.float() for p in p64], dev)
    cat = blk.branches_cat(x64.to(torch.bfloat16).to(dev).requires_grad_(True))
    assert type(cat.grad_fn).__name__ == 'ResizeCatBackward'
    assert cat.shape == (B, 7, 9, ops.rup8(72 + 4 * 20))
    with pytest.raises(ValueError):
        ops.PpmBranchesCat.apply(x64.to(torch.bfloat16).to(dev), True, case[4], *_branch_params(blk))
    blk32 = _block((7, 9, 72, 24, (1, 2, 3, 6)), torch.float32, R.make_case(12, B, 7, 9, 72, 24, case[4])[1], dev)
    cat32 = blk32.branches_cat(torch.randn((B, 7, 9, 72), device=dev).requires_grad_(True))
    assert type(cat32.grad_fn).__name__ == 'ResizeCatBackward'  # fp32 storage keeps the exact path
