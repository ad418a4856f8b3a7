"""Forward of the x2 bilinear heads at the neck's height (ops.UpHeadsFused.rows_route), kernel by kernel and as a whole:

  row conv   conv1x3_slab_mfma_kernel through vkas_conv_gemm_fwd (KH = 1, KW = 3) against an fp64 convolution of the same stored
             operands, at the bound tests/test_gpu_gemm.py asserts for the row-slab tile forms (TOL of test_gpu_ops)
  row pass   vkas_head_rows_fwd on integer-valued T and power-of-two parameters against tests/head_rows_reference.py: z bit for
             bit, the statistics and the maps up to the tail's own arithmetic; two launches bit-equal; every segment length
  patches    vkas_points_gather_patches_up2 bit-equal to vkas_points_gather_patches on the materialised upsample
  route      UpHeadsFused on the new route against today's (VKAS_HEAD_FWD_UPRES) and against an fp64 evaluation of the same stored
             inputs, maps, z and every gradient, at the bounds tests/test_gpu_ops.py asserts for the fused heads; both routes'
             errors go to the parity report (tests/parity_log.py)."""
import ctypes
import math

import pytest
import torch

from tests import head_rows_reference as R
from tests import parity_log
from tests.test_gpu_ops import TOL, q

pytestmark = pytest.mark.gpu

CODE = {torch.bfloat16: 1, torch.float16: 2}
IDS = {torch.bfloat16: 'bf16', torch.float16: 'f16'}
GUARD = 64
GELU_ERR = 5e-5  # vkas_common.h: |error| of the 16-bit storage modes' polynomial GELU


def p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def _measure(got, ref):
    """(norm-wise error, worst element over the peak) in fp64"""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    d = (got - ref).abs()
    return float(d.norm() / ref.norm()), float(d.max() / ref.abs().max())


# ------------------------------------------------------------------------------------------------------------ 1x3 row convolution
# the issue's grid (3N = 24: one 128-column tile; 3N = 600: 224-column tiles), and 3N = 192 / 216 on one 192 / 224-column tile
ROW_CONV = [(W, C, N) for W in (256, 512) for C in (64, 72) for N in (8, 200)] + [(256, 72, 64), (256, 72, 72)]


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('W,C,N', ROW_CONV)
def test_row_conv_matches_fp64(W, C, N, dtype):
    from vkit_ocr_model_adaptive_scaling_amd import _lib, ops
    from vkit_ocr_model_adaptive_scaling_amd._lib import lib, check
    B, h = 2, 2
    x = q(_randn((B, h, W, C), 1), dtype)
    w = q(_randn((N, C, 3, 3), 2, 1.0 / math.sqrt(3 * C)), dtype)
    bias = _randn((3 * N,), 3, 0.1).float().double()
    xd = x.to(dtype).cuda()
    Bw = torch.empty((3 * N * 3 * C,), dtype=dtype, device='cuda')
    check(lib.vkas_pack_conv_weight_slice(p(w.float().cuda().contiguous()), p(Bw), N, C, 3, 3, N, C, 3, 0, N, CODE[dtype], _stream()),
          'pack_conv_weight_slice')
    M = B * h * W
    out = torch.full((M * 3 * N + GUARD,), float('nan'), dtype=dtype, device='cuda')
    out[-GUARD:] = -3.0
    bd = bias.float().cuda()
    geom = _lib.ConvGeom(B, h, W, h, W, C, C, 1, 3, 1, 1)
    want = {24: 4, 600: 7, 192: 6, 216: 7}[3 * N]  # one tile, three tiles with a ragged last one, the two exact fits
    assert ops.gemm_kernel_name(xd, 0, geom, 3 * N) == 'conv1x3_slab_mfma_kernel<%d>' % want
    assert lib.vkas_conv_gemm_kernel_id(0, ctypes.byref(geom), 3 * N, 0, 0) == 1100 + want
    epi = _lib.Epilogue(_lib.EPI_NONE, bd.data_ptr(), out.data_ptr(), 3 * N)
    check(lib.vkas_conv_gemm_fwd(p(xd), ctypes.byref(geom), p(Bw), 3 * N, ctypes.byref(epi), CODE[dtype], _stream()), 'conv_gemm_fwd')
    torch.cuda.synchronize()
    assert bool((out[-GUARD:] == -3.0).all())
    got = out[:-GUARD].view(B, h, W, 3 * N).cpu()
    ref = R.row_conv(x, w).reshape(B, h, W, 3 * N) + bias  # column ky * N + n
    rel, worst = _measure(got, q(ref, dtype))
    print('row conv W=%d C=%d N=%d %s: norm-wise %.3e worst %.3e' % (W, C, N, IDS[dtype], rel, worst))
    parity_log.record('test_gpu_head_fwd_rows', 'row conv 1x3 slab %d, %s (W=%d C=%d N=3x%d)' % (want, IDS[dtype], W, C, N), rel,
                      TOL[dtype][0])
    assert rel < TOL[dtype][0] and worst <= TOL[dtype][1], (rel, worst)


@pytest.mark.parametrize('N', [24, 192, 216], ids=['slab4', 'slab6', 'slab7'])
def test_existing_3x3_slab_forms_keep_the_parent_bits(N):
    """conv3x3_slab_mfma_kernel<4 / 6 / 7, plain epilogue> share their body with the new 1x3 form: on fixed inputs (B = 2, 32
    rows of 256 pixels, C = 72: a channel tail; bf16) their outputs hash to what the parent commit's library wrote
    (tests/golden/slab3x3_parent_sha256.json, recorded from a build of the parent)."""
    import hashlib
    import json
    import os
    from vkit_ocr_model_adaptive_scaling_amd import _lib
    from vkit_ocr_model_adaptive_scaling_amd._lib import lib, check
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'slab3x3_parent_sha256.json')))[str(N)]
    B, H, W, C, dt = 2, 32, 256, 72, torch.bfloat16
    g = torch.Generator().manual_seed(1234 + N)
    x = torch.randn((B, H, W, C), generator=g).to(dt).cuda()
    w = (torch.randn((N, C, 3, 3), generator=g) / math.sqrt(9 * C)).cuda().contiguous()
    bias = (torch.randn((N,), generator=g) * 0.1).cuda()
    Bw = torch.empty((N * 9 * C,), dtype=dt, device='cuda')
    check(lib.vkas_pack_conv_weight(p(w), p(Bw), N, C, 3, 3, N, C, 0, 1, _stream()), 'pack_conv_weight')
    out = torch.zeros((B * H * W, N), dtype=dt, device='cuda')
    geom = _lib.ConvGeom(B, H, W, H, W, C, C, 3, 3, 1, 1)
    assert lib.vkas_conv_gemm_kernel_id(0, ctypes.byref(geom), N, 0, 0) == gold['kernel_id']
    epi = _lib.Epilogue(_lib.EPI_NONE, bias.data_ptr(), out.data_ptr(), N)
    check(lib.vkas_conv_gemm_fwd(p(x), ctypes.byref(geom), p(Bw), N, ctypes.byref(epi), 1, _stream()), 'conv_gemm_fwd')
    torch.cuda.synchronize()
    assert hashlib.sha256(out.view(torch.int16).cpu().numpy().tobytes()).hexdigest() == gold['sha256']


def test_row_conv_rejects_what_no_kernel_takes():
    """a row that is no multiple of 256 pixels, fp32 storage: an error, not another kernel"""
    from vkit_ocr_model_adaptive_scaling_amd import _lib
    from vkit_ocr_model_adaptive_scaling_amd._lib import lib
    x = torch.zeros((1, 2, 264, 64), dtype=torch.bfloat16, device='cuda')
    Bw = torch.zeros((24 * 3 * 64,), dtype=torch.bfloat16, device='cuda')
    out = torch.zeros((2 * 264 * 24,), dtype=torch.bfloat16, device='cuda')
    for W, code in ((264, 1), (256, 0)):
        geom = _lib.ConvGeom(1, 2, W, 2, W, 64, 64, 1, 3, 1, 1)
        epi = _lib.Epilogue(_lib.EPI_NONE, None, out.data_ptr(), 24)
        assert lib.vkas_conv_gemm_fwd(p(x), ctypes.byref(geom), p(Bw), 24, ctypes.byref(epi), code, _stream()) != 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------- row pass
HEAD_SETS = {'three': ((192, 193, 194), (1, 2, 4)), 'two': ((192, 193), (1, 2)), 'one': ((194,), (4,))}
# every height with the built-in segment rule; h = 3 in segments of one and two rows (a ragged last one); a taller map walks
# every phase of the unrolled row loop and, at seg 4, windows that start inside the image
ROW_PASS = [(h, 0, 'three') for h in (1, 2, 3)] + [(3, 1, 'three'), (3, 2, 'three'), (3, 0, 'two'), (3, 0, 'one'), (2, 1, 'two'),
                                                  (9, 0, 'one'), (9, 4, 'two')]


def _pow2(shape, seed, lo, hi):
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(lo, hi + 1, shape, generator=g).double()
    s = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return s * 2.0 ** e


def _row_pass_case(h, heads, dtype):
    cs, ocs = HEAD_SETS[heads]
    B, W2 = 2, 256
    nps = [(c + 7) // 8 * 8 for c in cs]
    offs = [sum(nps[:k]) for k in range(len(cs) + 1)]
    Nt, pw = offs[-1], 224
    g = torch.Generator().manual_seed(7 + h)
    T = torch.zeros((B, h, W2, 3, Nt), dtype=torch.float64)
    bias = torch.zeros((Nt,), dtype=torch.float64)
    params = torch.zeros((len(cs), 6 * pw + 8), dtype=torch.float64)
    tails = []
    for k, (c, oc) in enumerate(zip(cs, ocs)):  # pad columns stay zero, as the convolution leaves them
        T[..., offs[k]:offs[k] + c] = torch.randint(-3, 4, (B, h, W2, 3, c), generator=g).double()
        bias[offs[k]:offs[k] + c] = torch.randint(-2, 3, (c,), generator=g).double() * 0.5
        gamma, beta = _pow2((c,), 20 + k, -1, 1).abs(), _pow2((c,), 30 + k, -2, 0)
        wproj, bproj = _pow2((oc, c), 40 + k, -3, 0), _pow2((oc,), 50 + k, -2, 1)
        params[k, :c], params[k, pw:pw + c] = gamma, beta
        for r in range(oc):
            params[k, (2 + r) * pw:(2 + r) * pw + c] = wproj[r]
        params[k, 6 * pw:6 * pw + oc] = bproj
        tails.append((gamma, beta, wproj, bproj))
    return dict(B=B, h=h, W2=W2, cs=cs, ocs=ocs, nps=nps, offs=offs, Nt=Nt, pw=pw, T=T, bias=bias, params=params, tails=tails,
                Td=T.reshape(B, h, W2, 3 * Nt).to(dtype).cuda(), bd=bias.float().cuda(), pd=params.float().cuda())


def _row_pass_run(c, seg, dtype, keep=True):
    from vkit_ocr_model_adaptive_scaling_amd import _lib
    from vkit_ocr_model_adaptive_scaling_amd._lib import lib, check
    n, M = len(c['cs']), c['B'] * 2 * c['h'] * c['W2']
    z = torch.full((M * c['Nt'] + GUARD,), float('nan'), dtype=dtype, device='cuda')
    z[-GUARD:] = -3.0
    stats = torch.full((n * M * 2 + GUARD,), -3.0, device='cuda')
    proj = torch.full((n * M * 8 + GUARD,), -3.0, device='cuda')
    hd = _lib.HeadDesc()
    hd.n_heads, hd.pw = n, c['pw']
    for k in range(n):
        hd.n0[k], hd.np[k], hd.c[k], hd.oc[k] = c['offs'][k], c['nps'][k], c['cs'][k], c['ocs'][k]
    hd.params, hd.stats, hd.proj = c['pd'].data_ptr(), stats.data_ptr() if keep else None, proj.data_ptr()
    check(lib.vkas_head_rows_fwd(p(c['Td']), p(c['bd']), ctypes.byref(hd), p(z if keep else None), c['B'], c['h'], c['W2'], c['Nt'],
                                 seg, CODE[dtype], _stream()), 'head_rows_fwd')
    torch.cuda.synchronize()
    assert bool((z[-GUARD:] == -3.0).all() and (stats[-GUARD:] == -3.0).all() and (proj[-GUARD:] == -3.0).all())
    return (z[:-GUARD].view(c['B'], 2 * c['h'], c['W2'], c['Nt']), stats[:-GUARD].view(n, c['B'], 2 * c['h'], c['W2'], 2),
            proj[:-GUARD].view(n, c['B'], 2 * c['h'], c['W2'], 8))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('h,seg,heads', ROW_PASS)
def test_row_pass_matches_host_restatement(h, seg, heads, dtype):
    c = _row_pass_case(h, heads, dtype)
    z, stats, proj = _row_pass_run(c, seg, dtype)
    z2, stats2, proj2 = _row_pass_run(c, seg, dtype)
    assert torch.equal(z, z2) and torch.equal(stats, stats2) and torch.equal(proj, proj2)  # two launches: the same bits
    # z: integers blended with 0.25 / 0.75 plus multiples of 0.5 - quarter steps below 16, exact in fp32 and in both 16-bit types
    zr = R.rows_to_z(c['T'], c['bias'])
    assert torch.equal(z.double().cpu(), zr), 'z differs at %s' % (z.double().cpu() != zr).nonzero()[:4].tolist()
    # inference form: no z, no statistics, the same maps
    _, _, proj3 = _row_pass_run(c, seg, dtype, keep=False)
    assert torch.equal(proj, proj3)
    for k, (cc, oc) in enumerate(zip(c['cs'], c['ocs'])):
        gamma, beta, wproj, bproj = c['tails'][k]
        o = c['offs'][k]
        maps, mean, rstd = R.head_tail(zr[..., o:o + cc], cc, gamma, beta, wproj, bproj)
        # statistics: fp32 sums of exact quarter steps (exact: below 2^24 quarter steps), mean one division; the variance comes
        # from E[z^2] - mean^2, which loses E[z^2] / var of fp32's 2^-24 - |z| < 16 and var > 1 / 4 here: 2^-14 relative
        assert float(((stats[k, ..., 0].double().cpu() - mean).abs() - 2.0 ** -22 * mean.abs().clamp_min(1.0)).max()) <= 0
        assert float(((stats[k, ..., 1].double().cpu() - rstd).abs() / rstd).max()) <= 2.0 ** -14
        # maps: per element of the activation the GELU polynomial's error plus u's relative 2^-14 through |GELU'| <= 1.13, summed
        # over the projection row with its absolute weights
        u = (zr[..., o:o + cc] - mean[..., None]) * rstd[..., None] * gamma + beta
        allow = (GELU_ERR + 1.13 * 2.0 ** -14 * u.abs()) @ wproj.abs().T + 2.0 ** -20 * maps.abs()
        got = proj[k].double().cpu()
        assert float(got[..., oc:].abs().max()) == 0.0
        over = (got[..., :oc] - maps).abs() - allow
        assert float(over.max()) <= 0, (k, float(over.max()), float(allow.max()))


# --------------------------------------------------------------------------------------------------------- label-point patches
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
def test_patches_from_the_neck_feature_are_those_of_the_upsample(dtype):
    from vkit_ocr_model_adaptive_scaling_amd import ops
    B, h, w, Cp = 2, 5, 7, 24
    x = _randn((B, h, w, Cp), 5).to(dtype).cuda()
    H, W = 2 * h, 2 * w
    ys = [0, 0, H - 1, H - 1, 1, H - 2, 4, 5, 4, 9, 3, 3]  # the four corners, the rows and columns next to them, a duplicate
    xs = [0, W - 1, 0, W - 1, 1, W - 2, 6, 7, 13, 0, 8, 8]
    py = torch.tensor([ys, ys[::-1]], dtype=torch.int64, device='cuda')
    px = torch.tensor([xs, xs], dtype=torch.int64, device='cuda')
    _, _, pix, Mp = ops._points_prepare(py, px, B, H, W)
    up = ops.resize_fwd(x, (H, W), 0)
    a = ops._points_gather_patches(up, pix, Mp)
    b = ops._points_gather_patches_up2(x, pix, Mp)
    torch.cuda.synchronize()
    assert a.shape == b.shape == (1, 1, Mp, 9 * Cp) and float(a.float().abs().max()) > 0
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------- the whole route
ROUTE_SETS = {'rough': ((192, 192), (1, 1)), 'precise': ((192, 193, 194, 194), (1, 2, 4, 4))}
MAPS_BOUND, DX_BOUND, PARAM_BOUND = 8e-3, 1.5e-2, 2e-2  # tests/test_gpu_ops.py::test_heads_fused_matches_unfused_and_fp64


def _conv3x3_fp64(up, w, b):
    """(B, H, W, N) = conv3x3 (zero padded) of up (B, H, W, C) with w (N, C, 3, 3): nine shifted matrix products"""
    B, H, W, C = up.shape
    xp = torch.zeros((B, H + 2, W + 2, C), dtype=up.dtype, device=up.device)
    xp[:, 1:-1, 1:-1] = up
    return b + sum(xp[:, ky:ky + H, kx:kx + W] @ w[:, :, ky, kx].T for ky in range(3) for kx in range(3))


@pytest.mark.parametrize('name', ['rough', 'precise'])
def test_route_matches_upres_route_and_fp64(name, monkeypatch):
    from vkit_ocr_model_adaptive_scaling_amd import ops
    cs, ocs = ROUTE_SETS[name]
    B, h, w, C, dtype = 1, 128, 128, 384, torch.bfloat16
    H, W = 2 * h, 2 * w
    x = q(_randn((B, h, w, C), 50), dtype)
    convs = [(q(_randn((c, C, 3, 3), 51 + i, 1.0 / math.sqrt(C * 9)), dtype), _randn((c,), 61 + i, 0.1).float().double())
             for i, c in enumerate(cs)]
    tails = [((1 + _randn((c,), 71 + i, 0.1)).float().double(), _randn((c,), 81 + i, 0.1).float().double(),
              _randn((oc, c), 91 + i, 1.0 / math.sqrt(c)).float().double(), _randn((oc,), 101 + i, 0.1).float().double())
             for i, (c, oc) in enumerate(zip(cs, ocs))]
    cots = [_randn((B, H, W, oc), 111 + i) for i, oc in enumerate(ocs)]
    # fp64 evaluation of the same stored inputs, on the device
    xr = x.cuda().requires_grad_(True)
    ref_params, ref_maps, ref_z = [], [], []
    up = R.up2_axis(R.up2_axis(xr, 1), 2)
    for (wt, b), t in zip(convs, tails):
        ps = [v.cuda().requires_grad_(True) for v in (wt, b, *t)]
        ref_params.append(ps)
        z = _conv3x3_fp64(up, ps[0], ps[1])
        ref_z.append(z.detach())
        ref_maps.append(R.head_tail(z, z.shape[-1], ps[2], ps[3], ps[4], ps[5])[0])
    sum((m * c.cuda()).sum() for m, c in zip(ref_maps, cots)).backward()
    del up, z

    def run(upres):
        monkeypatch.setattr(ops, '_HEAD_FWD_UPRES', upres)
        xa = x.to(dtype).cuda().requires_grad_(True)
        dev = [[v.float().cuda().requires_grad_(True) for v in (wt, b, *t)] for (wt, b), t in zip(convs, tails)]
        assert ops.UpHeadsFused.eligible(xa, cs, ocs)
        assert ops.UpHeadsFused.rows_route(xa, False, [v for hd in dev for v in hd]) == (not upres)
        outs = ops.UpHeadsFused.apply(xa, True, False, *[v for hd in dev for v in hd])
        zs = outs[0].grad_fn.saved_tensors[1]
        assert outs[0].grad_fn.saved_tensors[0].shape[1] == (H if upres else h)  # the upsample is saved on today's route only
        sum((o[..., :oc] * c.float().cuda()).sum() for o, oc, c in zip(outs, ocs, cots)).backward()
        torch.cuda.synchronize()
        return [o.detach() for o in outs], zs, xa.grad, dev

    res = {'rows': run(False), 'upres': run(True)}
    names = ('conv w', 'conv b', 'gamma', 'beta', 'proj w', 'proj b')
    offs = [sum((c + 7) // 8 * 8 for c in cs[:k]) for k in range(len(cs))]
    for route, (outs, zs, gx, dev) in res.items():
        tag = 'test_gpu_head_fwd_rows[%s-%s]' % (name, route)
        for k, (o, oc, c) in enumerate(zip(outs, ocs, cs)):
            assert float(o[..., oc:].abs().max()) == 0.0
            rel, worst = _measure(o[..., :oc], ref_maps[k].detach())
            parity_log.record(tag, 'head %d maps' % k, rel, MAPS_BOUND, 'worst element %.3e of the peak (bound %.1e)' % (worst, TOL[dtype][1]))
            assert rel < MAPS_BOUND and worst <= TOL[dtype][1], (route, k, rel, worst)
            relz, worstz = _measure(zs[..., offs[k]:offs[k] + c], q(ref_z[k], dtype))
            parity_log.record(tag, 'head %d z' % k, relz, TOL[dtype][0], 'worst element %.3e of the peak (bound %.1e)' % (worstz, TOL[dtype][1]))
            assert relz < TOL[dtype][0] and worstz <= TOL[dtype][1], (route, k, relz, worstz)
        e = _measure(gx, xr.grad)[0]
        parity_log.record(tag, 'input gradient', e, DX_BOUND)
        assert e < DX_BOUND, (route, e)
        worst_p = 0.0
        for ps, rs in zip(dev, ref_params):
            for n, pp, r in zip(names, ps, rs):
                e = _measure(pp.grad, r.grad)[0]
                worst_p = max(worst_p, e)
                assert e < PARAM_BOUND, (route, n, e)
        parity_log.record(tag, 'worst parameter gradient', worst_p, PARAM_BOUND)
    # the two routes round at different places but compute the same thing
    for a, b in zip(res['rows'][0], res['upres'][0]):
        assert _measure(a, b)[0] < MAPS_BOUND
