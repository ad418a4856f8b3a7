"""Heads' backward at the neck's resolution (csrc/upconv_adj.hip, ops.UpHeadsFused).

* vkas_upconv_adj alone, through the C ABI, against vkas_resize_bwd applied to the nine moved, zero-filled copies of dz built
  with torch indexing: the same 16-bit inputs and fp32 arithmetic on both sides (the kernel applies the weights separably, the
  resize kernel as products), so the results differ by fp32 rounding in front of the one rounding to the storage type - the
  single-op tolerance of tests/test_gpu_ops.py (TOL / close).
* ops.UpHeadsFused against fp64 autograd of upsample -> conv3x3 -> LayerNorm -> GELU -> Linear, next to the path it replaces
  (ops.Resize + ops.HeadsFused, what VKAS_HEAD_BWD_UPRES=1 selects) on the same inputs: both round the same number of 16-bit
  operands, in different places, so every gradient's error against fp64 must stay within 1.5 x the old path's.
"""
import ctypes
import math

import pytest
import torch
from torch.nn import functional as F

from oracle import torch_oracle as O
from tests.helpers import rel_err
from tests.test_gpu_ops import close, from_act, ops_mod, q, rnd, to_act

pytestmark = pytest.mark.gpu

CODE = {torch.bfloat16: 1, torch.float16: 2}


def _moved(dz, ky, kx):
    """out[q] = dz[q + (ky - 1, kx - 1)], zero where that leaves the map.  dz (B, H, W, N)."""
    H, W = dz.shape[1], dz.shape[2]
    ty, tx = ky - 1, kx - 1
    out = torch.zeros(dz.shape, dtype=dz.dtype, device=dz.device)
    ys, yd = slice(max(ty, 0), H + min(ty, 0)), slice(max(-ty, 0), H + min(-ty, 0))
    xs, xd = slice(max(tx, 0), W + min(tx, 0)), slice(max(-tx, 0), W + min(-tx, 0))
    out[:, yd, xd, :] = dz[:, ys, xs, :]
    return out


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('case', [(2, 7, 9, 40, 0), (3, 5, 33, 24, 16), (1, 2, 2, 8, 0), (2, 16, 31, 200, 8), (1, 64, 64, 192, 0)],
                         ids=lambda c: 'B%d_%dx%d_N%d_ld%d' % c)
def test_upconv_adj_matches_resize_bwd_of_moved_copies(case, dtype):
    from vkit_ocr_model_adaptive_scaling_amd._lib import lib, check
    B, h, w, N, ld_extra = case
    H, W = 2 * h, 2 * w
    buf = torch.zeros((B, H, W, N + ld_extra), dtype=dtype, device='cuda')
    buf[..., :N] = rnd((B, H, W, N), 7).to(dtype).cuda()
    dz = buf[..., :N]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    E = torch.full((B, h, w, 9 * N), float('nan'), dtype=dtype, device='cuda')
    check(lib.vkas_upconv_adj(ctypes.c_void_p(dz.data_ptr()), N + ld_extra, ctypes.c_void_p(E.data_ptr()), B, h, w, N, CODE[dtype], st),
          'upconv_adj')
    for k in range(9):
        s = _moved(dz, k // 3, k % 3).contiguous()
        ref = torch.empty((B, h, w, N), dtype=dtype, device='cuda')
        check(lib.vkas_resize_bwd(ctypes.c_void_p(s.data_ptr()), N, ctypes.c_void_p(ref.data_ptr()), N, B, h, w, H, W, N, 0, 0,
                                  CODE[dtype], st), 'resize_bwd')
        close(E[..., k * N:(k + 1) * N], ref, dtype, 'E tap %d' % k)
    torch.cuda.synchronize()


class _MarkPoints(torch.autograd.Function):
    """Identity whose gradient is zero off the label points and says so (what the precise loss does for its point heads)."""

    @staticmethod
    def forward(ctx, y, py, px):
        ctx.pts = (py, px)
        return y.clone()

    @staticmethod
    def backward(ctx, g):
        from vkit_ocr_model_adaptive_scaling_amd import ops
        py, px = ctx.pts
        B = g.shape[0]
        keep = torch.zeros(g.shape[:3], dtype=torch.bool, device=g.device)
        keep[torch.arange(B, device=g.device)[:, None], py, px] = True
        out = (g * keep[..., None]).contiguous()
        return ops.point_sparse(out, py, px), None, None


HEAD_CASES = [((96,), (1,), False), ((40, 33), (1, 2), False), ((192, 192), (1, 1), False), ((48, 40, 33, 33), (1, 2, 4, 4), False),
              ((48, 40, 33, 33), (1, 2, 4, 4), True), ((96, 64), (1, 4), True)]


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('case', HEAD_CASES, ids=lambda c: 'c%s_oc%s_%s' % ('-'.join(map(str, c[0])), '-'.join(map(str, c[1])),
                                                                              'points' if c[2] else 'dense'))
def test_up_heads_fused_gradients_within_1p5x_of_upres_path(case, dtype):
    """1, 2 and 4 heads with out_channels 1 / 2 / 4, with and without label-point heads (every head but the first receives
    gradient at 24 points per image only and takes the compact path, in both runs)."""
    ops = ops_mod()
    cs, ocs, points = case
    B, Cin, h, w = 2, 64, 64, 72
    H, W = 2 * h, 2 * w
    x = q(rnd((B, Cin, h, w), 50), dtype)
    convs = [(q(rnd((c, Cin, 3, 3), 51 + i, 1.0 / math.sqrt(Cin * 9)), dtype), rnd((c,), 61 + i, 0.1)) for i, c in enumerate(cs)]
    tails = [(1 + rnd((c,), 71 + i, 0.1), rnd((c,), 81 + i, 0.1), rnd((oc, c), 91 + i, 1.0 / math.sqrt(c)), rnd((oc,), 101 + i, 0.1))
             for i, (c, oc) in enumerate(zip(cs, ocs))]
    g = torch.Generator().manual_seed(3)
    P = 24
    py, px = torch.randint(0, H, (B, P), generator=g), torch.randint(0, W, (B, P), generator=g)
    py[0, :4], px[0, :4] = torch.tensor([0, 0, H - 1, H - 1]), torch.tensor([0, W - 1, 0, W - 1])  # corners
    py[1, :2], px[1, :2] = 9, 9                                                                    # one pixel twice
    mask = torch.zeros((B, H, W), dtype=torch.float64)
    mask[torch.arange(B)[:, None], py, px] = 1.0
    # fp64 reference
    xr = x.clone().requires_grad_(True)
    xu = F.interpolate(xr, scale_factor=2, mode='bilinear', align_corners=False)
    ref_params, ref_outs = [], []
    for (wt, b), (gm, bt, wp, bp) in zip(convs, tails):
        ps = [t.clone().requires_grad_(True) for t in (wt, b, gm, bt, wp, bp)]
        ref_params.append(ps)
        a = O.gelu(O.layer_norm_nchw(F.conv2d(xu, ps[0], ps[1], padding=1), ps[2], ps[3]))
        ref_outs.append(O.linear_nchw(a, ps[4], ps[5]))
    cots = [rnd(tuple(o.shape), 111 + i) * (mask[:, None] if (points and i > 0) else 1.0) for i, o in enumerate(ref_outs)]
    sum((o * c).sum() for o, c in zip(ref_outs, cots)).backward()
    # fp16 gradients of small cotangents do not underflow here (O(1) cotangents): no loss scaling
    pyc, pxc = py.cuda(), px.cuda()

    def run(low):
        xa = to_act(x, dtype).requires_grad_(True)
        dev = [[t.float().cuda().requires_grad_(True) for t in (wt, b, gm, bt, wp, bp)] for (wt, b), (gm, bt, wp, bp) in zip(convs, tails)]
        fused = [t for head in dev for t in head]
        if low:
            assert ops.UpHeadsFused.eligible(xa, cs, ocs)
            outs = ops.UpHeadsFused.apply(xa, True, False, *fused)
        else:  # the path VKAS_HEAD_BWD_UPRES=1 selects
            up = ops.Resize.apply(xa, (H, W), 0)
            assert ops.HeadsFused.eligible(up, cs, ocs)
            outs = ops.HeadsFused.apply(up, True, *fused)
        loss = 0
        for i, (o, oc, c) in enumerate(zip(outs, ocs, cots)):
            if points and i > 0:
                o = _MarkPoints.apply(o, pyc, pxc)
            loss = loss + (o[..., :oc].permute(0, 3, 1, 2) * c.float().cuda()).sum()
        loss.backward()
        torch.cuda.synchronize()
        errs = {'dx': rel_err(from_act(xa.grad, Cin), xr.grad)}
        for hi, (ps, rs) in enumerate(zip(dev, ref_params)):
            for n, p, r in zip(('conv w', 'conv b', 'gamma', 'beta', 'proj w', 'proj b'), ps, rs):
                errs['head %d %s' % (hi, n)] = rel_err(p.grad, r.grad)
        return [o.detach().clone() for o in outs], errs

    outs_low, e_low = run(True)
    outs_up, e_up = run(False)
    for a, b in zip(outs_low, outs_up):
        assert torch.equal(a, b)  # forward: the same two launches
    for n in e_low:
        print('%-16s lowres %.3e  upres %.3e  ratio %.2f' % (n, e_low[n], e_up[n], e_low[n] / max(e_up[n], 1e-300)))
    for n in e_low:
        assert e_low[n] <= 1.5 * e_up[n], (n, e_low[n], e_up[n])


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('case', [c for c in HEAD_CASES if c[2]], ids=lambda c: 'c%s_oc%s' % ('-'.join(map(str, c[0])),
                                                                                                '-'.join(map(str, c[1]))))
def test_up_heads_fused_gradients_within_1p5x_of_upres_path_compact_path_off(case, dtype):
    """The label-point cases with the compact path switched off (VKAS_POINT_SPARSE_BWD=0): the marked heads stay dense and keep
    the convolution kernels, the unmarked head takes the neck-resolution path, and both input gradients meet in the U^T add.
    Same shapes, same fp64 reference, same criterion."""
    ops = ops_mod()
    old = ops._POINT_SPARSE
    ops._POINT_SPARSE = False
    try:
        test_up_heads_fused_gradients_within_1p5x_of_upres_path(case, dtype)
    finally:
        ops._POINT_SPARSE = old
