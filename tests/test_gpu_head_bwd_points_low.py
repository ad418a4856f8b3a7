"""ops.UpHeadsFused with label-point heads: their input gradient added straight onto the neck-resolution dx
(vkas_points_scatter3x3_low, ops._POINTS_LOW_SCATTER) next to the route it replaces (a zeroed 2h x 2w buffer, then
vkas_resize_bwd), on the same inputs, both against fp64 autograd of upsample -> conv3x3 -> LayerNorm -> GELU -> Linear.
The new route rounds the points' contribution once less, so every gradient's error against fp64 must stay within 1.5 x the old
route's (the rule of tests/test_gpu_head_bwd_lowres.py).  Smallest eligible map: B = 1, h = w = 64 (4 B h w = 16 384), C = 40.
The two runs must differ in some bits of dx, which shows that the switch selected two routes.  Cases: one dense head + two
label-point heads, and label-point heads only (dx is then zeros plus the points)."""
import math

import pytest
import torch
from torch.nn import functional as F

from oracle import torch_oracle as O
from tests.helpers import rel_err
from tests.test_gpu_head_bwd_lowres import _MarkPoints
from tests.test_gpu_ops import from_act, ops_mod, q, rnd, to_act

pytestmark = pytest.mark.gpu

CASES = [((48, 40, 33), (1, 2, 4), 1), ((40, 33), (2, 4), 0)]  # channels, out_channels, number of dense heads in front


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('case', CASES, ids=['dense1_points2', 'points2'])
def test_points_low_scatter_gradients_within_1p5x_of_upres_scatter(case, dtype):
    ops = ops_mod()
    cs, ocs, n_dense = case
    B, Cin, h, w = 1, 40, 64, 64
    H, W = 2 * h, 2 * w
    x = q(rnd((B, Cin, h, w), 50), dtype)
    convs = [(q(rnd((c, Cin, 3, 3), 51 + i, 1.0 / math.sqrt(Cin * 9)), dtype), rnd((c,), 61 + i, 0.1)) for i, c in enumerate(cs)]
    tails = [(1 + rnd((c,), 71 + i, 0.1), rnd((c,), 81 + i, 0.1), rnd((oc, c), 91 + i, 1.0 / math.sqrt(c)), rnd((oc,), 101 + i, 0.1))
             for i, (c, oc) in enumerate(zip(cs, ocs))]
    g = torch.Generator().manual_seed(3)
    P = 24
    py, px = torch.randint(0, H, (B, P), generator=g), torch.randint(0, W, (B, P), generator=g)
    py[0, :4], px[0, :4] = torch.tensor([0, 0, H - 1, H - 1]), torch.tensor([0, W - 1, 0, W - 1])  # corners
    py[0, 4:6], px[0, 4:6] = 9, 9                                                                  # one pixel twice
    py[0, 6:9], px[0, 6:9] = torch.tensor([20, 20, 21]), torch.tensor([30, 31, 30])                # neighbours
    mask = torch.zeros((B, H, W), dtype=torch.float64)
    mask[torch.arange(B)[:, None], py, px] = 1.0
    xr = x.clone().requires_grad_(True)
    xu = F.interpolate(xr, scale_factor=2, mode='bilinear', align_corners=False)
    ref_params, ref_outs = [], []
    for (wt, b), (gm, bt, wp, bp) in zip(convs, tails):
        ps = [t.clone().requires_grad_(True) for t in (wt, b, gm, bt, wp, bp)]
        ref_params.append(ps)
        a = O.gelu(O.layer_norm_nchw(F.conv2d(xu, ps[0], ps[1], padding=1), ps[2], ps[3]))
        ref_outs.append(O.linear_nchw(a, ps[4], ps[5]))
    cots = [rnd(tuple(o.shape), 111 + i) * (mask[:, None] if i >= n_dense else 1.0) for i, o in enumerate(ref_outs)]
    sum((o * c).sum() for o, c in zip(ref_outs, cots)).backward()
    pyc, pxc = py.cuda(), px.cuda()

    def run(low_scatter):
        old = ops._POINTS_LOW_SCATTER
        ops._POINTS_LOW_SCATTER = low_scatter
        try:
            xa = to_act(x, dtype).requires_grad_(True)
            dev = [[t.float().cuda().requires_grad_(True) for t in (wt, b, gm, bt, wp, bp)]
                   for (wt, b), (gm, bt, wp, bp) in zip(convs, tails)]
            assert ops.UpHeadsFused.eligible(xa, cs, ocs)
            outs = ops.UpHeadsFused.apply(xa, True, False, *[t for head in dev for t in head])
            loss = 0
            for i, (o, oc, c) in enumerate(zip(outs, ocs, cots)):
                if i >= n_dense:
                    o = _MarkPoints.apply(o, pyc, pxc)
                loss = loss + (o[..., :oc].permute(0, 3, 1, 2) * c.float().cuda()).sum()
            loss.backward()
            torch.cuda.synchronize()
        finally:
            ops._POINTS_LOW_SCATTER = old
        errs = {'dx': rel_err(from_act(xa.grad, Cin), xr.grad)}
        for hi, (ps, rs) in enumerate(zip(dev, ref_params)):
            for n, p, r in zip(('conv w', 'conv b', 'gamma', 'beta', 'proj w', 'proj b'), ps, rs):
                errs['head %d %s' % (hi, n)] = rel_err(p.grad, r.grad)
        return errs, xa.grad.detach().clone()

    (e_new, dx_new), (e_old, dx_old) = run(True), run(False)
    # the two runs took different routes: the old one rounds the points' contribution to the storage type before U^T
    assert not torch.equal(dx_new.view(torch.int16), dx_old.view(torch.int16))
    for n in e_new:
        print('%-16s new %.3e  old %.3e  ratio %.2f' % (n, e_new[n], e_old[n], e_new[n] / max(e_old[n], 1e-300)))
    for n in e_new:
        assert e_new[n] <= 1.5 * e_old[n], (n, e_new[n], e_old[n])
