"""The label-point kernels (csrc/points.hip, vkas_points_margin) on the MI355X, through the C ABI, against their host
restatement tests/points_reference.py (itself held to F.unfold / F.fold / np.unique in tests/test_cpu_points_reference.py).

The kernels are copies and short fp32 sums in a fixed order, so they are held exactly: every output buffer starts as NaN or a
canary with guard words behind it, and the comparisons are torch.equal.  vkas_points_scatter3x3 - one workgroup per touched
pixel, elected by "first contributor in tap order" - is run on integer operands of magnitude <= 8 (every sum <= 80: exact in
bf16, so bit-equal to the fp64 restatement in any order) with a large sentinel in the rows of duplicates and padding, and on
random operands under the bound of an fp32 sum of at most ten terms rounded once.  The point sets are those of
points_reference.POINT_SETS: pairs at distances 1 to 3, blocks, borders, the seam between two rows and between two images,
degenerate maps, clamped coordinates, duplicates, more than one workgroup of points.  The pix / map operands of every kernel
but prepare come from the restatement, so each kernel is judged on its own.

One composition test: ops.HeadsAtPoints, whose input gradient is zeros plus the scatter, against fp64 autograd and against
ops.HeadsFused on the dense kernels with the same masked cotangent."""
import ctypes
import math

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from oracle import torch_oracle as O
from tests import points_reference as R
from tests.helpers import rel_err
from tests.test_gpu_ops import ops_mod, q, rnd, to_act

pytestmark = pytest.mark.gpu

CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
IDS = {torch.bfloat16: 'bf16', torch.float16: 'f16', torch.float32: 'f32'}
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}  # one rounding to the storage type
SETS = list(R.POINT_SETS)
CPS = (8, 72, 520)  # 72: 81 8-wide vectors per patch, more than the 64 lanes; 520: the channel loop of the scatter runs twice
G = 64              # guard words behind every buffer a kernel writes
INT_CANARY = -7777


def _lib():
    from vkit_ocr_model_adaptive_scaling_amd import _lib as L
    return L.lib, L.check


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def guarded(shape, fill, dtype):
    """(view of the given shape, the G guard words behind it), both filled with ``fill``"""
    n = int(np.prod(shape))
    buf = torch.full((n + G,), fill, dtype=dtype, device='cuda')
    return buf[:n].view(shape), buf[n:]


def guard_ok(guard, fill):
    return bool((guard == fill).all())


def dev_points(name, Mp=None):
    """the restatement's (map, pix) of a point set on the device"""
    pmap, pix = R.prepared(name, Mp)
    return torch.from_numpy(pmap.copy()).cuda(), torch.from_numpy(pix.copy()).cuda(), pmap, pix


# ---------------------------------------------------------------------------------------------------------------- prepare
@pytest.mark.parametrize('name', SETS)
def test_prepare_matches_restatement(name):
    lib, check = _lib()
    c = R.POINT_SETS[name]
    B, P, H, W = c['B'], c['P'], c['H'], c['W']
    n, M = B * P, B * H * W
    py, px = torch.from_numpy(c['py']).cuda(), torch.from_numpy(c['px']).cuda()
    for Mp in sorted({c['Mp'], n, n + 3}):
        ref_map, ref_pix = R.prepared(name, Mp)
        pmap, gm = guarded((M,), INT_CANARY, torch.int32)
        pix, gp = guarded((Mp,), INT_CANARY, torch.int32)
        check(lib.vkas_points_prepare(p(py), p(px), B, P, H, W, p(pmap), p(pix), Mp, st()), 'points_prepare')
        torch.cuda.synchronize()
        assert guard_ok(gm, INT_CANARY) and guard_ok(gp, INT_CANARY), (Mp, 'guard words overwritten')
        assert np.array_equal(pmap.cpu().numpy(), ref_map), (Mp, 'map')
        assert np.array_equal(pix.cpu().numpy(), ref_pix), (Mp, 'pix')
        assert (pix[n:] == R.PAD).all()  # pix[n:Mp] is all padding


# ------------------------------------------------------------------------------------------------------------ gather_rows
ROWS_FORMS = [(8, 1), (200, 2), (776, 3), (200, 4), (8, 4), (776, 1)]  # (Ns, n_heads); 776: the 64-lane loop runs twice


def _rows_call(lib, z, ldz, c0, Ns, stats, dprojs, M, pix, Mp, zs, stats_s, dproj_s, code):
    ptrs = (ctypes.c_void_p * 4)(*[d.data_ptr() for d in dprojs])
    return lib.vkas_points_gather_rows(p(z), ldz, c0, Ns, p(stats), ptrs, len(dprojs), M, p(pix), Mp, p(zs), p(stats_s),
                                       p(dproj_s), code, st())


@pytest.mark.parametrize('dtype', DTYPES[:2], ids=['bf16', 'f16'])
@pytest.mark.parametrize('name', SETS)
def test_gather_rows_matches_restatement(name, dtype):
    lib, check = _lib()
    c = R.POINT_SETS[name]
    n, M, Mp = c['B'] * c['P'], c['B'] * c['H'] * c['W'], c['Mp']
    _, d_pix, _, pix = dev_points(name)
    for k, (Ns, nh) in enumerate(ROWS_FORMS):
        c0 = 8 + 8 * (k % 2)
        ldz = c0 + Ns + 16  # ldz > c0 + Ns
        g = gen(100 + k)
        z = torch.randn((M, ldz), generator=g).to(dtype)
        stats = torch.randn((nh, M, 2), generator=g)
        dprojs = [torch.randn((M, 8), generator=g) for _ in range(nh)]
        zs, g0 = guarded((Mp, Ns), float('nan'), dtype)
        stats_s, g1 = guarded((nh, Mp, 2), float('nan'), torch.float32)
        dproj_s, g2 = guarded((nh, Mp, 8), float('nan'), torch.float32)
        for gd in (g0, g1, g2):
            gd.fill_(-3.0)
        zd, sd, dd = z.cuda(), stats.cuda(), [d.cuda() for d in dprojs]
        check(_rows_call(lib, zd, ldz, c0, Ns, sd, dd, M, d_pix, Mp, zs, stats_s, dproj_s, CODE[dtype]), 'points_gather_rows')
        torch.cuda.synchronize()
        assert all(guard_ok(gd, -3.0) for gd in (g0, g1, g2)), (Ns, nh, 'guard words overwritten')
        e_zs, e_stats, e_dproj = R.gather_rows(z, c0, Ns, stats, dprojs, pix)
        assert torch.equal(zs.cpu(), e_zs), (Ns, nh, 'zs')
        assert torch.equal(stats_s.cpu(), e_stats), (Ns, nh, 'stats')  # head h reads stats at h*M + q
        assert torch.equal(dproj_s.cpu(), e_dproj), (Ns, nh, 'd(proj)')
        # said directly: owners get their d(proj) row, duplicates z and statistics but zero d(proj), padding rows zeros
        dup, pad = torch.from_numpy((pix < 0) & (pix != R.PAD)), torch.from_numpy(pix == R.PAD)
        qd = torch.from_numpy(-1 - pix[dup.numpy()].astype(np.int64))
        assert not dproj_s.cpu()[:, dup].any() and torch.equal(zs.cpu()[dup], z[qd, c0:c0 + Ns])
        assert torch.equal(stats_s.cpu()[:, dup], stats[:, qd])
        assert not zs.cpu()[pad].any() and not stats_s.cpu()[:, pad].any() and not dproj_s.cpu()[:, pad].any()
        assert int(pad.sum()) == Mp - n


def test_gather_rows_rejects_f32():
    lib, _ = _lib()
    M, Mp, Ns = 16, 8, 8
    pix = torch.full((Mp,), R.PAD, dtype=torch.int32, device='cuda')
    z = torch.zeros((M, Ns), device='cuda')
    zs, g0 = guarded((Mp, Ns), 5.0, torch.float32)
    stats_s, g1 = guarded((1, Mp, 2), 5.0, torch.float32)
    dproj_s, g2 = guarded((1, Mp, 8), 5.0, torch.float32)
    rc = _rows_call(lib, z, Ns, 0, Ns, torch.zeros((1, M, 2), device='cuda'), [torch.zeros((M, 8), device='cuda')], M, pix, Mp,
                    zs, stats_s, dproj_s, CODE[torch.float32])
    torch.cuda.synchronize()
    assert rc != 0 and b'16-bit' in lib.vkas_last_error(), (rc, lib.vkas_last_error())
    for t, gd in ((zs, g0), (stats_s, g1), (dproj_s, g2)):
        assert (t == 5.0).all() and guard_ok(gd, 5.0)  # nothing ran


# --------------------------------------------------------------------------------------------------------- gather_patches
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS.get)
@pytest.mark.parametrize('name', SETS)
def test_gather_patches_matches_restatement(name, dtype):
    lib, check = _lib()
    c = R.POINT_SETS[name]
    B, H, W, Mp = c['B'], c['H'], c['W'], c['Mp']
    _, d_pix, _, pix = dev_points(name)
    for Cp in CPS:
        ldx = Cp + 8  # ldx > Cp; the slack columns hold a value no patch may show
        x = torch.full((B, H, W, ldx), 777.0, dtype=dtype)
        x[..., :Cp] = torch.randn((B, H, W, Cp), generator=gen(Cp)).to(dtype)
        xs, gd = guarded((Mp, 9, Cp), float('nan'), dtype)
        gd.fill_(-3.0)
        xd = x.cuda()
        check(lib.vkas_points_gather_patches(p(xd), ldx, Cp, B, H, W, p(d_pix), Mp, p(xs), CODE[dtype], st()),
              'points_gather_patches')
        torch.cuda.synchronize()
        assert guard_ok(gd, -3.0), (Cp, 'guard words overwritten')
        got = xs.cpu()
        assert torch.equal(got, R.gather_patches(x[..., :Cp], pix)), Cp  # no leak across rows, images or into the slack
        assert not got[torch.from_numpy(pix < 0)].any(), (Cp, 'duplicate and padding rows are zero')
        for i in np.nonzero(pix >= 0)[0]:  # border taps are zero
            y, xx = (int(pix[i]) // W) % H, int(pix[i]) % W
            out = [t for t in range(9) if not (0 <= y + t // 3 - 1 < H and 0 <= xx + t % 3 - 1 < W)]
            assert not got[i, out].any(), (Cp, i, 'border taps')


# ------------------------------------------------------------------------------------------------------------- scatter3x3
def _scatter(lib, check, D, d_pix, d_map, Mp, B, H, W, Cp, dx0, lddx, dtype):
    """one launch on a fresh copy of dx0 (B,H,W,lddx); returns the buffer on the host after checking the guard words"""
    dx, gd = guarded((B, H, W, lddx), 0.0, dtype)
    gd.fill_(-3.0)
    dx.copy_(dx0)
    check(lib.vkas_points_scatter3x3(p(D), p(d_pix), p(d_map), Mp, B, H, W, Cp, p(dx), lddx, CODE[dtype], st()),
          'points_scatter3x3')
    torch.cuda.synchronize()
    assert guard_ok(gd, -3.0), 'guard words overwritten'
    return dx.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS.get)
@pytest.mark.parametrize('name', SETS)
def test_scatter3x3_integer_operands_bit_for_bit(name, dtype):
    lib, check = _lib()
    c = R.POINT_SETS[name]
    B, H, W, Mp = c['B'], c['H'], c['W'], c['Mp']
    d_map, d_pix, pmap, pix = dev_points(name)
    keep = ~R.touched(pix, B, H, W)
    for Cp in CPS:
        lddx, g = Cp + 8, gen(7 * Cp)
        D = torch.randint(-8, 9, (Mp, 9, Cp), generator=g).float()
        D[torch.from_numpy(pix < 0)] = 1e30  # rows of duplicates and padding: only owners' rows may be read
        dx0 = torch.full((B, H, W, lddx), 123.0, dtype=dtype)  # canaries in the slack columns
        dx0[..., :Cp] = torch.randint(-8, 9, (B, H, W, Cp), generator=g).to(dtype)
        ref = R.scatter3x3(D, pix, pmap, dx0[..., :Cp])
        assert float(ref.abs().max()) <= 80 and torch.equal(ref.to(dtype).double(), ref)  # exact in the storage type
        Dd = D.cuda()
        got = _scatter(lib, check, Dd, d_pix, d_map, Mp, B, H, W, Cp, dx0.cuda(), lddx, dtype)
        assert torch.equal(got[..., :Cp], ref.to(dtype)), Cp
        assert torch.equal(_bits(got[..., Cp:]), _bits(dx0[..., Cp:])), (Cp, 'slack columns touched')
        assert torch.equal(_bits(got[keep]), _bits(dx0[keep])), (Cp, 'a pixel outside every neighbourhood changed')
        again = _scatter(lib, check, Dd, d_pix, d_map, Mp, B, H, W, Cp, dx0.cuda(), lddx, dtype)
        assert torch.equal(_bits(again), _bits(got)), (Cp, 'two runs differ')


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS.get)
@pytest.mark.parametrize('name', SETS)
def test_scatter3x3_random_operands_within_fp32_sum_bound(name, dtype):
    """fp32 sum of at most 10 terms (dx and nine taps), one rounding to T:
    |out - ref| <= eps_T |ref| + 10 * 2^-24 * sum |terms|, element by element."""
    lib, check = _lib()
    c = R.POINT_SETS[name]
    B, H, W, Mp = c['B'], c['H'], c['W'], c['Mp']
    d_map, d_pix, pmap, pix = dev_points(name)
    for Cp in CPS:
        lddx, g = Cp + 8, gen(11 * Cp)
        D = torch.randn((Mp, 9, Cp), generator=g)
        D[torch.from_numpy(pix < 0)] = 1e30
        dx0 = torch.full((B, H, W, lddx), 123.0, dtype=dtype)
        dx0[..., :Cp] = torch.randn((B, H, W, Cp), generator=g).to(dtype)
        ref = R.scatter3x3(D, pix, pmap, dx0[..., :Cp])
        mag = R.scatter3x3(D.abs(), pix, pmap, dx0[..., :Cp].abs())
        got = _scatter(lib, check, D.cuda(), d_pix, d_map, Mp, B, H, W, Cp, dx0.cuda(), lddx, dtype)
        err, bound = (got[..., :Cp].double() - ref).abs(), EPS[dtype] * ref.abs() + 10 * 2.0 ** -24 * mag
        assert torch.isfinite(got[..., :Cp]).all() and bool((err <= bound).all()), (Cp, float((err / bound).max()))
        assert torch.equal(_bits(got[..., Cp:]), _bits(dx0[..., Cp:])), (Cp, 'slack columns touched')


# ------------------------------------------------------------------------------------------------------------------- vec8
# Mp = 192: 2 * Mp threads end in the middle of a 256-thread workgroup
VEC8_CASES = [(name, Mp) for name in SETS for Mp in (64, 192) if R.POINT_SETS[name]['B'] * R.POINT_SETS[name]['P'] <= Mp]
VEC8_CASES.append(('n300_Mp320', 320))


@pytest.mark.parametrize('name,Mp', VEC8_CASES)
def test_scatter_vec8_and_gather_vec8_match_restatement(name, Mp):
    lib, check = _lib()
    c = R.POINT_SETS[name]
    M = c['B'] * c['H'] * c['W']
    _, d_pix, _, pix = dev_points(name, Mp)
    g = gen(Mp)
    own = torch.from_numpy(pix >= 0)
    # scatter: owners' rows to their pixels, duplicates and padding skipped, every other element of dst as it was
    src, dst0 = torch.randn((Mp, 8), generator=g), torch.randn((M, 8), generator=g)
    dst, gd = guarded((M, 8), 0.0, torch.float32)
    gd.fill_(-3.0)
    dst.copy_(dst0)
    src_d = src.cuda()
    check(lib.vkas_points_scatter_vec8(p(src_d), p(d_pix), Mp, p(dst), st()), 'points_scatter_vec8')
    torch.cuda.synchronize()
    assert guard_ok(gd, -3.0)
    assert torch.equal(dst.cpu(), R.scatter_vec8(src, pix, dst0))
    # gather: owners' pixels, zeros in the rows of duplicates and padding
    maps = torch.randn((M, 8), generator=g)
    rows, gr = guarded((Mp, 8), float('nan'), torch.float32)
    gr.fill_(-3.0)
    maps_d = maps.cuda()
    check(lib.vkas_points_gather_vec8(p(maps_d), p(d_pix), Mp, p(rows), st()), 'points_gather_vec8')
    torch.cuda.synchronize()
    assert guard_ok(gr, -3.0)
    assert torch.equal(rows.cpu(), R.gather_vec8(maps, pix)) and not rows.cpu()[~own].any()
    # a scatter followed by a gather reproduces the owners' rows
    back, gb = guarded((Mp, 8), float('nan'), torch.float32)
    check(lib.vkas_points_gather_vec8(p(dst), p(d_pix), Mp, p(back), st()), 'points_gather_vec8')
    torch.cuda.synchronize()
    assert torch.equal(back.cpu()[own], src[own]) and not back.cpu()[~own].any()


# ----------------------------------------------------------------------------------------------------------------- margin
@pytest.mark.parametrize('outside', [None, 'last', 'first', 'middle'], ids=['inside', 'last', 'first', 'middle'])
@pytest.mark.parametrize('n', [1, 255, 256, 257, 1000])
def test_points_margin_matches_host_minimum(n, outside):
    lib, check = _lib()
    H, W = 50, 70
    g = np.random.default_rng(n)
    py, px = g.integers(2, H - 2, n), g.integers(2, W - 2, n)
    if outside is not None:
        i = {'last': n - 1, 'first': 0, 'middle': n // 2}[outside]
        if i % 2:
            py[i] = H + 2 + i % 5
        else:
            px[i] = -3 - i % 5
    exp = R.margin(py, px, H, W)
    assert (exp < 0) == (outside is not None)
    out, gd = guarded((1,), INT_CANARY, torch.int64)
    d_py, d_px = torch.from_numpy(py).cuda(), torch.from_numpy(px).cuda()
    check(lib.vkas_points_margin(p(d_py), p(d_px), n, H, W, p(out), st()), 'points_margin')
    torch.cuda.synchronize()
    assert guard_ok(gd, INT_CANARY) and int(out[0]) == exp


# ------------------------------------------------------------------------------------------------------------ composition
@pytest.mark.parametrize('dtype', DTYPES[:2], ids=['bf16', 'f16'])
def test_heads_at_points_gradients_on_touched_pixels_within_1p5x_of_dense(dtype):
    """ops.HeadsAtPoints: every head at the points, dx = zeros + vkas_points_scatter3x3, so the points' contribution is the
    whole of dx.  Against fp64 autograd of conv3x3 -> LayerNorm -> GELU -> Linear with the cotangent masked to the points, next
    to ops.HeadsFused on the dense kernels (compact path off) with the same cotangent: dx exactly zero outside the union of
    the 3x3 neighbourhoods; on the touched pixels alone its error against fp64 within 1.5 x the dense path's, and every
    parameter gradient likewise (the criterion of tests/test_gpu_head_bwd_lowres.py).  B = 2, 24 input channels, six points
    per image with a corner, a duplicate and a 2x2 block; the 82 x 100 map is the smallest of this kind HeadsFused.eligible
    takes (B*H*W >= 16384) - a 16 x 20 map is not eligible."""
    ops = ops_mod()
    cs, ocs = (40, 33), (2, 4)
    B, Cin, H, W = 2, 24, 82, 100
    x = q(rnd((B, Cin, H, W), 50), dtype)
    convs = [(q(rnd((c, Cin, 3, 3), 51 + i, 1.0 / math.sqrt(Cin * 9)), dtype), rnd((c,), 61 + i, 0.1)) for i, c in enumerate(cs)]
    tails = [(1 + rnd((c,), 71 + i, 0.1), rnd((c,), 81 + i, 0.1), rnd((oc, c), 91 + i, 1.0 / math.sqrt(c)), rnd((oc,), 101 + i, 0.1))
             for i, (c, oc) in enumerate(zip(cs, ocs))]
    py = torch.tensor([[0, 40, 40, 7, 60, 81], [30, 30, 31, 31, 81, 5]])  # image 0: corner (0,0), one pixel twice, (81, W-1)
    px = torch.tensor([[0, 41, 41, 99, 3, 99], [50, 51, 50, 51, 0, 5]])   # image 1: a 2x2 block, the corner (81, 0)
    mask = torch.zeros((B, H, W), dtype=torch.float64)
    mask[torch.arange(B)[:, None], py, px] = 1.0
    pix = R.prepare(py.numpy(), px.numpy(), B, py.shape[1], H, W, 64)[1]
    hit = R.touched(pix, B, H, W)
    assert int(mask.sum()) == 11 and 11 * 4 < int(hit.sum()) < 11 * 9
    # fp64 reference
    xr = x.clone().requires_grad_(True)
    ref_params, ref_outs = [], []
    for (wt, b), (gm, bt, wp, bp) in zip(convs, tails):
        ps = [t.clone().requires_grad_(True) for t in (wt, b, gm, bt, wp, bp)]
        ref_params.append(ps)
        a = O.gelu(O.layer_norm_nchw(F.conv2d(xr, ps[0], ps[1], padding=1), ps[2], ps[3]))
        ref_outs.append(O.linear_nchw(a, ps[4], ps[5]))
    cots = [rnd(tuple(o.shape), 111 + i) * mask[:, None] for i, o in enumerate(ref_outs)]
    sum((o * c).sum() for o, c in zip(ref_outs, cots)).backward()
    assert not xr.grad.permute(0, 2, 3, 1)[~hit].any()
    pyc, pxc = py.cuda(), px.cuda()

    def run(at_points):
        xa = to_act(x, dtype).requires_grad_(True)
        dev = [[t.float().cuda().requires_grad_(True) for t in (wt, b, gm, bt, wp, bp)] for (wt, b), (gm, bt, wp, bp) in zip(convs, tails)]
        fused = [t for head in dev for t in head]
        if at_points:
            outs = ops.HeadsAtPoints.apply(xa, pyc, pxc, *fused)
        else:
            assert ops.HeadsFused.eligible(xa, cs, ocs)
            outs = ops.HeadsFused.apply(xa, True, *fused)
        loss = 0
        for o, oc, c in zip(outs, ocs, cots):
            loss = loss + (o[..., :oc].permute(0, 3, 1, 2) * c.float().cuda()).sum()
        loss.backward()
        torch.cuda.synchronize()
        dx = xa.grad.cpu()
        errs = {'dx (touched pixels)': rel_err(dx[hit][:, :Cin], xr.grad.permute(0, 2, 3, 1)[hit])}
        for hi, (ps, rs) in enumerate(zip(dev, ref_params)):
            for n, pp, r in zip(('conv w', 'conv b', 'gamma', 'beta', 'proj w', 'proj b'), ps, rs):
                errs['head %d %s' % (hi, n)] = rel_err(pp.grad, r.grad)
        return dx, errs

    old = ops._POINT_SPARSE
    ops._POINT_SPARSE = False
    try:
        _, e_dense = run(False)
    finally:
        ops._POINT_SPARSE = old
    dx, e_pts = run(True)
    assert not dx[~hit].any(), 'dx is not exactly zero outside the 3x3 neighbourhoods of the points'
    assert not dx[..., Cin:].any()
    for n in e_pts:
        print('%-20s points %.3e  dense %.3e  ratio %.2f' % (n, e_pts[n], e_dense[n], e_pts[n] / max(e_dense[n], 1e-300)))
    for n in e_pts:
        assert e_pts[n] <= 1.5 * e_dense[n], (n, e_pts[n], e_dense[n])
