"""Settles on the host, before any GPU run, that tests/test_gpu_gemm.py can be trusted:
  1. its fp64 restatements (im2col in the (ky, kx, c) order of include/vkas.h, every epilogue, the PATCH scatter, the weight
     gradient) equal F.conv2d / F.conv_transpose2d / autograd / plain torch math on the same operands;
  2. every exact case of its tables meets the two conditions bit-exactness rests on: every stored value an integer of magnitude
     <= 256 (representable in bf16 and f16, so a one-term error cannot hide in a rounding) and sum |a||b| + |bias| < 2^24;
  3. its bounds leave room: a float32 emulation of every random case (fp32 accumulation in 64-wide steps, forward and reversed,
     the kernel's roundings, GELU / GELU' shifted by their documented error with the worst sign per element) passes the very
     comparison functions the GPU file uses, and the headroom is printed;
  4. those comparison functions can fail: each rejects a reference computed with one deliberate mistake.  No wrong kernel is
     built or run; the mistakes are made in the reference."""
import math

import pytest
import torch
from torch.nn import functional as F

from tests import test_gpu_gemm as G
from tests.test_gpu_gemm import NT, TN, DT, U, q

ALL_NT = list(dict.fromkeys(c for bm, bn in ((128, 128), (256, 128), (256, 192), (256, 224)) for c in G.nt_cases(bm, bn)))


def test_tables():
    G.test_case_tables_cover_every_form_and_mode()
    assert 100 < len(ALL_NT) < 200 and 15 < len(G.TN_CASES) < 30


# ------------------------------------------------------------------------------------------------------- 1. restatement
def _nchw(x, c):
    return x.view(c.B, c.H, c.W, c.Cp).permute(0, 3, 1, 2)


def _w_nchw(w, c):
    k = G.geom(c)['k']
    return w.view(c.Np, k, k, c.Cp).permute(0, 3, 1, 2)  # (Np, KH, KW, Cp) -> (N, C, KH, KW)


@pytest.mark.parametrize('c', [NT('pw', 2, 3, 5, 16, 24, 'none', (1,)), NT('s3', 2, 3, 256, 8, 16, 'none', (1,)), NT('c3', 2, 7, 5, 24, 16, 'none', (1,)),
                               NT('p2', 2, 6, 10, 16, 24, 'none', (1,)), NT('p4', 1, 8, 12, 8, 16, 'none', (1,))], ids=G.cid)
def test_im2col_and_wgrad_restate_conv2d(c):
    gg, o = G.geom(c), G.nt_operands(c, 'random', 'f32')
    x = _nchw(o['x'], c).clone().requires_grad_(True)
    w = _w_nchw(o['w'], c).clone().requires_grad_(True)
    y = F.conv2d(x, w, o['bias'], stride=gg['s'], padding=gg['p'])
    ref = G.nt_reference(c, o, 'f32')['out'][0]
    assert torch.allclose(ref, y.permute(0, 2, 3, 1).reshape(gg['M'], c.Np), rtol=0, atol=1e-6)  # ref is rounded to fp32
    t = TN(c.geo, c.B, c.H, c.W, c.Cp, c.Np, 'gb')
    ot = G.tn_operands(t, 'random', 'f32')
    y2 = F.conv2d(_nchw(ot['x'], t), w, o['bias'].clone().requires_grad_(True), stride=gg['s'], padding=gg['p'])
    gw, = torch.autograd.grad(y2, w, ot['dy'].view(c.B, gg['Ho'], gg['Wo'], c.Np).permute(0, 3, 1, 2))
    r = G.tn_reference(t, ot, 'f32')
    assert torch.allclose(r['gw'][0] - ot['gw0'], gw.permute(0, 2, 3, 1).reshape(c.Np, gg['K']), rtol=0, atol=1e-9)
    assert torch.allclose(r['gb'][0] - ot['gb0'], ot['dy'].sum(0), rtol=0, atol=1e-12)


def test_epilogues_restate_torch_math():
    x = torch.linspace(-6, 6, 1001, dtype=torch.float64).requires_grad_(True)
    ge = F.gelu(x)
    assert torch.allclose(G.gelu64(x.detach()), ge.detach(), rtol=0, atol=1e-14)
    assert torch.allclose(G.dgelu64(x.detach()), torch.autograd.grad(ge.sum(), x)[0], rtol=0, atol=1e-14)
    for mode, opt in (('gelu', ()), ('sres', (1, 1, 5)), ('sres', (0, 0, 5)), ('dgelu', ()), ('add', ())):
        c = NT('pw', 1, 1, 23, 16, 24, mode, opt)
        o = G.nt_operands(c, 'random', 'f32')
        v = q(o['x'] @ o['w'].T + (o['bias'] if o['bias'] is not None else 0.0), torch.float32)
        r = G.nt_reference(c, o, 'f32')
        if mode == 'gelu':
            assert torch.equal(r['out'][0], v) and torch.allclose(r['out2'][0], F.gelu(v), rtol=0, atol=1e-14)
        elif mode == 'sres':
            rs = o['rs'].repeat_interleave(5)[:23, None] if opt[1] else 1.0
            assert torch.allclose(r['out'][0], o['aux'] + rs * o['cs'] * v, rtol=0, atol=1e-14) and ('out2' in r) == bool(opt[0])
        elif mode == 'dgelu':
            h = o['aux'].clone().requires_grad_(True)
            assert torch.allclose(r['out'][0], torch.autograd.grad(F.gelu(h), h, v)[0], rtol=0, atol=1e-13)
        else:
            assert torch.equal(r['out'][0], v + o['aux'])


def test_patch_restates_conv_transpose2d():
    """The PATCH epilogue is the input gradient of a 2x2 / stride 2 patchify: rows (b, y, x), columns (ky, kx, c)."""
    c = NT('pw', 2, 3, 5, 16, 4 * 8, 'patch', (8,))
    o = G.nt_operands(c, 'random', 'f32')
    o['bias'] = None
    got = G.nt_reference(c, o, 'f32')['out'][0].view(c.B, 2 * c.H, 2 * c.W, 8).permute(0, 3, 1, 2)
    wt = o['w'].view(2, 2, 8, c.Cp).permute(3, 2, 0, 1)  # Bw[(ky, kx, co)][ci] -> conv_transpose2d weight (Cin, Cout, KH, KW)
    ref = F.conv_transpose2d(_nchw(o['x'], c), wt, stride=2)
    assert torch.allclose(got, ref, rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------------------- 2. exact-case preconditions
def _is_int_le(t, lim):
    return bool((t == t.round()).all()) and float(t.abs().max()) <= lim


@pytest.mark.parametrize('c', ALL_NT, ids=G.cid)
def test_exact_forward_preconditions(c):
    o = G.nt_operands(c, 'exact', 'bf16')
    A = G.im2col(o['x'], c)
    acc = A @ o['w'].T
    v = acc + o['bias'] if o['bias'] is not None else acc
    mag = A.abs() @ o['w'].abs().T + (o['bias'].abs() if o['bias'] is not None else 0.0)
    assert float(mag.max()) < 2 ** 24
    assert _is_int_le(v, 256) and _is_int_le(acc, 256)
    peak = float(v.abs().max())
    for dt in ('bf16', 'f16'):
        for name, (rv, allow) in G.nt_reference(c, G.nt_operands(c, 'exact', dt), dt).items():
            if allow is None:  # every output that is compared bit for bit
                assert _is_int_le(rv, 256), (name, float(rv.abs().max()))
                assert torch.equal(q(rv, DT[dt]), rv)
                peak = max(peak, float(rv.abs().max()))
    print('exact %-40s max sum |a||b| + |bias| %6d   largest stored value %4d' % (G.cid(c), int(mag.max()), int(peak)))


@pytest.mark.parametrize('c', G.TN_CASES, ids=G.cid)
def test_exact_wgrad_preconditions(c):
    for dt in ('bf16', 'f16'):
        o, ref = G.tn_case_data(c, 'exact', dt)
        A = G.im2col(o['x'], c)
        if c.entry == 'gelu':
            assert set(A.unique().tolist()) <= {0.0, 4.0}
            A = q(G.gelu64(A), DT[dt])
            assert set(A.unique().tolist()) <= {0.0, 4.0}, 'round_T(gelu(4)) must be 4'
            assert abs(float(G.gelu64(torch.tensor(4.0, dtype=torch.float64))) - 4.0) + G.GELU_ERR < 0.25 * U[dt] * 4  # far from the rounding boundary
        assert float((o['dy'].abs().T @ A.abs() + o['gw0'].abs()).max()) < 2 ** 24
        for name, (rv, _) in ref.items():
            assert _is_int_le(rv, 256), (name, float(rv.abs().max()))
    print('exact %-36s largest |gw| %4d' % (G.cid(c), int(ref['gw'][0].abs().max())))


# ------------------------------------------------------------------------------------------------ 3. room under the bounds
def _acc32(A, Bt, reverse, step=64):
    """fp32 accumulation over the reduction axis in `step`-wide pieces, in order or reversed."""
    acc = torch.zeros((A.shape[0], Bt.shape[0]), dtype=torch.float32)
    ks = list(range(0, A.shape[1], step))
    for k0 in (reversed(ks) if reverse else ks):
        acc += A[:, k0:k0 + step] @ Bt[:, k0:k0 + step].T
    return acc


def _worst_shift(exact64, err, ref64, T, scale=None):
    """round_T(value shifted by +-err), per element the sign that lands further from the reference."""
    a = exact64 + err if scale is None else (exact64 + err) * scale
    b = exact64 - err if scale is None else (exact64 - err) * scale
    a, b = a.float().to(T), b.float().to(T)
    return torch.where((a.double() - ref64).abs() >= (b.double() - ref64).abs(), a, b)


def emulate_nt(c, o, dt, reverse, err_scale=1.0):
    """What a correct kernel returns, to fp32 arithmetic: the outputs as tensors of the storage type."""
    T, gg = DT[dt], G.geom(c)
    gelu_err, dgelu_err = G.GELU_ERR * err_scale, G.DGELU_ERR * err_scale
    acc = _acc32(G.im2col(o['x'], c).float(), o['w'].float(), reverse)
    v = (acc + o['bias'].float() if o['bias'] is not None else acc).to(T)
    err16 = dt != 'f32'  # fp32 storage keeps the exact erf forms
    if c.mode == 'none':
        return {'out': v}
    if c.mode == 'gelu':
        g = G.gelu64(v.double())
        out2 = _worst_shift(g, (gelu_err if err16 else 0.0) * (v != 0), g, T)  # gelu(0) = 0 exactly in the kernel's form (x * cdf)
        return {'out': v, 'out2': out2, 'out2_nokeep': out2}
    if c.mode == 'sres':
        rs = o['rs'][torch.arange(gg['M']) // c.opt[2]][:, None].float() if c.opt[1] else 1.0
        r = {'out': (o['aux'].float() + rs * o['cs'].float()[None, :] * v.float()).to(T)}
        if c.opt[0]:
            r['out2'] = v
        return r
    if c.mode == 'dgelu':
        ref = q(v.double(), T) * G.dgelu64(o['aux'])
        return {'out': _worst_shift(G.dgelu64(o['aux']), dgelu_err if err16 else 0.0, ref, T, scale=v.double())}
    if c.mode == 'add':
        return {'out': (v.float() + o['aux'].float()).to(T)}
    return {'out': G.patch_scatter(v.double(), c).to(T)}


def emulate_tn(c, o, dt, reverse, sign=1.0):
    T = DT[dt]
    A = G.im2col(o['x'], c)
    if c.entry == 'gelu':
        A = q(G.gelu64(A) + sign * (G.GELU_ERR if dt != 'f32' else 0.0) * (A != 0), T)
    r = {'gw': (o['gw0'].float() + _acc32(o['dy'].T.float().contiguous(), A.T.float().contiguous(), reverse))}
    if c.entry in ('gb', 'gelu'):
        r['gb'] = o['gb0'].float() + _acc32(o['dy'].T.float().contiguous(), torch.ones((1, A.shape[0])), reverse)[:, 0]
    return r


def _headroom(tag):
    rows = {k: v for k, v in G._WORST.items() if k[0] == tag}
    for (_, mode, dt), (value, bound, what) in sorted(rows.items(), key=lambda kv: (kv[0][2], kv[0][1])):
        print('emulation %-4s %-48s %.3e / %.3e  (factor %8.3g to spare) at %s' % (dt, mode, value, bound, bound / max(value, 1e-300), what))
    return rows


def test_forward_bounds_leave_room():
    """Every random forward case, all three storage types, both accumulation orders, through the GPU file's own comparison."""
    for c in ALL_NT:
        for dt in ('bf16', 'f16', 'f32'):
            o = G.nt_case_data(c, 'random', dt)
            for reverse in (False, True):
                G.compare_nt(c, 'random', dt, emulate_nt(c, o, dt, reverse), form='emu-nt')
    rows = _headroom('emu-nt')
    assert rows and all(bound / max(value, 1e-300) > 1.5 for value, bound, _ in rows.values())


def test_exact_transcendental_bounds_leave_room():
    """The integer cases' GELU / GELU' outputs at |diff| <= error + u |ref|, with the error pushed to its worst sign.  The bound
    is first order in its two errors (round_T(g + e) is within u |g + e| of g + e, and the product u e is dropped), so the
    emulation shifts by e (1 - 2 u): the bound holds for every polynomial error up to 99.2 % of the documented maximum, at
    every integer v of the table, with the rounding falling the worst way."""
    for c in [c for c in ALL_NT if c.mode in ('gelu', 'dgelu')]:
        for dt in ('bf16', 'f16', 'f32'):
            G.compare_nt(c, 'exact', dt, emulate_nt(c, G.nt_case_data(c, 'exact', dt), dt, False, 1 - 2 * U[dt]), form='emu-exact')
    rows = _headroom('emu-exact')
    assert rows and all(value <= 1.0 for value, bound, _ in rows.values())


def test_wgrad_bounds_leave_room():
    for c in G.TN_CASES:
        for dt in ('bf16', 'f16', 'f32'):
            o, _ = G.tn_case_data(c, 'random', dt)
            for reverse in (False, True):
                for sign in ((1.0, -1.0) if c.entry == 'gelu' else (1.0,)):
                    G.compare_tn(c, 'random', dt, emulate_tn(c, o, dt, reverse, sign), form='emu-tn')
    rows = _headroom('emu-tn')
    assert rows and all(bound / max(value, 1e-300) > 1.5 for value, bound, _ in rows.values())


# ------------------------------------------------------------------------------------------- 4. the comparisons can fail
def _with_im2col(fn):
    """nt_reference / tn_reference with another im2col."""
    def ref(c, o, dt, *stored):
        keep = G.im2col
        G.im2col = fn
        try:
            return (G.nt_reference if isinstance(c, NT) else G.tn_reference)(c, o, dt, *stored)
        finally:
            G.im2col = keep
    return ref


_IM2COL = G.im2col


def _drop_k_term(x, c):
    A = _IM2COL(x, c).clone()
    A[:, A.shape[1] // 2 + 3] = 0.0
    return A


def _kx_reversed(x, c):
    k = G.geom(c)['k']
    A = _IM2COL(x, c).view(-1, k, k, c.Cp)
    return A.flip(2).reshape(A.shape[0], -1)


def _left_halo_is_first_pixel(x, c):
    gg = G.geom(c)
    A = _IM2COL(x, c).clone().view(c.B, gg['Ho'], gg['Wo'], 3, 3, c.Cp)
    A[:, :, 0, :, 0] = A[:, :, 0, :, 1]  # output column 0: the kx = 0 tap reads pixel 0 instead of the zero padding
    return A.reshape(gg['M'], gg['K'])


def _ld_ignored(x, c):
    wide = torch.full((x.shape[0] + 1, c.Cp + G.EXTRA), G.NEIGHBOUR, dtype=torch.float64)
    wide[:x.shape[0], G.OFF:G.OFF + c.Cp] = x
    return _IM2COL(wide.reshape(-1)[G.OFF:G.OFF + x.numel()].view(x.shape), c)


def _last_column_zeroed(c, o, dt, *stored):
    r = {k: (v.clone(), a) for k, (v, a) in G.nt_reference(c, o, dt, *stored).items()}
    for v, _ in r.values():
        v[:, G.n_real(c) - 1] = 0.0
    return r


def _rpi_off_by_one(c, o, dt, *stored):
    return G.nt_reference(c._replace(opt=(c.opt[0], c.opt[1], c.opt[2] + 1)), o, dt, *stored)


def _gw_overwritten(c, o, dt):
    return G.tn_reference(c, dict(o, gw0=torch.zeros_like(o['gw0'])), dt)


def _patch_swapped(c, o, dt, *stored):
    v = G.nt_reference(c._replace(mode='none', opt=(1,)), o, dt)['out'][0]
    pc = c.opt[0]
    t = v.view(c.B, c.H, c.W, 2, 2, pc).permute(0, 1, 4, 2, 3, 5)  # b, y, kx, x, ky, c: ky and kx swapped
    return {'out': (t.reshape(-1, pc), None)}


def _pick(table, **want):
    """The first case of the GPU file's table with these fields."""
    return next(c for c in table if all(getattr(c, k) == v for k, v in want.items()))


S3 = _pick(ALL_NT, geo='s3', mode='none', Cp=136, Np=232)
PW = _pick(ALL_NT, geo='pw', mode='none', W=257, Np=232)
MISTAKES = [
    # name, case, wrong reference, also caught on random data (a single K term of 1224 is below every rounding bound: that is
    # what the exact cases are for)
    ('one K term dropped', S3, _with_im2col(_drop_k_term), False),
    ('one K term dropped (wgrad)', _pick(G.TN_CASES, geo='c3', entry='gb'), _with_im2col(_drop_k_term), True),
    ('kx taps reversed', _pick(ALL_NT, geo='c3', mode='none'), _with_im2col(_kx_reversed), True),
    ('kx taps reversed (wgrad)', _pick(G.TN_CASES, geo='c3', entry='nogb'), _with_im2col(_kx_reversed), True),
    ('left halo pixel = first pixel of the tile', S3, _with_im2col(_left_halo_is_first_pixel), True),
    ('ld ignored', PW, _with_im2col(_ld_ignored), True),
    ('ld ignored (wgrad)', _pick(G.TN_CASES, geo='pw', W=257), _with_im2col(_ld_ignored), True),
    ('last N column of a ragged tile zeroed', PW, _last_column_zeroed, True),
    ('rows_per_image off by one', _pick(ALL_NT, geo='pw', mode='sres', opt=(1, 1, 49), Np=232), _rpi_off_by_one, True),
    ('gw overwritten', _pick(G.TN_CASES, geo='pw', W=1137, entry='gb'), _gw_overwritten, True),
    ('PATCH ky and kx swapped', _pick(ALL_NT, geo='pw', mode='patch', Np=256), _patch_swapped, True),
]


@pytest.mark.parametrize('name,c,wrong,on_random', MISTAKES, ids=[m[0] for m in MISTAKES])
def test_comparisons_reject_a_wrong_reference(name, c, wrong, on_random):
    """got = what a right kernel returns (the exact reference / the fp32 emulation); reference = one with the mistake."""
    nt = isinstance(c, NT)
    assert c in (ALL_NT if nt else G.TN_CASES), 'a shape of the GPU file\'s table'
    cmp, emu = (G.compare_nt, emulate_nt) if nt else (G.compare_tn, emulate_tn)
    for dt in ('bf16', 'f16'):
        for kind in G.KINDS:
            o = G.nt_case_data(c, kind, dt) if nt else G.tn_case_data(c, kind, dt)[0]
            got = emu(c, o, dt, False)
            cmp(c, kind, dt, got)  # the right reference accepts it
            if kind == 'exact' or on_random:
                with pytest.raises(AssertionError):
                    cmp(c, kind, dt, got, ref_fn=wrong)
