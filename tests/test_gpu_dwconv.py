"""Direct parity of the five depthwise 7x7 kernels of csrc/dwconv.hip, through the C ABI (vkas_dwconv7x7_fwd,
vkas_dwconv7x7_wgrad, vkas_pack_dw_weight, vkas_unpack_dw_wgrad) with ctypes, so pixel strides, workspaces and output modes are
the test's own.

Reference everywhere: F.conv2d(x, w, b, padding=3, groups=C) in fp64 on the host and its autograd, on the values the kernels
see (activations and depthwise weights rounded to the storage type first, bias fp32).  With the operands pre-rounded the only
differences from fp64 are fp32 accumulation and one output rounding, so the bounds are the single-op table of test_gpu_ops
(TOL: 2e-5 / 4e-3 / 6e-4 norm-wise, 1e-4 / 2e-2 / 4e-3 of the peak).  A host emulation (fp32 convolution of the rounded
operands, rounded once, against fp64) gives 6e-8 / 1.7e-3 / 2.1e-4 norm-wise and 2.7e-3 / 3.4e-4 of the peak (bf16 / f16) on these
cases: the table leaves a factor 2.4 - 2.9 over what the formats alone cost.

The case table is chosen from the dispatch arithmetic of the matrix-core kernels (persistent walkers over 16 x 32 tiles): the
expected tile / walker counts are asserted from the geometry and checked against vkas_dwconv7x7_wgrad_parts, so a retuned
dispatch cannot silently turn a many-tiles-per-walker case into a one-tile case.
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import pytest
import torch
from torch.nn import functional as F

from tests import parity_log
from tests.helpers import rel_err
from tests.test_gpu_ops import DTYPES, TOL, close, q, rnd

pytestmark = pytest.mark.gpu

IDS = {torch.float32: 'f32', torch.bfloat16: 'bf16', torch.float16: 'f16'}
CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}  # VKAS_F32 / VKAS_BF16 / VKAS_F16

# (B, C, H, W) -> matrix-core geometry (spatial tiles, walkers, most tiles of one walker, idle walkers), derived by hand
CASES = {
    (2, 96, 100, 200): (98, 80, 2, 0),    # some walkers do 2 tiles, some 1; ragged H (4 rows) and W (8 columns)
    (3, 768, 40, 70): (27, 8, 4, 0),      # 48 slices, 3 - 4 tiles per walker, walks cross image boundaries
    (2, 96, 256, 256): (256, 80, 4, 0),   # stage-0 shape of the benchmark
    (1, 128, 256, 192): (96, 64, 2, 0),   # Base width
    (1, 33, 37, 53): (6, 8, 1, 2),        # Cp = 40: the last slice has one 8-channel chunk, 7 pad channels
    (2, 24, 130, 33): (36, 40, 1, 4),     # a second tile column one pixel wide; fp32: 17 y tiles, a last group of one
    (1, 1536, 17, 9): (2, 8, 1, 6),       # 96 slices (walker count at its floor), second tile row one pixel high
    (2, 200, 45, 97): (24, 24, 1, 0),     # Cp = 200: 13 slices, half-empty last slice, odd everything
    (1, 16, 1, 1): (1, 8, 1, 7),          # maps smaller than the kernel: every tap but the centre is padding somewhere
    (2, 16, 3, 70): (6, 8, 1, 2),
    (1, 16, 7, 7): (1, 8, 1, 7),
    (1, 192, 16, 32): (1, 8, 1, 7),       # exact tile multiples, no ragged edge
    (1, 192, 32, 64): (4, 8, 1, 4),
}
STRUCTURED = [(2, 96, 100, 200), (1, 33, 37, 53)]
REPEAT = [(3, 768, 40, 70), (2, 96, 256, 256)]
AB_CASES = [(2, 96, 100, 200), (1, 33, 37, 53)]
GUARD = 4096          # floats behind the workspace that no launch may touch
SENTINEL = -12352.0   # exact in all three storage types, far outside every output here

_WORST = {}


def cdiv(a, b):
    return (a + b - 1) // b


def cp_of(C):
    return cdiv(C, 8) * 8


def mfma_geometry(B, C, H, W):
    """Python copy of dw_mfma_walkers (dwconv.hip): (spatial tiles, walkers, most tiles of one walker, idle walkers)."""
    slices = cdiv(cp_of(C), 16)
    tiles = cdiv(W, 32) * cdiv(H, 16) * B
    walkers = max(8, (512 // slices) // 8 * 8)
    if walkers > tiles:
        walkers = cdiv(tiles, 8) * 8
    return tiles, walkers, cdiv(tiles, walkers), max(0, walkers - tiles)


def valu_parts(B, H, W):
    """Partial rows of dwconv7x7_wgrad_kernel: tiles of 8 x 32, 4 y tiles per workgroup."""
    return B * cdiv(cdiv(H, 8), 4) * cdiv(W, 32)


def vk():
    from vkit_ocr_model_adaptive_scaling_amd import _lib
    return _lib.lib


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def slab(t64, dtype, width, off=8, fill=0.0, pad_fill=None):
    """(B, C, H, W) fp64 host tensor -> channels [off, off + Cp) of a (B, H, W, width) device buffer filled with ``fill``; pad
    channels C..Cp are zero unless pad_fill is given.  Returns (buffer, view of the slice)."""
    B, C, H, W = t64.shape
    Cp = cp_of(C)
    assert off % 8 == 0 and width % 8 == 0 and off + Cp <= width
    buf = torch.full((B, H, W, width), fill, dtype=dtype, device='cuda')
    view = buf[..., off:off + Cp]
    view[..., C:] = 0.0 if pad_fill is None else pad_fill
    view[..., :C] = t64.permute(0, 2, 3, 1).to(dtype).cuda()
    return buf, view


def unslab(view, C):
    return view[..., :C].permute(0, 3, 1, 2).double().cpu()


def pack_weight(w64, C, flip):
    lib = vk()
    Cp = cp_of(C)
    wd = w64.float().cuda().contiguous()
    out = torch.full((lib.vkas_dw_weight_elems(Cp),), float('nan'), device='cuda')
    assert lib.vkas_pack_dw_weight(wd.data_ptr(), out.data_ptr(), C, Cp, flip, stream()) == 0
    return out


def pad_vec(v64, Cp):
    out = torch.zeros((Cp,), device='cuda')
    out[:v64.numel()] = v64.float().cuda()
    return out


def run_fwd(x64, w64, b64, add64, dtype, flip, add_pad=None):
    """One vkas_dwconv7x7_fwd call with x, addend and y as channel slices of wider buffers with different pixel strides
    (Cp + 8, Cp + 24, Cp + 16).  Checks what holds for every call: columns of the y buffer outside the slice bit-unchanged,
    every element inside written and finite, pad channels exactly 0 (or exactly the addend's).  Returns y as (B, C, H, W) fp64."""
    lib = vk()
    B, C, H, W = x64.shape
    Cp = cp_of(C)
    _, xv = slab(x64, dtype, Cp + 8)
    ybuf = torch.full((B, H, W, Cp + 16), SENTINEL, dtype=dtype, device='cuda')
    yv = ybuf[..., 8:8 + Cp]
    before = ybuf.clone()
    wp = pack_weight(w64, C, flip)
    bias = pad_vec(b64, Cp) if b64 is not None else None
    av = None
    if add64 is not None:
        _, av = slab(add64, dtype, Cp + 24, pad_fill=add_pad)
    rc = lib.vkas_dwconv7x7_fwd(xv.data_ptr(), Cp + 8, wp.data_ptr(), bias.data_ptr() if bias is not None else None,
                                av.data_ptr() if av is not None else None, Cp + 24 if av is not None else 0,
                                yv.data_ptr(), Cp + 16, B, H, W, Cp, CODE[dtype], stream())
    assert rc == 0, vk().vkas_last_error()
    torch.cuda.synchronize()
    outside = [i for i in range(Cp + 16) if not 8 <= i < 8 + Cp]
    assert torch.equal(bits(ybuf)[..., outside], bits(before)[..., outside]), 'columns outside the y slice were written'
    assert torch.isfinite(yv).all() and not (yv == SENTINEL).any(), 'an element of y was not written'
    if Cp > C:
        if av is None:
            assert float(yv[..., C:].float().abs().max()) == 0.0, 'pad channels of y must be exactly 0'
        else:
            assert torch.equal(bits(yv[..., C:].contiguous()), bits(av[..., C:].contiguous())), 'pad channels of y must be the addend\'s'
    return unslab(yv, C)


def run_wgrad(x64, dy64, dtype, mode):
    """One vkas_dwconv7x7_wgrad call (x and dy slices with pixel strides Cp + 8 / Cp + 24; workspace of exactly
    vkas_dwconv7x7_wgrad_ws_bytes floats, NaN-filled, a guard block behind it).  mode 'fused': gb == gw + 49 Cp, 'split': gw
    and gb in separate tensors, 'parts': gw = gb = NULL and the partial rows summed in fp64 here.  Returns (gw [49][Cp], gb [Cp])
    as device tensors (fp32 for the first two modes, fp64 for 'parts')."""
    lib = vk()
    B, C, H, W = x64.shape
    Cp = cp_of(C)
    _, xv = slab(x64, dtype, Cp + 8)
    _, dv = slab(dy64, dtype, Cp + 24)
    nbytes = lib.vkas_dwconv7x7_wgrad_ws_bytes(B, H, W, Cp)
    assert nbytes % 4 == 0 and nbytes > 0
    ws = torch.full((nbytes // 4 + GUARD,), float('nan'), device='cuda')
    ws[nbytes // 4:] = 7.25
    nan = float('nan')
    if mode == 'fused':
        gwb = torch.full((50 * Cp,), nan, device='cuda')
        gw, gb = gwb[:49 * Cp], gwb[49 * Cp:]
    elif mode == 'split':
        gw, gb = torch.full((49 * Cp,), nan, device='cuda'), torch.full((Cp,), nan, device='cuda')
    else:
        gw = gb = None
    rc = lib.vkas_dwconv7x7_wgrad(xv.data_ptr(), Cp + 8, dv.data_ptr(), Cp + 24, gw.data_ptr() if gw is not None else None,
                                  gb.data_ptr() if gb is not None else None, ws.data_ptr(), nbytes, B, H, W, Cp, CODE[dtype],
                                  stream())
    assert rc == 0, vk().vkas_last_error()
    torch.cuda.synchronize()
    assert float((ws[nbytes // 4:] - 7.25).abs().max()) == 0.0, 'the launch wrote behind its workspace'
    if mode == 'parts':
        parts = lib.vkas_dwconv7x7_wgrad_parts(B, H, W, Cp, CODE[dtype])
        assert 0 < parts * 50 * Cp * 4 <= nbytes
        rows = ws[:parts * 50 * Cp].view(parts, 50 * Cp)
        assert torch.isfinite(rows).all(), 'a partial row was not written (NaN left in the workspace)'
        tot = rows.double().sum(0)
        gw, gb = tot[:49 * Cp], tot[49 * Cp:]
    assert torch.isfinite(gw).all() and torch.isfinite(gb).all(), 'weight / bias gradient not fully written'
    if Cp > C:
        assert float(gw.view(49, Cp)[:, C:].abs().max()) == 0.0 and float(gb[C:].abs().max()) == 0.0, 'pad channels must be 0'
    return gw.view(49, Cp), gb


def unpack(gw, C, accumulate_onto=None):
    """vkas_unpack_dw_wgrad: [49][Cp] -> (C, 49); overwrite mode into a NaN-filled tensor, or accumulate onto a copy."""
    lib = vk()
    Cp = gw.shape[1]
    grad = torch.full((C, 49), float('nan'), device='cuda') if accumulate_onto is None else accumulate_onto.clone()
    gwf = gw.float().contiguous()
    assert lib.vkas_unpack_dw_wgrad(gwf.data_ptr(), grad.data_ptr(), C, Cp, 0 if accumulate_onto is None else 1, stream()) == 0
    torch.cuda.synchronize()
    return grad


_REF = {}


def operands(case, dtype):
    """What the kernels see, as fp64: activations and depthwise weights rounded to the storage type, bias fp32."""
    C = case[1]
    return {'x': q(rnd(case, 31), dtype), 'w': q(rnd((C, 1, 7, 7), 32, 0.15), dtype), 'b': rnd((C,), 33, 0.1).float().double(),
            'dy': q(rnd(case, 34), dtype), 'add': q(rnd(case, 35), dtype)}


def reference(case, dtype):
    """Operands (rounded to the storage type, kept in it: exact) and the fp64 reference of one case, computed once per
    (case, dtype) and shared by the forward, gradient, repeatability and A/B tests.  The parametrised module fixture below keeps
    the tests of one (case, dtype) together, so only the latest entry is kept, next to those the later tests come back to."""
    key = (case, dtype)
    if key not in _REF:
        B, C, H, W = case
        o = operands(case, dtype)
        xr, wr, br = (o[k].clone().requires_grad_(True) for k in ('x', 'w', 'b'))
        y = F.conv2d(xr, wr, br, padding=3, groups=C)
        y.backward(o['dy'])
        for k in [k for k in _REF if not (k[1] == torch.bfloat16 and k[0] in REPEAT + AB_CASES)]:
            del _REF[k]
        _REF[key] = {'x': o['x'].to(dtype), 'w': o['w'], 'b': o['b'], 'dy': o['dy'].to(dtype), 'add': o['add'].to(dtype),
                     'y': y.detach(), 'dx': xr.grad, 'gw': wr.grad.reshape(C, 49), 'gb': o['dy'].sum((0, 2, 3))}
    r = dict(_REF[key])
    for k in ('x', 'dy', 'add'):
        r[k] = r[k].double()
    return r


@pytest.fixture(scope='module', params=[(c, d) for c in CASES for d in DTYPES],
                ids=lambda p: '%s-%s' % ('x'.join(map(str, p[0])), IDS[p[1]]))
def cd(request):
    return request.param


@pytest.fixture(scope='module', autouse=True)
def worst_rows():
    yield
    for (what, dtype), (v, case) in sorted(_WORST.items(), key=lambda kv: (kv[0][0], IDS[kv[0][1]])):
        parity_log.record('test_gpu_dwconv', 'worst %s, %s' % (what, IDS[dtype]), v, TOL[dtype][0], 'at ' + 'x'.join(map(str, case)))


def measure(what, case, dtype, actual, expected):
    r = rel_err(actual, expected)
    print('dwconv %-15s %-18s %-4s norm-wise %.3e  max abs / peak %.3e' % (
        what, 'x'.join(map(str, case)), IDS[dtype], r,
        float((actual.double().cpu() - expected).abs().max()) / max(float(expected.abs().max()), 1e-30)))
    parity_log.record('test_gpu_dwconv', '%s %s %s' % (what, 'x'.join(map(str, case)), IDS[dtype]), r, TOL[dtype][0])
    key = (what, dtype)
    if key not in _WORST or r > _WORST[key][0]:
        _WORST[key] = (r, case)
    return r


# ------------------------------------------------------------------------------------------------------------ 1. geometry
def test_case_geometry():
    """The tile / walker numbers the case table was chosen for, from a Python copy of the dispatch formula that is itself checked
    against vkas_dwconv7x7_wgrad_parts: at least one walker with four tiles, at least one case with idle walkers."""
    lib = vk()
    most, idle_cases = 0, 0
    for case, expected in CASES.items():
        B, C, H, W = case
        geo = mfma_geometry(*case)
        assert geo == expected, (case, geo, expected)
        for code in (1, 2):
            assert lib.vkas_dwconv7x7_wgrad_parts(B, H, W, cp_of(C), code) == geo[1], case
        if 'VKAS_DW_VALU' not in os.environ:
            assert lib.vkas_dwconv7x7_wgrad_parts(B, H, W, cp_of(C), 0) == valu_parts(B, H, W), case
        ws = lib.vkas_dwconv7x7_wgrad_ws_bytes(B, H, W, cp_of(C))
        assert ws == max(geo[1], valu_parts(B, H, W)) * 50 * cp_of(C) * 4, case
        most = max(most, geo[2])
        idle_cases += geo[3] > 0
    assert most >= 4 and idle_cases >= 1
    assert mfma_geometry(3, 768, 40, 70)[2] == 4 and mfma_geometry(1, 33, 37, 53)[3] == 2
    # fp32 kernels: (2, 24, 130, 33) has 17 y tiles of 8 rows, i.e. a last group of one, and a second tile column
    assert cdiv(130, 8) == 17 and 17 % 4 == 1 and valu_parts(2, 130, 33) == 2 * 5 * 2


# ------------------------------------------------------------------------------------- 2. forward and input gradient
def test_forward_and_input_gradient(cd):
    """vkas_dwconv7x7_fwd with bias and no addend (the forward), and with flipped weights, addend and no bias (the
    input-gradient call of ConvNextLayer.backward, against autograd's dx + addend)."""
    case, dtype = cd
    r = reference(case, dtype)
    y = run_fwd(r['x'], r['w'], r['b'], None, dtype, 0)
    measure('forward', case, dtype, y, r['y'])
    close(y, r['y'], dtype, 'dw forward %s' % (case,))
    dx = run_fwd(r['dy'], r['w'], None, r['add'], dtype, 1, add_pad=1.5)
    measure('input gradient', case, dtype, dx, r['dx'] + r['add'])
    close(dx, r['dx'] + r['add'], dtype, 'dw input gradient + addend %s' % (case,))


def test_adjoint_identity_fp32():
    """<fwd(x; w), dy> == <x, fwd(dy; flip(w))> in fp32 on a multi-tile case: pins flip = 1 independently of autograd."""
    case = (2, 96, 100, 200)
    x, dy, w = rnd(case, 41).float().double(), rnd(case, 42).float().double(), rnd((96, 1, 7, 7), 43, 0.15).float().double()
    y = run_fwd(x, w, None, None, torch.float32, 0)
    dx = run_fwd(dy, w, None, None, torch.float32, 1)
    lhs, rhs = float((y * dy).sum()), float((x * dx).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), 1.0), (lhs, rhs)


def structured(case, seed):
    """One-hot weights (tap c % 49 of channel c), integer-valued input, |x| <= 64: exact in every storage type."""
    B, C, H, W = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-64, 65, case, generator=g).double()
    w = torch.zeros((C, 49), dtype=torch.float64)
    w[torch.arange(C), torch.arange(C) % 49] = 1.0
    return x, w.view(C, 1, 7, 7)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('case', STRUCTURED, ids=lambda c: 'x'.join(map(str, c)))
def test_forward_structured_exact(case, dtype):
    """The output is the input shifted by each channel's tap with zero fill: a wrong tap, a transposed band or a halo off by one
    shows as a shifted image.  Exact, so compared with ==, with the plain and with the flipped weights."""
    B, C, H, W = case
    x, w = structured(case, 51)
    for flip in (0, 1):
        ref = F.conv2d(x, w.flip(2, 3) if flip else w, None, padding=3, groups=C)
        y = run_fwd(x, w, None, None, dtype, flip)
        bad = (y != ref).reshape(B, C, -1).any(2).any(0).nonzero().flatten().tolist()
        assert not bad, 'flip %d: channels (tap = c %% 49) that differ from the shifted input: %s' % (flip, bad[:20])


# ----------------------------------------------------------------------------------------- 3. weight and bias gradient
def test_weight_and_bias_gradient(cd):
    """vkas_dwconv7x7_wgrad in its three output modes against autograd's w.grad and dy.sum((0, 2, 3)); the two finalized modes are
    bit-equal; unpack in overwrite and accumulate mode.  The operands' products are exact in fp32, so the error is fp32
    accumulation order over B * H * W terms: TOL[dtype] is the cap, the measured figure goes to the parity report."""
    case, dtype = cd
    B, C, H, W = case
    r = reference(case, dtype)
    gw_f, gb_f = run_wgrad(r['x'], r['dy'], dtype, 'fused')
    gw_s, gb_s = run_wgrad(r['x'], r['dy'], dtype, 'split')
    gw_p, gb_p = run_wgrad(r['x'], r['dy'], dtype, 'parts')
    assert torch.equal(gw_f, gw_s) and torch.equal(gb_f, gb_s), 'one finalize launch and two differ'
    got = unpack(gw_f, C)
    measure('weight gradient', case, dtype, got, r['gw'])
    measure('bias gradient', case, dtype, gb_f[:C], r['gb'])
    close(got, r['gw'], dtype, 'dw weight gradient %s' % (case,))
    close(gb_f[:C], r['gb'], dtype, 'dw bias gradient %s' % (case,))
    close(unpack(gw_p, C), r['gw'], dtype, 'dw weight gradient from the partial rows %s' % (case,))
    close(gb_p[:C], r['gb'], dtype, 'dw bias gradient from the partial rows %s' % (case,))
    base = rnd((C, 49), 36).float().cuda()
    assert torch.equal(unpack(gw_f, C, accumulate_onto=base), base + got), 'unpack, accumulate mode'


def edge_points(H, W):
    """Isolated positions within 3 pixels of the image edge and of the 16 x 32 / 8 x 32 tile edges, and a few inside."""
    pts = [(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0), (2, W - 3), (H - 3, 2), (15, 31), (16, 32), (14, 29), (18, 34), (7, 30),
           (8, 33), (31, 63), (32, 64), (H // 2, W // 2), (H // 2 + 5, 3), (45, 100), (63, 96)]
    return sorted({(y, x) for y, x in pts if 0 <= y < H and 0 <= x < W})


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('case', STRUCTURED, ids=lambda c: 'x'.join(map(str, c)))
def test_weight_gradient_structured_exact(case, dtype):
    """Integer x and a dy of a few isolated ones: every tap of the gradient is a small integer sum, exact in fp32, so tap-by-tap
    equality pins the D[i][j] -> gw[6 - i][j] mapping and the bias column."""
    B, C, H, W = case
    x, _ = structured(case, 52)
    dy = torch.zeros(case, dtype=torch.float64)
    pts = edge_points(H, W)
    for n, (py, px) in enumerate(pts):
        dy[n % B, :, py, px] = 1.0
    wr = torch.zeros((C, 1, 7, 7), dtype=torch.float64, requires_grad=True)
    F.conv2d(x, wr, None, padding=3, groups=C).backward(dy)
    ref = wr.grad.reshape(C, 49)
    for mode in ('fused', 'parts'):
        gw, gb = run_wgrad(x, dy, dtype, mode)
        got = unpack(gw, C).double().cpu()
        bad = (got != ref).nonzero().tolist()
        assert not bad, '%s: (channel, tap) that differ: %s' % (mode, bad[:20])
        assert torch.equal(gb[:C].double().cpu(), dy.sum((0, 2, 3))), mode


# ------------------------------------------------------------------------------------------------------- 4. repeatability
@pytest.mark.parametrize('case', REPEAT, ids=lambda c: 'x'.join(map(str, c)))
def test_repeatable(case):
    """Race screen for the tile loops (raw barriers, prefetch in flight over compute): none of these paths has a float atomic, so
    12 launches on the same operands agree bit for bit.  A fixed 12 launches, one pass."""
    lib = vk()
    dtype = torch.bfloat16
    B, C, H, W = case
    Cp = cp_of(C)
    r = reference(case, dtype)
    _, xv = slab(r['x'], dtype, Cp + 8)
    _, dv = slab(r['dy'], dtype, Cp + 24)
    _, av = slab(r['add'], dtype, Cp + 16)
    wp, wf, bias = pack_weight(r['w'], C, 0), pack_weight(r['w'], C, 1), pad_vec(r['b'], Cp)
    nbytes = lib.vkas_dwconv7x7_wgrad_ws_bytes(B, H, W, Cp)
    ws = torch.empty((nbytes // 4,), device='cuda')
    ys, dxs, gws = [], [], []
    for _ in range(12):
        y = torch.empty((B, H, W, Cp), dtype=dtype, device='cuda')
        dx = torch.empty_like(y)
        gwb = torch.empty((50 * Cp,), device='cuda')
        assert lib.vkas_dwconv7x7_fwd(xv.data_ptr(), Cp + 8, wp.data_ptr(), bias.data_ptr(), None, 0, y.data_ptr(), Cp, B, H, W,
                                      Cp, CODE[dtype], stream()) == 0
        assert lib.vkas_dwconv7x7_fwd(dv.data_ptr(), Cp + 24, wf.data_ptr(), None, av.data_ptr(), Cp + 16, dx.data_ptr(), Cp, B,
                                      H, W, Cp, CODE[dtype], stream()) == 0
        assert lib.vkas_dwconv7x7_wgrad(xv.data_ptr(), Cp + 8, dv.data_ptr(), Cp + 24, gwb.data_ptr(),
                                        gwb.data_ptr() + 4 * 49 * Cp, ws.data_ptr(), nbytes, B, H, W, Cp, CODE[dtype],
                                        stream()) == 0
        ys.append(y)
        dxs.append(dx)
        gws.append(gwb)
    torch.cuda.synchronize()
    for i in range(1, 12):
        assert torch.equal(bits(ys[i]), bits(ys[0])), ('forward differs between launches', i)
        assert torch.equal(bits(dxs[i]), bits(dxs[0])), ('input gradient differs between launches', i)
        assert torch.equal(bits(gws[i]), bits(gws[0])), ('weight gradient differs between launches', i)
    close(unslab(ys[0], C), r['y'], dtype, 'repeatable forward')
    close(unslab(dxs[0], C), r['dx'] + r['add'], dtype, 'repeatable input gradient')


# ------------------------------------------------------------------------------------------------------ 5. the A/B kernels
def ab_child(path):
    """Runs in a child process (the A/B switches are read once per process): bf16 forward, input gradient and weight gradient of
    AB_CASES, written to ``path``."""
    dtype = torch.bfloat16
    out = {}
    for i, case in enumerate(AB_CASES):
        B, C, H, W = case
        r = operands(case, dtype)
        out['y%d' % i] = run_fwd(r['x'], r['w'], r['b'], None, dtype, 0)
        out['dx%d' % i] = run_fwd(r['dy'], r['w'], None, r['add'], dtype, 1, add_pad=1.5)
        gw, gb = run_wgrad(r['x'], r['dy'], dtype, 'fused')
        out['gw%d' % i] = unpack(gw, C).double().cpu()
        out['gb%d' % i] = gb[:C].double().cpu()
        out['parts%d' % i] = torch.tensor([vk().vkas_dwconv7x7_wgrad_parts(B, H, W, cp_of(C), CODE[dtype])])
    torch.save(out, path)


def test_ab_kernels_against_fp64():
    """The two kernels kept for A/B runs (VKAS_DW_VALU=1: the vector-ALU kernels for 16-bit types, VKAS_DW_PLANAR=1: the planar
    forward) and the default, each in a process of its own, against the fp64 reference at TOL[bf16].  They differ in
    accumulation order, so they are not compared bit-wise with each other.  A child that fails ends the test there."""
    dtype = torch.bfloat16
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = 'import sys\nfrom tests import test_gpu_dwconv as T\nT.ab_child(sys.argv[1])\n'
    for switch in ('VKAS_DW_VALU', 'VKAS_DW_PLANAR', None):
        env = {k: v for k, v in os.environ.items() if k not in ('VKAS_DW_VALU', 'VKAS_DW_PLANAR')}
        if switch:
            env[switch] = '1'
        with tempfile.NamedTemporaryFile(suffix='.pt') as f:
            subprocess.run([sys.executable, '-c', code, f.name], check=True, env=env, cwd=root, timeout=600)
            out = torch.load(f.name, weights_only=True)
        for i, case in enumerate(AB_CASES):
            B, C, H, W = case
            r = reference(case, dtype)
            parts = valu_parts(B, H, W) if switch == 'VKAS_DW_VALU' else mfma_geometry(*case)[1]
            assert int(out['parts%d' % i]) == parts, (switch, case, 'the switch did not reach the dispatch')
            for what, got, ref in (('forward', out['y%d' % i], r['y']), ('input gradient', out['dx%d' % i], r['dx'] + r['add']),
                                   ('weight gradient', out['gw%d' % i], r['gw']), ('bias gradient', out['gb%d' % i], r['gb'])):
                v = rel_err(got, ref)
                parity_log.record('test_gpu_dwconv', '%s %s bf16, %s' % (what, 'x'.join(map(str, case)), switch or 'default, child'),
                                  v, TOL[dtype][0])
                close(got, ref, dtype, '%s: %s %s' % (switch or 'default', what, case))


# ------------------------------------------------------------------------------------- 6. argument checks, empty batch
def test_argument_checks_and_empty_batch():
    """Refused through the C ABI, with no kernel launched: Cp not a multiple of 8, a pixel stride below Cp or not a multiple of 8,
    a pointer that is not 16-byte aligned, a workspace one byte short, gw without gb (and gb without gw).  B = 0 is accepted:
    the forward leaves y alone, the weight gradient zeroes gw / gb and reports no partial rows."""
    lib = vk()
    B, C, H, W = 1, 16, 9, 11
    Cp, code, st = 16, CODE[torch.bfloat16], stream()
    x = torch.zeros((B, H, W, 32), dtype=torch.bfloat16, device='cuda')
    y = torch.full((B, H, W, 32), SENTINEL, dtype=torch.bfloat16, device='cuda')
    wp = pack_weight(rnd((C, 1, 7, 7), 61), C, 0)
    gw, gb = torch.full((49 * Cp,), float('nan'), device='cuda'), torch.full((Cp,), float('nan'), device='cuda')
    nbytes = lib.vkas_dwconv7x7_wgrad_ws_bytes(B, H, W, Cp)
    ws = torch.empty((nbytes // 4 + 4,), device='cuda')
    X, Y, WP, GW, GB, WS = (t.data_ptr() for t in (x, y, wp, gw, gb, ws))

    def fwd(xp=X, ldx=32, add=None, ldadd=0, yp=Y, ldy=32, b=B, cp=Cp):
        return lib.vkas_dwconv7x7_fwd(xp, ldx, WP, None, add, ldadd, yp, ldy, b, H, W, cp, code, st)

    def wgrad(xp=X, ldx=32, dp=X, lddy=32, g=GW, gbp=GB, nb=nbytes, b=B, cp=Cp):
        return lib.vkas_dwconv7x7_wgrad(xp, ldx, dp, lddy, g, gbp, WS, nb, b, H, W, cp, code, st)

    assert fwd() == 0 and wgrad() == 0  # the accepted call, so that every refusal below is down to its one argument
    torch.cuda.synchronize()
    y.fill_(SENTINEL)
    gw.fill_(float('nan'))
    refused = [fwd(cp=12), fwd(ldx=8), fwd(ldx=36), fwd(ldy=8), fwd(ldy=36), fwd(add=X, ldadd=8), fwd(add=X, ldadd=36),
               fwd(xp=X + 2), fwd(yp=Y + 2), fwd(add=X + 2, ldadd=32), fwd(xp=None), fwd(yp=None),
               wgrad(cp=12), wgrad(ldx=8), wgrad(ldx=36), wgrad(lddy=8), wgrad(lddy=36), wgrad(xp=X + 2), wgrad(dp=X + 2),
               wgrad(nb=nbytes - 1), wgrad(gbp=None), wgrad(g=None)]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in refused), refused
    assert bool((y == SENTINEL).all()) and bool(torch.isnan(gw).all()), 'a refused call launched a kernel'
    # B = 0: nothing to do in the forward; the weight gradient of no pixels is zero
    assert fwd(b=0) == 0
    assert lib.vkas_dwconv7x7_wgrad_ws_bytes(0, H, W, Cp) == 0
    assert wgrad(b=0, nb=0) == 0
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())
    assert float(gw.abs().max()) == 0.0 and float(gb.abs().max()) == 0.0
    for c in (0, 1, 2):
        assert lib.vkas_dwconv7x7_wgrad_parts(0, H, W, Cp, c) == 0
