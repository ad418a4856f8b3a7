"""Direct parity of the nine kernels of csrc/resize.hip through the C ABI (vkas_resize_fwd, vkas_resize_bwd, vkas_resize_bwd_ws,
vkas_resize_bwd_ws_bytes, vkas_adaptive_avgpool_fwd, vkas_adaptive_avgpool_bwd) with ctypes, so pixel strides, workspaces and
accumulate targets are the test's own.

References, all on the host in fp64 on operands rounded to the storage type first:
  bilinear    F.interpolate(mode='bilinear', align_corners=False) and its autograd
  nearest     index vectors from F.interpolate(mode='nearest') applied to a float32 index ramp (the arithmetic the reference
              model runs), the fp64 values gathered with index_select; the backward is the matching index_add_
  pooling     nn.AdaptiveAvgPool2d and its autograd
  accumulate  the fp64 sum of the prior content and the result
With the operands pre-rounded the only differences from fp64 are fp32 accumulation (and fp32 interpolation weights) and one
output rounding, so the bounds are the single-op table of test_gpu_ops as it stands (TOL: 2e-5 / 4e-3 / 6e-4 norm-wise,
1e-4 / 2e-2 / 4e-3 of the peak; f32 / bf16 / f16).  Worst norm-wise error measured per kernel on the MI355X, the larger of
the plain and the accumulate launches (every figure goes to the parity report as 'worst <kernel>, <type>'); the 16-bit figures
are the one output rounding, the f32 ones the fp32 interpolation weights at non-integer ratios:

  kernel                          f32       bf16      f16
  avgpool bwd                     4.9e-08   1.7e-03   2.3e-04 
  avgpool fwd                     1.8e-07   2.0e-03   2.6e-04 
  bwd one-pass R16                6.5e-07   1.7e-03   2.2e-04 
  bwd one-pass R8                 1.8e-06   1.8e-03   2.2e-04 
  bwd small                       5.7e-07   2.0e-03   2.4e-04 
  bwd two-pass R16                4.5e-07   1.7e-03   2.1e-04 
  bwd two-pass R8                 7.6e-08   1.7e-03   2.1e-04 
  bwd x2                          6.9e-08   1.8e-03   2.1e-04 
  fwd generic                     1.8e-06   1.8e-03   2.3e-04 
  fwd x2                          4.2e-08   1.7e-03   2.1e-04 

Every tensor is a channel slice [8, 8 + Cp) of a wider buffer filled with a sentinel (operands: with another constant), pad
channels C..Cp zero: after each launch
everything outside the slice is the sentinel bit for bit and the pad channels of the output are zero.  The fp32 workspace of the
two-pass backward is followed by a guard block that no launch may touch.  Every backward launch is made twice on the same
operands and gives the same bits (no atomics anywhere in the file).

The case table sits at the smallest sizes that still reach each dispatch branch; the branch is derived from the geometry by a
Python copy of the dispatch arithmetic (resize_bwd_separable, the `small` predicate, 2 * cdiv(Wout, Win) <= 8, the vb loop of the
pooling forward), compared with the table and, for the two-pass branch, with vkas_resize_bwd_ws_bytes: a retuned dispatch
cannot silently move a case to another kernel.
"""
import ctypes
import os
import subprocess
import sys
import tempfile
from collections import namedtuple

import pytest
import torch
from torch.nn import functional as F

from tests import parity_log
from tests.golden import recipe
from tests.helpers import rel_err
from tests.test_gpu_ops import DTYPES, TOL, close, q, rnd

pytestmark = pytest.mark.gpu

IDS = {torch.float32: 'f32', torch.bfloat16: 'bf16', torch.float16: 'f16'}
CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}  # VKAS_F32 / VKAS_BF16 / VKAS_F16
P_BITS = {torch.float32: 24, torch.bfloat16: 8, torch.float16: 11}  # significand bits, the hidden one included
MODES = {0: 'bilinear', 1: 'nearest'}
GUARD = 4096          # floats behind the workspace that no launch may touch
SENTINEL = -12352.0   # exact in all three storage types, far outside every output here
# around every operand slice: another value than the sentinel, so that a kernel which reads and writes one vector too many (a
# copy or a mean of the surroundings) does not write the sentinel onto the sentinel; exact in all three storage types
IN_FILL = 776.0
OFF = 8               # first channel of every slice

_WORST = {}


def cdiv(a, b):
    return (a + b - 1) // b


def cp_of(C):
    return cdiv(C, 8) * 8


def vk():
    from vkit_ocr_model_adaptive_scaling_amd import _lib
    return _lib.lib


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def slab(t64, dtype, extra, fill=None, pad_fill=0.0):
    """(B, C, H, W) fp64 host tensor -> channels [OFF, OFF + Cp) of a (B, H, W, OFF + Cp + extra) device buffer filled with
    ``fill`` (default IN_FILL, for operands; accumulate targets take the sentinel); pad channels C..Cp are zero.  Returns
    (buffer, view of the slice, pixel stride)."""
    B, C, H, W = t64.shape
    Cp = cp_of(C)
    assert extra % 8 == 0
    width = OFF + Cp + extra
    buf = torch.full((B, H, W, width), IN_FILL if fill is None else fill, dtype=dtype, device='cuda')
    view = buf[..., OFF:OFF + Cp]
    view[..., C:] = pad_fill
    view[..., :C] = t64.permute(0, 2, 3, 1).to(dtype).cuda()
    return buf, view, width


def empty_slab(shape, dtype, extra):
    B, C, H, W = shape
    Cp = cp_of(C)
    width = OFF + Cp + extra
    buf = torch.full((B, H, W, width), SENTINEL, dtype=dtype, device='cuda')
    return buf, buf[..., OFF:OFF + Cp], width


def unslab(view, C):
    return view[..., :C].permute(0, 3, 1, 2).double().cpu()


def check_output(buf, before, view, C, fresh, what):
    """What holds after every launch: columns outside the slice bit-unchanged, every element of the slice finite (and, where the
    slice held the sentinel before, written), pad channels exactly zero."""
    Cp = view.shape[-1]
    outside = [i for i in range(buf.shape[-1]) if not OFF <= i < OFF + Cp]
    assert torch.equal(bits(buf[..., outside]), bits(before[..., outside])), what + ': columns outside the slice were written'
    assert torch.isfinite(view).all(), what + ': non-finite output'
    if fresh:
        assert not (view == SENTINEL).any(), what + ': an element of the slice was not written'
    if Cp > C:
        assert float(view[..., C:].float().abs().max()) == 0.0, what + ': pad channels must be exactly 0'


# ------------------------------------------------------------------------------------------ the dispatch, restated
def is_small(hi, wi, ho, wo, cp):
    return hi * wi <= 64 and ho * wo >= 16 * hi * wi and cp // 8 <= 256


def is_separable(B, hi, wi, ho, wo, cp):
    """resize_bwd_separable (without its environment switch, which no test sets)."""
    return (not is_small(hi, wi, ho, wo, cp)) and ho >= 3 * hi and wo >= 3 * wi and B * ho * wo * (cp // 8) >= (1 << 16)


def is_x2(mode, hi, wi, ho, wo):
    return mode == 0 and ho == 2 * hi and wo == 2 * wi and hi > 1 and wi > 1


def fwd_branch(mode, hi, wi, ho, wo):
    return 'x2' if is_x2(mode, hi, wi, ho, wo) else 'generic'


def regs(wi, wo):
    return 8 if 2 * cdiv(wo, wi) <= 8 else 16


def bwd_branch(mode, B, hi, wi, ho, wo, cp, ws):
    """Kernel that vkas_resize_bwd_ws (ws given) or vkas_resize_bwd (ws NULL) runs."""
    if ws and is_separable(B, hi, wi, ho, wo, cp):
        return 'two-pass R%d' % regs(wi, wo)
    small = is_small(hi, wi, ho, wo, cp)
    if is_x2(mode, hi, wi, ho, wo) and not small:
        return 'x2'
    return 'small' if small else 'one-pass R%d' % regs(wi, wo)


def vb_of(H, W, s, nvec):
    """Vectors per workgroup of avgpool_fwd_kernel and its vector groups."""
    bin_px = cdiv(H, s) * cdiv(W, s)
    vb = nvec
    while vb > 4 and bin_px * vb > 64 * 256:
        vb = (vb + 1) // 2
    groups = [min(vb, nvec - g * vb) for g in range(cdiv(nvec, vb))]
    return vb, groups


# ------------------------------------------------------------------------------------------------- fp64 references
def nearest_index(n_in, n_out):
    """Source index per destination index as F.interpolate(mode='nearest') computes it: from a float32 ramp."""
    ramp = torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in)
    return F.interpolate(ramp, size=(1, n_out), mode='nearest').view(-1).to(torch.int64)


def ref_fwd(x64, size, mode):
    if mode == 0:
        return F.interpolate(x64, size=size, mode='bilinear', align_corners=False)
    hi, wi = x64.shape[-2:]
    return x64.index_select(2, nearest_index(hi, size[0])).index_select(3, nearest_index(wi, size[1]))


def ref_bwd(dy64, src, mode):
    B, C, ho, wo = dy64.shape
    hi, wi = src
    if mode == 0:
        x = torch.zeros((B, C, hi, wi), dtype=torch.float64, requires_grad=True)
        F.interpolate(x, size=(ho, wo), mode='bilinear', align_corners=False).backward(dy64)
        return x.grad
    rows = torch.zeros((B, C, hi, wo), dtype=torch.float64).index_add_(2, nearest_index(hi, ho), dy64)
    return torch.zeros((B, C, hi, wi), dtype=torch.float64).index_add_(3, nearest_index(wi, wo), rows)


def x_footprint(wi, wo, mode):
    """Most destination columns (first to last, inclusive) that read one source column, from the fp64 index function."""
    first, last = {}, {}
    for d in range(wo):
        if mode == 0:
            s = max((d + 0.5) * wi / wo - 0.5, 0.0)
            i0 = min(int(s), wi - 1)
            i1 = min(i0 + 1, wi - 1)
            w1 = s - i0
            srcs = ([i0] if w1 != 1.0 else []) + ([i1] if w1 != 0.0 else [])
        else:
            srcs = [int(nearest_index(wi, wo)[d])]
        for i in srcs:
            first.setdefault(i, d)
            last[i] = d
    return max(last[i] - first[i] + 1 for i in first)


# ------------------------------------------------------------------------------------------------------ launches
def run_fwd(x64, size, mode, dtype, prior64=None, raw=False):
    """One vkas_resize_fwd call: x and y are channel slices of wider buffers with different pixel strides.  prior64: content of
    y before an accumulate = 1 launch.  Returns y as (B, C, Hout, Wout) fp64 (raw: the bits of the slice)."""
    lib = vk()
    B, C, hi, wi = x64.shape
    ho, wo = size
    Cp = cp_of(C)
    _, xv, ldx = slab(x64, dtype, 8)
    if prior64 is None:
        ybuf, yv, ldy = empty_slab((B, C, ho, wo), dtype, 16)
    else:
        ybuf, yv, ldy = slab(prior64, dtype, 16, fill=SENTINEL)
    before = ybuf.clone()
    rc = lib.vkas_resize_fwd(xv.data_ptr(), ldx, yv.data_ptr(), ldy, B, hi, wi, ho, wo, Cp, mode, int(prior64 is not None),
                             CODE[dtype], stream())
    assert rc == 0, lib.vkas_last_error()
    torch.cuda.synchronize()
    check_output(ybuf, before, yv, C, prior64 is None, 'resize forward')
    return bits(yv).cpu() if raw else unslab(yv, C)


def run_bwd(dy64, src, mode, dtype, prior64=None, how='plain', raw=False):
    """The resize backward, launched twice on the same operands (the two results must agree bit for bit).  how: 'plain'
    vkas_resize_bwd; 'ws' vkas_resize_bwd_ws with a NaN-filled workspace of exactly vkas_resize_bwd_ws_bytes and a guard block
    behind it; 'ws-null' vkas_resize_bwd_ws with ws = NULL.  Returns dx as (B, C, Hin, Win) fp64."""
    lib = vk()
    B, C, ho, wo = dy64.shape
    hi, wi = src
    Cp = cp_of(C)
    _, dv, lddy = slab(dy64, dtype, 24)
    nbytes = lib.vkas_resize_bwd_ws_bytes(B, hi, wi, ho, wo, Cp) if how == 'ws' else 0
    assert nbytes % 16 == 0
    ws = torch.full((nbytes // 4 + GUARD,), float('nan'), device='cuda')
    ws[nbytes // 4:] = 7.25
    outs = []
    for _ in range(2):
        if prior64 is None:
            xbuf, xv, lddx = empty_slab((B, C, hi, wi), dtype, 16)
        else:
            xbuf, xv, lddx = slab(prior64, dtype, 16, fill=SENTINEL)
        before = xbuf.clone()
        acc = int(prior64 is not None)
        if how == 'plain':
            rc = lib.vkas_resize_bwd(dv.data_ptr(), lddy, xv.data_ptr(), lddx, B, hi, wi, ho, wo, Cp, mode, acc, CODE[dtype],
                                     stream())
        else:
            rc = lib.vkas_resize_bwd_ws(dv.data_ptr(), lddy, xv.data_ptr(), lddx, ws.data_ptr() if how == 'ws' else None, nbytes,
                                        B, hi, wi, ho, wo, Cp, mode, acc, CODE[dtype], stream())
        assert rc == 0, lib.vkas_last_error()
        torch.cuda.synchronize()
        check_output(xbuf, before, xv, C, prior64 is None, 'resize backward (%s)' % how)
        assert float((ws[nbytes // 4:] - 7.25).abs().max()) == 0.0, 'the launch wrote behind its workspace'
        outs.append(xv)
    assert torch.equal(bits(outs[0]), bits(outs[1])), 'two launches on the same operands differ (%s)' % how
    return bits(outs[0]).cpu() if raw else unslab(outs[0], C)


def run_pool_fwd(x64, s, dtype):
    lib = vk()
    B, C, H, W = x64.shape
    Cp = cp_of(C)
    _, xv, ldx = slab(x64, dtype, 8)
    ybuf, yv, ldy = empty_slab((B, C, s, s), dtype, 16)
    before = ybuf.clone()
    rc = lib.vkas_adaptive_avgpool_fwd(xv.data_ptr(), ldx, yv.data_ptr(), ldy, B, H, W, s, Cp, CODE[dtype], stream())
    assert rc == 0, lib.vkas_last_error()
    torch.cuda.synchronize()
    check_output(ybuf, before, yv, C, True, 'pool forward')
    return unslab(yv, C)


def run_pool_bwd(dy64s, scales, hw, dtype, prior64=None):
    """vkas_adaptive_avgpool_bwd for each scale in turn into one dx: the first launch overwrites (or accumulates onto prior64),
    the later ones accumulate.  Twice, bit-compared."""
    lib = vk()
    B, C = dy64s[0].shape[:2]
    H, W = hw
    Cp = cp_of(C)
    outs = []
    for _ in range(2):
        if prior64 is None:
            xbuf, xv, lddx = empty_slab((B, C, H, W), dtype, 16)
        else:
            xbuf, xv, lddx = slab(prior64, dtype, 16, fill=SENTINEL)
        before = xbuf.clone()
        for n, (dy64, s) in enumerate(zip(dy64s, scales)):
            _, dv, lddy = slab(dy64, dtype, 24)
            rc = lib.vkas_adaptive_avgpool_bwd(dv.data_ptr(), lddy, xv.data_ptr(), lddx, B, H, W, s, Cp,
                                               int(n > 0 or prior64 is not None), CODE[dtype], stream())
            assert rc == 0, lib.vkas_last_error()
        torch.cuda.synchronize()
        check_output(xbuf, before, xv, C, prior64 is None, 'pool backward')
        outs.append(xv)
    assert torch.equal(bits(outs[0]), bits(outs[1])), 'two pool backward launches on the same operands differ'
    return unslab(outs[0], C)


def measure(kernel, tag, dtype, actual, expected, what):
    """Prints and records the figures, then asserts TOL."""
    r = rel_err(actual, expected)
    peak = max(float(expected.abs().max()), 1e-30)
    print('resize %-16s %-34s %-4s norm-wise %.3e  max abs / peak %.3e' % (
        kernel, tag, IDS[dtype], r, float((actual.double().cpu() - expected).abs().max()) / peak))
    key = (kernel, dtype)
    if key not in _WORST or r > _WORST[key][0]:
        _WORST[key] = (r, tag)
    close(actual, expected, dtype, '%s %s: %s' % (kernel, tag, what))
    return r


@pytest.fixture(scope='module', autouse=True)
def worst_rows():
    yield
    for (kernel, dtype), (v, tag) in sorted(_WORST.items(), key=lambda kv: (kv[0][0], IDS[kv[0][1]])):
        parity_log.record('test_gpu_resize', 'worst %s, %s' % (kernel, IDS[dtype]), v, TOL[dtype][0], 'at ' + tag)


# --------------------------------------------------------------------------------------------------- the case table
# fwd / bwd: the kernels that run in bilinear mode ('bwd' through vkas_resize_bwd_ws with a workspace where the two-pass runs,
# else through vkas_resize_bwd); nearest never takes the x2 kernels.  acc: also run with accumulate = 1 onto a random target.
# tail: some source column has more destination columns than the R kept in registers (bilinear), so the loop behind them runs.
Case = namedtuple('Case', 'B C src dst modes fwd bwd acc tail')
BOTH, BILINEAR = (0, 1), (0,)
CASES = {
    # generic forward
    'up-5x7-12x20': Case(2, 24, (5, 7), (12, 20), BOTH, 'generic', 'one-pass R8', True, False),
    'down-13x17-5x6': Case(2, 24, (13, 17), (5, 6), BOTH, 'generic', 'one-pass R8', True, False),   # non-integer downsample
    'updown-6x20-15x7': Case(2, 24, (6, 20), (15, 7), BOTH, 'generic', 'one-pass R8', False, False),  # up in y, down in x
    'identity-7x9': Case(2, 24, (7, 9), (7, 9), BOTH, 'generic', 'one-pass R8', False, False),
    'point-1x1-5x3': Case(2, 24, (1, 1), (5, 3), BOTH, 'generic', 'one-pass R8', False, False),
    'x2-but-one-row-1x6-2x12': Case(2, 24, (1, 6), (2, 12), BOTH, 'generic', 'one-pass R8', False, False),
    # 280 row entries: two chunks of 256, the second ragged; 7 vectors; 21 rows (not a multiple of 8, for xcd_row)
    'two-chunks-3x5-7x40': Case(3, 56, (3, 5), (7, 40), BOTH, 'generic', 'small', True, False),
    # exact x2 (bilinear only); 2 rows / columns: the first and the last are neighbours
    'x2-2x2': Case(2, 24, (2, 2), (4, 4), BILINEAR, 'x2', 'x2', False, False),
    'x2-2x9': Case(2, 24, (2, 9), (4, 18), BILINEAR, 'x2', 'x2', True, False),
    'x2-9x2': Case(2, 24, (9, 2), (18, 4), BILINEAR, 'x2', 'x2', False, False),
    'x2-two-chunks-5x40': Case(2, 56, (5, 40), (10, 80), BILINEAR, 'x2', 'x2', False, False),
    # one-pass backward
    'r8-10x10-25x33': Case(2, 16, (10, 10), (25, 33), BOTH, 'generic', 'one-pass R8', False, False),
    # 40 source columns of 7 vectors: the R = 8 one-pass backward at two row chunks and a vector count that is no power of two
    'r8-two-chunks-3x40-5x60': Case(2, 56, (3, 40), (5, 60), BOTH, 'generic', 'one-pass R8', True, False),
    'r16-9x9-60x70': Case(2, 16, (9, 9), (60, 70), BOTH, 'generic', 'one-pass R16', True, False),
    'beyond-r-9x9-100x95': Case(1, 16, (9, 9), (100, 95), BOTH, 'generic', 'one-pass R16', True, True),  # 19 000 < 65 536 entries
    # two-pass backward: 66 500 entries (just over the threshold), R = 16 with the tail loop; x4 with R = 8
    'two-pass-9x9-100x95': Case(1, 56, (9, 9), (100, 95), BOTH, 'generic', 'two-pass R16', True, True),
    'two-pass-x4-16x24-64x96': Case(1, 96, (16, 24), (64, 96), BOTH, 'generic', 'two-pass R8', True, False),
    'under-threshold-9x9-100x95': Case(1, 48, (9, 9), (100, 95), BOTH, 'generic', 'one-pass R16', False, True),  # 57 000 entries
    # the pairs on which floor(dst * in / out) in integers and torch's float32 product part (both axes, both orders)
    'nearest-14x21-46x69': Case(2, 8, (14, 21), (46, 69), BOTH, 'generic', 'one-pass R8', False, False),
    'nearest-21x14-69x46': Case(2, 8, (21, 14), (69, 46), BOTH, 'generic', 'one-pass R8', False, False),
    'nearest-30x26-58x22': Case(2, 8, (30, 26), (58, 22), BOTH, 'generic', 'one-pass R8', False, False),
    'nearest-26x30-22x58': Case(2, 8, (26, 30), (22, 58), BOTH, 'generic', 'one-pass R8', False, False),
    # 257 vectors: one more than the small kernel takes
    'not-small-257-2x3-32x32': Case(1, 2056, (2, 3), (32, 32), BOTH, 'generic', 'two-pass R16', False, True),
}
# small backward: PPM-sized sources to 32 x 32; nvec = 1, 7 (36 lanes, 4 idle threads), 50 (5 lanes, 6 idle), 96 (2 lanes, 64
# idle), 200 and 256 (one lane per vector: no reduction loop)
SMALL_C = (8, 56, 400, 768, 1600, 2048)
for _src in ((1, 1), (2, 3), (6, 6)):
    for _C in SMALL_C:
        CASES['small-%dx%d-c%d' % (_src + (_C,))] = Case(2 if _C <= 56 else 1, _C, _src, (32, 32), BOTH, 'generic', 'small',
                                                          _src == (2, 3) and _C in (56, 1600), False)
NEAREST_PAIRS = ((14, 46), (21, 69), (30, 58), (26, 22))
X2_CASES = [k for k, c in CASES.items() if c.fwd == 'x2']

POOL_CASES = [(2, 24) + c for c in recipe.POOL_CASES] + [
    (2, 136, 32, 32, 1),   # 17 vectors, vb = 9: groups of 9 and 8
    (1, 768, 32, 32, 1),   # vb = 12: eight groups
    (1, 40, 64, 64, 1),    # 5 vectors, vb = 3: groups of 3 and 2
    (1, 2048, 3, 5, 2),    # 256 vectors in one group: one lane per vector
]
POOL_GROUPS = {(136, 32, 32, 1): (9, [9, 8]), (768, 32, 32, 1): (12, [12] * 8), (40, 64, 64, 1): (3, [3, 2]),
               (2048, 3, 5, 2): (256, [256])}


def operands(name, dtype):
    c = CASES[name]
    seed = 7000 + 10 * sorted(CASES).index(name)
    x = q(rnd((c.B, c.C) + c.src, seed), dtype)
    dy = q(rnd((c.B, c.C) + c.dst, seed + 1), dtype)
    return c, x, dy, seed


# ------------------------------------------------------------------------------------------------------ 1. geometry
def test_case_geometry():
    """Every case runs the kernels its table row names, by the restated dispatch and by vkas_resize_bwd_ws_bytes."""
    lib = vk()
    seen_fwd, seen_bwd = set(), set()
    for name, c in CASES.items():
        (hi, wi), (ho, wo), Cp = c.src, c.dst, cp_of(c.C)
        assert fwd_branch(0, hi, wi, ho, wo) == c.fwd, name
        assert bwd_branch(0, c.B, hi, wi, ho, wo, Cp, True) == c.bwd, name
        sep = is_separable(c.B, hi, wi, ho, wo, Cp)
        assert sep == c.bwd.startswith('two-pass'), name
        assert lib.vkas_resize_bwd_ws_bytes(c.B, hi, wi, ho, wo, Cp) == (c.B * ho * wi * Cp * 4 if sep else 0), name
        if c.bwd not in ('small', 'x2'):  # the kernels with R register columns
            assert (x_footprint(wi, wo, 0) > regs(wi, wo)) == c.tail, (name, x_footprint(wi, wo, 0))
        seen_fwd.add(c.fwd)
        seen_bwd.add(c.bwd + (' tail' if c.tail else ''))
    assert seen_fwd == {'generic', 'x2'}
    assert seen_bwd == {'x2', 'small', 'one-pass R8', 'one-pass R16', 'one-pass R16 tail', 'two-pass R8', 'two-pass R16 tail'}
    # accumulate = 1 reaches every branch
    assert {CASES[k].fwd for k in CASES if CASES[k].acc} == seen_fwd
    assert {CASES[k].bwd + (' tail' if CASES[k].tail else '') for k in CASES if CASES[k].acc} >= seen_bwd
    c = CASES['two-chunks-3x5-7x40']
    assert cdiv(c.dst[1] * cp_of(c.C) // 8, 256) == 2 and c.dst[1] * 7 % 256 != 0 and (c.B * c.dst[0]) % 8 != 0
    c = CASES['r8-two-chunks-3x40-5x60']
    assert cdiv(c.src[1] * cp_of(c.C) // 8, 256) == 2 and not is_small(3, 40, 5, 60, 56)
    c = CASES['x2-two-chunks-5x40']
    assert cdiv(c.src[1] * cp_of(c.C) // 8, 256) == 2
    c = CASES['beyond-r-9x9-100x95']
    assert 2 * cdiv(95, 9) == 22 and c.B * 100 * 95 * 2 == 19000
    c = CASES['two-pass-9x9-100x95']
    assert c.B * 100 * 95 * 7 == 66500 >= 1 << 16 > CASES['under-threshold-9x9-100x95'].B * 100 * 95 * 6
    # the 257-vector case is small in everything but its vector count; without a workspace it runs the one-pass kernel
    assert is_small(2, 3, 32, 32, 2048) and not is_small(2, 3, 32, 32, 2056)
    assert bwd_branch(0, 1, 2, 3, 32, 32, 2056, False) == 'one-pass R16'
    assert [256 // n for n in (1, 7, 50, 96, 200, 256)] == [256, 36, 5, 2, 1, 1] and 256 - 36 * 7 == 4 and 256 - 5 * 50 == 6
    for (B, C, H, W, s) in POOL_CASES:
        if (C, H, W, s) in POOL_GROUPS:
            assert vb_of(H, W, s, cp_of(C) // 8) == POOL_GROUPS[(C, H, W, s)], (C, H, W, s)
        else:
            assert vb_of(H, W, s, cp_of(C) // 8) == (3, [3]), (C, H, W, s)
    for pair in NEAREST_PAIRS:  # where the integer form and torch's float32 form of the nearest index part
        old = torch.clamp((torch.arange(pair[1]) * pair[0]) // pair[1], max=pair[0] - 1)
        assert not torch.equal(old, nearest_index(*pair)), pair


# ------------------------------------------------------------------------------------------ 2. parity of every branch
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('name,mode', [(k, m) for k, c in CASES.items() for m in c.modes],
                         ids=['%s-%s' % (k, MODES[m]) for k, c in CASES.items() for m in c.modes])
def test_resize(name, mode, dtype):
    """Forward and backward of one case against fp64; with accumulate where the table says so; the two-pass cases also with
    ws = NULL (the one-pass kernels), both held to fp64 and to each other within TOL."""
    c, x, dy, seed = operands(name, dtype)
    (hi, wi), (ho, wo), Cp = c.src, c.dst, cp_of(c.C)
    tag = '%s %s' % (name, MODES[mode])
    fk = 'fwd ' + fwd_branch(mode, hi, wi, ho, wo)
    y_ref = ref_fwd(x, c.dst, mode)
    y = run_fwd(x, c.dst, mode, dtype)
    if mode == 1:
        assert torch.equal(y, y_ref), tag + ': nearest forward is a copy and must be exact'
    measure(fk, tag, dtype, y, y_ref, 'forward')
    dx_ref = ref_bwd(dy, c.src, mode)
    sep = is_separable(c.B, hi, wi, ho, wo, Cp)
    bk = 'bwd ' + bwd_branch(mode, c.B, hi, wi, ho, wo, Cp, True)
    dx = run_bwd(dy, c.src, mode, dtype, how='ws' if sep else 'plain')
    measure(bk, tag, dtype, dx, dx_ref, 'backward')
    unread = None
    if mode == 1:
        unread = ref_bwd(torch.ones_like(dy), c.src, mode) == 0  # sources that no destination reads
        assert float(dx[unread].abs().max()) == 0.0 if unread.any() else True, tag + ': dx of an unread source must be exactly 0'
    if name == 'down-13x17-5x6':
        assert mode == 0 or int(unread.sum()) > c.B * c.C * 100, 'most sources have no destination here'
    if sep or name == 'under-threshold-9x9-100x95':
        # the same call without a workspace falls back to the one-pass kernels; a workspace of zero bytes is left alone
        ok = 'bwd ' + bwd_branch(mode, c.B, hi, wi, ho, wo, Cp, False)
        assert ok.startswith('bwd one-pass')
        dx1 = run_bwd(dy, c.src, mode, dtype, how='ws-null')
        measure(ok, tag + ' ws=NULL', dtype, dx1, dx_ref, 'backward without workspace')
        if sep:
            close(dx, dx1, dtype, tag + ': two-pass against one-pass')
        else:
            assert vk().vkas_resize_bwd_ws_bytes(c.B, hi, wi, ho, wo, Cp) == 0
            assert torch.equal(run_bwd(dy, c.src, mode, dtype, how='ws'), dx1), 'under the threshold the workspace is not used'
    if c.acc:
        py = q(rnd((c.B, c.C) + c.dst, seed + 2), dtype)
        px = q(rnd((c.B, c.C) + c.src, seed + 3), dtype)
        measure(fk + ' acc', tag, dtype, run_fwd(x, c.dst, mode, dtype, prior64=py), py + y_ref, 'forward, accumulate')
        dxa = run_bwd(dy, c.src, mode, dtype, prior64=px, how='ws' if sep else 'plain')
        measure(bk + ' acc', tag, dtype, dxa, px + dx_ref, 'backward, accumulate')
        if unread is not None and unread.any():
            assert torch.equal(dxa[unread], px[unread]), tag + ': accumulate must leave an unread source as it was'
        if sep:
            dxb = run_bwd(dy, c.src, mode, dtype, prior64=px, how='ws-null')
            measure('bwd ' + bwd_branch(mode, c.B, hi, wi, ho, wo, Cp, False) + ' acc', tag + ' ws=NULL', dtype, dxb,
                    px + dx_ref, 'backward without workspace, accumulate')


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('case', POOL_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_pool(case, dtype):
    B, C, H, W, s = case
    tag = 'pool ' + 'x'.join(map(str, case))
    x = q(rnd((B, C, H, W), 8100 + C + s), dtype)
    dy = q(rnd((B, C, s, s), 8200 + C + s), dtype)
    prior = q(rnd((B, C, H, W), 8300 + C + s), dtype)
    xr = x.clone().requires_grad_(True)
    ref = torch.nn.AdaptiveAvgPool2d(s)(xr)
    ref.backward(dy)
    measure('avgpool fwd', tag, dtype, run_pool_fwd(x, s, dtype), ref.detach(), 'forward')
    measure('avgpool bwd', tag, dtype, run_pool_bwd([dy], [s], (H, W), dtype), xr.grad, 'backward')
    measure('avgpool bwd acc', tag, dtype, run_pool_bwd([dy], [s], (H, W), dtype, prior64=prior), prior + xr.grad,
            'backward, accumulate')


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
def test_pool_backward_two_scales_into_one_dx(dtype):
    """The PPM's input gradient: the first scale overwrites dx, the second accumulates.  The intermediate dx is rounded to the
    storage type once more than the fp64 sum: two roundings of at most 2^-9 (bf16) / 2^-12 (f16) of an element each, about
    1.6e-3 / 2e-4 norm-wise, inside TOL as it stands."""
    B, C, H, W = 2, 24, 13, 10
    scales = (3, 6)
    dys = [q(rnd((B, C, s, s), 8400 + s), dtype) for s in scales]
    xr = torch.zeros((B, C, H, W), dtype=torch.float64, requires_grad=True)
    sum((torch.nn.AdaptiveAvgPool2d(s)(xr) * dy).sum() for s, dy in zip(scales, dys)).backward()
    measure('avgpool bwd acc', 'pool two scales 13x10', dtype, run_pool_bwd(dys, scales, (H, W), dtype), xr.grad,
            'backward of two scales')


def test_pool_forward_refuses_more_than_2048_channels():
    lib = vk()
    B, C, H, W, s = 1, 2056, 3, 5, 2
    for dtype in DTYPES:
        _, xv, ldx = slab(rnd((B, C, H, W), 8500), dtype, 8)
        ybuf, yv, ldy = empty_slab((B, C, s, s), dtype, 16)
        rc = lib.vkas_adaptive_avgpool_fwd(xv.data_ptr(), ldx, yv.data_ptr(), ldy, B, H, W, s, C, CODE[dtype], stream())
        torch.cuda.synchronize()
        assert rc != 0
        assert bool((ybuf == SENTINEL).all()), 'a refused call wrote its output'


# ------------------------------------------------------------------------------------------------- 3. bit for bit
def ints(shape, m, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-m, m + 1, shape, generator=g).double()


def representable(t64, dtype):
    return bool((t64.to(dtype).double() == t64).all())


EXACT_BILINEAR = [(f, d) for f in (2, 4, 8) for d in DTYPES if not (f == 8 and d == torch.bfloat16)]


@pytest.mark.parametrize('f,dtype', EXACT_BILINEAR, ids=['x%d-%s' % (f, IDS[d]) for f, d in EXACT_BILINEAR])
def test_bilinear_integer_factors_exact(f, dtype):
    """Bilinear at x f, f a power of two, on small integers.  Along one axis the weights are multiples of 1 / (2 f), so a
    forward output is k / (4 f^2) with an integer |k| <= 4 f^2 M for inputs |x| <= M (the four weights sum to 1): representable
    in a type of p significand bits once 4 f^2 M <= 2^p, i.e. M = 2^p / (4 f^2): 16 / 4 (/ 1) in bf16, 128 / 32 / 8 in f16 at
    x2 / x4 / x8 (capped at 64).  bf16 at x8 would leave M = 1 and is not asked for.  Every partial sum is such a multiple too
    and fp32 holds them all, so the kernel has nothing to round: compared with ==.  A source pixel's weights sum to f^2, so
    the backward needs 4 f^4 M <= 2^p: M = 4 in bf16 at x2, 32 / 2 in f16 at x2 / x4, and it is run where M >= 1.
    Sources 5 x 7 (the small backward kernel from x4 on) and 9 x 10 (x2, one-pass R8, one-pass R16)."""
    p = P_BITS[dtype]
    for src in ((5, 7), (9, 10)):
        dst = (src[0] * f, src[1] * f)
        m = min(64, 2 ** p // (4 * f * f))
        assert m >= 1
        x = ints((2, 20) + src, m, 9000 + f)
        ref = ref_fwd(x, dst, 0)
        assert representable(ref, dtype) and float(ref.abs().max()) <= m
        assert bool((ref * (4 * f * f) == (ref * (4 * f * f)).round()).all())
        y = run_fwd(x, dst, 0, dtype)
        assert torch.equal(y, ref), 'forward x%d from %s: %d elements differ' % (f, src, int((y != ref).sum()))
        mb = min(64, 2 ** p // (4 * f ** 4))
        if mb >= 1:  # bf16 at x4 and f16 at x8 leave no integer magnitude for the backward: forward only there
            dy = ints((2, 20) + dst, mb, 9100 + f)
            dref = ref_bwd(dy, src, 0)
            assert representable(dref, dtype) and float(dref.abs().max()) <= f * f * mb
            dx = run_bwd(dy, src, 0, dtype)
            assert torch.equal(dx, dref), 'backward x%d to %s: %d elements differ' % (f, src, int((dx != dref).sum()))


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
def test_nearest_backward_and_power_of_two_pooling_exact(dtype):
    """Nearest backward sums at most 4 x 4 destinations here: |dy| <= 4 keeps every sum an integer of at most 64.  Pooling with
    16-pixel bins of |x| <= 8 (sums of at most 128, divided by 16) and with one 1024-pixel bin of x in {-1, 0, 1} (the sums,
    about 26 in standard deviation, stay below 256: asserted on the reference) is exact too, and so is its backward (a
    division of integers |dy| <= 64 by 16 or 1024)."""
    for src, dst in (((3, 5), (12, 20)), ((14, 21), (46, 69)), ((13, 17), (5, 6)), ((26, 30), (22, 58))):
        dy = ints((2, 20) + dst, 4, 9200 + src[0])
        ref = ref_bwd(dy, src, 1)
        assert representable(ref, dtype) and float(ref.abs().max()) <= 64
        assert torch.equal(run_bwd(dy, src, 1, dtype), ref), (src, dst)
    for (H, W, s, m) in ((8, 8, 2, 8), (32, 32, 1, 1)):
        x = ints((2, 20, H, W), m, 9300 + s)
        dy = ints((2, 20, s, s), 64, 9400 + s)
        xr = x.clone().requires_grad_(True)
        ref = torch.nn.AdaptiveAvgPool2d(s)(xr)
        ref.backward(dy)
        assert representable(ref.detach(), dtype) and representable(xr.grad, dtype)
        assert torch.equal(run_pool_fwd(x, s, dtype), ref.detach()), (H, W, s)
        assert torch.equal(run_pool_bwd([dy], [s], (H, W), dtype), xr.grad), (H, W, s)


# -------------------------------------------------------------------------------- 4. the x2 kernels against the generic
def ab_child(path):
    """Runs in a child process (VKAS_RESIZE_NO2X is read once per process): forward and backward of the x2 cases in bilinear
    mode on random data, all three types, with and without accumulate; the raw bits go to ``path``."""
    out = {}
    for dtype in DTYPES:
        for name in X2_CASES:
            c, x, dy, seed = operands(name, dtype)
            py = q(rnd((c.B, c.C) + c.dst, seed + 2), dtype)
            px = q(rnd((c.B, c.C) + c.src, seed + 3), dtype)
            key = '%s %s ' % (name, IDS[dtype])
            out[key + 'forward'] = run_fwd(x, c.dst, 0, dtype, raw=True)
            out[key + 'forward, accumulate'] = run_fwd(x, c.dst, 0, dtype, prior64=py, raw=True)
            out[key + 'backward'] = run_bwd(dy, c.src, 0, dtype, raw=True)
            out[key + 'backward, accumulate'] = run_bwd(dy, c.src, 0, dtype, prior64=px, raw=True)
    torch.save(out, path)


def test_x2_kernels_bit_identical_to_generic():
    """resize2x_fwd_kernel and resize2x_bwd_kernel promise the bits of the generic kernels.  One child process with the default
    dispatch, one with VKAS_RESIZE_NO2X=1 (the generic kernels at the same sizes), one at a time; a child that fails ends the
    test there."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = 'import sys\nfrom tests import test_gpu_resize as T\nT.ab_child(sys.argv[1])\n'
    outs = []
    for switch in (None, '1'):
        env = {k: v for k, v in os.environ.items() if k != 'VKAS_RESIZE_NO2X'}
        if switch:
            env['VKAS_RESIZE_NO2X'] = switch
        with tempfile.NamedTemporaryFile(suffix='.pt') as f:
            subprocess.run([sys.executable, '-c', code, f.name], check=True, env=env, cwd=root, timeout=300)
            outs.append(torch.load(f.name, weights_only=True))
    assert sorted(outs[0]) == sorted(outs[1]) and len(outs[0]) == 4 * 3 * len(X2_CASES)
    differ = {k: int((outs[0][k] != outs[1][k]).sum()) for k in outs[0] if not torch.equal(outs[0][k], outs[1][k])}
    assert not differ, 'elements whose bits differ between the x2 and the generic kernels: %s' % differ


# ------------------------------------------------------------------------------------- 5. argument checks, empty batch
def test_argument_checks_and_empty_batch():
    """Refused through the C ABI before any launch: a mode other than 0 / 1, a pixel stride below Cp, Cp not a multiple of 8, a
    pointer that is not 16-byte aligned, a workspace one byte short, s = 0.  Every call has valid buffers and only the argument
    under test wrong (the buffers are 48 channels wide for Cp = 16, so a smaller stride or a shifted pointer stays inside them).
    B = 0 is accepted and writes nothing."""
    lib = vk()
    dtype, code, st = torch.bfloat16, CODE[torch.bfloat16], stream()
    B, Cp, hi, wi, ho, wo, s = 1, 16, 5, 7, 12, 20, 3
    x = torch.zeros((B, hi, wi, 48), dtype=dtype, device='cuda')
    y = torch.full((B, ho, wo, 48), SENTINEL, dtype=dtype, device='cuda')
    X, Y = x.data_ptr() + 16, y.data_ptr() + 16

    def fwd(xp=X, ldx=48, yp=Y, ldy=48, b=B, cp=Cp, mode=0):
        return lib.vkas_resize_fwd(xp, ldx, yp, ldy, b, hi, wi, ho, wo, cp, mode, 0, code, st)

    def bwd(dp=Y, lddy=48, xp=X, lddx=48, b=B, cp=Cp, mode=0):
        return lib.vkas_resize_bwd(dp, lddy, xp, lddx, b, hi, wi, ho, wo, cp, mode, 0, code, st)

    def pool_f(xp=Y, ldx=48, yp=X, ldy=48, b=B, cp=Cp, ss=s):  # pools the 12 x 20 map into the 5 x 7 buffer's first 3 x 3 pixels
        return lib.vkas_adaptive_avgpool_fwd(xp, ldx, yp, ldy, b, ho, wo, ss, cp, code, st)

    def pool_b(dp=X, lddy=48, xp=Y, lddx=48, b=B, cp=Cp, ss=s):
        return lib.vkas_adaptive_avgpool_bwd(dp, lddy, xp, lddx, b, ho, wo, ss, cp, 0, code, st)

    # the accepted calls first, so that every refusal below is down to its one argument
    assert fwd() == 0 and bwd() == 0 and pool_f() == 0 and pool_b() == 0 and fwd(mode=1) == 0 and bwd(mode=1) == 0
    torch.cuda.synchronize()
    x.fill_(SENTINEL)
    y.fill_(SENTINEL)
    refused = {
        'fwd mode 2': fwd(mode=2), 'fwd mode -1': fwd(mode=-1), 'fwd ldx < Cp': fwd(ldx=8), 'fwd ldy < Cp': fwd(ldy=8),
        'fwd Cp 12': fwd(cp=12), 'fwd x misaligned': fwd(xp=X + 2), 'fwd y misaligned': fwd(yp=Y + 2),
        'bwd mode 2': bwd(mode=2), 'bwd lddy < Cp': bwd(lddy=8), 'bwd lddx < Cp': bwd(lddx=8), 'bwd Cp 12': bwd(cp=12),
        'bwd dy misaligned': bwd(dp=Y + 2), 'bwd dx misaligned': bwd(xp=X + 2),
        'pool fwd ldx < Cp': pool_f(ldx=8), 'pool fwd ldy < Cp': pool_f(ldy=8), 'pool fwd Cp 12': pool_f(cp=12),
        'pool fwd misaligned': pool_f(xp=Y + 2), 'pool fwd s 0': pool_f(ss=0),
        'pool bwd lddy < Cp': pool_b(lddy=8), 'pool bwd lddx < Cp': pool_b(lddx=8), 'pool bwd Cp 12': pool_b(cp=12),
        'pool bwd misaligned': pool_b(xp=Y + 2), 'pool bwd s 0': pool_b(ss=0),
    }
    # the two-pass entry point, at a size where the two-pass runs
    b2, cp2, h2, w2, H2, W2 = 1, 96, 16, 24, 64, 96
    nbytes = lib.vkas_resize_bwd_ws_bytes(b2, h2, w2, H2, W2, cp2)
    assert nbytes == b2 * H2 * w2 * cp2 * 4
    dy2 = torch.zeros((b2, H2, W2, 128), dtype=dtype, device='cuda')
    dx2 = torch.full((b2, h2, w2, 128), SENTINEL, dtype=dtype, device='cuda')
    ws = torch.full((nbytes // 4 + GUARD,), 7.25, device='cuda')
    D2, X2, WS = dy2.data_ptr() + 16, dx2.data_ptr() + 16, ws.data_ptr()

    def bws(dp=D2, lddy=128, xp=X2, lddx=128, wsp=WS, nb=nbytes, b=b2, cp=cp2, mode=0):
        return lib.vkas_resize_bwd_ws(dp, lddy, xp, lddx, wsp, nb, b, h2, w2, H2, W2, cp, mode, 0, code, st)

    assert bws() == 0
    torch.cuda.synchronize()
    dx2.fill_(SENTINEL)
    ws.fill_(7.25)
    refused.update({
        'ws mode 2': bws(mode=2), 'ws lddy < Cp': bws(lddy=88), 'ws lddx < Cp': bws(lddx=88), 'ws Cp 92': bws(cp=92),
        'ws dy misaligned': bws(dp=D2 + 2), 'ws dx misaligned': bws(xp=X2 + 2), 'ws one byte short': bws(nb=nbytes - 1),
        'ws misaligned workspace': bws(wsp=WS + 4), 'ws NULL, mode 2': bws(wsp=None, mode=2),
    })
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in refused.values()), {k: rc for k, rc in refused.items() if rc == 0}
    # B = 0: accepted, nothing launched
    assert fwd(b=0) == 0 and bwd(b=0) == 0 and pool_f(b=0) == 0 and pool_b(b=0) == 0 and bws(b=0) == 0
    assert lib.vkas_resize_bwd_ws_bytes(0, h2, w2, H2, W2, cp2) == 0
    torch.cuda.synchronize()
    for t in (x, y, dx2):
        assert bool((t == SENTINEL).all()), 'a refused or empty call wrote to a tensor'
    assert bool((ws == 7.25).all()), 'a refused or empty call wrote to the workspace'
