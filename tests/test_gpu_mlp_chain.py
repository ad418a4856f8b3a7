"""Direct parity of the fused ConvNeXt MLP kernels of csrc/mlp_chain.hip (nine instantiations of mlp_chain_kernel and the pair-split
mlp_chain_pair_kernel, both directions, the LayerNorm-fused and the inference forward, both packed weight images), through the C
ABI (vkas_mlp_chain_image_elems, vkas_mlp_chain_pack, vkas_mlp_chain_fwd, vkas_mlp_chain_ln_fwd, vkas_mlp_chain_bwd) with ctypes,
so strides, M and rows_per_image are the test's own and the host's eligibility rules (ops.mlp_chain_eligible: no pair kernel
below 16384 rows, nothing above 384 channels) do not decide which kernel runs.

Reference: fp64 on the host, stage by stage, on the values the kernel sees (include/vkas.h is the contract; W1, W2 and the
activations pre-rounded to the storage type, b1, b2, colscale, rowscale, gamma, beta fp32):
  yn, stats  LayerNorm of y (eps 1e-6, biased variance): yn at TOL, mean | rstd at the fp32 row of TOL.  The stored yn is then
             the input of a plain vkas_mlp_chain_fwd call whose h, z and out must be BIT-equal to the fused call's.
  h          yn W1^T + b1, one rounding: TOL.
  z          round_T(gelu(h_stored)) W2^T + b2 with the exact erf GELU and the kernel's own h read back: TOL + the allowance below.
  out        round_T(x + rowscale colscale z_stored): TOL.  Also end to end, fp64 straight from yn (and from y for the fused
             call) with no rounding in between, at the forward bound of test_convnext_layer (TOL): its element half per case,
             its norm-wise half over the rows of all cases of a width (one row is too few elements for a norm).
  dh         round_T((dz W2) gelu'(h)): TOL + the allowance below.  dyn from the stored dh and W1: TOL.  End to end dyn: from dz and the
             stored h (the backward's own inputs; not from yn) with
             nothing rounded in between: the gradient bound of test_convnext_layer (1.5e-2 bf16 / 3e-3 f16, norm-wise).
The 16-bit kernels evaluate GELU and GELU' by polynomials; vkas_common.h documents |gelu error| <= 5e-5 and |gelu' error| <=
1.8e-4.  Propagated linearly that is 5e-5 sum_k |W2[n, k]| per element of z and 1.8e-4 |dg| per element of dh, and norm-wise the
norm of those allowances over the norm of the reference.  The test computes both from its own operands; nothing is fitted.

Whether TOL and these allowances leave room was settled on the host before any GPU run (tests/test_cpu_mlp_chain_reference.py:
fp32 accumulation, the roundings above, exact GELU / GELU' shifted by the documented error with all-plus signs, random signs and
the worst sign per output).  Largest measured / smallest bound over C = 40, 96, 272 (M = 805, 805, 421), norm-wise, and in
brackets the worst element beyond its allowance over the peak:
  bf16  yn 1.5e-5 / 4e-3   mean, rstd 6e-8 / 2e-5   h 1.67e-3 / 4e-3 (3.3e-3 / 2e-2)   z 1.80e-3 / 4.73e-3 (2.8e-3 / 2e-2)
        out 2.4e-6 / 4e-3   dh 1.12e-3 / 4.27e-3 (3.3e-3 / 2e-2)   dyn 1.67e-3 / 4e-3 (2.6e-3 / 2e-2)
        out end to end 2.09e-3 / 4e-3   dyn end to end 2.37e-3 / 1.5e-2
  f16   yn 8e-6 / 6e-4   mean, rstd 6e-8 / 2e-5   h 2.09e-4 / 6e-4 (4.1e-4 / 4e-3)   z 2.77e-4 / 1.33e-3 (2.4e-4 / 4e-3)
        out 2.5e-6 / 6e-4   dh 4.11e-4 / 8.65e-4 (6.9e-4 / 4e-3)   dyn 2.09e-4 / 6e-4 (3.3e-4 / 4e-3)
        out end to end 2.60e-4 / 6e-4   dyn end to end 4.0e-4 / 3e-3
A z column with every GELU error pushed towards the sign of that column's own weights stays at 2.7e-3 (bf16) / 3.3e-4 (f16) of
the peak beyond its allowance, against 2e-2 / 4e-3.  So every stage bound has a factor 2.1 (f16 dh) to 9 to spare and the
allowances are used as derived: nothing was raised.  The two end-to-end comparisons keep the layer bounds of test_convnext_layer
untouched; bf16 out sits at 2.09e-3 of 4e-3 there (a factor 1.9), which is the one rounding of out = x + scale z itself.

The exact-mapping tests are what catches a single wrong k term (at K = 4C = 1536 one misplaced term moves z by ~0.4 % of its
peak: under every bound above).  Their operands are small integers, every product and partial sum is exactly representable, so
the kernel must match fp64 BIT for BIT; gelu(0) = 0 and gelu'(0) = 0.5 exactly in the kernel's form (x * cdf, fma(0, p, 0.5)) and
round_T(gelu(8)) = 8 because 5e-5 is far below half an ulp at 8.  The CPU file asserts these preconditions.

The case table is derived from chain_ks / launch_chain (Python copies below, asserted against vkas_mlp_chain_image_elems), so a
retuned dispatch cannot silently move a case to another kernel form.
"""
import ctypes
import math
import os

import pytest
import torch

from tests import parity_log
from tests.test_gpu_ops import DTYPES, TOL, q, rnd

pytestmark = pytest.mark.gpu

CDT = [d for d in DTYPES if d != torch.float32]  # the chain kernels are 16-bit only
IDS = {torch.bfloat16: 'bf16', torch.float16: 'f16'}
CODE = {torch.bfloat16: 1, torch.float16: 2}  # VKAS_BF16 / VKAS_F16
GELU_ERR, DGELU_ERR = 5e-5, 1.8e-4  # vkas_common.h: |gelu error|, |gelu' error| of the 16-bit polynomial forms
LAYER_GTOL = {torch.bfloat16: 1.5e-2, torch.float16: 3e-3}  # gradient bound of test_gpu_ops.test_convnext_layer
SENTINEL = -12352.0  # exact in both storage types (and fp32), far outside every value here
TAIL = 64            # rows behind M that no launch may touch (inputs: NaN there)
OFF = 8              # first column of every operand inside its wider buffer
BLOCK = 8192         # rows per block of the fp64 reference


# ---------------------------------------------------------------------------------------------------- dispatch, case table
def chain_ks(C):
    """Python copy of chain_ks (mlp_chain.hip): 32-wide K steps of the instantiation that covers C, 0 = not covered."""
    if C <= 0 or C % 8 != 0 or C > 512:
        return 0
    ks = (C + 31) // 32
    return ks if ks <= 4 else (6 if ks <= 6 else (8 if ks <= 8 else (12 if ks <= 12 else 16)))


def chain_img_elems(ks):
    """Python copy of chain_img_elems: GEMM-a tile [32][KA] + GEMM-b tile [32 KS][32] + the 1-KB bias piece, per chunk."""
    return 32 * ((ks + 1) // 2) * 64 + ks * 32 * 32 + 512


def kernel_form(C, pair=True):
    """Python copy of launch_chain: (kernel form, rows per workgroup).  mlp_chain_kernel<KS, TM>: 4 waves x TM x 16 rows, TM = 4
    up to KS = 3 and 2 beyond; KS = 12 with C % 16 == 0 (and VKAS_CHAIN_PAIR unset): mlp_chain_pair_kernel, 128 rows."""
    ks = chain_ks(C)
    if ks == 12 and C % 16 == 0 and pair:
        return 'pair12', 128
    return 'ks%d' % ks, 4 * (4 if ks <= 3 else 2) * 16


def cdiv(a, b):
    return (a + b - 1) // b


# width -> (kernel form, rows per workgroup), written by hand: the top of every KS range, and below it a width with C % 32 != 0
# and C / 8 odd (an odd chunk count: the last chunk pair of the 4C-wide tensor is half a pair, padding columns next to live
# memory).  272: the second wave of a pair owns 80 live and 112 padding columns; 360 / 264: C % 16 != 0 -> the one-wave KS = 12.
WIDTHS = {
    32: ('ks1', 256), 8: ('ks1', 256), 24: ('ks1', 256), 64: ('ks2', 256), 40: ('ks2', 256), 96: ('ks3', 256), 72: ('ks3', 256),
    128: ('ks4', 128), 104: ('ks4', 128), 192: ('ks6', 128), 136: ('ks6', 128), 256: ('ks8', 128), 200: ('ks8', 128),
    384: ('pair12', 128), 272: ('pair12', 128), 360: ('ks12', 128), 264: ('ks12', 128), 512: ('ks16', 128), 392: ('ks16', 128),
}
# what is counted: the eight KS values launch_chain instantiates mlp_chain_kernel for (KS = 12 appears once in its switch, as the
# one-wave form) and the pair-split kernel: nine forward forms, each with its backward twin and both storage types
FORMS = ['ks1', 'ks2', 'ks3', 'ks4', 'ks6', 'ks8', 'ks12', 'pair12', 'ks16']
RPIS = [49, 1, 196, 5, 3]  # rows_per_image; 3 and 1 put several image boundaries inside one epilogue row step (64 / (C / 8) rows)
# one large case per production width: more workgroups than the device holds at once (256 CUs x 2 workgroups of
# mlp_chain_kernel, x 1 of the pair kernel), ragged except the stage-2 benchmark shape
LARGE = {96: (160001, 626), 192: (80001, 626), 384: (65536, 512)}


def small_ms(tile):
    """M -> expected workgroups: one row, not a multiple of 8, one row below / above a whole workgroup tile, several tiles with a
    ragged last one."""
    return {1: 1, 13: 1, tile - 1: 1, tile + 1: 2, 3 * tile + 37: 4}


def case_list():
    """(C, M, rows_per_image, rowscale given) of every random-data case."""
    out = []
    for wi, (C, (form, tile)) in enumerate(WIDTHS.items()):
        for mi, M in enumerate(small_ms(tile)):
            out.append((C, M, RPIS[(wi + mi) % len(RPIS)], M != 13))
    for C, (M, _) in LARGE.items():
        out.append((C, M, 196, True))
    return out


CASES = case_list()


# ------------------------------------------------------------------------------------------------ operands and reference
def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * torch.exp(-0.5 * x * x) * 0.3989422804014327


def f32(t):
    return t.float().double()


def rowscale_values(n):
    """A different value per image, 1.25 and 0.0 among them (stochastic depth: kept / dropped sample)."""
    i = torch.arange(n, dtype=torch.float64)
    v = 0.5 + (i % 61) / 64.0
    v[i % 7 == 0] = 1.25
    v[i % 7 == 1] = 0.0
    return v


def operands(C, M, rpi, dtype, seed=0):
    """What the kernels see, as fp64 host tensors: weights and activations rounded to the storage type, the rest fp32.  The
    scales are those of test_convnext_layer.  y (the LayerNorm input) has one constant row and one row with mean near 100 and
    unit spread."""
    H, s = 4 * C, 1000 * C + seed
    y = rnd((M, C), s + 6, 1.5) + 0.3
    if M > 2:
        y[M // 2] = 0.75
    if M > 1:
        y[M - 1] = rnd((C,), s + 7) + 100.0
    return {
        'w1': q(rnd((H, C), s + 1, 1 / math.sqrt(C)), dtype), 'b1': f32(rnd((H,), s + 2, 0.1)),
        'w2': q(rnd((C, H), s + 3, 0.5 / math.sqrt(C)), dtype), 'b2': f32(rnd((C,), s + 4, 0.1)),
        'cs': f32(1 + rnd((C,), s + 5, 0.2)), 'y': q(y, dtype), 'gamma': f32(1 + rnd((C,), s + 8, 0.1)),
        'beta': f32(rnd((C,), s + 9, 0.1)), 'x': q(rnd((M, C), s + 10), dtype), 'dz': q(rnd((M, C), s + 11), dtype),
        'rs': f32(rowscale_values(cdiv(M, rpi))),
    }


def ln64(y, gamma, beta):
    mean = y.mean(1, keepdim=True)
    var = ((y - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-6)
    return (y - mean) * rstd * gamma + beta, mean[:, 0], rstd[:, 0]


class Err:
    """Error of one stage against its reference, accumulated over row blocks: norm-wise, and the worst element after the
    per-element allowance, to be judged against the peak of the whole reference."""

    def __init__(self):
        self.d2 = self.r2 = self.a2 = self.dmax = self.peak = 0.0

    def add(self, got, ref, allow=None):
        assert got.shape == ref.shape and bool(torch.isfinite(got).all())
        d = (got - ref).abs()
        self.d2 += float((d * d).sum())
        self.r2 += float((ref * ref).sum())
        self.peak = max(self.peak, float(ref.abs().max()))
        if allow is not None:
            allow = allow.expand_as(d)
            self.a2 += float((allow * allow).sum())
            d = (d - allow).clamp_min(0.0)
        self.dmax = max(self.dmax, float(d.max()))

    def figures(self):
        n = math.sqrt(self.r2) if self.r2 > 0 else 1.0
        return math.sqrt(self.d2) / n, math.sqrt(self.a2) / n, self.dmax / max(self.peak, 1e-30)


def stage_refs(o, dtype, rows, yn, hs, zs, dhs=None, fwd=True, bwd=True):
    """fp64 references of the stages for the rows of one block.  yn: the forward's input rows, hs / zs / dhs: the kernel's stored
    h, z and dh read back.  Returns name -> (reference, per-element allowance or None)."""
    r = {}
    if fwd:
        h_ref = yn @ o['w1'].T + o['b1']
        r['h'] = (h_ref, None)
        r['z'] = (q(gelu64(hs), dtype) @ o['w2'].T + o['b2'], GELU_ERR * o['w2'].abs().sum(1)[None, :])
        scale = (o['rs'][rows] if o.get('use_rs', True) else torch.ones(len(rows), dtype=torch.float64))[:, None] * o['cs'][None, :]
        r['out'] = (q(o['x'][rows] + scale * zs, dtype), None)
        r['out e2e'] = (o['x'][rows] + scale * (gelu64(h_ref) @ o['w2'].T + o['b2']), None)
    if bwd:
        dg = o['dz'][rows] @ o['w2']
        r['dh'] = (q(dg * dgelu64(hs), dtype), DGELU_ERR * dg.abs())
        r['dyn'] = (dhs @ o['w1'], None)
        r['dyn e2e'] = ((dg * dgelu64(hs)) @ o['w1'], None)
    return r


def bounds(stage, dtype):
    """(norm-wise bound before the allowance, element bound as a fraction of the peak or None)."""
    if stage == 'dyn e2e':
        return LAYER_GTOL[dtype], None
    if stage in ('mean', 'rstd'):
        return TOL[torch.float32]
    return TOL[dtype]


def judge(errs, dtype, what, log=None):
    for stage, e in errs.items():
        rel, allow, worst = e.figures()
        bn, bp = bounds(stage, dtype)
        print('mlp_chain %-8s %-22s %-4s norm-wise %.3e (bound %.1e + %.2e)  worst element / peak %.3e' % (
            stage, what, IDS[dtype], rel, bn, allow, worst))
        if log is not None:
            key = (stage, dtype)
            if key not in log or rel / (bn + allow) > log[key][0] / (log[key][1] + log[key][2]):
                log[key] = (rel, bn, allow, what)
    for stage, e in errs.items():
        rel, allow, worst = e.figures()
        bn, bp = bounds(stage, dtype)
        assert rel < bn + allow, '%s %s %s: norm-wise %.3e >= %.1e + %.2e' % (what, stage, IDS[dtype], rel, bn, allow)
        assert bp is None or worst <= bp, '%s %s %s: worst element %.3e of the peak > %.1e' % (what, stage, IDS[dtype], worst, bp)


# ---------------------------------------------------------------------------------------------------------- device side
def vk():
    from vkit_ocr_model_adaptive_scaling_amd import _lib
    return _lib.lib


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


class Wide:
    """An (M, width) operand as columns [OFF, OFF + width) of a (M + TAIL, width + extra) buffer filled with SENTINEL.  Input
    (data given): rows >= M of the slice hold NaN, so a result that leans on them shows.  Output (data None): the slice is
    NaN-filled, so 'finite' means 'written'."""

    def __init__(self, M, width, extra, dtype, data=None):
        assert extra >= OFF and extra % 8 == 0
        self.M, self.width, self.ld, self.is_input = M, width, width + extra, data is not None
        self.buf = torch.full((M + TAIL, self.ld), SENTINEL, dtype=dtype, device='cuda')
        if data is not None:
            self.buf[:M, OFF:OFF + width] = data.to(dtype).cuda() if data.device.type == 'cpu' else data
            self.buf[M:, OFF:OFF + width] = float('nan')
        else:
            self.buf[:M, OFF:OFF + width] = float('nan')

    @property
    def ptr(self):
        return self.buf.data_ptr() + OFF * self.buf.element_size()

    @property
    def inside(self):
        return self.buf[:self.M, OFF:OFF + self.width]

    def rows(self, r0, r1):
        return self.buf[r0:r1, OFF:OFF + self.width].double().cpu()

    def check(self, name):
        """Outside columns and rows >= M bit-unchanged, every element inside written and finite."""
        b, M, w = self.buf, self.M, self.width
        assert bool((b[:, :OFF] == SENTINEL).all()) and bool((b[:, OFF + w:] == SENTINEL).all()), name + ': columns outside written'
        assert bool((b[M:, OFF:OFF + w] == SENTINEL).all()), name + ': rows >= M written'
        assert bool(torch.isfinite(self.inside).all()), name + ': an element inside was not written (or is not finite)'


def vec(t64):
    return t64.float().cuda().contiguous()


def pack(o, C, dtype):
    """Both weight images, each with a sentinel block behind it that the pack kernel must leave alone."""
    lib = vk()
    n = lib.vkas_mlp_chain_image_elems(C)
    assert n == (C // 8) * chain_img_elems(chain_ks(C)), (C, n)
    w1, w2, b1 = vec(o['w1']), vec(o['w2']), vec(o['b1'])
    imgs = []
    for mode in (0, 1):
        img = torch.full((n + 512,), SENTINEL, dtype=dtype, device='cuda')
        rc = lib.vkas_mlp_chain_pack(w1.data_ptr(), w2.data_ptr(), b1.data_ptr() if mode == 0 else None, C, mode, img.data_ptr(),
                                     CODE[dtype], stream())
        assert rc == 0, lib.vkas_last_error()
        torch.cuda.synchronize()
        assert bool((img[n:] == SENTINEL).all()), 'the pack kernel wrote behind its image'
        imgs.append(img)
    return imgs


class Dev:
    """Device-side parameters of one case (images, fp32 vectors), built once and shared by its launches."""

    def __init__(self, o, C, M, rpi, dtype, use_rs=True):
        self.C, self.M, self.rpi, self.dtype = C, M, rpi, dtype
        self.img, self.img_t = pack(o, C, dtype)
        self.b2, self.cs, self.gamma, self.beta = vec(o['b2']), vec(o['cs']), vec(o['gamma']), vec(o['beta'])
        self.rs = vec(o['rs']) if use_rs else None

    def rs_ptr(self):
        return self.rs.data_ptr() if self.rs is not None else None


def run_fwd(dv, yn_in, x_in, train=True):
    """vkas_mlp_chain_fwd: yn (ld C + 8), x (C + 16) -> h (4C + 8), z (C + 16), out (C + 24); train False: h = z = NULL."""
    lib, C, M, dt = vk(), dv.C, dv.M, dv.dtype
    h = Wide(M, 4 * C, 8, dt) if train else None
    z = Wide(M, C, 16, dt) if train else None
    out = Wide(M, C, 24, dt)
    rc = lib.vkas_mlp_chain_fwd(yn_in.ptr, yn_in.ld, dv.img.data_ptr(), dv.b2.data_ptr(), x_in.ptr, x_in.ld, dv.cs.data_ptr(),
                                dv.rs_ptr(), dv.rpi, h.ptr if train else None, h.ld if train else 0, z.ptr if train else None,
                                z.ld if train else 0, out.ptr, out.ld, M, C, CODE[dt], stream())
    assert rc == 0, lib.vkas_last_error()
    torch.cuda.synchronize()
    for name, w in (('h', h), ('z', z), ('out', out)):
        if w is not None:
            w.check('fwd ' + name)
    return {'h': h, 'z': z, 'out': out}


def run_ln_fwd(dv, y_in, x_in, train=True):
    """vkas_mlp_chain_ln_fwd: y (ld C + 16), x (C + 16) -> yn (C + 24), stats, h (4C + 24), z (C + 8), out (C + 16)."""
    lib, C, M, dt = vk(), dv.C, dv.M, dv.dtype
    yn = Wide(M, C, 24, dt) if train else None
    h = Wide(M, 4 * C, 24, dt) if train else None
    z = Wide(M, C, 8, dt) if train else None
    out = Wide(M, C, 16, dt)
    stats = None
    if train:
        stats = torch.full((M + TAIL, 2), SENTINEL, device='cuda')
        stats[:M] = float('nan')
    P = lambda w: w.ptr if w is not None else None
    L = lambda w: w.ld if w is not None else 0
    rc = lib.vkas_mlp_chain_ln_fwd(y_in.ptr, y_in.ld, dv.gamma.data_ptr(), dv.beta.data_ptr(), P(yn), L(yn),
                                   stats.data_ptr() if train else None, dv.img.data_ptr(), dv.b2.data_ptr(), x_in.ptr, x_in.ld,
                                   dv.cs.data_ptr(), dv.rs_ptr(), dv.rpi, P(h), L(h), P(z), L(z), out.ptr, out.ld, M, C, CODE[dt],
                                   stream())
    assert rc == 0, lib.vkas_last_error()
    torch.cuda.synchronize()
    for name, w in (('yn', yn), ('h', h), ('z', z), ('out', out)):
        if w is not None:
            w.check('ln fwd ' + name)
    if train:
        assert bool((stats[M:] == SENTINEL).all()), 'ln fwd stats: rows >= M written'
        assert bool(torch.isfinite(stats[:M]).all()), 'ln fwd stats: a row was not written'
    return {'yn': yn, 'stats': stats, 'h': h, 'z': z, 'out': out}


def run_bwd(dv, dz_in, h_in):
    """vkas_mlp_chain_bwd: dz (ld C + 24), h (4C + 16) -> dh (4C + 24), dyn (C + 16)."""
    lib, C, M, dt = vk(), dv.C, dv.M, dv.dtype
    dh, dyn = Wide(M, 4 * C, 24, dt), Wide(M, C, 16, dt)
    rc = lib.vkas_mlp_chain_bwd(dz_in.ptr, dz_in.ld, dv.img_t.data_ptr(), h_in.ptr, h_in.ld, dh.ptr, dh.ld, dyn.ptr, dyn.ld, M, C,
                                CODE[dt], stream())
    assert rc == 0, lib.vkas_last_error()
    torch.cuda.synchronize()
    dh.check('bwd dh')
    dyn.check('bwd dyn')
    return {'dh': dh, 'dyn': dyn}


def same_bits(a, b, what):
    assert torch.equal(bits(a), bits(b)), what


_WORST = {}


@pytest.fixture(scope='module', autouse=True)
def worst_rows():
    yield
    for (stage, dtype), (rel, bn, allow, what) in sorted(_WORST.items(), key=lambda kv: (kv[0][0], IDS[kv[0][1]])):
        parity_log.record('test_gpu_mlp_chain', 'worst %s, %s' % (stage, IDS[dtype]), rel, bn + allow,
                          'at %s; bound %.1e + allowance %.2e' % (what, bn, allow))


# ---------------------------------------------------------------------------------------------------------- 1. the table
def test_case_table():
    """The table against the Python copy of the dispatch, and that copy against the library: every width runs the form it is
    listed under, every form has a case with more than one workgroup and a ragged last tile, the pair kernel and KS = 16 are
    there, and the image size the library reports is (C / 8) chunks of chain_img_elems(KS)."""
    lib = vk()
    assert os.environ.get('VKAS_CHAIN_PAIR', '1')[:1] != '0', 'VKAS_CHAIN_PAIR=0 turns the pair12 rows of the table into ks12'
    for C, (form, tile) in WIDTHS.items():
        assert kernel_form(C) == (form, tile), (C, kernel_form(C))
        assert lib.vkas_mlp_chain_image_elems(C) == (C // 8) * chain_img_elems(chain_ks(C)), C
    assert [chain_ks(C) for C in (32, 64, 96, 128, 192, 256, 384, 512)] == [1, 2, 3, 4, 6, 8, 12, 16]  # the top of every range
    assert [chain_ks(C) for C in (8, 24, 40, 72, 104, 136, 200, 264, 392)] == [1, 1, 2, 3, 4, 6, 8, 12, 16]
    assert all(lib.vkas_mlp_chain_image_elems(C) == 0 and chain_ks(C) == 0 for C in (0, 12, 520, 768))
    assert kernel_form(384, pair=False) == ('ks12', 128)
    ragged_multi = set()
    for C, M, rpi, use_rs in CASES:
        form, tile = WIDTHS[C]
        wgs = cdiv(M, tile)
        expected = LARGE[C][1] if C in LARGE and M == LARGE[C][0] else small_ms(tile)[M]
        assert wgs == expected, (C, M, wgs, expected)
        print('mlp_chain case C=%-3d M=%-6d rows_per_image=%-3d rowscale=%-4s -> %-6s %d workgroup(s) of %d rows%s' % (
            C, M, rpi, 'yes' if use_rs else 'NULL', form, wgs, tile, ', ragged' if M % tile else ''))
        if wgs > 1 and M % tile:
            ragged_multi.add(form)
    assert ragged_multi == set(FORMS), sorted(set(FORMS) - ragged_multi)
    for C, (M, wgs) in LARGE.items():
        assert wgs > 512 // (2 if WIDTHS[C][0] == 'pair12' else 1) and WIDTHS[C][0] in ('ks3', 'ks6', 'pair12')
    # odd chunk counts (the last chunk pair is half a pair) and a rows_per_image below the epilogue's row step are in the table
    assert sum((C // 8) % 2 for C in WIDTHS) >= 9
    assert any(rpi < 64 // (C // 8) for C, M, rpi, _ in CASES if M > 256)


# ------------------------------------------------------------------------------------------------- 2. random data, fp64
def run_random_case(C, M, rpi, use_rs, dtype, pool, repeats=1):
    o = operands(C, M, rpi, dtype)
    o['use_rs'] = use_rs
    dv = Dev(o, C, M, rpi, dtype, use_rs)
    what = 'C=%d M=%d' % (C, M)
    y_in, x_in, dz_in = Wide(M, C, 16, dtype, o['y']), Wide(M, C, 16, dtype, o['x']), Wide(M, C, 24, dtype, o['dz'])
    ln = run_ln_fwd(dv, y_in, x_in)
    # the stored yn is the input of the plain forward: same kernel, same fragments -> bit-equal h, z, out
    yn_in = Wide(M, C, 8, dtype, ln['yn'].inside)
    fw = run_fwd(dv, yn_in, x_in)
    for k in ('h', 'z', 'out'):
        same_bits(ln[k].inside, fw[k].inside, '%s: %s of the LayerNorm-fused forward differs from the plain forward on its yn' % (what, k))
    # inference forms: nothing stored, the same out
    same_bits(run_fwd(dv, yn_in, x_in, train=False)['out'].inside, fw['out'].inside, what + ': inference out (plain)')
    same_bits(run_ln_fwd(dv, y_in, x_in, train=False)['out'].inside, ln['out'].inside, what + ': inference out (LayerNorm-fused)')
    h_in = Wide(M, 4 * C, 16, dtype, fw['h'].inside)
    bw = run_bwd(dv, dz_in, h_in)
    for rep in range(1, repeats):  # race screen: no atomics anywhere, so every launch gives the same bits
        ln2, fw2, bw2 = run_ln_fwd(dv, y_in, x_in), run_fwd(dv, yn_in, x_in), run_bwd(dv, dz_in, h_in)
        for k in ('yn', 'stats', 'h', 'z', 'out'):
            same_bits(ln2[k] if k == 'stats' else ln2[k].inside, ln[k] if k == 'stats' else ln[k].inside,
                      '%s: LayerNorm-fused forward, %s differs in launch %d' % (what, k, rep + 1))
        for k in ('h', 'z', 'out'):
            same_bits(fw2[k].inside, fw[k].inside, '%s: forward, %s differs in launch %d' % (what, k, rep + 1))
        for k in ('dh', 'dyn'):
            same_bits(bw2[k].inside, bw[k].inside, '%s: backward, %s differs in launch %d' % (what, k, rep + 1))
        del ln2, fw2, bw2
    names = ['yn', 'mean', 'rstd', 'h', 'z', 'out', 'out e2e', 'dh', 'dyn', 'dyn e2e'] + (['out e2e ln'] if M <= 4096 else [])
    errs = {k: Err() for k in names}
    for r0 in range(0, M, BLOCK):
        r1 = min(M, r0 + BLOCK)
        rows = torch.arange(r0, r1) // rpi
        yb = o['y'][r0:r1]
        yn_ref, mean, rstd = ln64(yb, o['gamma'], o['beta'])
        errs['yn'].add(ln['yn'].rows(r0, r1), q(yn_ref, dtype))
        st = ln['stats'][r0:r1].double().cpu()
        errs['mean'].add(st[:, 0], mean)
        errs['rstd'].add(st[:, 1], rstd)
        ob = dict(o, x=o['x'][r0:r1], dz=o['dz'][r0:r1], rs=o['rs'][rows])
        ref = stage_refs(ob, dtype, torch.arange(r1 - r0), yn_in.rows(r0, r1), fw['h'].rows(r0, r1), fw['z'].rows(r0, r1),
                         bw['dh'].rows(r0, r1))
        got = {'h': fw['h'], 'z': fw['z'], 'out': fw['out'], 'out e2e': fw['out'], 'dh': bw['dh'], 'dyn': bw['dyn'], 'dyn e2e': bw['dyn']}
        for k, (rv, allow) in ref.items():
            errs[k].add(got[k].rows(r0, r1), rv, allow)
        if 'out e2e ln' in errs:  # the fused call end to end: fp64 LayerNorm -> MLP -> residual straight from y
            e2e = stage_refs(ob, dtype, torch.arange(r1 - r0), yn_ref, fw['h'].rows(r0, r1), fw['z'].rows(r0, r1), bwd=False)['out e2e'][0]
            errs['out e2e ln'].add(ln['out'].rows(r0, r1), e2e)
    # out end to end: the layer bound is a norm over a feature map, and a case of one row is 8 - 512 elements, over which the one
    # rounding of out alone reaches it with the exact contract (tests/test_cpu_mlp_chain_reference.py asserts that).  So the
    # element half of the bound is asserted here, per case, and the norm-wise half over the rows of all cases of the width.
    for k in [k for k in errs if k.startswith('out e2e')]:
        e = errs.pop(k)
        assert e.dmax <= bounds(k, dtype)[1] * e.peak, '%s %s %s: worst element %.3e vs peak %.3e' % (what, k, IDS[dtype], e.dmax, e.peak)
        t = pool.setdefault(k, Err())
        t.d2, t.r2, t.dmax, t.peak = t.d2 + e.d2, t.r2 + e.r2, max(t.dmax, e.dmax), max(t.peak, e.peak)
    judge(errs, dtype, what, _WORST)


@pytest.mark.parametrize('dtype', CDT, ids=['bf16', 'f16'])
@pytest.mark.parametrize('C', list(WIDTHS), ids=lambda c: 'C%d' % c)
def test_stages_against_fp64(C, dtype):
    """LayerNorm-fused forward, plain forward on its stored yn, both inference forms and the backward at every M of one width,
    every operand a channel slice of a wider buffer with its own ld; each stage of each case against fp64 on the values the
    kernel saw, out end to end per element in each case and norm-wise over the width's rows."""
    pool = {}
    for case in [c for c in CASES if c[0] == C and c[1] <= 4096]:
        run_random_case(*case, dtype, pool)
    judge(pool, dtype, 'C=%d all M' % C, _WORST)


@pytest.mark.parametrize('dtype', CDT, ids=['bf16', 'f16'])
@pytest.mark.parametrize('case', [c for c in CASES if c[1] > 4096], ids=lambda c: 'C%d-M%d-rpi%d' % c[:3])
def test_large_stages_and_repeatability(case, dtype):
    """The same at the large case of each production width (more workgroups than the device holds at once), and three launches
    of every kernel on the same operands agree bit for bit in every output: a race screen for the LDS-DMA rings, as
    test_rowslab_kernels_repeatable is for the slab kernels.  A fixed three launches, one pass, nothing retried."""
    pool = {}
    run_random_case(*case, dtype, pool, repeats=3)
    judge(pool, dtype, 'C=%d M=%d' % case[:2], _WORST)


# ------------------------------------------------------------------------------------------------------ 3. exact mapping
def exact_m(C):
    """Ragged, several workgroup tiles at every width, and >= 4C."""
    return max(4 * C, 2 * kernel_form(C)[1]) + 37


def sparse_rows(M, C, nnz, seed):
    """(M, C) rows with nnz entries of +-1 at channels base + i C / 8; the first C rows rotate the base with the row index, so
    every channel is hit, the rest draw it at random, so that over M rows the channels meet every row slot of the fragments."""
    g = torch.Generator().manual_seed(seed)
    base = torch.arange(M) % C
    base[C:] = torch.randint(0, C, (max(M - C, 0),), generator=g)
    cols = (base[:, None] + torch.arange(nnz)[None, :] * (C // 8)) % C
    sign = torch.randint(0, 2, (M, nnz), generator=g).double() * 2 - 1
    t = torch.zeros((M, C), dtype=torch.float64)
    t.scatter_(1, cols, sign)
    return t


def int_matrix(shape, lim, seed, pattern):
    """Integers in [-lim, lim]: random, or (pattern) a distinct value per (row, column) modulo the range - 2 row + column modulo
    2 lim + 1 - so that neighbours in either direction differ at every shape."""
    if pattern:
        idx = 2 * torch.arange(shape[0], dtype=torch.int64)[:, None] + torch.arange(shape[1], dtype=torch.int64)[None, :]
        return (idx % (2 * lim + 1) - lim).double()
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-lim, lim + 1, shape, generator=g).double()


def exact_h_operands(C, pattern):
    """h = yn W1^T + b1 with yn rows of at most 8 entries +-1, W1 in {-2 .. 2}, b1 in {-3 .. 3}: |h| <= 19."""
    M, H = exact_m(C), 4 * C
    o = {'w1': int_matrix((H, C), 2, 11, pattern), 'b1': int_matrix((H, 1), 3, 12, False)[:, 0], 'w2': torch.zeros((C, H), dtype=torch.float64),
         'b2': torch.zeros(C, dtype=torch.float64), 'cs': torch.ones(C, dtype=torch.float64), 'yn': sparse_rows(M, C, min(8, C), 13),
         'x': torch.zeros((M, C), dtype=torch.float64), 'rs': torch.ones(cdiv(M, 49), dtype=torch.float64)}
    o['h'] = o['yn'] @ o['w1'].T + o['b1']
    o['bound'] = o['yn'].abs() @ o['w1'].abs().T + o['b1'].abs()
    return M, o


def exact_z_operands(C, quarter, pattern):
    """Row m is one-hot at channel m mod C and W1 holds a single 8 per row of ONE quarter of the hidden units (row quarter C +
    c, column c; a one-hot input row reaches all four hidden units that share its channel, so one active unit per row takes one
    launch per quarter): h = 8 at hidden unit j = quarter C + m mod C and 0 elsewhere, gelu(0) = 0, round_T(gelu(8)) = 8, so
    z[m, n] = 8 W2[n, j] + b2[n] exactly; over the four launches every column of every GEMM-b tile is probed.  W2 in {-6 .. 6},
    b2 in {-4 .. 4}, x in {-16 .. 16}, colscale and rowscale in {0, 1, 2}: |out| <= 16 + 4 * 52 = 224."""
    M, H = exact_m(C), 4 * C
    g = torch.Generator().manual_seed(21 + quarter)
    yn = torch.zeros((M, C), dtype=torch.float64)
    yn[torch.arange(M), torch.arange(M) % C] = 1.0
    w1 = torch.zeros((H, C), dtype=torch.float64)
    w1[quarter * C + torch.arange(C), torch.arange(C)] = 8.0
    o = {'w1': w1, 'b1': torch.zeros(H, dtype=torch.float64), 'w2': int_matrix((C, H), 6, 22, pattern),
         'b2': int_matrix((C, 1), 4, 23, False)[:, 0], 'cs': torch.randint(0, 3, (C,), generator=g).double(), 'yn': yn,
         'x': torch.randint(-16, 17, (M, C), generator=g).double(), 'rs': torch.randint(0, 3, (cdiv(M, 49),), generator=g).double()}
    o['h'] = yn @ w1.T
    j = quarter * C + torch.arange(M) % C
    o['z'] = 8.0 * o['w2'][:, j].T + o['b2']
    o['out'] = o['x'] + o['rs'][torch.arange(M) // 49][:, None] * o['cs'][None, :] * o['z']
    o['bound'] = torch.maximum(o['z'].abs().max(), (o['x'].abs() + 4 * o['z'].abs()).max())
    return M, o


def exact_bwd_operands(C, pattern):
    """h = 0, where gelu' is exactly 0.5: dh = 0.5 (dz W2), dyn = dh W1.  dz rows of at most 4 entries +-1, W2 in {-3 .. 3}
    (|dg| <= 12, |dh| <= 6 in steps of 0.5); W1 has two entries of +-1 / +-2 per row, at columns j and j + 1 + 2 (j / C) mod C, so a
    column of W1 holds exactly 8 of them and |dyn| <= 6 * 8 * 2 = 96 with every partial sum below it."""
    M, H = exact_m(C), 4 * C
    g = torch.Generator().manual_seed(31)
    j = torch.arange(H)
    w1 = torch.zeros((H, C), dtype=torch.float64)
    vals = torch.randint(1, 3, (H, 2), generator=g).double() * (torch.randint(0, 2, (H, 2), generator=g).double() * 2 - 1)
    w1[j, j % C] = vals[:, 0]
    w1[j, (j + 1 + 2 * (j // C)) % C] = vals[:, 1]
    o = {'w1': w1, 'b1': torch.zeros(H, dtype=torch.float64), 'w2': int_matrix((C, H), 3, 32, pattern), 'dz': sparse_rows(M, C, min(4, C), 33)}
    dg = o['dz'] @ o['w2']
    o['dh'] = 0.5 * dg
    o['dyn'] = o['dh'] @ w1
    o['bound'] = torch.maximum((o['dz'].abs() @ o['w2'].abs()).max(), ((0.5 * o['dz'].abs() @ o['w2'].abs()) @ w1.abs()).max())
    return M, o


def first_mismatch(got, ref):
    bad = (got != ref).nonzero()
    return 'equal' if bad.numel() == 0 else '%d elements differ, first (row, column) %s: got %s, expected %s' % (
        bad.shape[0], bad[0].tolist(), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])]))


def fwd_exact(C, M, o, dtype):
    z1 = torch.zeros(C, dtype=torch.float64)
    dv = Dev(dict(o, gamma=z1, beta=z1), C, M, 49, dtype)
    fw = run_fwd(dv, Wide(M, C, 8, dtype, o['yn']), Wide(M, C, 16, dtype, o['x']))
    return {k: fw[k].rows(0, M) for k in ('h', 'z', 'out')}


@pytest.mark.parametrize('dtype', CDT, ids=['bf16', 'f16'])
@pytest.mark.parametrize('pattern', [False, True], ids=['random', 'indexed'])
@pytest.mark.parametrize('C', list(WIDTHS), ids=lambda c: 'C%d' % c)
def test_exact_h(C, pattern, dtype):
    """Forward GEMM-a and the A region of the forward image: integer operands, h bit for bit.  'indexed': W1 holds a distinct
    value per (hidden unit, channel) modulo its range (the pack-image check for W1)."""
    M, o = exact_h_operands(C, pattern)
    got = fwd_exact(C, M, o, dtype)
    assert torch.equal(got['h'], o['h']), 'h, %s C=%d: %s' % (kernel_form(C)[0], C, first_mismatch(got['h'], o['h']))


@pytest.mark.parametrize('dtype', CDT, ids=['bf16', 'f16'])
@pytest.mark.parametrize('pattern', [False, True], ids=['random', 'indexed'])
@pytest.mark.parametrize('C', list(WIDTHS), ids=lambda c: 'C%d' % c)
def test_exact_z_and_out(C, pattern, dtype):
    """Forward GEMM-b, the B region of the forward image with its baked-in k permutation, b2 and the residual epilogue: one
    active hidden unit per row, z and out bit for bit.  'indexed': a distinct W2 value per (channel, hidden unit)."""
    for quarter in range(4):
        M, o = exact_z_operands(C, quarter, pattern)
        got = fwd_exact(C, M, o, dtype)
        for k in ('h', 'z', 'out'):
            assert torch.equal(got[k], o[k]), '%s, %s C=%d, hidden quarter %d: %s' % (k, kernel_form(C)[0], C, quarter, first_mismatch(got[k], o[k]))


@pytest.mark.parametrize('dtype', CDT, ids=['bf16', 'f16'])
@pytest.mark.parametrize('pattern', [False, True], ids=['random', 'indexed'])
@pytest.mark.parametrize('C', list(WIDTHS), ids=lambda c: 'C%d' % c)
def test_exact_backward(C, pattern, dtype):
    """Backward GEMM-a (A region of the backward image = W2 transposed), GELU' at 0 and GEMM-b (B region = W1 under the k
    permutation): dh and dyn bit for bit."""
    M, o = exact_bwd_operands(C, pattern)
    z1 = torch.zeros(C, dtype=torch.float64)
    dv = Dev(dict(o, b2=z1, cs=z1, gamma=z1, beta=z1, rs=z1[:1]), C, M, 49, dtype)
    bw = run_bwd(dv, Wide(M, C, 24, dtype, o['dz']), Wide(M, 4 * C, 16, dtype, torch.zeros((M, 4 * C), dtype=torch.float64)))
    for k in ('dh', 'dyn'):
        got = bw[k].rows(0, M)
        assert torch.equal(got, o[k]), '%s, %s C=%d: %s' % (k, kernel_form(C)[0], C, first_mismatch(got, o[k]))


# --------------------------------------------------------------------------------------------- 4. empty input, refusals
def test_empty_and_refused_calls():
    """M = 0 returns 0 and writes nothing; h without z, a pixel stride below the width or not a multiple of 8, a misaligned
    pointer and an uncovered width are refused with no kernel launched."""
    lib = vk()
    C, M, dtype = 24, 40, torch.bfloat16
    o = operands(C, M, 49, dtype)
    dv = Dev(o, C, M, 49, dtype)
    yn, x, dz = Wide(M, C, 8, dtype, o['y']), Wide(M, C, 16, dtype, o['x']), Wide(M, C, 24, dtype, o['dz'])
    h, z, out, dh, dyn = Wide(M, 4 * C, 8, dtype), Wide(M, C, 16, dtype), Wide(M, C, 24, dtype), Wide(M, 4 * C, 24, dtype), Wide(M, C, 16, dtype)
    hin = Wide(M, 4 * C, 16, dtype, torch.zeros((M, 4 * C), dtype=torch.float64))
    stats = torch.full((M, 2), SENTINEL, device='cuda')

    def fwd(m=M, c=C, ynp=yn.ptr, ldyn=yn.ld, hp=h.ptr, zp=z.ptr, ldo=out.ld):
        return lib.vkas_mlp_chain_fwd(ynp, ldyn, dv.img.data_ptr(), dv.b2.data_ptr(), x.ptr, x.ld, dv.cs.data_ptr(), dv.rs_ptr(), 49,
                                      hp, h.ld, zp, z.ld, out.ptr, ldo, m, c, CODE[dtype], stream())

    def bwd(m=M, c=C, lddh=dh.ld, dzp=dz.ptr):
        return lib.vkas_mlp_chain_bwd(dzp, dz.ld, dv.img_t.data_ptr(), hin.ptr, hin.ld, dh.ptr, lddh, dyn.ptr, dyn.ld, m, c,
                                      CODE[dtype], stream())

    refused = [fwd(c=12), fwd(c=520), fwd(ldyn=C - 8), fwd(ldyn=C + 4), fwd(ynp=yn.ptr + 2), fwd(hp=None), fwd(zp=None),
               fwd(ldo=C - 8), fwd(m=-1), bwd(c=12), bwd(lddh=4 * C - 8), bwd(dzp=dz.ptr + 2), bwd(m=-1)]
    ln0 = lib.vkas_mlp_chain_ln_fwd(yn.ptr, yn.ld, dv.gamma.data_ptr(), dv.beta.data_ptr(), z.ptr, z.ld, stats.data_ptr(),
                                    dv.img.data_ptr(), dv.b2.data_ptr(), x.ptr, x.ld, dv.cs.data_ptr(), dv.rs_ptr(), 49, h.ptr, h.ld,
                                    z.ptr, z.ld, out.ptr, out.ld, 0, C, CODE[dtype], stream())
    assert fwd(m=0) == 0 and bwd(m=0) == 0 and ln0 == 0
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in refused), refused
    for w in (h, z, out, dh, dyn):
        assert bool(torch.isnan(w.inside).all()) and bool((w.buf[M:] == SENTINEL).all()), 'a refused or empty call wrote'
    assert bool((stats == SENTINEL).all()), 'the empty LayerNorm-fused call wrote stats'
    assert fwd() == 0 and bwd() == 0  # the accepted calls: every refusal above was down to its one argument
    torch.cuda.synchronize()
