"""Direct parity of the implicit-GEMM kernels of csrc/gemm_mfma.hip (and the fp32 kernels of csrc/gemm_simple.hip) through the C
ABI (vkas_conv_gemm_fwd, vkas_conv_gemm_wgrad, vkas_conv_gemm_wgrad_gelu, vkas_conv_gemm_wgrad_ordered) with ctypes: geometry,
strides, M and N are the test's own, Bw is built here in the contract's (Np, KH, KW, Cp) layout (no pack kernel), and the host's
dispatch rules do not decide which kernel a case reaches.

Kernel forms.  VKAS_NT_TILE, VKAS_TN_TILE, VKAS_NT_RING, VKAS_NT_NOSLAB, VKAS_NT_NOBUF and VKAS_TN_NOBUF are read once per process,
so every entry of SETTINGS is one child process (started lazily, one at a time, each under a time limit; after a child that
timed out or ended abnormally no further child is started and the remaining tests fail with that message).  A child runs all
cases of its setting in both 16-bit types (the default child also in fp32: gemm_simple.hip and epi_store4), records
vkas_conv_gemm_kernel_id / vkas_conv_gemm_tile of every case (a retuned dispatch cannot silently move a case to another kernel),
checks the guards on the device and saves the outputs; the parent computes fp64 references on the host and compares per case.
The kernel id names the tile, the ring depth and the slab kernel; buffer against non-buffer and the NOBIAS / PW instantiations
come from vkas_conv_gemm_plan, the plan the launchers execute (csrc/gemm_plan.h; tests/test_cpu_gemm_plan.py holds it to the
previous launchers): the child records it per case and the parent asserts it against the setting.  NOBIAS exists with buffer
loads only: 'no gb' on a non-buffer tile is the plain non-buffer kernel with a null gb.
  forward   register-staged 128x128, ring 2 / 3 / 4, 256x128 / 192 / 224 buffer and non-buffer, row-slab 4 / 6 / 7
  wgrad     tile 128 / 192 / 224 / 384 x buffer / non-buffer x plain (gb) / plain (no gb: NOBIAS at 192 / 384 pointwise) / GELU / ordered

Guards of every case: outputs live in columns [8, 8 + Np) of a buffer that is 16 columns wider and 16 rows longer, pre-filled
with a sentinel that is exact in every storage type (NaN inside, so 'finite' means 'written'); nothing outside may change (fp32 gw
/ gb: 64 floats behind them).  Inputs are such slices too (x, dy, aux): their neighbour columns hold 1024 (a kernel that uses them
moves an exact result by >= 1024), the rows behind the last one NaN, as do the rows behind Bw, bias, colscale and rowscale.
Weight rows / bias / aux columns [N, Np), N = Np - 3, are zero, and the outputs must be zero there.  gw / gb are pre-filled with an
integer pattern (the ABI adds).

Two kinds of comparison per case.
  exact   x, dy in {-1, 0, 1} (thinned so that sums stay small), weights, bias, aux in {-2 .. 2}, colscale in {-1, 1, 2}, rowscale
          in {0, 1, 2}: every product and partial sum is an integer below 2^24, every stored value an integer of magnitude <= 256,
          so the result must match fp64 BIT for BIT in any summation order (tests/test_cpu_gemm_reference.py asserts both
          conditions for every case of the table).  GELU's out2 and DGELU's out are compared with the kernel's own stored
          pre-activation (resp. the exact v) at |diff| <= 5e-5 (1.8e-4 |v|) + u |ref|, u = 2^-8 bf16, 2^-11 f16: the polynomial
          errors documented in vkas_common.h.  fp32 storage keeps erff / expf (gelu_f, dgelu_f), gets no allowance and is held
          to the plain TOL there.  The GELU weight gradient uses x in {0, 4}: round_T(gelu(4)) = 4 in both 16-bit types.
  random  normal operands pre-rounded to the storage type, fp64 reference on the stored values with the kernel's one extra rounding
          (nt_epilogue rounds acc + bias to the storage type before the mode's arithmetic); bounds: TOL of test_gpu_ops
          (norm-wise, peak-relative), fp32 weight gradients 1e-5 norm-wise, the GELU / GELU' allowances (bf16 and f16 only; none
          for fp32) propagated linearly as in test_gpu_mlp_chain.py.  The GELU weight gradient's operand is round_T(gelu(x)): a
          value moved by up to 5e-5 may round to the neighbouring number, a whole ulp away, which 1e-5 cannot absorb.  Rounding is
          monotone, so per element the operand moves by at most max |round_T(g +- 5e-5) - round_T(g)| (zero for most elements);
          that, propagated through |dy|, is the allowance.
Consistency: ring 2 / 3 / 4 and the register-staged kernel agree bit for bit; buffer and non-buffer agree bit for bit (forward)
and to 1e-6 (wgrad); slab and generic 256-row tile agree exactly on the integer cases and to TOL otherwise; _ordered is
bit-identical over three launches; GELU with out == NULL gives the bits of the call that keeps out.

Whether the bounds leave room was settled on the host first (tests/test_cpu_gemm_reference.py: fp32 accumulation in 64-wide K steps
forward and reversed, the kernel's roundings, GELU / GELU' shifted by their documented error with the worst sign per element).
Largest emulated error / bound over the whole table, norm-wise (the reference carries the kernel's own roundings, so what is left
of the plain modes is the few values fp32 accumulation rounds the other way):
  bf16  none 6.0e-5 / 4e-3   gelu out2 1.75e-3 / 4.09e-3   scale_res 3.7e-5 / 4e-3   dgelu 1.72e-3 / 4.26e-3   add 3.2e-5 / 4e-3
        patch 3.8e-5 / 4e-3   gw, gb 9.7e-8 / 1e-5   gw of the GELU entry 4.7e-4 / 1.00e-3 (1e-5 + allowance)
  f16   none 1.3e-5 / 6e-4   gelu out2 2.4e-4 / 6.9e-4   scale_res 1.8e-5 / 6e-4   dgelu 3.9e-4 / 8.6e-4   add 9.8e-6 / 6e-4
        patch 1.1e-5 / 6e-4   gw, gb 1.6e-7 / 1e-5   gw of the GELU entry 1.4e-4 / 5.4e-4
  f32   every output, GELU and GELU' included, <= 1.8e-7 / 2e-5 (no allowance)   gw, gb, gw of the GELU entry <= 1.9e-7 / 1e-5
so every bound has a factor 2.2 (f16 dgelu: two roundings and the full GELU' error, worst sign) to 390 to spare and none was
raised.  The integer cases' transcendental bound is first order (error + u |ref|; the product u x error is dropped): with the
polynomial error at 99.2 % of its documented maximum and the rounding falling the worst way the largest element sits at 0.999 of
it (f16 gelu).  With VKAS_PARITY_REPORT set the file records the largest measured error per kernel form, mode and type beside its
bound (tests/parity_log.py).
"""
import collections
import ctypes
import functools
import math
import os
import subprocess
import sys
import tempfile
import zlib

import pytest
import torch

from tests import parity_log
from tests.test_gpu_ops import TOL, q

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
CODE = {'f32': 0, 'bf16': 1, 'f16': 2}  # VKAS_F32 / VKAS_BF16 / VKAS_F16
U = {'f32': 2.0 ** -23, 'bf16': 2.0 ** -8, 'f16': 2.0 ** -11}
GELU_ERR, DGELU_ERR = 5e-5, 1.8e-4  # vkas_common.h: |gelu error|, |gelu' error| of the 16-bit polynomial forms
TRANSCENDENTAL = {('gelu', 'out2'), ('dgelu', 'out')}  # (mode, output) that goes through GELU / GELU'
WGRAD_TOL = 1e-5                    # norm-wise, fp32 weight gradients (test_wgrad_ordered_is_one_split_and_reproducible)
SENTINEL = -12352.0                 # exact in bf16, f16 and fp32, far outside every value here
NEIGHBOUR = 1024.0                  # what the columns next to an input slice hold
TAIL, OFF, EXTRA = 16, 8, 16        # rows behind an operand, first column of a slice, columns a buffer is wider than its slice
KINDS = ('exact', 'random')
SWITCHES = ('VKAS_NT_TILE', 'VKAS_TN_TILE', 'VKAS_NT_RING', 'VKAS_NT_NOSLAB', 'VKAS_NT_NOBUF', 'VKAS_TN_NOBUF', 'VKAS_TN_NOSLAB',
            'VKAS_TN_NO96', 'VKAS_GEMM', 'VKAS_LIB_PATH')
CHILD_TIMEOUT = 240

# ------------------------------------------------------------------------------------------------------------ settings
Setting = collections.namedtuple('Setting', 'env form BM BN kid slab tn dtypes')
_NB = {'VKAS_NT_NOBUF': '1', 'VKAS_TN_NOBUF': '1', 'VKAS_NT_NOSLAB': '1'}  # no slab kernel: the non-buffer tile runs its geometry
SETTINGS = {
    # name: environment, forward form, BM, BN, kernel id, slab kernel for eligible geometry, wgrad tile (None: no wgrad cases)
    'default': Setting({}, 'ring 4 (by the rule)', 128, 128, 14, False, 128, ('bf16', 'f16', 'f32')),
    'ring0': Setting({'VKAS_NT_RING': '0'}, 'register-staged 128x128', 128, 128, 1, False, None, ('bf16', 'f16')),
    'ring2': Setting({'VKAS_NT_RING': '2'}, 'ring 2', 128, 128, 12, False, None, ('bf16', 'f16')),
    'ring3': Setting({'VKAS_NT_RING': '3'}, 'ring 3', 128, 128, 13, False, None, ('bf16', 'f16')),
    'ring4': Setting({'VKAS_NT_RING': '4'}, 'ring 4', 128, 128, 14, False, None, ('bf16', 'f16')),
    't128': Setting({'VKAS_NT_TILE': '128', 'VKAS_TN_TILE': '192'}, '256x128 buffer', 256, 128, 128, True, 192, ('bf16', 'f16')),
    't192': Setting({'VKAS_NT_TILE': '192', 'VKAS_TN_TILE': '224'}, '256x192 buffer', 256, 192, 192, True, 224, ('bf16', 'f16')),
    't224': Setting({'VKAS_NT_TILE': '224', 'VKAS_TN_TILE': '384'}, '256x224 buffer', 256, 224, 224, True, 384, ('bf16', 'f16')),
    't128nb': Setting(dict(_NB, VKAS_NT_TILE='128', VKAS_TN_TILE='192'), '256x128 non-buffer', 256, 128, 128, False, 192, ('bf16', 'f16')),
    't192nb': Setting(dict(_NB, VKAS_NT_TILE='192', VKAS_TN_TILE='224'), '256x192 non-buffer', 256, 192, 192, False, 224, ('bf16', 'f16')),
    't224nb': Setting(dict(_NB, VKAS_NT_TILE='224', VKAS_TN_TILE='384'), '256x224 non-buffer', 256, 224, 224, False, 384, ('bf16', 'f16')),
    # the generic buffer tile on the slab cases' geometry; its wgrad cases: tile 128 non-buffer
    't224noslab': Setting({'VKAS_NT_TILE': '224', 'VKAS_NT_NOSLAB': '1', 'VKAS_TN_NOBUF': '1'}, '256x224 buffer, no slab', 256, 224, 224,
                          False, 128, ('bf16', 'f16')),
}
TN_BUFFER = {name: 'VKAS_TN_NOBUF' not in s.env for name, s in SETTINGS.items()}

# ---------------------------------------------------------------------------------------------------------- case tables
NT = collections.namedtuple('NT', 'geo B H W Cp Np mode opt')   # B, H, W: the INPUT image; opt: see nt_cases
TN = collections.namedtuple('TN', 'geo B H W Cp Np entry')      # entry: gb | nogb | gelu | ordered
GEO = {'pw': (1, 1, 0), 's3': (3, 1, 1), 'c3': (3, 1, 1), 'p2': (2, 2, 0), 'p4': (4, 4, 0)}  # kernel edge, stride, pad
CPS = [8, 72, 136, 200]  # K tails of BK = 64 (and of the wgrad K tiles)
NT_NPS = {128: [8, 120, 136, 392], 192: [8, 184, 200, 392], 224: [8, 216, 232, 200, 456]}
PATCH_CP = {128: 40, 192: 56, 224: 64}  # Np = 4 patch_Cp: two N tiles, the last one ragged


def geom(c):
    k, s, p = GEO[c.geo]
    Ho, Wo = (c.H + 2 * p - k) // s + 1, (c.W + 2 * p - k) // s + 1
    return dict(k=k, s=s, p=p, Ho=Ho, Wo=Wo, M=c.B * Ho * Wo, K=k * k * c.Cp, npix=c.B * c.H * c.W)


def nt_cases(BM, BN):
    """Forward cases of a form with BM x BN tiles.  opt: 'none' (bias given?,), 'sres' (out2 given?, rowscale given?,
    rows_per_image), 'patch' (patch_Cp,).  's3' is the slab-eligible geometry (W = 256, H = 3, B = 2: both halos, first and last
    image row, the image boundary); M of the pointwise cases: 1, 13, BM - 1, BM + 1, 3 BM + 37."""
    nps, rag, L = NT_NPS[BN], BN + 8, []
    for i, M in enumerate([1, 13, BM - 1, BM + 1, 3 * BM + 37]):
        L.append(NT('pw', 1, 1, M, CPS[i % 4], nps[i % len(nps)], 'none', (1,)))
    for j, Np in enumerate(nps):
        L.append(NT('pw', 1, 1, BM + 1, CPS[(j + 1) % 4], Np, 'none', (1,)))
        L.append(NT('s3', 2, 3, 256, CPS[j % 4], Np, 'none', (1,)))
    epis = [('none', (0,)), ('gelu', ()), ('sres', (1, 1, 1)), ('sres', (0, 0, 5)), ('sres', (1, 1, 49)), ('dgelu', ()), ('add', ())]
    for j, (mode, opt) in enumerate(epis):
        L.append(NT('pw', 1, 1, BM + 1, CPS[(j + 1) % 4], rag, mode, opt))  # ragged M and ragged N
        L.append(NT('s3', 2, 3, 256, CPS[(j + 2) % 4], rag, mode, opt))
    pc = PATCH_CP[BN]
    L.append(NT('pw', 2, 5, 27 if BM == 256 else 13, 72, 4 * pc, 'patch', (pc,)))
    L.append(NT('s3', 2, 3, 256, 136, 4 * pc, 'patch', (pc,)))
    L += [NT('c3', 2, 19, 37, 72, rag, 'none', (1,)), NT('c3', 2, 19, 37, 200, nps[-1], 'add', ()),
          NT('c3', 2, 19, 37, 8, nps[1], 'gelu', ()), NT('p2', 3, 22, 26, 136, rag, 'none', (1,)),
          NT('p2', 3, 22, 26, 8, nps[1], 'sres', (1, 1, 49)), NT('p4', 3, 40, 44, 8, rag, 'none', (1,)), NT('p4', 3, 40, 44, 8, 8, 'dgelu', ())]
    return list(dict.fromkeys(L))


TN_NPS = [8, 120, 200, 392]
ENTRIES = ['gb', 'nogb', 'gelu', 'ordered']


def tn_cases():
    """Weight-gradient cases (the same for every tile: Np and K = KH KW Cp have tails against 128 / 192 / 224 / 384 and 128 / 256).
    M: 1, 13, 63, 65, 257 and 1137 (several splits of whole 64-row steps with a ragged last one)."""
    L = []
    for i, M in enumerate([1, 13, 63, 65, 257, 1137]):
        L.append(TN('pw', 1, 1, M, CPS[i % 4], TN_NPS[(i + 1) % 4], ENTRIES[i % 4]))
    for j, ent in enumerate(ENTRIES):
        L.append(TN('pw', 1, 1, 1137, CPS[(j + 2) % 4], TN_NPS[j], ent))
        L.append(TN('c3', 1, 3, 379, CPS[j % 4], TN_NPS[(j + 3) % 4], ent))
        L.append(TN('p2', 1, 6, 758, CPS[(j + 1) % 4], TN_NPS[(j + 2) % 4], ent))
    L += [TN('c3', 1, 5, 13, 136, 200, 'gb'), TN('p2', 1, 10, 26, 200, 120, 'nogb')]
    return list(dict.fromkeys(L))


TN_CASES = tn_cases()


def cid(c):
    return '-'.join(str(v) if not isinstance(v, tuple) else 'o' + '_'.join(map(str, v)) for v in c)


def expected_kid(s, c):
    return 1000 + s.BN // 32 if (s.slab and c.geo == 's3') else s.kid


def plan_record(_lib, wgrad, G, Np, lddy, flags, has_gb):
    """[buf, pw, nobias, ring depth, kernel name] of the plan this process's launchers execute for the call."""
    info = _lib.GemmPlanInfo()
    rc = _lib.lib.vkas_conv_gemm_plan(wgrad, ctypes.byref(G), Np, lddy, 0, flags, int(has_gb), None, ctypes.byref(info))
    return [info.buf, info.pw, info.nobias, info.ring, info.name.decode() if rc == 0 else 'rc %d' % rc]


# ------------------------------------------------------------------------------------------------------------- operands
def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * torch.exp(-0.5 * x * x) * 0.3989422804014327


def cdiv(a, b):
    return (a + b - 1) // b


def _gen(c, kind):
    return torch.Generator().manual_seed(zlib.crc32((cid(c) + kind).encode()))


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _signs(g, shape, p):
    """-1 / 0 / 1, non-zero with probability p."""
    return (torch.rand(shape, generator=g) < p).double() * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)


def _normal(g, shape, scale, dt):
    return q(torch.randn(shape, generator=g, dtype=torch.float64) * scale, DT[dt])


def rowscale_values(n):
    i = torch.arange(n, dtype=torch.float64)
    v = 0.5 + (i % 61) / 64.0
    v[i % 7 == 0] = 1.25
    v[i % 7 == 1] = 0.0
    return v


def n_real(c):
    """Logical output channels: the last 3 of Np are padding (zero weights, bias, aux) except in the PATCH layout."""
    return c.Np if c.mode == 'patch' or c.Np < 16 else c.Np - 3


def nt_operands(c, kind, dt):
    """What the kernel sees, as fp64 host tensors (16-bit operands representable in the storage type, the rest fp32)."""
    g, gg = _gen(c, kind), geom(c)
    K, M, N = gg['K'], gg['M'], n_real(c)
    o = {}
    if kind == 'exact':
        o['x'] = _signs(g, (gg['npix'], c.Cp), min(2.0 / 3.0, 48.0 / K))  # acc: variance <= 96 whatever K
        o['w'], o['bias'], o['aux'] = _ints(g, (c.Np, K), -2, 2), _ints(g, (c.Np,), -2, 2), _ints(g, (M, c.Np), -2, 2)
        o['cs'] = torch.tensor([-1.0, 1.0, 2.0])[torch.randint(0, 3, (c.Np,), generator=g)].double()
    else:
        o['x'] = _normal(g, (gg['npix'], c.Cp), 1.0, dt)
        o['w'] = _normal(g, (c.Np, K), 1.0 / math.sqrt(K), dt)
        o['bias'] = (torch.randn((c.Np,), generator=g) * 0.1).double()
        o['aux'] = _normal(g, (M, c.Np), 1.5 if c.mode == 'dgelu' else 1.0, dt)
        o['cs'] = (1 + 0.2 * torch.randn((c.Np,), generator=g)).double()
    o['w'][N:], o['bias'][N:], o['aux'][:, N:] = 0.0, 0.0, 0.0
    if c.mode == 'sres':
        n_img = cdiv(M, c.opt[2])
        o['rs'] = _ints(g, (n_img,), 0, 2) if kind == 'exact' else rowscale_values(n_img).float().double()
    if c.mode == 'dgelu' or (c.mode == 'none' and not c.opt[0]):
        o['bias'] = None  # DGELU: out = (acc) gelu'(aux)
    return o


def tn_operands(c, kind, dt):
    g, gg = _gen(c, kind), geom(c)
    M, K = gg['M'], gg['K']
    o = {}
    if kind == 'exact':
        # GELU entry: x in {0, 4}, round_T(gelu(4)) = 4 in both 16-bit types (5e-5 + 1.3e-4 is far below half an ulp at 4)
        o['x'] = (torch.rand((gg['npix'], c.Cp), generator=g) < 1.0 / 12).double() * 4.0 if c.entry == 'gelu' else \
            _signs(g, (gg['npix'], c.Cp), 2.0 / 3.0)
        o['dy'] = _signs(g, (M, c.Np), 2.0 / 3.0)
    else:
        o['x'] = _normal(g, (gg['npix'], c.Cp), 1.5 if c.entry == 'gelu' else 1.0, dt)
        o['dy'] = _normal(g, (M, c.Np), 1.0, dt)
    o['gw0'] = (torch.arange(c.Np * K) % 7 - 3).double().view(c.Np, K)  # the ABI adds: a known integer pattern, not zeros
    o['gb0'] = (torch.arange(c.Np) % 5 - 2).double()
    return o


# ------------------------------------------------------------------------------------------------------------ reference
def im2col(x, c):
    """A(m, k) of include/vkas.h: x (npix, Cp) -> (M, KH KW Cp), k = (ky, kx, c), zero padding."""
    gg = geom(c)
    k, s, p = gg['k'], gg['s'], gg['p']
    xp = torch.zeros((c.B, c.H + 2 * p, c.W + 2 * p, c.Cp), dtype=torch.float64)
    xp[:, p:p + c.H, p:p + c.W] = x.view(c.B, c.H, c.W, c.Cp)
    taps = [xp[:, ky:ky + s * gg['Ho']:s, kx:kx + s * gg['Wo']:s] for ky in range(k) for kx in range(k)]
    return torch.cat(taps, dim=3).reshape(gg['M'], gg['K'])


def patch_scatter(v, c):
    """VKAS_EPI_PATCH: rows are the (B, Hs, Ws) grid, columns (ky, kx, c) -> pixel (b, 2 y + ky, 2 x + kx) of the (B, 2 Hs, 2 Ws,
    patch_Cp) target: the transposed 2x2 / stride 2 placement."""
    pc = c.opt[0]
    t = v.view(c.B, c.H, c.W, 2, 2, pc).permute(0, 1, 3, 2, 4, 5)  # b, y, ky, x, kx, c
    return t.reshape(c.B * c.H * 2 * c.W * 2, pc)


def poly_err(err, dt):
    """The documented error of a polynomial form: bf16 and f16 storage only.  fp32 storage keeps the erf / exp forms
    (gelu_f, dgelu_f), so it gets no allowance and is held to the plain bounds."""
    return err if dt != 'f32' else None


def staged(c, o, dt):
    """round_T(acc + bias): nt_epilogue rounds it to the storage type before the mode's arithmetic."""
    acc = im2col(o['x'], c) @ o['w'].T
    return q(acc + o['bias'] if o['bias'] is not None else acc, DT[dt])


def nt_reference(c, o, dt, stored=None, vs=None):
    """name -> (fp64 reference, per-element transcendental allowance or None).  stored: the kernel's own pre-activation (GELU:
    out) or z (SCALE_RES: out2) read back, where the contract has it stored; else the reference's.  vs: staged(c, o, dt) when
    the caller has it already."""
    gg = geom(c)
    vs = staged(c, o, dt) if vs is None else vs
    if c.mode == 'none':
        return {'out': (vs, None)}
    if c.mode == 'gelu':
        h = stored if stored is not None else vs
        return {'out': (vs, None), 'out2': (gelu64(h), torch.full_like(h, GELU_ERR) if poly_err(GELU_ERR, dt) else None)}
    if c.mode == 'sres':
        z = stored if stored is not None else vs
        rs = o['rs'][torch.arange(gg['M']) // c.opt[2]][:, None] if c.opt[1] else 1.0
        r = {'out': (o['aux'] + rs * o['cs'][None, :] * z, None)}
        if c.opt[0]:
            r['out2'] = (vs, None)
        return r
    if c.mode == 'dgelu':
        return {'out': (vs * dgelu64(o['aux']), DGELU_ERR * vs.abs() if poly_err(DGELU_ERR, dt) else None)}
    if c.mode == 'add':
        return {'out': (vs + o['aux'], None)}
    if c.mode == 'patch':
        return {'out': (patch_scatter(vs, c), None)}
    raise ValueError(c.mode)


def tn_reference(c, o, dt):
    """gw = gw0 + dy^T A (A = round_T(gelu(A)) for the GELU entry), gb = gb0 + column sums of dy.  The GELU entry's allowance
    (16-bit storage): rounding is monotone, so round_T(g + e), |e| <= GELU_ERR, lies between round_T(g - GELU_ERR) and
    round_T(g + GELU_ERR); the larger of the two distances to round_T(g) is the most one operand can move (zero for most
    elements, one ulp for the few next to a rounding boundary), propagated linearly through |dy|.  gelu(0) = 0 in the kernel."""
    A = im2col(o['x'], c)
    r = {}
    allow = None
    if c.entry == 'gelu':
        ge = gelu64(A)
        A = q(ge, DT[dt])
        if poly_err(GELU_ERR, dt):
            move = torch.maximum((q(ge + GELU_ERR, DT[dt]) - A).abs(), (q(ge - GELU_ERR, DT[dt]) - A).abs()) * (ge != 0)
            allow = o['dy'].abs().T @ move
    r['gw'] = (o['gw0'] + o['dy'].T @ A, allow)
    if c.entry in ('gb', 'gelu'):
        r['gb'] = (o['gb0'] + o['dy'].sum(0), None)
    return r


@functools.lru_cache(maxsize=None)
def nt_case_data(c, kind, dt):
    return nt_operands(c, kind, dt)


@functools.lru_cache(maxsize=None)
def nt_case_staged(c, kind, dt):
    """Computed once and shared by every setting that runs the case."""
    return staged(c, nt_case_data(c, kind, dt), dt)


@functools.lru_cache(maxsize=None)
def tn_case_data(c, kind, dt):
    o = tn_operands(c, kind, dt)
    return o, tn_reference(c, o, dt)


# ---------------------------------------------------------------------------------------------------------- comparisons
def first_mismatch(got, ref):
    bad = (got != ref).nonzero()
    return 'equal' if bad.numel() == 0 else '%d elements differ, first %s: got %s, expected %s' % (
        bad.shape[0], bad[0].tolist(), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])]))


def check_exact(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.equal(got.double(), ref), '%s: %s' % (what, first_mismatch(got.double(), ref))


def check_transcendental_exact(got, ref, allow, dt, what):
    """|got - ref| <= allowance + u |ref| per element."""
    d = (got.double() - ref).abs()
    over = d - (allow + U[dt] * ref.abs())
    assert bool(torch.isfinite(d).all()) and float(over.max()) <= 0.0, '%s: worst excess %.3e' % (what, float(over.max()))
    return float((d / (allow + U[dt] * ref.abs()).clamp_min(1e-30)).max())


def measure(got, ref, allow=None):
    """(norm-wise error, norm-wise allowance, worst element beyond its allowance over the peak)."""
    got = got.double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    d = (got - ref).abs()
    n = float(ref.norm()) or 1.0
    a = 0.0
    if allow is not None:
        a = float(allow.expand_as(d).norm()) / n
        d2 = (d - allow).clamp_min(0.0)
    else:
        d2 = d
    return float(d.norm()) / n, a, float(d2.max()) / max(float(ref.abs().max()), 1e-30)


def check_random(got, ref, allow, dt, what, wgrad=False):
    """TOL of test_gpu_ops (norm-wise + propagated allowance, worst element over the peak); fp32 weight gradients: 1e-5 norm-wise."""
    rel, a, worst = measure(got, ref, allow)
    bn, bp = (WGRAD_TOL, None) if wgrad else TOL[DT[dt]]
    assert rel < bn + a, '%s: norm-wise %.3e >= %.1e + %.2e' % (what, rel, bn, a)
    assert bp is None or worst <= bp, '%s: worst element %.3e of the peak > %.1e' % (what, worst, bp)
    return rel, bn + a, worst


# ---------------------------------------------------------------------------------------------------------- child process
class Slice:
    """(rows, width) operand as columns [OFF, OFF + width) of a (rows + TAIL, width + EXTRA) device buffer.  Input (data given):
    neighbour columns NEIGHBOUR, rows behind the last one NaN.  Output: SENTINEL outside, NaN inside ('finite' = 'written')."""

    def __init__(self, rows, width, dtype, data=None):
        self.rows, self.width, self.ld, self.is_input = rows, width, width + EXTRA, data is not None
        self.buf = torch.full((rows + TAIL, self.ld), NEIGHBOUR if data is not None else SENTINEL, dtype=dtype, device='cuda')
        if data is not None:
            self.buf[rows:] = float('nan')
            self.buf[:rows, OFF:OFF + width] = data.to(dtype).cuda()
        else:
            self.buf[:rows, OFF:OFF + width] = float('nan')

    @property
    def ptr(self):
        return self.buf.data_ptr() + OFF * self.buf.element_size()

    @property
    def inside(self):
        return self.buf[:self.rows, OFF:OFF + self.width]

    def guard(self, name):
        b, r, w = self.buf, self.rows, self.width
        m = []
        if not (bool((b[:, :OFF] == SENTINEL).all()) and bool((b[:, OFF + w:] == SENTINEL).all())):
            m.append(name + ': columns outside the slice written')
        if not bool((b[r:] == SENTINEL).all()):
            m.append(name + ': rows behind the last one written')
        if not bool(torch.isfinite(self.inside).all()):
            m.append(name + ': an element inside was not written (or is not finite)')
        return m


def _vec(t64, n_tail=8):
    """fp32 device vector with NaN behind it."""
    v = torch.full((t64.numel() + n_tail,), float('nan'), device='cuda')
    v[:t64.numel()] = t64.float().cuda()
    return v


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _geom_struct(_lib, c, ldx):
    gg = geom(c)
    return _lib.ConvGeom(c.B, c.H, c.W, gg['Ho'], gg['Wo'], c.Cp, ldx, gg['k'], gg['k'], gg['s'], gg['p'])


def child_nt(_lib, s, c, kind, dt):
    lib, T, gg = _lib.lib, DT[dt], geom(c)
    o = nt_operands(c, kind, dt)
    M, K, Np = gg['M'], gg['K'], c.Np
    x = Slice(gg['npix'], c.Cp, T, o['x'])
    w = torch.full((Np + 8, K), float('nan'), dtype=T, device='cuda')
    w[:Np] = o['w'].to(T).cuda()
    G = _geom_struct(_lib, c, x.ld)
    msgs, res = [], {}
    if dt != 'f32':
        kid, tile = lib.vkas_conv_gemm_kernel_id(0, ctypes.byref(G), Np, 0, 0), lib.vkas_conv_gemm_tile(0, M, Np, K)
        if kid != expected_kid(s, c) or tile != (1 if s.BM == 128 else s.BN):
            msgs.append('kernel id %d / tile %d, expected %d / %d' % (kid, tile, expected_kid(s, c), 1 if s.BM == 128 else s.BN))
        res['plan'] = plan_record(_lib, 0, G, Np, 0, 0, False)
    bias = _vec(o['bias']) if o['bias'] is not None else None

    def launch(tag, mode, out=None, out2=None, aux=None, cs=None, rs=None, rpi=0, patch=None):
        E = _lib.Epilogue()
        E.mode, E.bias = mode, bias.data_ptr() if bias is not None else None
        if out is not None:
            E.out, E.ldo = out.ptr, out.ld
        if out2 is not None:
            E.out2, E.ldo2 = out2.ptr, out2.ld
        if aux is not None:
            E.aux, E.ldaux = aux.ptr, aux.ld
        E.colscale, E.rowscale, E.rows_per_image = cs.data_ptr() if cs is not None else None, rs.data_ptr() if rs is not None else None, rpi
        if patch:
            E.patch, E.patch_Hs, E.patch_Ws, E.patch_Cp = 2, c.H, c.W, patch
        rc = lib.vkas_conv_gemm_fwd(x.ptr, ctypes.byref(G), w.data_ptr(), Np, ctypes.byref(E), CODE[dt], _stream())
        torch.cuda.synchronize()
        if rc != 0:
            msgs.append('launch%s: rc %d: %s' % (tag, rc, lib.vkas_last_error().decode()))
        for name, sl in (('out', out), ('out2', out2)):
            if sl is not None:
                msgs.extend(sl.guard(tag + ' ' + name))
                res[name + tag] = sl.inside.cpu()

    aux = Slice(M, Np, T, o['aux']) if c.mode in ('sres', 'dgelu', 'add') else None
    if c.mode == 'none':
        launch('', _lib.EPI_NONE, out=Slice(M, Np, T))
    elif c.mode == 'gelu':
        launch('', _lib.EPI_GELU, out=Slice(M, Np, T), out2=Slice(M, Np, T))
        launch('_nokeep', _lib.EPI_GELU, out2=Slice(M, Np, T))  # out == NULL: the inference form
    elif c.mode == 'sres':
        cs, rs = _vec(o['cs']), _vec(o['rs']) if c.opt[1] else None
        launch('', _lib.EPI_SCALE_RES, out=Slice(M, Np, T), out2=Slice(M, Np, T) if c.opt[0] else None, aux=aux, cs=cs, rs=rs, rpi=c.opt[2])
    elif c.mode == 'dgelu':
        launch('', _lib.EPI_DGELU, out=Slice(M, Np, T), aux=aux)
    elif c.mode == 'add':
        launch('', _lib.EPI_ADD, out=Slice(M, Np, T), aux=aux)
    elif c.mode == 'patch':
        launch('', _lib.EPI_PATCH, out=Slice(4 * M, c.opt[0], T), patch=c.opt[0])
    res['msg'] = '; '.join(msgs)
    return res


def child_tn(_lib, s, c, kind, dt):
    lib, T, gg = _lib.lib, DT[dt], geom(c)
    o = tn_operands(c, kind, dt)
    M, K, Np = gg['M'], gg['K'], c.Np
    x, dy = Slice(gg['npix'], c.Cp, T, o['x']), Slice(M, Np, T, o['dy'])
    G = _geom_struct(_lib, c, x.ld)
    msgs, res = [], {}
    if dt != 'f32':
        kid, tile = lib.vkas_conv_gemm_kernel_id(1, ctypes.byref(G), Np, dy.ld, 0), lib.vkas_conv_gemm_tile(1, M, Np, K)
        if kid != s.tn or tile != s.tn:
            msgs.append('kernel id %d / tile %d, expected %d' % (kid, tile, s.tn))
        res['plan'] = plan_record(_lib, 1, G, Np, dy.ld, {'gelu': 1, 'ordered': 2}.get(c.entry, 0), c.entry in ('gb', 'gelu'))

    def fresh(v0):
        t = torch.full((v0.numel() + 64,), SENTINEL, device='cuda')
        t[:v0.numel()] = v0.reshape(-1).float().cuda()
        return t

    runs = []
    for rep in range(3 if c.entry == 'ordered' else 1):
        gw, gb = fresh(o['gw0']), fresh(o['gb0']) if c.entry in ('gb', 'gelu') else None
        a = (x.ptr, ctypes.byref(G), dy.ptr, dy.ld, Np, gw.data_ptr())
        if c.entry == 'ordered':
            rc = lib.vkas_conv_gemm_wgrad_ordered(*a, CODE[dt], _stream())
        elif c.entry == 'gelu':
            rc = lib.vkas_conv_gemm_wgrad_gelu(*a, gb.data_ptr(), CODE[dt], _stream())
        else:
            rc = lib.vkas_conv_gemm_wgrad(*a, gb.data_ptr() if gb is not None else None, CODE[dt], _stream())
        torch.cuda.synchronize()
        if rc != 0:
            msgs.append('rc %d: %s' % (rc, lib.vkas_last_error().decode()))
        for name, t, n in (('gw', gw, Np * K), ('gb', gb, Np)):
            if t is not None and not bool((t[n:] == SENTINEL).all()):
                msgs.append('the floats behind %s were written' % name)
        runs.append(gw)
    if any(not torch.equal(runs[0], r) for r in runs[1:]):
        msgs.append('_ordered differs between launches')
    res['gw'] = runs[0][:Np * K].view(Np, K).cpu()
    if gb is not None:
        res['gb'] = gb[:Np].cpu()
    res['msg'] = '; '.join(msgs)
    return res


def child_main(name, path):
    from vkit_ocr_model_adaptive_scaling_amd import _lib
    s = SETTINGS[name]
    for k in SWITCHES:  # what this process's static switches were read from
        assert os.environ.get(k) == s.env.get(k), (k, os.environ.get(k))
    res = {}
    for dt in s.dtypes:
        for kind in KINDS:
            for c in nt_cases(s.BM, s.BN):
                res['nt|%s|%s|%s' % (cid(c), kind, dt)] = child_nt(_lib, s, c, kind, dt)
            for c in (TN_CASES if s.tn else []):
                res['tn|%s|%s|%s' % (cid(c), kind, dt)] = child_tn(_lib, s, c, kind, dt)
    torch.save(res, path)


# ------------------------------------------------------------------------------------------------------------- parent side
_RUNS, _STOP = {}, []


def child_results(name):
    """The outputs of one setting's child, run once per session.  Children run one at a time; after one that timed out or
    ended abnormally none is started."""
    if name in _RUNS:
        r = _RUNS[name]
    elif _STOP:
        r = 'not started: ' + _STOP[0]
    else:
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env.update(SETTINGS[name].env)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, 'out.pt')
            code = 'import sys; from tests import test_gpu_gemm as t; t.child_main(sys.argv[1], sys.argv[2])'
            try:
                p = subprocess.run([sys.executable, '-c', code, name, path], cwd=ROOT, env=env, timeout=CHILD_TIMEOUT,
                                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                r = torch.load(path, weights_only=True) if p.returncode == 0 else \
                    'child %s ended with status %d: %s' % (name, p.returncode, p.stdout[-2000:])
            except subprocess.TimeoutExpired:
                r = 'child %s did not finish within %d s' % (name, CHILD_TIMEOUT)
        if isinstance(r, str):
            _STOP.append(r)
        _RUNS[name] = r
    assert not isinstance(r, str), r
    return r


_WORST = {}


def _log(form, mode, dt, value, bound, what):
    key = (form, mode, dt)
    if key not in _WORST or value / bound > _WORST[key][0] / _WORST[key][1]:
        _WORST[key] = (value, bound, what)


@pytest.fixture(scope='module', autouse=True)
def worst_rows():
    yield
    for (form, mode, dt), (value, bound, what) in sorted(_WORST.items()):
        parity_log.record('test_gpu_gemm', '%s, %s, %s' % (form, mode, dt), value, bound, 'at ' + what)


def compare_nt(c, kind, dt, got, form=None, ref_fn=None):
    """One forward case against fp64: exact kinds bit for bit (transcendental outputs at their documented error), random kinds
    at TOL + the propagated allowance; pad columns zero; GELU without out gives the bits of the call that keeps it.  ref_fn: the
    reference to judge against (tests/test_cpu_gemm_reference.py hands in deliberately wrong ones)."""
    o = nt_case_data(c, kind, dt)
    stored = got.get('out') if c.mode == 'gelu' else (got.get('out2') if c.mode == 'sres' else None)
    stored = stored.double() if stored is not None else None
    ref = ref_fn(c, o, dt, stored) if ref_fn else nt_reference(c, o, dt, stored, nt_case_staged(c, kind, dt))
    what = '%s %s %s' % (cid(c), kind, dt)
    assert set(ref) <= set(got), (what, sorted(got))
    for name, (rv, allow) in ref.items():
        g = got[name]
        if kind == 'exact' and (c.mode, name) not in TRANSCENDENTAL:
            check_exact(g, rv, what + ' ' + name)
        elif kind == 'exact' and allow is not None:
            ratio = check_transcendental_exact(g, rv, allow, dt, what + ' ' + name)
            if form:
                _log(form, c.mode + ' ' + name + ' (integer v; element error / its bound)', dt, ratio, 1.0, cid(c))
        else:
            rel, bound, worst = check_random(g, q(rv, DT[dt]) if allow is None else rv, allow, dt, what + ' ' + name)
            if form:
                _log(form, c.mode + ' ' + name, dt, rel, bound, cid(c))
        if c.mode != 'patch' and n_real(c) < c.Np:
            assert float(g[:, n_real(c):].double().abs().max()) == 0.0, what + ' ' + name + ': pad columns [N, Np) not zero'
    if c.mode == 'gelu':
        assert torch.equal(got['out2_nokeep'].view(torch.int32 if dt == 'f32' else torch.int16),
                           got['out2'].view(torch.int32 if dt == 'f32' else torch.int16)), what + ': out2 with out == NULL differs'


def compare_tn(c, kind, dt, got, form=None, ref_fn=None):
    o, ref = tn_case_data(c, kind, dt)
    if ref_fn is not None:
        ref = ref_fn(c, o, dt)
    what = '%s %s %s' % (cid(c), kind, dt)
    assert set(ref) <= set(got), (what, sorted(got))
    for name, (rv, allow) in ref.items():
        if kind == 'exact' and not (c.entry == 'gelu' and dt == 'f32'):  # fp32 storage: gelu(4) is no integer
            check_exact(got[name], rv, what + ' ' + name)
        else:
            rel, bound, _ = check_random(got[name], rv, allow, dt, what + ' ' + name, wgrad=True)
            if form:
                _log(form, c.entry + ' ' + name, dt, rel, bound, cid(c))


NT_PARAMS = [(n, c, dt) for n, s in SETTINGS.items() for dt in s.dtypes for c in nt_cases(s.BM, s.BN)]
TN_PARAMS = [(n, c, dt) for n, s in SETTINGS.items() if s.tn for dt in s.dtypes for c in TN_CASES]


def _ids(params):
    return ['%s-%s-%s' % (n, cid(c), dt) for n, c, dt in params]


@pytest.mark.parametrize('name,c,dt', NT_PARAMS, ids=_ids(NT_PARAMS))
def test_forward(name, c, dt):
    """vkas_conv_gemm_fwd: one case of one kernel form, integer operands bit for bit and random operands at TOL, with the guards
    (nothing outside the slice written, every element inside written, the expected kernel id) the child checked on the device."""
    res, s = child_results(name), SETTINGS[name]
    form = 'simple (fp32)' if dt == 'f32' else ('slab %d' % (s.BN // 32) if s.slab and c.geo == 's3' else s.form)
    for kind in KINDS:
        got = res['nt|%s|%s|%s' % (cid(c), kind, dt)]
        assert got['msg'] == '', '%s %s %s: %s' % (cid(c), kind, dt, got['msg'])
        compare_nt(c, kind, dt, got, form)
        if dt != 'f32':  # the plan behind the launch: buffer loads unless VKAS_NT_NOBUF, the ring depth and the name of the kernel id
            from tests.test_cpu_gemm_plan import nt_kernel_name
            assert got['plan'] == [int('VKAS_NT_NOBUF' not in s.env), 0, 0, s.kid - 10 if 12 <= s.kid <= 14 else 0,
                                   nt_kernel_name(expected_kid(s, c), False)], (cid(c), kind, dt, got['plan'])


@pytest.mark.parametrize('name,c,dt', TN_PARAMS, ids=_ids(TN_PARAMS))
def test_wgrad(name, c, dt):
    """vkas_conv_gemm_wgrad / _gelu / _ordered: gw (+=, onto an integer pattern) and gb of one case of one tile, buffer or
    non-buffer; _ordered bit-identical over three launches (checked in the child)."""
    res, s = child_results(name), SETTINGS[name]
    form = 'simple (fp32) wgrad' if dt == 'f32' else 'wgrad %d %s' % (s.tn, 'buffer' if TN_BUFFER[name] else 'non-buffer')
    for kind in KINDS:
        got = res['tn|%s|%s|%s' % (cid(c), kind, dt)]
        assert got['msg'] == '', '%s %s %s: %s' % (cid(c), kind, dt, got['msg'])
        compare_tn(c, kind, dt, got, form)
        if dt != 'f32':  # non-buffer in the ...nb settings and t224noslab; NOBIAS: no gb pointer ('nogb', and _ordered, which has
            # none), pointwise, tile 192 / 384, buffer loads only
            from tests.test_cpu_gemm_plan import tn_kernel_name
            buf = int(TN_BUFFER[name])
            nobias = int(c.entry in ('nogb', 'ordered') and c.geo == 'pw' and s.tn in (192, 384) and buf)
            assert got['plan'] == [buf, int(buf and c.geo == 'pw'), nobias, 0, tn_kernel_name(s.tn)], (cid(c), kind, dt, got['plan'])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32),
                                                                     b.view(torch.int16 if b.element_size() == 2 else torch.int32))


def _tensors(r):
    return {k: v for k, v in r.items() if k not in ('msg', 'plan')}


@pytest.mark.parametrize('other', ['ring2', 'ring3', 'ring4', 'default'])
def test_ring_depths_match_register_staged_kernel_bitwise(other):
    """Same geometry decode, K order and epilogue: every output of every forward case, bit for bit."""
    a, b = child_results('ring0'), child_results(other)
    keys = [k for k in a if k.startswith('nt|') and not k.endswith('|f32')]
    assert len(keys) == 2 * 2 * len(nt_cases(128, 128))
    for k in keys:
        for name, t in _tensors(a[k]).items():
            assert _same_bits(t, b[k][name]), (other, k, name)


@pytest.mark.parametrize('tile', ['t128', 't192', 't224'])
def test_buffer_and_non_buffer_forms_agree(tile):
    """Forward: bit for bit on every case both settings run on the generic tile; the slab cases' geometry (slab kernel against the
    non-buffer generic tile): exact on the integer operands, TOL otherwise.  Weight gradients: 1e-6 norm-wise."""
    a, b, s = child_results(tile), child_results(tile + 'nb'), SETTINGS[tile]
    for c in nt_cases(s.BM, s.BN):
        for kind in KINDS:
            for dt in s.dtypes:
                k = 'nt|%s|%s|%s' % (cid(c), kind, dt)
                for name, t in _tensors(a[k]).items():
                    if c.geo != 's3' or kind == 'exact':
                        assert _same_bits(t, b[k][name]), (k, name, first_mismatch(t.double(), b[k][name].double()))
                    else:
                        check_random(t, b[k][name].double(), None, dt, k + ' ' + name + ' slab against generic')
    for k in [k for k in a if k.startswith('tn|')]:
        for name, t in _tensors(a[k]).items():
            rel = measure(t, b[k][name].double())[0]
            assert rel < 1e-6, (k, name, rel)


def test_slab_and_generic_buffer_tile_agree():
    """conv3x3_slab_mfma_kernel<7> against gemm_nt_mfma_kernel<4,2,4,7,true> (VKAS_NT_NOSLAB) on the same geometry."""
    a, b, s = child_results('t224'), child_results('t224noslab'), SETTINGS['t224']
    n = 0
    for c in [c for c in nt_cases(s.BM, s.BN) if c.geo == 's3']:
        for kind in KINDS:
            for dt in s.dtypes:
                k = 'nt|%s|%s|%s' % (cid(c), kind, dt)
                for name, t in _tensors(a[k]).items():
                    n += 1
                    if kind == 'exact':
                        assert _same_bits(t, b[k][name]), (k, name)
                    else:
                        check_random(t, b[k][name].double(), None, dt, k + ' ' + name + ' slab against generic')
    assert n >= 40


def test_case_tables_cover_every_form_and_mode():
    """Every epilogue mode on every forward form with a ragged-M and a ragged-N case (slab: ragged N; its M is whole tiles by
    construction), the five M values with NONE, every Cp; every wgrad entry point at every M and on every geometry."""
    for BM, BN in ((128, 128), (256, 128), (256, 192), (256, 224)):
        L = nt_cases(BM, BN)
        for mode in ('none', 'gelu', 'sres', 'dgelu', 'add', 'patch'):
            for geo in ('pw', 's3'):
                cs = [c for c in L if c.mode == mode and c.geo == geo]
                assert any(c.Np % BN and c.Np > BN for c in cs), (BM, BN, mode, geo)
                assert geo == 's3' or any(geom(c)['M'] % BM and geom(c)['M'] > BM for c in cs), (BM, BN, mode)
        assert {geom(c)['M'] for c in L if c.geo == 'pw' and c.mode == 'none'} >= {1, 13, BM - 1, BM + 1, 3 * BM + 37}
        assert {c.Np for c in L} >= set(NT_NPS[BN]) and {c.Cp for c in L if c.geo in ('pw', 's3', 'c3')} == set(CPS)
        assert {c.geo for c in L} == set(GEO)
        assert {c.opt for c in L if c.mode == 'sres'} == {(1, 1, 1), (0, 0, 5), (1, 1, 49)} and {c.opt for c in L if c.mode == 'none'} == {(0,), (1,)}
    assert {geom(c)['M'] for c in TN_CASES if c.geo == 'pw'} == {1, 13, 63, 65, 257, 1137}
    for ent in ENTRIES:
        assert {c.geo for c in TN_CASES if c.entry == ent} == {'pw', 'c3', 'p2'}
    assert {c.Np for c in TN_CASES} == set(TN_NPS) and {c.Cp for c in TN_CASES} == set(CPS)
    assert {(s.tn, TN_BUFFER[n]) for n, s in SETTINGS.items() if s.tn} == {(t, b) for t in (128, 192, 224, 384) for b in (True, False)}
    assert {s.kid for s in SETTINGS.values()} == {1, 12, 13, 14, 128, 192, 224} and sum(s.slab for s in SETTINGS.values()) == 3
