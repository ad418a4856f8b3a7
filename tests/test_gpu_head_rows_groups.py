"""Row pass of the heads' forward (vkas_head_rows_fwd, csrc/head.hip) at the shapes where its lane layout can go wrong: eight
lanes per (pixel, head) with up to four 8-channel vectors each, a wave of eight pixel columns per head, 32 / NH columns per
workgroup, the previous row's T0 / T1 waiting in LDS.

  widths   c = 5 (one partly filled vector, seven idle lanes), 64 (one vector per lane), 72 (one lane with a second vector),
           191 / 192 / 193 (three vectors full, and spilling into the fourth), 224 (pw = 224) and 256 (pw = 256, the entry's
           limit), each as a single head and inside a four-head set with a different oc per head
  maps     W2 = 13 and 40 (the column clamp and the masked columns), B = 1 and 3, h = 1, 2, 5, seg_rows = 0 .. 3 (a ragged last
           segment, windows that start inside the image)
  values   real-valued T (seeded normal, rounded to the storage type) against tests/head_rows_reference.py in fp64 on the stored
           values

z:  |z - z64| <= 2^-8 |z64| + 2^-20 S for bf16 (2^-11 for fp16), S the sum of the element's absolute terms: one rounding to
storage plus the fp32 accumulation of at most thirteen terms.  Statistics and maps are compared with fp64 ones of the fp64 z at
bounds that follow the kernel's own arithmetic (derived at _tail_bounds).  Pad columns of z and proj[..., oc:] are exact zeros,
the guard regions behind z, the statistics and the maps stay untouched, two launches give the same bits."""
import pytest
import torch

from tests import head_rows_reference as R
from tests.test_gpu_head_fwd_rows import GELU_ERR, _row_pass_run

pytestmark = pytest.mark.gpu

IDS = {torch.bfloat16: 'bf16', torch.float16: 'f16'}
STORE = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}  # half an ulp of the storage type, relative
U = 2.0 ** -24  # fp32 unit roundoff

HEAD_SETS = {
    'c5': ((5,), (3,), 224), 'c64': ((64,), (1,), 224), 'c72': ((72,), (2,), 224), 'c191': ((191,), (4,), 224),
    'c192': ((192,), (1,), 224), 'c193': ((193,), (2,), 224), 'c224': ((224,), (3,), 224), 'c256': ((256,), (4,), 256),
    'four-narrow': ((5, 64, 72, 191), (2, 4, 1, 3), 224),
    'four-wide': ((192, 193, 224, 72), (1, 2, 4, 3), 224),
    'four-limit': ((256, 5, 193, 64), (4, 1, 3, 2), 256),
    'two': ((72, 193), (3, 1), 224),  # NH = 2: sixteen columns per workgroup
}
# (B, h, W2, seg_rows): every value of the issue's lists, every segment length on the tallest map (seg 2: 2 + 2 + 1, seg 3:
# 3 + 2 rows), a segment longer than the map, one-row maps (top and bottom in the same row)
SHAPES = [(1, 1, 13, 0), (3, 1, 40, 2), (1, 2, 13, 0), (3, 2, 40, 1), (3, 5, 13, 0), (1, 5, 40, 1), (3, 5, 40, 2), (1, 5, 13, 3)]

_CASES = {}


def _randn(shape, g, scale=1.0):
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale


def _case(heads, shape, dtype):
    """inputs and the fp64 reference of one case, built once"""
    key = (heads, shape, dtype)
    if key in _CASES:
        return _CASES[key]
    cs, ocs, pw = HEAD_SETS[heads]
    B, h, W2, _ = shape
    nps = [(c + 7) // 8 * 8 for c in cs]
    offs = [sum(nps[:k]) for k in range(len(cs) + 1)]
    Nt = offs[-1]
    g = torch.Generator().manual_seed(1000 * sorted(HEAD_SETS).index(heads) + 10 * SHAPES.index(shape))
    T = torch.zeros((B, h, W2, 3, Nt), dtype=torch.float64)
    bias = torch.zeros((Nt,), dtype=torch.float64)
    params = torch.zeros((len(cs), 6 * pw + 8), dtype=torch.float64)
    tails = []
    for k, (c, oc) in enumerate(zip(cs, ocs)):  # pad columns stay zero, as the convolution leaves them
        T[..., offs[k]:offs[k] + c] = _randn((B, h, W2, 3, c), g).to(dtype).double()
        bias[offs[k]:offs[k] + c] = _randn((c,), g, 0.5).float().double()
        gamma, beta = (1 + _randn((c,), g, 0.1)).float().double(), _randn((c,), g, 0.1).float().double()
        wproj, bproj = _randn((oc, c), g, c ** -0.5).float().double(), _randn((oc,), g, 0.1).float().double()
        params[k, :c], params[k, pw:pw + c] = gamma, beta
        for r in range(oc):
            params[k, (2 + r) * pw:(2 + r) * pw + c] = wproj[r]
        params[k, 6 * pw:6 * pw + oc] = bproj
        tails.append((gamma, beta, wproj, bproj))
    c = dict(B=B, h=h, W2=W2, cs=cs, ocs=ocs, nps=nps, offs=offs, Nt=Nt, pw=pw, T=T, bias=bias, params=params, tails=tails,
             Td=T.reshape(B, h, W2, 3 * Nt).to(dtype).cuda(), bd=bias.float().cuda(), pd=params.float().cuda(),
             z64=R.rows_to_z(T, bias), S=R.rows_to_z(T.abs(), bias.abs()))
    _CASES[key] = c
    return c


def _tail_bounds(z, ez, cc, gamma, beta, wproj, maps, mean, rstd):
    """What the kernel's arithmetic may differ by from the fp64 tail of the fp64 z (cc channels, ez the bound of its fp32 z):
    mean  the fp32 sum of cc terms ((cc - 1) U sum |z|), the terms' own errors, one division
    rstd  var = (sum z^2 - s mean) / cc: sum z^2 carries (cc + 1) U of itself, s mean (cc + 3) U of cc mean^2, the subtraction
          and the division U each - below 2 (cc + 3) U E[z^2] in all; the terms' errors move var by 2 sqrt(var) max ez; half of
          the relative error of var + eps reaches rstd, whose rsqrt and division add 2^-22
    maps  u = (z - mean) rstd gamma + beta moves by |gamma| rstd (ez + d mean) + |u - beta| d rstd / rstd + 2^-22 |u|; the GELU
          polynomial adds GELU_ERR, |GELU'| <= 1.13; the projection's fp32 sum of cc products (cc + 2) U sum |a w|, as the
          existing row-pass test allows it"""
    dmean = ez.mean(-1) + (cc - 1) * U * z.abs().mean(-1) + 2 * U * mean.abs()
    ez2, var = (z * z).mean(-1), 1.0 / (rstd * rstd)  # var + eps
    drstd = 0.5 * (2 * (cc + 3) * U * ez2 + 2 * (var.sqrt() + ez.amax(-1)) * ez.amax(-1)) / var + 2.0 ** -22
    u = (z - mean[..., None]) * rstd[..., None] * gamma + beta
    du = gamma.abs() * rstd[..., None] * (ez + dmean[..., None]) + (u - beta).abs() * drstd[..., None] + 2.0 ** -22 * u.abs()
    a = 0.5 * u * (1.0 + torch.erf(u / 2.0 ** 0.5))
    dmaps = (GELU_ERR + 1.13 * du + (cc + 2) * U * a.abs()) @ wproj.abs().T + 2.0 ** -20 * maps.abs()
    return dmean, drstd, dmaps


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('shape', SHAPES, ids=['B%d-h%d-W%d-seg%d' % s for s in SHAPES])
@pytest.mark.parametrize('heads', sorted(HEAD_SETS))
def test_row_pass_lane_groups_match_fp64(heads, shape, dtype):
    c = _case(heads, shape, dtype)
    seg = shape[3]
    z, stats, proj = _row_pass_run(c, seg, dtype)  # asserts the guard regions behind z, the statistics and the maps
    z2, stats2, proj2 = _row_pass_run(c, seg, dtype)
    assert torch.equal(z, z2) and torch.equal(stats, stats2) and torch.equal(proj, proj2)  # two launches: the same bits
    _, _, proj3 = _row_pass_run(c, seg, dtype, keep=False)  # inference form: no z, no statistics, the same maps
    assert torch.equal(proj, proj3)
    z, stats, proj = z.double().cpu(), stats.double().cpu(), proj.double().cpu()
    z64, S = c['z64'], c['S']
    assert bool(torch.isfinite(z).all())
    over = (z - z64).abs() - (STORE[dtype] * z64.abs() + 2.0 ** -20 * S)
    print('%s %s %s: z worst |z - z64| / bound %.3f' % (heads, shape, IDS[dtype], float(((z - z64).abs() / (
        STORE[dtype] * z64.abs() + 2.0 ** -20 * S).clamp_min(1e-30)).max())))
    assert float(over.max()) <= 0, 'z beyond its bound at %s' % (over > 0).nonzero()[:4].tolist()
    for k, (cc, oc) in enumerate(zip(c['cs'], c['ocs'])):
        o, npk = c['offs'][k], c['nps'][k]
        assert float(z[..., o + cc:o + npk].abs().max() if npk > cc else 0.0) == 0.0  # pad columns: exact zeros
        gamma, beta, wproj, bproj = c['tails'][k]
        zk = z64[..., o:o + cc]
        maps, mean, rstd = R.head_tail(zk, cc, gamma, beta, wproj, bproj)
        dmean, drstd, dmaps = _tail_bounds(zk, 2.0 ** -20 * S[..., o:o + cc], cc, gamma, beta, wproj, maps, mean, rstd)
        em, er = (stats[k, ..., 0] - mean).abs(), (stats[k, ..., 1] - rstd).abs() / rstd
        ep = (proj[k, ..., :oc] - maps).abs()
        print('  head %d (c = %d, oc = %d): worst error / bound: mean %.3f rstd %.3f maps %.3f'
              % (k, cc, oc, float((em / dmean).max()), float((er / drstd).max()), float((ep / dmaps).max())))
        assert float((em - dmean).max()) <= 0 and float((er - drstd).max()) <= 0, (k, float(em.max()), float(er.max()))
        assert float(proj[k, ..., oc:].abs().max()) == 0.0
        assert float((ep - dmaps).max()) <= 0, (k, float(ep.max()), float(dmaps.max()))
