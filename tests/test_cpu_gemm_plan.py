"""The launch plan of the 16-bit implicit GEMMs (csrc/gemm_plan.hip) through vkas_conv_gemm_plan with explicit switches: pure
host arithmetic, so every setting runs in this process and nothing is launched.

Agreement with the parent: tests/golden/gemm_plan.json was recorded from the library of the commit its header names (before the
plan existed): vkas_conv_gemm_kernel_id / vkas_conv_gemm_tile per case and setting, and what its launchers were about to launch
(instantiation, grid, splits, rows or chunks per split, tiles), printed in front of each launch.  The cases straddle every
threshold of the rule under the twelve settings of tests/test_gpu_gemm.py and three more (VKAS_NT_TILE=1, VKAS_TN_NOSLAB,
VKAS_TN_NO96).  One label differs from the parent's by intent: the parent's kernel id ignored the entry
point, so its Python label called an `ordered` product on slab-eligible geometry the slab kernel; the fixture's launch record
(what ran) is what the plan is held to.

32-bit limits: operand spans of 0xFFFFFFF0 - 2 and 0xFFFFFFF0 bytes (x, Bw, dy; pixel strides wider than the operand) flip buffer
addressing, drop the ring and refuse both slab kernels.  Some of these geometries have odd channel counts: the launch entry
points would reject them, the plan is arithmetic.
"""
import collections
import ctypes
import json
import os

import pytest

from tests.test_gpu_gemm import SETTINGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'gemm_plan.json')
LIMIT = 0xFFFFFFF0

ENVS = {name: s.env for name, s in SETTINGS.items()}
ENVS.update(nt1={'VKAS_NT_TILE': '1'}, tnnoslab={'VKAS_TN_NOSLAB': '1'}, tnno96={'VKAS_TN_NO96': '1'})
assert len(SETTINGS) == 12 and 'default' in SETTINGS

# wgrad: 0 forward, 1 weight gradient.  heads: columns of each fused head (forward).  entry: gb | nogb | gelu | ordered.
Case = collections.namedtuple('Case', 'name wgrad B Hin Win Cp ldx k stride pad Np lddy heads entry')
FLAGS = {'gb': 0, 'nogb': 0, 'gelu': 1, 'ordered': 2}


def out_hw(c):
    return (c.Hin + 2 * c.pad - c.k) // c.stride + 1, (c.Win + 2 * c.pad - c.k) // c.stride + 1


def rows_of(c):
    ho, wo = out_hw(c)
    return c.B * ho * wo


def _both(name, B, H, W, Cp, Np, k=1, stride=1, pad=0, ldx=None, lddy=None, entries=('gb',), fwd=True):
    """The forward case (fwd) and the weight-gradient cases (entries) of one geometry."""
    ldx, lddy = ldx or Cp, lddy or Np
    L = [Case(name + '-fwd', 0, B, H, W, Cp, ldx, k, stride, pad, Np, 0, (), '')] if fwd else []
    return L + [Case('%s-%s' % (name, e), 1, B, H, W, Cp, ldx, k, stride, pad, Np, lddy, (), e) for e in entries]


def cases():
    L, c3, ALL = [], dict(k=3, stride=1, pad=1), ('gb', 'nogb', 'gelu', 'ordered')
    for M in (0, 1, 65, 257, 1137, 16383, 16384):  # small M (splits of whole 64-row steps), the NT tile threshold
        L += _both('pw-M%d' % M, 1 if M else 0, 1, max(M, 1), 72, 200, ldx=80, lddy=208, fwd=M not in (65, 257, 1137),
                   entries=('gb', 'ordered') if M in (1137, 16384) else ('gb',))
    for M in (2048, 2049, 32768, 32769):  # cdiv(M, 128) cdiv(Np, 128) = 256 / 272 (rule) and 256 / 257 (VKAS_NT_TILE=1): ring 4 / 2
        L += _both('ring-M%d' % M, 1, 1, M, 64, 2048 if M < 16384 else 128, entries=())
    for W, H in ((256, 64), (192, 96), (64, 256)):  # forward slab eligibility by Win
        L += _both('c3-W%d-H%d' % (W, H), 1, H, W, 128, 128, ldx=136, entries=(), **c3)
    L += _both('c3-W256-H256', 1, 256, 256, 128, 128, ldx=136, lddy=136, entries=ALL, **c3)  # every entry on slab-eligible geometry
    # wgrad slab eligibility by Win and M; M = 65472 is the largest below 65536 that whole 64-pixel rows reach
    for W, H in ((192, 352), (64, 1024), (64, 1023), (96, 704)):
        L += _both('c3-W%d-H%d' % (W, H), 1, H, W, 128, 128, ldx=136, lddy=136, fwd=False, **c3)
    L += _both('c3-M65280', 1, 255, 256, 128, 128, fwd=False, **c3)  # M = 65280 < 65536 on whole 256-pixel rows
    L += _both('c3-M65536-B4', 4, 64, 256, 128, 128, fwd=False, **c3)
    L += _both('c3-stride2', 1, 512, 512, 128, 128, 3, 2, 1)         # never slab
    L += _both('c3-pad0', 1, 258, 258, 128, 128, 3, 1, 0)
    for Np in (192, 112, 224, 128, 136, 104, 384):                   # slab 96 / 112 / 128, NT BN by least padding
        L += _both('c3-Np%d' % Np, 1, 256, 256, 128, Np, fwd=Np != 104, **c3)
    for Cp in (120, 128):
        L += _both('c3-Cp%d' % Cp, 1, 256, 256, Cp, 128, fwd=False, **c3)
    for Np, K in ((192, 184), (192, 192), (384, 512), (768, 384), (200, 256)):  # wgrad tiles 128 .. 384
        L += _both('pw-Np%d-K%d' % (Np, K), 1, 128, 128, K, Np, fwd=False)
    for Np, K in ((192, 256), (384, 384), (224, 256)):               # pointwise against 2x2 stride 2 at tiles 192 / 384 / 224: pw, nobias
        L += _both('pw-Np%d-K%d' % (Np, K), 1, 128, 128, K, Np, fwd=False, entries=ALL if Np == 192 else ALL[:3])
        L += _both('p2-Np%d-K%d' % (Np, K), 1, 256, 256, K // 4, Np, 2, 2, 0, fwd=False, entries=ALL[:2])
    for w in (8, 128, 136, 192, 200, 224):                           # fused heads: slab (Win = 256) and the 8-wave tile
        for W in (256, 320):
            L.append(Case('head-%d-W%d' % (w, W), 0, 1, 64, W, 128, 128, 3, 1, 1, w + 8, 0, (w, 8), ''))
    return L


def limit_cases():
    """name -> (case just below the limit, case at the limit, which span).  Spans in bytes:
    x ((B Hin Win - 1) ldx + Cp) 2, Bw Np K 2, dy ((M - 1) lddy + Np) 2."""
    D = {}
    # pointwise, 2^27 pixels of stride 16: ((2^27 - 1) 16 + 7 | 8) 2
    D['x-pw'] = (_both('lim-x-pw-lo', 1, 8192, 16384, 7, 8, ldx=16)[0], _both('lim-x-pw-hi', 1, 8192, 16384, 8, 8, ldx=16)[0], 'a')
    D['x-pw-tn'] = (_both('lim-x-pwtn-lo', 1, 8192, 16384, 7, 8, ldx=16)[1], _both('lim-x-pwtn-hi', 1, 8192, 16384, 8, 8, ldx=16)[1], 'a')
    # 2147483639 = 119 x 18046081, 2147483640 = 120 x 17895697 elements of Bw
    D['bw'] = (_both('lim-bw-lo', 1, 1, 64, 18046081, 119, ldx=18046088)[0], _both('lim-bw-hi', 1, 1, 64, 17895697, 120, ldx=17895704)[0], 'b')
    D['dy-pw'] = (_both('lim-dy-pw-lo', 1, 8192, 16384, 8, 7, lddy=16)[1], _both('lim-dy-pw-hi', 1, 8192, 16384, 8, 8, lddy=16)[1], 'b')
    # slab geometry, 2^20 pixels (4096 rows of 256) of stride 2048: ((2^20 - 1) 2048 + 2039 | 2040) 2
    g = dict(k=3, stride=1, pad=1)
    D['x-slab'] = (_both('lim-x-slab-lo', 1, 4096, 256, 2039, 128, ldx=2048, **g)[0], _both('lim-x-slab-hi', 1, 4096, 256, 2040, 128, ldx=2048, **g)[0], 'a')
    D['x-slab-tn'] = (_both('lim-x-slabtn-lo', 1, 4096, 256, 2039, 128, ldx=2048, **g)[1], _both('lim-x-slabtn-hi', 1, 4096, 256, 2040, 128, ldx=2048, **g)[1], 'a')
    D['dy-slab'] = (_both('lim-dy-slab-lo', 1, 4096, 256, 128, 2039, lddy=2048, **g)[1], _both('lim-dy-slab-hi', 1, 4096, 256, 128, 2040, lddy=2048, **g)[1], 'b')
    # Bw of the forward slab: Np K 2 with K = 9 Cp: neither 2147483639 nor 2147483640 has a factor 9; the two nearest neighbours
    D['bw-slab'] = (_both('lim-bw-slab-lo', 1, 64, 256, 8, 29826161, ldx=16, **g)[0], _both('lim-bw-slab-hi', 1, 64, 256, 8, 29826162, ldx=16, **g)[0], 'b')
    return D


CASES, LIMITS = cases(), limit_cases()


# ------------------------------------------------------------------------------------------------ the entry point
@pytest.fixture(scope='module')
def L():
    from vkit_ocr_model_adaptive_scaling_amd import _lib
    return _lib


def switches(L, env):
    return L.GemmSwitches(nt_tile=int(env.get('VKAS_NT_TILE', 0)), tn_tile=int(env.get('VKAS_TN_TILE', 0)),
                          nt_ring=int(env.get('VKAS_NT_RING', -1)), nt_noslab=int('VKAS_NT_NOSLAB' in env),
                          nt_nobuf=int('VKAS_NT_NOBUF' in env), tn_nobuf=int('VKAS_TN_NOBUF' in env),
                          tn_noslab=int('VKAS_TN_NOSLAB' in env), tn_no96=int('VKAS_TN_NO96' in env))


def geom_struct(L, c):
    ho, wo = out_hw(c)
    return L.ConvGeom(c.B, c.Hin, c.Win, ho, wo, c.Cp, c.ldx, c.k, c.k, c.stride, c.pad)


def plan(L, c, env, entry=None, sw_null=False):
    """The plan as a dict; entry overrides the case's own (None: the case's)."""
    entry = c.entry if entry is None else entry
    info, sw = L.GemmPlanInfo(), switches(L, env)
    rc = L.lib.vkas_conv_gemm_plan(c.wgrad, ctypes.byref(geom_struct(L, c)), c.Np, c.lddy, max(c.heads, default=0), FLAGS.get(entry, 0),
                                   int(entry in ('gb', 'gelu')), None if sw_null else ctypes.byref(sw), ctypes.byref(info))
    assert rc == 0
    d = {n: getattr(info, n) for n, _ in info._fields_}
    d['name'] = d['name'].decode()
    return d


# the two tables ops.py kept before the plan existed: kernel id -> the name bench.py groups by
def nt_kernel_name(kid, head):
    if kid == 0:
        return 'gemm_nt_simple'
    if kid >= 1000:
        return 'conv3x3_slab_mfma_kernel<%d,%d>' % (kid - 1000, int(head))
    if 12 <= kid <= 14:
        return 'gemm_nt_ring_kernel<%d>' % (kid - 10)
    return 'gemm_nt_mfma_kernel<%s>' % {1: '2,2,4,4', 128: '4,2,4,4', 192: '4,2,4,6', 224: '4,2,4,7'}[kid]


def tn_kernel_name(kid):
    if kid == 0:
        return 'gemm_tn_simple'
    if kid >= 2000:
        return 'conv3x3_wgrad_slab_kernel<%d>' % (kid - 2000)
    return 'gemm_tn_mfma_kernel<%s>' % {128: '2,2,4,4', 192: '2,4,6,4', 224: '2,4,7,4', 384: '4,2,6,4'}[kid]


NT_FAMILY = {0: 'register-staged', 1: 'ring', 2: 'tile256', 3: 'slab'}
TN_WAVES = {128: '2,2,4,4', 192: '2,4,6,4', 224: '2,4,7,4', 384: '4,2,6,4'}


def launch_record(c, p):
    """What the parent's launcher printed in front of the launch this plan describes."""
    if rows_of(c) == 0:
        return None  # the launchers return before planning
    if not c.wgrad:
        grid = (p['grid_m'] * (len(c.heads) or p['grid_n'])) & 0xFFFFFFFF
        if p['family'] == 3:
            return 'nt_slab %d head=%d grid=%d' % (p['bn'] // 32, p['head'], grid)
        if p['family'] == 1:
            return 'nt_ring %d grid=%d' % (p['ring'], grid)
        return 'nt_mfma %s,4,%d buf=%d head=%d grid=%d' % ('2,2' if p['family'] == 0 else '4,2', p['bn'] // 32, p['buf'], p['head'], grid)
    if p['family'] == 1:
        return 'tn_slab %d grid=%d splits=%d cps=%d tiles=%d' % (p['bn'] // 16, p['grid'], p['splits'], p['rows'], p['tiles'])
    return 'tn_mfma %s xg=%d buf=%d pw=%d nobias=%d grid=%d splits=%d rows=%d tiles=%d' % (
        TN_WAVES[p['bn']], p['xg'], p['buf'], p['pw'], p['nobias'], p['grid'], p['splits'], p['rows'], p['tiles'])


def derived_ids(L, c, env):
    """(kernel id, tile) as vkas_conv_gemm_kernel_id / vkas_conv_gemm_tile define them, from plans: the id is that of a plain
    call; the tile is the generic rule's (a slab case: what its GELU entry, which never takes the slab, runs) and ignores heads."""
    p = plan(L, c, env, entry='nogb')
    if c.wgrad:
        return p['kernel_id'], plan(L, c, env, entry='gelu')['bn']
    q = plan(L, c._replace(heads=()), env)
    return p['kernel_id'], q['bn'] if q['family'] >= 2 else 1


def check_invariants(c, p):
    M = rows_of(c)
    assert p['grid'] == (p['tiles'] * p['splits']) & 0xFFFFFFFF and 1 <= p['splits'] <= 65535 and p['tiles'] >= (M > 0), (c.name, p)
    if not c.wgrad:
        assert p['tiles'] == p['grid_m'] * p['grid_n'] and p['grid_n'] == -(-c.Np // p['bn']), (c.name, p)
        assert p['grid_m'] * (256 if p['family'] >= 2 else 128) >= M and p['ring'] in (0, 2, 3, 4) and (p['ring'] > 0) == (p['family'] == 1)
        assert p['name'] == nt_kernel_name(p['kernel_id'], p['head']) and (p['buf'] or p['family'] in (0, 2)), (c.name, p)
    elif p['family'] == 1:
        assert p['rows'] * p['splits'] >= M // 64 and M % 64 == 0 and p['buf'] and not (p['pw'] or p['nobias'] or p['xg']), (c.name, p)
        assert p['name'] == tn_kernel_name(p['kernel_id']) == 'conv3x3_wgrad_slab_kernel<%d>' % (p['bn'] // 16), (c.name, p)
    else:
        assert p['splits'] * p['rows'] >= M and p['rows'] % 64 == 0 and p['rows'] >= 64, (c.name, p)
        assert (p['splits'] - 1) * p['rows'] < max(M, 1), (c.name, p)  # no empty split
        assert p['name'] == tn_kernel_name(p['kernel_id']) and p['kernel_id'] == p['bn'], (c.name, p)
        assert p['pw'] <= p['buf'] and p['nobias'] <= p['pw'], (c.name, p)


# ------------------------------------------------------------------------------------------------------------ tests
@pytest.fixture(scope='module')
def golden():
    """setting -> case -> [kernel id, tile, launch].  The file keeps one record per case and group of settings that share it
    ('*': every setting not named by another record of the case)."""
    with open(FIXTURE) as f:
        d = json.load(f)
    assert d['settings'] == ENVS
    out = {s: {} for s in ENVS}
    for case, records in d['cases'].items():
        named = {s for r in records for s in r[3].split() if s != '*'}
        for kid, tile, launch, who in records:
            for s in (set(ENVS) - named if who == '*' else who.split()):
                assert case not in out[s]
                out[s][case] = [kid, tile, launch]
    return out


@pytest.mark.parametrize('setting', sorted(ENVS))
def test_plan_agrees_with_the_parent_and_keeps_its_invariants(L, golden, setting):
    env, rec = ENVS[setting], golden[setting]
    assert set(rec) == {c.name for c in CASES}
    for c in CASES:
        p, (kid, tile, launch) = plan(L, c, env), rec[c.name]
        check_invariants(c, p)
        assert derived_ids(L, c, env) == (kid, tile), (setting, c.name, derived_ids(L, c, env), kid, tile)
        assert launch_record(c, p) == launch, (setting, c.name, launch_record(c, p), launch)


def test_rule_lands_where_the_issue_expects(L):
    """Spot checks of the thresholds by name, under no switches."""
    by = {c.name: c for c in CASES}
    P = lambda name, env={}: plan(L, by[name], env)
    assert (P('pw-M16383-fwd')['family'], P('pw-M16384-fwd')['family']) == (1, 2)
    assert (P('ring-M2048-fwd')['ring'], P('ring-M2049-fwd')['ring']) == (4, 2)
    assert (P('ring-M32768-fwd', ENVS['nt1'])['ring'], P('ring-M32769-fwd', ENVS['nt1'])['ring']) == (4, 2)
    assert [P('c3-W%d-H%d-fwd' % wh)['family'] for wh in ((256, 64), (192, 96), (64, 256))] == [3, 2, 2]
    assert [P('c3-W%d-H%d-gb' % wh)['family'] for wh in ((256, 256), (192, 352), (64, 1024), (96, 704))] == [1, 1, 1, 0]
    assert (P('c3-M65280-gb')['family'], P('c3-W64-H1023-gb')['family'], P('c3-M65536-B4-gb')['family']) == (0, 0, 1)
    assert [P('c3-%s-%s' % (g, d))['family'] for g in ('stride2', 'pad0') for d in ('fwd', 'gb')] == [2, 0, 2, 0]
    assert [P('c3-Np%d-gb' % n)['bn'] for n in (192, 112, 224, 128, 136, 384)] == [96, 112, 112, 128, 96, 128]
    assert P('c3-Np192-gb', ENVS['tnno96'])['bn'] == 112 and P('c3-Np104-gb')['family'] == 0
    assert [P('c3-Np%d-fwd' % n)['bn'] for n in (192, 112, 224, 128, 136, 384)] == [192, 128, 224, 128, 192, 192]  # 384: tie, wider
    assert (P('c3-Cp120-gb')['family'], P('c3-Cp128-gb')['family']) == (0, 1)
    assert [P('pw-Np%d-K%d-gb' % nk)['bn'] for nk in ((192, 184), (192, 192), (384, 384), (384, 512), (768, 384), (224, 256), (200, 256))] == \
        [128, 192, 384, 192, 384, 224, 224]
    for nk, tile in (((192, 256), 192), ((384, 384), 384), ((224, 256), 224)):
        for geo in ('pw', 'p2'):
            got = {e: P('%s-Np%d-K%d-%s' % ((geo,) + nk + (e,))) for e in ('gb', 'nogb', 'gelu')[:3 if geo == 'pw' else 2]}
            assert all(p['bn'] == tile and p['buf'] and p['pw'] == (geo == 'pw') for p in got.values()), (nk, geo)
            assert [p['nobias'] for p in got.values()] == [0, int(geo == 'pw' and tile != 224), 0][:len(got)], (nk, geo)
            assert P('%s-Np%d-K%d-nogb' % ((geo,) + nk), {'VKAS_TN_NOBUF': '1'})['nobias'] == 0
    for e in ('gelu', 'ordered'):  # the slab kernel is the plain entry's only
        p = P('c3-W256-H256-' + e)
        assert p['family'] == 0 and p['name'].startswith('gemm_tn_mfma_kernel<') and (e != 'ordered' or p['splits'] == 1), p
    for w, bn in ((8, 128), (128, 128), (136, 192), (192, 192), (200, 224), (224, 224)):
        a, b = P('head-%d-W256' % w), P('head-%d-W320' % w)
        assert (a['family'], a['bn'], a['head'], a['name']) == (3, bn, 1, 'conv3x3_slab_mfma_kernel<%d,1>' % (bn // 32))
        assert (b['family'], b['bn'], b['head'], b['name']) == (2, bn, 1, 'gemm_nt_mfma_kernel<4,2,4,%d>' % (bn // 32))
    assert P('pw-M0-gb')['splits'] == 1 and P('pw-M0-gb')['rows'] == 64 and P('pw-M0-fwd')['grid'] == 0


@pytest.mark.parametrize('which', sorted(LIMITS))
def test_32_bit_limits(L, which):
    lo, hi, field = LIMITS[which]
    a, b = plan(L, lo, {}), plan(L, hi, {})
    assert a[field + '_bytes'] < LIMIT <= b[field + '_bytes'] and (which == 'bw-slab' or (a[field + '_bytes'], b[field + '_bytes']) == (LIMIT - 2, LIMIT)), (a, b)
    assert a['buf'] == 1 and b['buf'] == 0 and b['pw'] == 0 and b['nobias'] == 0 and b['ring'] == 0, (a, b)
    if 'slab' in which:
        assert a['family'] == (1 if lo.wgrad else 3) and b['family'] == (0 if lo.wgrad else 2), (a, b)
    elif not lo.wgrad:
        assert (a['family'], b['family']) == ((2, 2) if rows_of(lo) >= 16384 else (1, 0)), (a, b)
    for c, p in ((lo, a), (hi, b)):
        check_invariants(c, p)
        for env in ENVS.values():
            check_invariants(c, plan(L, c, env))


def test_out_of_range_tile_values_count_as_unset(L):
    for c in CASES:
        for entry in ((c.entry,) if c.wgrad else ('',)):
            assert plan(L, c, {'VKAS_NT_TILE': '5', 'VKAS_TN_TILE': '100'}, entry) == plan(L, c, {}, entry), c.name
            assert plan(L, c, {'VKAS_NT_TILE': '-1', 'VKAS_TN_TILE': '1'}, entry) == plan(L, c, {}, entry), c.name


def test_plan_is_pure_and_the_reporters_read_it(L):
    """Explicit switches: the process environment does not matter (two different ones, set after the library read its own once).
    NULL switches: the same plan the kernel id and the tile come from."""
    names = ('VKAS_NT_TILE', 'VKAS_TN_TILE', 'VKAS_NT_RING', 'VKAS_NT_NOSLAB', 'VKAS_TN_NOSLAB', 'VKAS_NT_NOBUF', 'VKAS_TN_NOBUF', 'VKAS_TN_NO96')
    saved = {k: os.environ.get(k) for k in names}
    want = {(s, c.name): plan(L, c, ENVS[s]) for s in ('default', 't192nb') for c in CASES}
    own = {c.name: plan(L, c, {}, sw_null=True) for c in CASES}
    try:
        for values in ({'VKAS_NT_TILE': '224', 'VKAS_TN_TILE': '384', 'VKAS_NT_RING': '0'}, dict.fromkeys(names[3:], '1')):
            for k in names:
                os.environ.pop(k, None)
            os.environ.update(values)
            assert {(s, c.name): plan(L, c, ENVS[s]) for s in ('default', 't192nb') for c in CASES} == want
            assert {c.name: plan(L, c, {}, sw_null=True) for c in CASES} == own
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    for c in CASES:
        g, p = geom_struct(L, c), plan(L, c, {}, entry='nogb', sw_null=True)
        assert L.lib.vkas_conv_gemm_kernel_id(c.wgrad, ctypes.byref(g), c.Np, c.lddy, max(c.heads, default=0)) == p['kernel_id'], c.name
        if not c.wgrad and not c.heads and p['kernel_id']:
            assert L.lib.vkas_conv_gemm_tile(0, rows_of(c), c.Np, c.k * c.k * c.Cp) == (p['bn'] if p['family'] >= 2 else 1), c.name
        if c.wgrad and p['family'] == 0 and p['kernel_id']:
            assert L.lib.vkas_conv_gemm_tile(1, rows_of(c), c.Np, c.k * c.k * c.Cp) == p['bn'], c.name
