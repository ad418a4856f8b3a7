"""vkas_upconv_adj_colsum (csrc/upconv_adj.hip) through the C ABI: its E is that of vkas_upconv_adj bit for bit, and its
column sums are those of vkas_colsum over dz - exact on integer dz, within the fp32 summation bound of an fp64 sum on random
dz, added onto what the destination holds when asked to, and the same bits in two launches."""
import ctypes

import pytest
import torch

from tests.test_gpu_ops import rnd

pytestmark = pytest.mark.gpu

CODE = {torch.bfloat16: 1, torch.float16: 2}
# the last case: 2 048 source rows of three chunks (10 pixels of 25 vectors each), so two workgroups per row and the first of
# them walks two chunks - the strided chunk loop with its sums carried in LDS, as at the benchmark's shapes
CASES = [(2, 7, 9, 40, 0), (1, 2, 2, 8, 0), (2, 16, 31, 200, 8), (1, 64, 64, 192, 0), (2, 1024, 23, 200, 8)]
G = 64


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def _dz(case, dtype, integer):
    B, h, w, N, ld_extra = case
    buf = torch.full((B, 2 * h, 2 * w, N + ld_extra), 99.0, dtype=dtype, device='cuda')  # the slack columns are never summed
    if integer:
        v = torch.randint(-3, 4, (B, 2 * h, 2 * w, N), generator=torch.Generator().manual_seed(5)).double()
    else:
        v = rnd((B, 2 * h, 2 * w, N), 7)
    buf[..., :N] = v.to(dtype).cuda()
    return buf[..., :N]


def _run(case, dtype, dz, out0, accumulate):
    """(E, column sums, guards intact) of one launch; out0 is what the destination holds before"""
    from vkit_ocr_model_adaptive_scaling_amd._lib import lib, check
    B, h, w, N, ld_extra = case
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    Eb = torch.full((B * h * w * 9 * N + G,), float('nan'), dtype=dtype, device='cuda')
    Eb[-G:] = -3.0
    ob = torch.full((N + G,), -3.0, device='cuda')
    ob[:N] = out0
    nbytes = lib.vkas_upconv_adj_colsum_ws_bytes(B, h, w, N)
    assert nbytes > 0 and nbytes % (4 * N * B * h) == 0
    if B * h >= 2048:  # fewer workgroups per row than chunks: the chunk loop runs more than once
        assert nbytes // (4 * N * B * h) < -(-w // (256 // (N // 8)))
    ws = torch.full((nbytes // 4 + G,), -3.0, device='cuda')
    check(lib.vkas_upconv_adj_colsum(p(dz), N + ld_extra, p(Eb), B, h, w, N, p(ob), accumulate, p(ws), nbytes, CODE[dtype], st),
          'upconv_adj_colsum')
    torch.cuda.synchronize()
    ok = bool((Eb[-G:] == -3.0).all() and (ob[N:] == -3.0).all() and (ws[nbytes // 4:] == -3.0).all())
    return Eb[:-G].view(B, h, w, 9 * N), ob[:N].clone(), ok


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'B%d_%dx%d_N%d_ld%d' % c)
def test_upconv_adj_colsum_matches_its_two_parts(case, dtype):
    from vkit_ocr_model_adaptive_scaling_amd._lib import lib, check
    B, h, w, N, ld_extra = case
    M = B * 4 * h * w
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for integer in (True, False):
        dz = _dz(case, dtype, integer)
        E_ref = torch.full((B, h, w, 9 * N), float('nan'), dtype=dtype, device='cuda')
        check(lib.vkas_upconv_adj(p(dz), N + ld_extra, p(E_ref), B, h, w, N, CODE[dtype], st), 'upconv_adj')
        E, cs, ok = _run(case, dtype, dz, torch.full((N,), float('nan'), device='cuda'), 0)
        assert ok, 'guard words overwritten'
        assert torch.equal(E.view(torch.int16), E_ref.view(torch.int16)), 'E differs from vkas_upconv_adj'
        ref = dz.double().sum(dim=(0, 1, 2))
        if integer:  # |sum| <= 3 M < 2^24: exact in fp32 in any order
            assert 3 * M < 2 ** 24 and torch.equal(cs.double(), ref)
        else:  # fp32 sums of M terms in a tree of partial sums: well inside M * 2^-24 * sum |terms|
            bound = M * 2.0 ** -24 * dz.double().abs().sum(dim=(0, 1, 2))
            err = (cs.double() - ref).abs()
            print('colsum: largest error %.3e, bound there %.3e' % (float(err.max()), float(bound[err.argmax()])))
            assert bool((err <= bound).all())
        # accumulate: onto what the destination holds, as vkas_colsum does it
        base = torch.arange(N, device='cuda').float() - 7.0 if integer else rnd((N,), 9).float().cuda()
        _, cs_acc, ok = _run(case, dtype, dz, base, 1)
        assert ok
        nb = lib.vkas_colsum_ws_bytes(M, N)
        ws = torch.empty((nb // 4 + 4,), device='cuda')
        plain, acc = torch.empty((N,), device='cuda'), base.clone()
        check(lib.vkas_colsum(p(dz), N + ld_extra, M, N, p(plain), 0, p(ws), nb, CODE[dtype], st), 'colsum')
        check(lib.vkas_colsum(p(dz), N + ld_extra, M, N, p(acc), 1, p(ws), nb, CODE[dtype], st), 'colsum')
        torch.cuda.synchronize()
        assert torch.equal(cs_acc, base + cs), 'accumulate is not "out + sum"'
        assert torch.equal(acc, base + plain), 'vkas_colsum accumulates differently'
        if integer:
            assert torch.equal(cs, plain) and torch.equal(cs_acc, acc)
        # two launches: the same bits
        E2, cs2, _ = _run(case, dtype, dz, torch.zeros((N,), device='cuda'), 0)
        assert torch.equal(E2.view(torch.int16), E.view(torch.int16)) and torch.equal(cs2.view(torch.int32), cs.view(torch.int32))
