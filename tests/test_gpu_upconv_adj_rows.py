"""The row walk of vkas_upconv_adj_colsum (csrc/upconv_adj.hip) through the C ABI, with the segment length given
(vkas_upconv_adj_colsum_seg): at the smallest shapes that can go wrong its E is that of vkas_upconv_adj bit for bit and, on
small-integer dz, the fp64 sum E_k[s, n] = sum_q U[q, s] dz[q + k - 1, n] rounded once to the storage type; its column sums are
those of vkas_colsum exactly; both with accumulate off and on, and two launches give the same bits."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

CODE = {torch.bfloat16: 1, torch.float16: 2}
G = 64  # guard words behind every output
# (B, h, w, N, ld_extra, seg_rows); seg_rows 0 = the plain entry's rule
BORDERS = [(1, h, w, 8, 0, 0) for h in (1, 2, 3, 5) for w in (1, 2, 7)]  # every border combination, windows taller than the map
# several segments, a ragged last one, one longer than the image, all three phases of the unrolled walk; two images
SEGMENTS = [(2, 7, 5, 24, 0, s) for s in (1, 2, 3, 7, 100)]
# a single vector, nvec not dividing 256 (one and several pixels per chunk, several chunks), wide rows, lddz > N
WIDTHS = [(2, 5, 3, 8, 0, 2), (1, 7, 23, 24, 0, 3), (2, 7, 12, 200, 0, 3), (1, 4, 3, 200, 8, 2), (1, 3, 2, 2048, 0, 2)]
CASES = BORDERS + SEGMENTS + WIDTHS
# more (segment, chunk) pairs than the workspace has rows: a workgroup walks several chunks (B * h = 1400 source rows of
# three chunks in segments of one row, two workgroups per segment).  Too large for the host sum: against the two kernels only.
LOOPED = (1, 1400, 21, 200, 0, 1)


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def _dz(case, dtype):
    B, h, w, N, ld_extra, _ = case
    buf = torch.full((B, 2 * h, 2 * w, N + ld_extra), 99.0, dtype=dtype, device='cuda')  # the slack columns are never read
    v = torch.randint(-3, 4, (B, 2 * h, 2 * w, N), generator=torch.Generator().manual_seed(11)).double()
    buf[..., :N] = v.to(dtype).cuda()
    return buf[..., :N], v


def _run(case, dtype, dz, out0, accumulate):
    """(E, column sums, guards intact) of one launch; out0 is what the destination holds before"""
    from vkit_ocr_model_adaptive_scaling_amd._lib import lib, check
    B, h, w, N, ld_extra, seg = case
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    Eb = torch.full((B * h * w * 9 * N + G,), float('nan'), dtype=dtype, device='cuda')
    Eb[-G:] = -3.0
    ob = torch.full((N + G,), -3.0, device='cuda')
    ob[:N] = out0
    nbytes = lib.vkas_upconv_adj_colsum_ws_bytes(B, h, w, N)
    assert nbytes > 0
    ws = torch.full((nbytes // 4 + G,), -3.0, device='cuda')
    check(lib.vkas_upconv_adj_colsum_seg(p(dz), N + ld_extra, p(Eb), B, h, w, N, p(ob), accumulate, p(ws), nbytes, CODE[dtype],
                                         st, seg), 'upconv_adj_colsum_seg')
    torch.cuda.synchronize()
    ok = bool((Eb[-G:] == -3.0).all() and (ob[N:] == -3.0).all() and (ws[nbytes // 4:] == -3.0).all())
    return Eb[:-G].view(B, h, w, 9 * N), ob[:N].clone(), ok


def _upsample_matrix(n):
    """U (2n, n) in fp64: the x2 bilinear upsample, align_corners=False, as torch states it - source coordinate
    (q + 0.5) / 2 - 0.5 clamped at 0, its two neighbours clamped into the map"""
    U = torch.zeros((2 * n, n), dtype=torch.float64)
    for q in range(2 * n):
        x = max((q + 0.5) / 2 - 0.5, 0.0)
        x0 = int(x)
        x1 = min(x0 + 1, n - 1)
        U[q, x0] += 1.0 - (x - x0)
        U[q, x1] += x - x0
    return U


def _tap_matrices(n):
    """A (3, n, 2n): A[k][s, Q] = U[Q - (k - 1), s], zero where Q - (k - 1) leaves the map"""
    U = _upsample_matrix(n)
    A = torch.zeros((3, n, 2 * n), dtype=torch.float64)
    for k in range(3):
        for Q in range(2 * n):
            q = Q - (k - 1)
            if 0 <= q < 2 * n:
                A[k, :, Q] = U[q]
    return A


def _host_E(v, h, w):
    """E (B, h, w, 9 N) in fp64 from dz (B, 2h, 2w, N) in fp64"""
    Ay, Ax = _tap_matrices(h), _tap_matrices(w)
    E = torch.einsum('kiY,ljX,bYXn->bijkln', Ay, Ax, v)
    return E.reshape(v.shape[0], h, w, 9 * v.shape[3])


def _check(case, dtype, host):
    from vkit_ocr_model_adaptive_scaling_amd._lib import lib, check
    B, h, w, N, ld_extra, seg = case
    M = B * 4 * h * w
    assert 3 * M < 2 ** 24  # |sum| <= 3 M: exact in fp32 in any order
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dz, v = _dz(case, dtype)
    E_ref = torch.full((B, h, w, 9 * N), float('nan'), dtype=dtype, device='cuda')
    check(lib.vkas_upconv_adj(p(dz), N + ld_extra, p(E_ref), B, h, w, N, CODE[dtype], st), 'upconv_adj')
    nb = lib.vkas_colsum_ws_bytes(M, N)
    wsc = torch.empty((nb // 4 + 4,), device='cuda')
    plain = torch.empty((N,), device='cuda')
    check(lib.vkas_colsum(p(dz), N + ld_extra, M, N, p(plain), 0, p(wsc), nb, CODE[dtype], st), 'colsum')
    E, cs, ok = _run(case, dtype, dz, torch.full((N,), float('nan'), device='cuda'), 0)
    assert ok, 'guard words overwritten'
    assert torch.equal(E.view(torch.int16), E_ref.view(torch.int16)), 'E differs from vkas_upconv_adj'
    assert torch.equal(cs, plain), 'column sums differ from vkas_colsum'
    if host:
        # the weights are multiples of 1/16 and |dz| <= 3: every partial sum is exact in fp32 (and in fp64), so the kernel's
        # one rounding to the storage type is the only one
        want = _host_E(v, h, w).float().to(dtype)
        assert torch.equal(E.cpu().view(torch.int16), want.view(torch.int16)), 'E differs from the fp64 sum rounded once'
        assert torch.equal(cs.cpu().double(), v.sum(dim=(0, 1, 2)))
    base = torch.arange(N, device='cuda').float() - 7.0
    E_acc, cs_acc, ok = _run(case, dtype, dz, base, 1)
    assert ok
    assert torch.equal(E_acc.view(torch.int16), E_ref.view(torch.int16))
    assert torch.equal(cs_acc, base + cs), 'accumulate is not "out + sum"'
    E2, cs2, _ = _run(case, dtype, dz, torch.zeros((N,), device='cuda'), 0)
    assert torch.equal(E2.view(torch.int16), E.view(torch.int16)) and torch.equal(cs2.view(torch.int32), cs.view(torch.int32))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'B%d_%dx%d_N%d_ld%d_seg%d' % c)
def test_rows_match_both_kernels_and_the_host_sum(case, dtype):
    _check(case, dtype, host=True)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
def test_rows_workgroup_walks_several_chunks(dtype):
    from vkit_ocr_model_adaptive_scaling_amd._lib import lib
    B, h, w, N, _, seg = LOOPED
    chunks = -(-w // (256 // (N // 8)))
    rows = lib.vkas_upconv_adj_colsum_ws_bytes(B, h, w, N) // (4 * N)
    assert rows < B * -(-h // seg) * chunks  # fewer partial rows than (segment, chunk) pairs: the chunk loop runs twice
    _check(LOOPED, dtype, host=False)


def test_rows_plain_entry_is_the_seg_entry_with_the_rule():
    """the plain entry and seg_rows = 0 are the same launch: same bits, column sums included"""
    from vkit_ocr_model_adaptive_scaling_amd._lib import lib, check
    case = (2, 37, 9, 40, 0, 0)
    B, h, w, N, _, _ = case
    dz, _ = _dz(case, torch.bfloat16)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    E, cs, ok = _run(case, torch.bfloat16, dz, torch.zeros((N,), device='cuda'), 0)
    nbytes = lib.vkas_upconv_adj_colsum_ws_bytes(B, h, w, N)
    ws = torch.empty((nbytes // 4,), device='cuda')
    E1 = torch.empty_like(E)
    cs1 = torch.empty((N,), device='cuda')
    check(lib.vkas_upconv_adj_colsum(p(dz), N, p(E1), B, h, w, N, p(cs1), 0, p(ws), nbytes, 1, st), 'upconv_adj_colsum')
    torch.cuda.synchronize()
    assert ok and torch.equal(E1.view(torch.int16), E.view(torch.int16)) and torch.equal(cs1.view(torch.int32), cs.view(torch.int32))
    assert lib.vkas_upconv_adj_colsum_seg(p(dz), N, p(E1), B, h, w, N, p(cs1), 0, p(ws), nbytes, 1, st, -1) == -1
    assert b'segment length' in lib.vkas_last_error()
