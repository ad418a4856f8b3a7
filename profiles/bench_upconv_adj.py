#!/usr/bin/env python3
"""Time the E pass of the dense heads' backward alone, through the C ABI, at the two shapes of the benchmark (B = 8,
h = w = 256; N = 384 rough pass, N = 192 precise probability head): vkas_upconv_adj, vkas_colsum over the same dz, and
vkas_upconv_adj_colsum, which delivers both.  Milliseconds per launch: median of 5 rounds of 10 launches, and the spread
(max - min) of the rounds.  VKAS_LIB_PATH selects a variant build.  Arguments, if any, are segment lengths: the row walk of
vkas_upconv_adj_colsum_seg is timed at each of them as well (the plain entry chooses its own, csrc/upconv_adj.hip)."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from vkit_ocr_model_adaptive_scaling_amd import _lib  # noqa: E402

lib = _lib.lib
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def timed(fn, iters=10, rounds=5):
    ts = []
    for r in range(rounds + 1):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        if r:
            ts.append(s.elapsed_time(e) / iters)
    ts.sort()
    return ts[len(ts) // 2], ts[-1] - ts[0]


def p(t):
    return ctypes.c_void_p(t.data_ptr())


B, h, w = 8, 256, 256
g = torch.Generator(device='cuda').manual_seed(0)
for N in (384, 192):
    M = B * 4 * h * w
    dz = torch.randn((M, N), generator=g, device='cuda').bfloat16()
    E = torch.empty((B * h * w, 9 * N), dtype=torch.bfloat16, device='cuda')
    out = torch.zeros((N,), device='cuda')
    nb = lib.vkas_colsum_ws_bytes(M, N)
    ws = torch.empty((nb // 4 + 4,), device='cuda')
    has_cs = hasattr(lib, 'vkas_upconv_adj_colsum')
    if has_cs:
        nb2 = lib.vkas_upconv_adj_colsum_ws_bytes(B, h, w, N)
        ws2 = torch.empty((nb2 // 4 + 4,), device='cuda')

    def adj():
        assert lib.vkas_upconv_adj(p(dz), N, p(E), B, h, w, N, _lib.BF16, st) == 0

    def colsum():
        assert lib.vkas_colsum(p(dz), N, M, N, p(out), 1, p(ws), nb, _lib.BF16, st) == 0

    def adj_cs():
        assert lib.vkas_upconv_adj_colsum(p(dz), N, p(E), B, h, w, N, p(out), 1, p(ws2), nb2, _lib.BF16, st) == 0

    e = 2.0 * M * N
    for name, fn, nbytes in (('upconv_adj', adj, 3.25 * e), ('colsum', colsum, e)) + ((('upconv_adj_colsum', adj_cs, 3.25 * e),)
                                                                                     if has_cs else ()):
        ms, spread = timed(fn)
        print(f'N={N:4d} {name:18s} {ms:7.3f} ms  spread {spread:6.3f} ms  {nbytes / ms / 1e9:5.2f} TB/s', flush=True)
    for seg in [int(a) for a in sys.argv[1:]]:
        ms, spread = timed(lambda: lib.vkas_upconv_adj_colsum_seg(p(dz), N, p(E), B, h, w, N, p(out), 1, p(ws2), nb2, _lib.BF16, st,
                                                                  seg))
        print(f'N={N:4d} seg_rows {seg:9d} {ms:7.3f} ms  spread {spread:6.3f} ms  {3.25 * e / ms / 1e9:5.2f} TB/s', flush=True)
    del dz, E
