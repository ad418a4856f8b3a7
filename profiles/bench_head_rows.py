#!/usr/bin/env python3
"""Time the heads' row pass alone (vkas_head_rows_fwd, csrc/head.hip) through the C ABI at the benchmark's shapes: B = 8,
h = 256, W2 = 512, bf16; the rough set (192, 192) with oc (1, 1) and the precise set (192, 193, 194, 194) with oc
(1, 2, 4, 4), each with z and the statistics kept (training) and without (inference).  Milliseconds per launch: median of 5
rounds of 10 launches and the spread (max - min) of the rounds; GB/s of the algorithmic bytes (T read once, z, statistics and
maps written once) beside the 6.3 TB/s this card's HBM delivers.  Arguments, if any, are segment lengths: the pass is timed
at each of them as well (0, the default, lets the launcher choose).  VKAS_LIB_PATH selects another build of the library (the
entry's signature is that of the parent commit, so a parent library built with profiles/build_variant.sh runs the same inputs).
Each workload runs in a child process of its own under `timeout`; the parent process never touches the GPU."""
import argparse
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_LOG = os.path.join(ROOT, 'profiles', 'head_rows_groups.log')
HBM = 6.3e12
B, H, W2 = 8, 256, 512
WORKLOADS = {
    'rough-train': ((192, 192), (1, 1), True),
    'rough-infer': ((192, 192), (1, 1), False),
    'precise-train': ((192, 193, 194, 194), (1, 2, 4, 4), True),
    'precise-infer': ((192, 193, 194, 194), (1, 2, 4, 4), False),
}


def run_workload(name, segs, say):
    import torch
    from vkit_ocr_model_adaptive_scaling_amd import _lib
    lib = _lib.lib
    cs, ocs, keep = WORKLOADS[name]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = len(cs)
    nps = [(c + 7) // 8 * 8 for c in cs]
    offs = [sum(nps[:k]) for k in range(n + 1)]
    Nt, pw = offs[-1], 224
    M = B * 2 * H * W2
    g = torch.Generator(device='cuda').manual_seed(0)
    T = torch.zeros((B * H * W2, 3, Nt), device='cuda', dtype=torch.bfloat16)
    bias = torch.zeros((Nt,), device='cuda')
    params = torch.zeros((n, 6 * pw + 8), device='cuda')
    for k, (c, oc) in enumerate(zip(cs, ocs)):  # pad columns stay zero, as the convolution leaves them
        T[..., offs[k]:offs[k] + c] = torch.randn((B * H * W2, 3, c), generator=g, device='cuda').bfloat16()
        bias[offs[k]:offs[k] + c] = torch.randn((c,), generator=g, device='cuda') * 0.1
        params[k, :c] = 1.0 + 0.1 * torch.randn((c,), generator=g, device='cuda')
        params[k, pw:pw + c] = 0.1 * torch.randn((c,), generator=g, device='cuda')
        for r in range(oc):
            params[k, (2 + r) * pw:(2 + r) * pw + c] = torch.randn((c,), generator=g, device='cuda') * c ** -0.5
        params[k, 6 * pw:6 * pw + oc] = 0.1
    z = torch.empty((M, Nt), device='cuda', dtype=torch.bfloat16) if keep else None
    stats = torch.empty((n, M, 2), device='cuda') if keep else None
    proj = torch.empty((n, M, 8), device='cuda')
    hd = _lib.HeadDesc()
    hd.n_heads, hd.pw = n, pw
    for k in range(n):
        hd.n0[k], hd.np[k], hd.c[k], hd.oc[k] = offs[k], nps[k], cs[k], ocs[k]
    hd.params, hd.stats, hd.proj = params.data_ptr(), stats.data_ptr() if keep else None, proj.data_ptr()
    pz = ctypes.c_void_p(z.data_ptr() if keep else None)
    nbytes = T.numel() * 2 + proj.numel() * 4 + ((z.numel() * 2 + stats.numel() * 4) if keep else 0)

    def timed(seg, iters=10, rounds=5):
        ts = []
        for r in range(rounds + 1):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                rc = lib.vkas_head_rows_fwd(ctypes.c_void_p(T.data_ptr()), ctypes.c_void_p(bias.data_ptr()), ctypes.byref(hd), pz, B,
                                            H, W2, Nt, seg, _lib.BF16, st)
                assert rc == 0, rc
            e.record()
            torch.cuda.synchronize()
            if r:
                ts.append(s.elapsed_time(e) / iters)
        ts.sort()
        return ts[len(ts) // 2], ts[-1] - ts[0]

    for seg in [0] + segs:
        ms, spread = timed(seg)
        rate = nbytes / (ms * 1e-3)
        say(f'[{name}] seg_rows {seg:3d}: {ms:7.3f} ms  spread {spread:6.3f} ms  {nbytes / 1e9:5.2f} GB = {rate / 1e9:6.0f} GB/s, '
            f'{rate / HBM:4.2f} of {HBM / 1e12:.1f} TB/s')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('segs', nargs='*', type=int, help='segment lengths to time beside the launcher\'s own choice')
    ap.add_argument('--log', nargs='?', const=DEFAULT_LOG, default=None, help='also append the lines to this file')
    ap.add_argument('--limit', type=int, default=120, help='seconds per workload')
    ap.add_argument('--workload', choices=sorted(WORKLOADS), default=None, help='run this one here (what the parent starts)')
    a = ap.parse_args()
    if a.workload:
        lines = []

        def say(line):
            print(line, flush=True)
            lines.append(line)

        say(f'[{a.workload}] library {os.environ.get("VKAS_LIB_PATH") or "libvkas.so (this tree)"}')
        run_workload(a.workload, a.segs, say)
        if a.log:
            with open(a.log, 'a') as f:
                f.write('\n'.join(lines) + '\n')
        return
    for name in WORKLOADS:  # the parent never touches the GPU: a fresh child per workload, each under its own limit
        cmd = ['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--workload', name] + \
              (['--log', a.log] if a.log else []) + [str(s) for s in a.segs]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f'[{name}] ended with status {rc}: nothing more is started', flush=True)
            sys.exit(rc)


if __name__ == '__main__':
    main()
