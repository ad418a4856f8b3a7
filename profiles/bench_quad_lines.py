"""Grouping character quadrilaterals into text lines at a page's size: synthetic pages of 512, 2048 and 8192 characters in
straight text lines (Latin proportions: height 1.9 x width, a word space every five characters, the page turned by 0.05 rad,
index order scrambled), for one image and for eight.  Per size:

* ops.quad_lines (eight launches, csrc/quadlines.hip), eager and replayed from a captured graph;
* the host route it replaces: inferencing/lines.py::quad_lines_lists_host on the same quads (match_rows, the numpy pair test
  over all pairs, a Python union-find and sort);
* what ``stats`` says: links per character, lines per image.

Device times are HIP-event times after warm-up; host times are wall times.  Every workload runs in a child process of its
own under its own time limit; after a child that fails or runs out of time nothing more is started.

    python profiles/bench_quad_lines.py [--iters N] [--log PATH] [--limit SECONDS]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from profiles.bench_quad_match import event_time  # noqa: E402

SIZES = (512, 2048, 8192)
BATCHES = (1, 8)
SIDE = 2048.0  # the page is about SIDE x SIDE pixels whatever it holds


def synthetic_page(n, seed):
    """``n`` characters in straight lines that fill a SIDE x SIDE page -> (n, 4, 2) float64 (y, x), index order scrambled"""
    g = np.random.default_rng(seed)
    height = (SIDE * SIDE / n / (1.4 * 0.7)) ** 0.5  # leading 1.4 heights, pitch 0.7 heights (with its share of word spaces)
    width, pitch, leading, space = height / 1.9, 0.62 * height, 1.4 * height, 0.4 * height
    per_line = max(int(SIDE / (pitch + space / 5)), 1)
    k = np.arange(n)
    c, l = k % per_line, k // per_line
    cx = c * pitch + (c // 5) * space + g.uniform(-0.02, 0.02, n) * height
    cy = l * leading + g.uniform(-0.02, 0.02, n) * height
    h, w = height * g.uniform(0.95, 1.05, n), width * g.uniform(0.9, 1.1, n)
    base = np.stack([np.stack([-h / 2, -w / 2], 1), np.stack([-h / 2, w / 2], 1), np.stack([h / 2, w / 2], 1),
                     np.stack([h / 2, -w / 2], 1)], axis=1) + np.stack([cy, cx], 1)[:, None, :]
    t = 0.05
    quads = np.stack([base[..., 0] * np.cos(t) + base[..., 1] * np.sin(t), -base[..., 0] * np.sin(t) + base[..., 1] * np.cos(t)], -1)
    return quads[g.permutation(n)]


def workload(kind, n, B, iters):
    import torch
    from vkit_ocr_model_adaptive_scaling_amd import ops
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import quad_lines_host, quad_lines_lists_host
    pages = [synthetic_page(n, 100 + b) for b in range(B)]
    if kind == 'device':
        dev = torch.device('cuda', 0)
        torch.zeros((1 << 20,), device=dev).cpu()  # the context and both copy directions exist before anything is timed
        torch.cuda.synchronize()
        d_quads = torch.from_numpy(np.stack(pages)).to(dev)
        d_count = torch.full((B,), n, dtype=torch.int32, device=dev)
        d_rows = ops.quad_rows(d_quads)
        call = lambda: ops.quad_lines(d_rows, d_count)
        eager = event_time(call, iters)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = call()
        replay = event_time(graph.replay, iters)
        stats = out[3].cpu().numpy()
        if n * B <= 2048:  # the answer is the oracle's (the larger sizes are held to it in tests/test_gpu_quad_lines.py)
            ref = quad_lines_host(d_rows.cpu().numpy(), d_count.cpu().numpy())
            assert all(np.array_equal(o.cpu().numpy(), r) for o, r in zip(out, ref))
        print(f'{n} characters x {B} images: ops.quad_lines {eager * 1e6:.1f} us eager, {replay * 1e6:.1f} us replayed; '
              f'{stats[:, 2].sum() / (n * B):.2f} links per character, {stats[:, 3].mean():.1f} lines per image', flush=True)
    else:
        t0 = time.perf_counter()
        _, stats = quad_lines_lists_host(pages)
        t_host = time.perf_counter() - t0
        print(f'{n} characters x {B} images: host route {t_host * 1e3:.0f} ms ({int(stats[2])} links, {int(stats[3])} lines)',
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--log', default=None, help='also append the lines to this file')
    ap.add_argument('--limit', type=int, default=120, help='seconds per workload')
    ap.add_argument('--child', nargs=3, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        workload(a.child[0], int(a.child[1]), int(a.child[2]), a.iters)
        return
    lines = []
    for n in SIZES:
        for B in BATCHES:
            for kind in ('device', 'host'):
                cmd = [sys.executable, os.path.abspath(__file__), '--iters', str(a.iters), '--child', kind, str(n), str(B)]
                try:
                    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.limit)
                except subprocess.TimeoutExpired:
                    print(f'{kind} {n} x {B}: no result within {a.limit} s; stopping', flush=True)
                    sys.exit(1)
                print(r.stdout, end='', flush=True)
                if r.returncode != 0:
                    print(f'{kind} {n} x {B}: exit status {r.returncode}; stopping', flush=True)
                    sys.exit(1)
                lines += [ln for ln in r.stdout.splitlines() if 'characters x' in ln]
    if a.log:
        with open(a.log, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
