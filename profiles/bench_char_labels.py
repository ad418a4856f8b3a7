"""Training label maps from character quadrilaterals at the train step's size: B = 8, 512 x 512 maps (1024 x 1024 images,
f = 2, core box = the map minus 10 pixels per side), 500 and 4000 synthetic text-line-like quads per image.  Per size:

* the device call (ops.char_label_maps, csrc/labels.hip: mask, height and score in one launch), eager and replayed from a
  captured graph, with its achieved bytes per second - the three maps written plus the table read - beside the achievable
  HBM rate;
* the host oracle route on the same tables (dataset/labels.py::char_label_maps_host, plain numpy, a loop over quads) plus
  the upload of its three maps: what a loader without the kernel would do;
* the host side that remains either way: building the rows (quad_rows) and uploading them.

Device times are HIP-event times after warm-up; host times are wall times around a synchronise.  Every workload runs in a
child process of its own under its own time limit; after a child that fails or runs out of time nothing more is started.

    python profiles/bench_char_labels.py [--iters N] [--log PATH] [--limit SECONDS]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12  # bytes per second: what a streaming kernel reaches on this part
B, H, W, F, MARGIN = 8, 512, 512, 2, 10
SIZES = (500, 4000)


def synthetic_quads(n, seed):
    """``n`` character boxes in text lines that fill the (H, W) map: height 1.5 x width, a slant of up to 4 degrees per
    line, a little jitter per character; map pixels times F"""
    g = np.random.default_rng(seed)
    cw = (H * W / n / 1.5) ** 0.5
    ch = 1.5 * cw
    quads = []
    y = 0.6 * ch
    while len(quads) < n:
        if y > H - 0.6 * ch:
            y = 0.6 * ch + g.random() * 0.3 * ch  # page full: another pass of lines over it (overlapping characters)
        t = np.radians(g.uniform(-4, 4))
        right, down = np.array([np.sin(t), np.cos(t)]), np.array([np.cos(t), -np.sin(t)])
        x = 0.6 * cw
        while x < W - 0.6 * cw and len(quads) < n:
            c = np.array([y + (x - W / 2) * np.tan(t), x]) + g.uniform(-0.05, 0.05, 2) * cw
            hw, hh = 0.45 * cw * g.uniform(0.8, 1.1), 0.45 * ch * g.uniform(0.8, 1.1)
            quads.append([c - hw * right - hh * down, c + hw * right - hh * down, c + hw * right + hh * down,
                          c - hw * right + hh * down])
            x += cw
        y += ch
    return np.array(quads) * F


def event_time(fn, iters):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def workload(kind, n, iters):
    import torch
    from vkit_ocr_model_adaptive_scaling_amd import ops
    from vkit_ocr_model_adaptive_scaling_amd.dataset import quad_rows, char_label_maps_host
    dev = torch.device('cuda', 0)
    torch.zeros((1 << 20,), device=dev).cpu()  # the context and both copy directions exist before anything is timed
    torch.cuda.synchronize()
    box = (MARGIN, H - MARGIN - 1, MARGIN, W - MARGIN - 1)
    quads = [synthetic_quads(n, 100 + b) for b in range(B)]
    t0 = time.perf_counter()
    tabs = [quad_rows(q, H, W, F) for q in quads]
    t_rows = time.perf_counter() - t0
    rows = np.stack([r for r, _ in tabs])
    count = np.full((B,), n, dtype=np.int32)
    valid = sum(int(ok.sum()) for _, ok in tabs)
    ch, cw = box[1] - box[0] + 1, box[3] - box[2] + 1
    nbytes = 3 * B * ch * cw * 4 + rows.nbytes
    if kind == 'device':
        t0 = time.perf_counter()
        d_rows, d_count = torch.from_numpy(rows).to(dev), torch.from_numpy(count).to(dev)
        torch.cuda.synchronize()
        t_up = time.perf_counter() - t0
        call = lambda: ops.char_label_maps(d_rows, d_count, H, W, box)
        eager = event_time(call, iters)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = call()
        replay = event_time(graph.replay, iters)
        covered = float(out[1].mean())
        rate = nbytes / replay
        print(f'{n} quads x {B} images ({valid} valid, {100 * covered:.0f} % of the core box covered), {ch} x {cw} maps: device '
              f'{eager * 1e6:.1f} us eager, {replay * 1e6:.1f} us replayed = {rate / 1e12:.3f} TB/s of {nbytes / 1e6:.2f} MB '
              f'(three maps + table), {100 * rate / HBM_ACHIEVABLE:.1f} % of the achievable HBM rate '
              f'({HBM_ACHIEVABLE / 1e12:.1f} TB/s); quad_rows {t_rows * 1e3:.1f} ms host, upload of the table '
              f'{t_up * 1e3:.2f} ms', flush=True)
    else:
        t0 = time.perf_counter()
        _, mask, height, score = char_label_maps_host(rows, count, H, W, box)
        t_host = time.perf_counter() - t0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        up = [torch.from_numpy(a).to(dev) for a in (mask, height, score)]
        torch.cuda.synchronize()
        t_up = time.perf_counter() - t0
        print(f'{n} quads x {B} images: host oracle route {t_host * 1e3:.0f} ms + upload of the three maps {t_up * 1e3:.2f} ms '
              f'({up[0].numel() * 12 / 1e6:.1f} MB)', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=2000)
    ap.add_argument('--log', default=None, help='also append the lines to this file')
    ap.add_argument('--limit', type=int, default=120, help='seconds per workload')
    ap.add_argument('--child', nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        workload(a.child[0], int(a.child[1]), a.iters)
        return
    lines = []
    for n in SIZES:
        for kind in ('device', 'host'):
            cmd = [sys.executable, os.path.abspath(__file__), '--iters', str(a.iters), '--child', kind, str(n)]
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print(f'{kind} {n}: no result within {a.limit} s; stopping', flush=True)
                sys.exit(1)
            print(r.stdout, end='', flush=True)
            if r.returncode != 0:
                print(f'{kind} {n}: exit status {r.returncode}; stopping', flush=True)
                sys.exit(1)
            lines += [ln for ln in r.stdout.splitlines() if 'quads x' in ln]
    if a.log:
        with open(a.log, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
