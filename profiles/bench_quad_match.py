"""Scoring character quadrilaterals at a validation pass's size: B = 8 pages of 500 and of 4000 annotated characters in
text lines, with predictions of them that are jittered, 10 % missing, 10 % duplicated, plus 4 % spurious.  Per size:

* the device call (ops.match_quads, csrc/quadmatch.hip: four launches), eager and replayed from a captured graph;
* the host oracle route on the same tables (inferencing/evaluation.py::match_quads_host: numpy box pruning, then a Python
  clip per pair and the sorted greedy matching): what a validation pass without the kernels would do;
* the host side that remains either way: building the rows (match_rows) and uploading them;
* two ratios from ``stats`` and ``rounds``: box-overlapping pairs per annotated character, and matching rounds per image.

Device times are HIP-event times after warm-up; host times are wall times.  Every workload runs in a child process of its
own under its own time limit; after a child that fails or runs out of time nothing more is started.

    python profiles/bench_quad_match.py [--iters N] [--log PATH] [--limit SECONDS]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, W = 8, 2048, 2048
SIZES = (500, 4000)


def synthetic_page(n, seed):
    """``n`` character boxes in text lines that fill an (H, W) image - height 1.5 x width, a slant of up to 2 degrees per
    line - and predictions of them -> (gt (n, 4, 2), pred (m, 4, 2)) in image pixels"""
    g = np.random.default_rng(seed)
    cw = (H * W / n / 1.5) ** 0.5 * 0.95
    ch = 1.5 * cw
    gt = []
    y = 0.6 * ch
    while len(gt) < n and y < H - 0.6 * ch:
        t = np.radians(g.uniform(-2, 2))
        right, down = np.array([np.sin(t), np.cos(t)]), np.array([np.cos(t), -np.sin(t)])
        x = 0.6 * cw
        while x < W - 0.6 * cw and len(gt) < n:
            c = np.array([y + (x - W / 2) * np.tan(t), x]) + g.uniform(-0.05, 0.05, 2) * cw
            hw, hh = 0.45 * cw * g.uniform(0.8, 1.1), 0.45 * ch * g.uniform(0.8, 1.1)
            gt.append([c - hw * right - hh * down, c + hw * right - hh * down, c + hw * right + hh * down,
                       c - hw * right + hh * down])
            x += cw
        y += ch
    gt = np.array(gt)
    jitter = lambda q: q + g.normal(0, 0.04 * cw, (4, 2)) + g.normal(0, 0.06 * cw, (1, 2))
    pred = []
    for q in gt:
        u = g.uniform()
        if u < 0.1:
            continue
        pred.append(jitter(q))
        if u > 0.9:
            pred.append(jitter(q))
    for _ in range(max(1, n // 25)):
        c = g.uniform(0, 1, 2) * (H, W)
        pred.append(np.array([[-0.5 * ch, -0.5 * cw], [-0.5 * ch, 0.5 * cw], [0.5 * ch, 0.5 * cw], [0.5 * ch, -0.5 * cw]]) + c)
    pred = np.array(pred)
    return gt, pred[g.permutation(len(pred))]


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
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import evaluation_tables, match_quads_host
    pages = [synthetic_page(n, 100 + b) for b in range(B)]
    t0 = time.perf_counter()
    tables = evaluation_tables([p for _, p in pages], [g for g, _ in pages])
    t_rows = time.perf_counter() - t0
    chars = int(tables[1].sum())
    if kind == 'device':
        dev = torch.device('cuda', 0)
        torch.zeros((1 << 20,), device=dev).cpu()  # the context and both copy directions exist before anything is timed
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d = [torch.from_numpy(t).to(dev) for t in tables[:4]]
        torch.cuda.synchronize()
        t_up = time.perf_counter() - t0
        rounds = torch.zeros((B,), dtype=torch.int32, device=dev)
        call = lambda: ops.match_quads(*d, rounds=rounds)
        eager = event_time(call, iters)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = call()
        replay = event_time(graph.replay, iters)
        stats, r = out[3].cpu().numpy(), rounds.cpu().numpy()
        assert not stats[:, 5].any()
        tp, n_pred = int(stats[:, 0].sum()), int(stats[:, 2].sum())
        print(f'{n} characters x {B} images ({chars} annotated, {n_pred} predicted, tp {tp}): device {eager * 1e6:.1f} us eager, '
              f'{replay * 1e6:.1f} us replayed; {stats[:, 3].sum() / chars:.2f} box pairs and {stats[:, 4].sum() / chars:.2f} '
              f'candidates per character, {r.mean():.1f} rounds per image (most {r.max()}); match_rows {t_rows * 1e3:.1f} ms '
              f'host, upload of the tables {t_up * 1e3:.2f} ms', flush=True)
    else:
        t0 = time.perf_counter()
        stats = match_quads_host(*tables[:4])[3]
        t_host = time.perf_counter() - t0
        print(f'{n} characters x {B} images: host oracle route {t_host * 1e3:.0f} ms (tp {int(stats[:, 0].sum())}, '
              f'{int(stats[:, 3].sum())} pairs clipped)', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=500)
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
            lines += [ln for ln in r.stdout.splitlines() if 'characters x' in ln]
    if a.log:
        with open(a.log, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
