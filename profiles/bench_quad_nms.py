"""Suppressing duplicate character quadrilaterals at a page's size: B = 8 pages of 500 and of 4000 characters in text lines
(the pages of bench_quad_match.py), every character predicted once with a small jitter and one in ten a second time, with
random probs.  Per size:

* ops.quad_rows (one launch) and ops.nms_quads (four launches, csrc/quadmatch.hip), eager and replayed from a captured graph;
* the host side they replace: match_rows on the same quads, and the host oracle route on the same tables
  (inferencing/nms.py::nms_quads_host: numpy box pruning, then a Python clip per pair and the sorted greedy rule);
* ratios from ``stats`` and ``rounds``: box-overlapping outranking pairs and candidates per character, rounds per image.

Device times are HIP-event times after warm-up; host times are wall times.  Every workload runs in a child process of its
own under its own time limit; after a child that fails or runs out of time nothing more is started.

    python profiles/bench_quad_nms.py [--iters N] [--log PATH] [--limit SECONDS]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from profiles.bench_quad_match import B, H, W, SIZES, event_time, synthetic_page  # noqa: E402


def duplicated_page(n, seed):
    """the ``n`` annotated characters of ``synthetic_page``, each predicted once and 10 % twice -> (quads (m, 4, 2), probs (m,)
    float32), shuffled"""
    gt, _ = synthetic_page(n, seed)
    g = np.random.default_rng(5000 + seed)
    cw = (H * W / n / 1.5) ** 0.5 * 0.95
    jitter = lambda q: q + g.normal(0, 0.02 * cw, (4, 2)) + g.normal(0, 0.03 * cw, (1, 2))
    dup = g.permutation(len(gt))[:len(gt) // 10]
    quads = np.stack([jitter(q) for q in gt] + [jitter(gt[k]) for k in dup])
    order = g.permutation(len(quads))
    return quads[order], g.uniform(0.7, 1.0, len(quads)).astype(np.float32)[order]


def workload(kind, n, iters):
    import torch
    from vkit_ocr_model_adaptive_scaling_amd import ops
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import match_rows, nms_quads_host
    pages = [duplicated_page(n, 100 + b) for b in range(B)]
    K = max(len(q) for q, _ in pages)
    quads, probs = np.zeros((B, K, 4, 2)), np.zeros((B, K), np.float32)
    count = np.array([len(q) for q, _ in pages], np.int32)
    for b, (q, p) in enumerate(pages):
        quads[b, :len(q)], probs[b, :len(q)] = q, p
    t0 = time.perf_counter()
    rows = np.stack([match_rows(quads[b])[0] for b in range(B)])
    t_rows = time.perf_counter() - t0
    chars = int(count.sum())
    if kind == 'device':
        dev = torch.device('cuda', 0)
        torch.zeros((1 << 20,), device=dev).cpu()  # the context and both copy directions exist before anything is timed
        torch.cuda.synchronize()
        d_quads, d_probs, d_count = (torch.from_numpy(t).to(dev) for t in (quads, probs, count))
        d_rows = ops.quad_rows(d_quads)
        assert np.array_equal(d_rows.cpu().numpy(), rows)
        rounds = torch.zeros((B,), dtype=torch.int32, device=dev)
        t_rows_dev = event_time(lambda: ops.quad_rows(d_quads), iters)
        call = lambda: ops.nms_quads(d_rows, d_count, d_probs, rounds=rounds)
        eager = event_time(call, iters)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            r_out = ops.quad_rows(d_quads)
            out = ops.nms_quads(r_out, d_count, d_probs, rounds=rounds)
        both = event_time(graph.replay, iters)
        graph2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph2):
            out = call()
        replay = event_time(graph2.replay, iters)
        stats, r = out[2].cpu().numpy(), rounds.cpu().numpy()
        assert not stats[:, 5].any()
        print(f'{n} characters x {B} images ({chars} quads, {int(stats[:, 0].sum())} kept): quad_rows {t_rows_dev * 1e6:.1f} us '
              f'eager, nms_quads {eager * 1e6:.1f} us eager, {replay * 1e6:.1f} us replayed, both replayed {both * 1e6:.1f} us; '
              f'{stats[:, 3].sum() / chars:.2f} box pairs and {stats[:, 4].sum() / chars:.2f} candidates per character, '
              f'{r.mean():.1f} rounds per image (most {r.max()}); match_rows {t_rows * 1e3:.1f} ms host', flush=True)
    else:
        t0 = time.perf_counter()
        stats = nms_quads_host(rows, count, probs)[2]
        t_host = time.perf_counter() - t0
        print(f'{n} characters x {B} images: host oracle route {t_host * 1e3:.0f} ms ({int(stats[:, 0].sum())} kept, '
              f'{int(stats[:, 3].sum())} pairs clipped); match_rows {t_rows * 1e3:.1f} ms host', flush=True)


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
