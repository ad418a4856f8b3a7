"""Average precision of character quadrilaterals at a validation pass's size: the pages of profiles/bench_quad_match.py
(B = 8 pages of 500 and of 4000 annotated characters, predictions jittered, 10 % missing, 10 % duplicated, 4 % spurious)
with random probs and 5 % of the annotations turned into don't-care boxes, each laid over three neighbouring characters in
their place.  Per size:

* the device call (ops.match_quads_ranked, csrc/quadmatch.hip: four launches) at T = 1 (0.5) and T = 10 (0.5 : 0.05 : 0.95),
  eager and replayed from a captured graph;
* ops.match_quads at 0.5 on the same tables as a yardstick: the three shared passes and one matching workgroup per image;
* the host oracle route on the same tables (inferencing/ranking.py::match_quads_ranked_host) at T = 10;
* the curve on the host (ranked_score: sorting and AP at T thresholds), which remains either way;
* from ``stats`` and ``rounds``: candidates per character at 0.5 and rounds per (image, threshold).

Device times are HIP-event times after warm-up; host times are wall times.  Every workload runs in a child process of its
own under its own time limit; after a child that fails or runs out of time nothing more is started.

    python profiles/bench_quad_ap.py [--iters N] [--log PATH] [--limit SECONDS]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from profiles.bench_quad_match import B, SIZES, event_time, synthetic_page  # noqa: E402

T10 = tuple(0.5 + 0.05 * i for i in range(10))


def ranked_page(n, seed):
    """a page of ``synthetic_page`` with n // 20 don't-care boxes, each the bounding box of three characters that follow
    one another, in their place -> (gt, care, pred, probs)"""
    gt, pred = synthetic_page(n, seed)
    g = np.random.default_rng(9000 + seed)
    starts = np.sort(g.permutation(len(gt) // 4)[:n // 20]) * 4  # runs of three, a character apart at the least
    gone, boxes = [], []
    for s in starts.tolist():
        if s + 3 > len(gt) or not (np.diff(gt[s:s + 3].mean(axis=1)[:, 1]) > 0).all():
            continue  # the run would wrap into the next line
        run = gt[s:s + 3].reshape(-1, 2)
        y0, x0, y1, x1 = run[:, 0].min(), run[:, 1].min(), run[:, 0].max(), run[:, 1].max()
        boxes.append([[y0, x0], [y0, x1], [y1, x1], [y1, x0]])
        gone += [s, s + 1, s + 2]
    keep = np.setdiff1d(np.arange(len(gt)), gone)
    quads = np.concatenate([gt[keep], np.array(boxes, dtype=np.float64).reshape(-1, 4, 2)])
    care = np.r_[np.ones(len(keep), np.uint8), np.zeros(len(boxes), np.uint8)]
    return quads, care, pred, g.uniform(0.3, 1.0, len(pred)).astype(np.float32)


def tables_of(n):
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import padded_sides, quad_rows_host
    pages = [ranked_page(n, 100 + b) for b in range(B)]
    h_gt, gt_count, care, h_pred, pred_count, probs = padded_sides([p[2] for p in pages], [p[0] for p in pages],
                                                                   [p[1] for p in pages], [p[3] for p in pages])
    return quad_rows_host(h_gt), gt_count, care, quad_rows_host(h_pred), pred_count, probs


def workload(kind, n, iters):
    import torch
    from vkit_ocr_model_adaptive_scaling_amd import ops
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import match_quads_ranked_host, ranked_score
    tables = tables_of(n)
    chars = int(tables[1].sum())
    if kind == 'device':
        dev = torch.device('cuda', 0)
        torch.zeros((1 << 20,), device=dev).cpu()  # the context and both copy directions exist before anything is timed
        d = [torch.from_numpy(t).to(dev) for t in tables]
        torch.cuda.synchronize()
        yard = lambda: ops.match_quads(d[0], d[1], d[3], d[4])
        y_eager = event_time(yard, iters)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            yard()
        y_replay = event_time(graph.replay, iters)
        print(f'{n} characters x {B} images: ops.match_quads at 0.5 on the same tables {y_eager * 1e6:.1f} us eager, '
              f'{y_replay * 1e6:.1f} us replayed', flush=True)
        for thrs in ((0.5,), T10):
            T = len(thrs)
            rounds = torch.zeros((B, T), dtype=torch.int32, device=dev)
            call = lambda: ops.match_quads_ranked(*d, thrs, rounds=rounds)
            eager = event_time(call, iters)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = call()
            replay = event_time(graph.replay, iters)
            outs = [o.cpu().numpy() for o in out]
            stats, dc, r = outs[5], outs[6], rounds.cpu().numpy()
            assert not stats[:, :, 7].any()
            ranked_score(outs, tables[4], tables[5], thrs)  # warm-up, as for the device
            t0 = time.perf_counter()
            score = ranked_score(outs, tables[4], tables[5], thrs)
            t_curve = time.perf_counter() - t0
            print(f'{n} characters x {B} images, T = {T} ({chars} annotations, {int(dc[:, 0].sum())} of them don\'t-care, '
                  f'{int(stats[:, 0, 4].sum())} predictions, {int(dc[:, 2].sum())} covered): device {eager * 1e6:.1f} us eager, '
                  f'{replay * 1e6:.1f} us replayed; {stats[:, 0, 6].sum() / chars:.2f} candidates per character at 0.5, '
                  f'{r.mean():.2f} rounds per (image, threshold) (most {r.max()}); AP at {thrs[0]} = {score.ap[0]:.4f}, '
                  f'mAP {score.map:.4f}; the curve on the host {t_curve * 1e3:.1f} ms', flush=True)
    else:
        t0 = time.perf_counter()
        outs = match_quads_ranked_host(*tables, T10)
        t_host = time.perf_counter() - t0
        print(f'{n} characters x {B} images, T = 10: host oracle route {t_host * 1e3:.0f} ms (tp at 0.5 '
              f'{int(outs[5][:, 0, 0].sum())}, {int(outs[5][:, 0, 5].sum() + outs[6][:, 1].sum())} pairs clipped)', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--log', default=None, help='also append the lines to this file')
    ap.add_argument('--limit', type=int, default=150, help='seconds per workload')
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
