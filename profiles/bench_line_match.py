"""The text-line score at a validation pass's size: B = 8 synthetic pages of 64 and of 1024 annotated lines.  About a third
of the lines are predicted as two or three words, a sixth are merged in pairs, one in twenty is missing, the rest are whole
and jittered; one prediction in twenty is spurious, one annotation in twenty a don't-care one; the order is shuffled.  Per size:

* the device call (ops.match_lines, csrc/linematch.hip: four launches), eager and replayed from a captured graph;
* the host oracle route on the same tables (inferencing/line_evaluation.py::match_lines_host) - the comparison, because
  before this entry the project had no line score at all;
* from ``stats``: the rounds of each phase and the box pairs and candidates per annotated line.

Device times are HIP-event times after warm-up; host times are wall times.  Every workload runs in a child process of its
own under its own time limit; after a child that fails or runs out of time nothing more is started.

    python profiles/bench_line_match.py [--iters N] [--log PATH] [--limit SECONDS]
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

B = 8
SIZES = (64, 1024)


def _seg(y0, x0, deg, s0, s1, h):
    """the stretch [s0, s1] of a text row that starts at (y0, x0) and runs at ``deg``, h high -> (4, 2) (y, x)"""
    t = np.deg2rad(deg)
    c = np.array([y0 + (s0 + s1) / 2 * np.sin(t), x0 + (s0 + s1) / 2 * np.cos(t)])
    right, down = np.array([np.sin(t), np.cos(t)]), np.array([np.cos(t), -np.sin(t)])
    hw, hh = (s1 - s0) / 2, h / 2
    return np.array([c - hw * right - hh * down, c + hw * right - hh * down, c + hw * right + hh * down, c - hw * right + hh * down])


def line_page(n, seed):
    """``n`` annotated lines, eight to a text row -> (gt (n, 4, 2), care (n,) uint8, pred (m, 4, 2))"""
    g = np.random.default_rng(seed)
    gt, pred, k, row = [], [], 0, 0
    while k < n:
        y0, deg, h = 40.0 + 44.0 * row, g.uniform(-1, 1), g.uniform(20, 30)
        s, spans = 0.0, []
        for _ in range(min(8, n - k)):
            w = g.uniform(80, 200)
            spans.append((s, s + w))
            s += w + g.uniform(6, 14)
        k, row = k + len(spans), row + 1
        gt += [_seg(y0, 20.0, deg, a, b, h) for a, b in spans]
        jit = lambda a, b: _seg(y0 + g.normal(0, 0.8), 20.0 + g.normal(0, 0.8), deg + g.normal(0, 0.2), a, b, h * g.uniform(0.9, 1.1))
        i = 0
        while i < len(spans):
            a, b = spans[i]
            u = g.uniform()
            nxt = spans[i + 1] if i + 1 < len(spans) else None
            # a merge in which one line fills under 0.4 of the detection would be a one-to-one match of the other line
            if u < 1 / 3 and nxt and min(b - a, nxt[1] - nxt[0]) > 0.43 * (nxt[1] - a):
                pred.append(jit(a, nxt[1]))
                i += 2
                continue
            if u < 1 / 2:
                cuts = np.r_[0.0, np.sort(g.uniform(0.25, 0.75, g.integers(1, 3))), 1.0] * (b - a) + a
                pred += [jit(cuts[j] + 2, cuts[j + 1] - 2) for j in range(len(cuts) - 1) if cuts[j + 1] - cuts[j] > 8]
            elif u < 0.95:
                pred.append(jit(a + g.normal(0, 2), b + g.normal(0, 2)))
            i += 1
    for _ in range(max(1, n // 20)):
        pred.append(_seg(g.uniform(20, 40 + 44 * row), g.uniform(20, 1200), g.uniform(-10, 10), 0, g.uniform(40, 120),
                         g.uniform(15, 30)))
    gt, pred = np.stack(gt), np.stack(pred)
    return gt, (g.uniform(size=len(gt)) >= 0.05).astype(np.uint8), pred[g.permutation(len(pred))]


def tables_of(n):
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import padded_sides, quad_rows_host
    pages = [line_page(n, 100 + b) for b in range(B)]
    h_gt, gt_count, care, h_pred, pred_count = padded_sides([p[2] for p in pages], [p[0] for p in pages], [p[1] for p in pages])
    return quad_rows_host(h_gt), gt_count, care, quad_rows_host(h_pred), pred_count


def workload(kind, n, iters):
    import torch
    from vkit_ocr_model_adaptive_scaling_amd import ops
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import LineScore, match_lines_host
    tables = tables_of(n)
    lines = int(tables[1].sum())
    if kind == 'device':
        dev = torch.device('cuda', 0)
        torch.zeros((1 << 20,), device=dev).cpu()  # the context and both copy directions exist before anything is timed
        d = [torch.from_numpy(t).to(dev) for t in tables]
        torch.cuda.synchronize()
        call = lambda: ops.match_lines(*d)
        eager = event_time(call, iters)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = call()
        replay = event_time(graph.replay, iters)
        stats = out[4].cpu().numpy()
        assert not stats[:, 11].any()
        score = LineScore()
        for st in stats:
            score.add(st)
        print(f'{n} lines x {B} images ({lines} annotations, {int(stats[:, 7].sum())} of them don\'t-care, '
              f'{int(tables[4].sum())} predictions, {int(stats[:, 8].sum())} ignored): device {eager * 1e6:.1f} us eager, '
              f'{replay * 1e6:.1f} us replayed; {stats[:, 9].sum() / lines:.2f} box pairs and {stats[:, 10].sum() / lines:.2f} '
              f'candidates per annotated line; split rounds {stats[:, 12].tolist()}, merge rounds {stats[:, 13].tolist()}; '
              f'one-to-one {score.one_to_one}, split {score.split_gt} into {score.split_pred}, merged {score.merged_gt} into '
              f'{score.merge_pred}; recall {score.recall:.4f}, precision {score.precision:.4f}, F1 {score.f1:.4f}', flush=True)
    else:
        t0 = time.perf_counter()
        outs = match_lines_host(*tables)
        t_host = time.perf_counter() - t0
        print(f'{n} lines x {B} images: host oracle route {t_host * 1e3:.0f} ms (one-to-one {int(outs[4][:, 2].sum())}, '
              f'{int(outs[4][:, 9].sum())} pairs clipped)', flush=True)


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
            lines += [ln for ln in r.stdout.splitlines() if 'lines x' in ln]
    if a.log:
        with open(a.log, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
