"""The ribbon score at a validation pass's size: B = 8 synthetic pages of 64 and of 1024 annotated lines bent to a radius of
400 px, about 10 segments each.  About a third of the lines are predicted as two words, a sixth are merged in pairs, one in
twenty is missing, the rest are whole and jittered, every prediction with knots of its own; one prediction in twenty is
spurious, one annotation in twenty a don't-care one; the order is shuffled.  Per size:

* ``device``: ops.match_ribbons (csrc/ribbonmatch.hip: four launches), eager and replayed from a captured graph; from
  ``stats`` the rounds and the box pairs and candidates per annotated line;
* ``flat``: the same pages with every line as ONE segment (the quad through its end knots): ops.match_lines, the call the
  project had before, next to ops.match_ribbons on the one-segment tables;
* ``host``: the host oracle route on the same tables (inferencing/ribbon_evaluation.py::match_ribbons_host), and the
  segment pairs it clips per annotated line.

Device times are HIP-event means after warm-up; host times are wall times.  Every workload runs in a child process of its
own under its own time limit; after a child that fails or runs out of time nothing more is started.

    python profiles/bench_ribbon_match.py [--iters N] [--log PATH] [--limit SECONDS]
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
RADIUS = 400.0


def arc(cy, cx, h, a0, a1, n):
    """a line ``h`` high along the circle of RADIUS about (cy, cx) from angle a0 to a1 (degrees; 120 -> 60 runs left to
    right over the top), n segments -> ribbon (n + 1, 2, 2)"""
    a = np.deg2rad(np.linspace(a0, a1, n + 1))
    rail = lambda r: np.stack([cy - r * np.sin(a), cx + r * np.cos(a)], axis=1)
    return np.stack([rail(RADIUS + h / 2), rail(RADIUS - h / 2)], axis=1)


def ribbon_page(n, seed):
    """``n`` annotated lines, three to a text row -> (gt ribbons, care (n,) uint8, pred ribbons)"""
    g = np.random.default_rng(seed)
    gt, pred, row = [], [], 0
    nseg = lambda span: max(1, int(g.integers(6, 13) * span / 18.0 + 0.5))
    while len(gt) < n:
        cy, cx, h = 460.0 + 44.0 * row, 500.0, g.uniform(20, 28)
        row += 1
        a, spans = 120.0, []
        for _ in range(min(3, n - len(gt))):
            w = g.uniform(15, 19)
            spans.append((a, a - w))
            a -= w + g.uniform(1.0, 2.0)
        gt += [arc(cy, cx, h, a0, a1, nseg(a0 - a1)) for a0, a1 in spans]
        jit = lambda a0, a1: arc(cy + g.normal(0, 0.8), cx + g.normal(0, 0.8), h * g.uniform(0.9, 1.1), a0 + g.normal(0, 0.15),
                                 a1 + g.normal(0, 0.15), nseg(a0 - a1))
        i = 0
        while i < len(spans):
            a0, a1 = spans[i]
            u = g.uniform()
            if u < 1 / 3 and i + 1 < len(spans):
                pred.append(jit(a0, spans[i + 1][1]))
                i += 2
                continue
            if u < 1 / 2:
                cut = a0 - (a0 - a1) * g.uniform(0.3, 0.7)
                pred += [jit(a0, cut + 0.3), jit(cut - 0.3, a1)]
            elif u < 0.95:
                pred.append(jit(a0, a1))
            i += 1
    for _ in range(max(1, n // 20)):
        a0 = g.uniform(70, 120)
        pred.append(arc(g.uniform(300, 460 + 44 * row), g.uniform(300, 700), g.uniform(15, 25), a0, a0 - g.uniform(4, 10), 4))
    return gt, (g.uniform(size=len(gt)) >= 0.05).astype(np.uint8), [pred[i] for i in g.permutation(len(pred))]


def tables_of(n, flat=False):
    """the seven tables of ``ops.match_ribbons``; ``flat``: every line as the one quad through its end knots"""
    from vkit_ocr_model_adaptive_scaling_amd.inferencing.ribbon_evaluation import evaluation_ribbon_tables
    pages = [ribbon_page(n, 100 + b) for b in range(B)]
    ends = lambda lines: np.stack([np.stack([r[0, 0], r[-1, 0], r[-1, 1], r[0, 1]]) for r in lines]) if flat else lines
    return evaluation_ribbon_tables([ends(p[2]) for p in pages], [ends(p[0]) for p in pages], [p[1] for p in pages])


def timed(call, iters):
    import torch
    eager = event_time(call, iters)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    return eager, event_time(graph.replay, iters), out


def workload(kind, n, iters):
    import torch
    from vkit_ocr_model_adaptive_scaling_amd import ops
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import LineScore
    from vkit_ocr_model_adaptive_scaling_amd.inferencing.evaluation import box_pairs
    from vkit_ocr_model_adaptive_scaling_amd.inferencing.ribbon_evaluation import match_ribbons_host, ribbon_segments
    tables = tables_of(n, flat=kind == 'flat')
    lines = int(tables[1].sum())
    if kind == 'host':
        t0 = time.perf_counter()
        outs = match_ribbons_host(*tables)
        t_host = time.perf_counter() - t0
        clipped = 0
        for b in range(B):
            g, p = tables[0][b, :tables[1][b]], tables[4][b, :tables[5][b]]
            for a, c in zip(*(x.tolist() for x in box_pairs(g, p))):
                clipped += len(box_pairs(ribbon_segments(g[a], tables[3][b]), ribbon_segments(p[c], tables[6][b]))[0])
        print(f'{n} lines x {B} images: host oracle route {t_host * 1e3:.0f} ms (one-to-one {int(outs[4][:, 2].sum())}, '
              f'{int(outs[4][:, 9].sum())} box pairs of ribbons, {clipped} segment pairs clipped = {clipped / lines:.1f} per '
              f'annotated line)', flush=True)
        return
    dev = torch.device('cuda', 0)
    torch.zeros((1 << 20,), device=dev).cpu()  # the context and both copy directions exist before anything is timed
    d = [torch.from_numpy(t).to(dev) for t in tables]
    torch.cuda.synchronize()
    eager, replay, out = timed(lambda: ops.match_ribbons(*d), iters)
    stats = out[4].cpu().numpy()
    assert not stats[:, 11].any()
    if kind == 'flat':  # the segment tables of one-segment ribbons are the match rows of the same quads
        for rows, count, segs in ((tables[0], tables[1], tables[3]), (tables[4], tables[5], tables[6])):
            assert segs.shape == rows.shape and all((rows[b, :c, 0] == np.arange(c)).all() for b, c in enumerate(count))
        l_eager, l_replay, l_out = timed(lambda: ops.match_lines(d[3], d[1], d[2], d[6], d[5]), iters)
        same = all(torch.equal(x, y) for x, y in zip(out, l_out))
        print(f'{n} lines x {B} images, every line ONE segment: ops.match_lines {l_eager * 1e6:.1f} us eager, '
              f'{l_replay * 1e6:.1f} us replayed; ops.match_ribbons {eager * 1e6:.1f} us eager, {replay * 1e6:.1f} us replayed '
              f'({eager / l_eager:.2f}x, {replay / l_replay:.2f}x); {stats[:, 9].sum() / lines:.2f} box pairs and '
              f'{stats[:, 10].sum() / lines:.2f} candidates per annotated line; all outputs equal: {same}', flush=True)
        return
    score = LineScore()
    for st in stats:
        score.add(st)
    segs = float(np.concatenate([tables[0][b, :tables[1][b], 1] for b in range(B)]).mean())
    print(f'{n} lines x {B} images ({lines} annotations of {segs:.1f} segments on average, {int(stats[:, 7].sum())} of them '
          f'don\'t-care, {int(tables[5].sum())} predictions, {int(stats[:, 8].sum())} ignored): device {eager * 1e6:.1f} us eager, '
          f'{replay * 1e6:.1f} us replayed; {stats[:, 9].sum() / lines:.2f} box pairs and {stats[:, 10].sum() / lines:.2f} '
          f'candidates per annotated line; split rounds {stats[:, 12].tolist()}, merge rounds {stats[:, 13].tolist()}; '
          f'one-to-one {score.one_to_one}, split {score.split_gt} into {score.split_pred}, merged {score.merged_gt} into '
          f'{score.merge_pred}; recall {score.recall:.4f}, precision {score.precision:.4f}, F1 {score.f1:.4f}', flush=True)


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
        for kind in ('device', 'flat', 'host'):
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
