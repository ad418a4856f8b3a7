"""Curved text lines cut along their spines (ops.spine_strips_u8, csrc/spines.hip) against the straight route
(ops.quad_strips_u8, csrc/strips.hip) on §4q's workload: 1 and 8 images of 1024 x 1024 with 64 lines each of
about 600 x 40 px - 25 characters of 24 x 40 px -, cut to height 32 with the default parameters -

* straight lines turned by 0.05 rad: the spine route on the characters against the straight route on the same lines'
  rectangles (``line_quads`` of the grouped characters' frame: here the rectangle around the characters) - both routes
  then write the same number of pixels;
* the same lines bent to a radius of 400 px about their midpoints: the spine route alone, and the straight route on the
  chord rectangles for scale (it cuts other pixels: more of them, and not the line);
* the straight lines turned by 0.8 rad, the direction the ends of the bent lines reach (their tangent runs from -0.7 to 0.8
  rad): what a slanted direction costs without a bend.

For every workload: both launches of the spine route (columns, then strips), eager and replayed; the columns launch alone;
the straight route's one launch, eager and replayed; the ratio of the replayed times.  The two routes are timed in
alternation, three rounds, and the spread of the rounds is printed.  On the straight lines the two tables are compared
on the host: how far the routes put the centre of the same strip column from one another.

Device times are HIP-event times after warm-up.  No figure of this script is quoted anywhere until a log of it exists.

    python profiles/bench_spine_strips.py [--iters N] [--log PATH]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from profiles.bench_region_pack import event_time  # noqa: E402
from vkit_ocr_model_adaptive_scaling_amd import ops  # noqa: E402
from vkit_ocr_model_adaptive_scaling_amd.inferencing.spines import check_spine_rows, spine_columns_host, spine_rows, spine_table  # noqa: E402
from vkit_ocr_model_adaptive_scaling_amd.inferencing.strips import check_strip_rows, strip_rows, strip_table  # noqa: E402

SIDE, LINES, HEIGHT, CHARS = 1024, 64, 32, 25


def char_lines(angle, length, height, radius, seed):
    """64 lines of 25 characters, about ``length`` x ``height`` px each, 14 px apart (they overlap, as a cut may), the page
    turned by ``angle`` about the image's centre; ``radius``: None for straight lines, else every line is bent to that radius
    about its midpoint (its centre of curvature above it).  -> (list of (25, 4, 2) quads, (64, 4, 2) chord rectangles)."""
    g = np.random.default_rng(seed)
    c, s = np.cos(angle), np.sin(angle)
    turn = lambda y, x: (SIDE / 2 + y * c + x * s, SIDE / 2 - y * s + x * c)  # upright page coordinates about the centre
    lines, rects = [], np.zeros((LINES, 4, 2))
    for k in range(LINES):
        ln, ht = length * g.uniform(0.95, 1.05), height * g.uniform(0.95, 1.05)
        cy, cx = (k - (LINES - 1) / 2) * 14.0 + g.uniform(-2, 2), g.uniform(-40, 40)
        quads = np.zeros((CHARS, 4, 2))
        for m in range(CHARS):
            along = (m + 0.5) / CHARS * ln - ln / 2                # the character's centre along the line
            for corner, (a, d) in enumerate(((-1, -1), (1, -1), (1, 1), (-1, 1))):
                u, v = along + a * ln / CHARS / 2, d * ht / 2      # along the line, across it
                if radius is None:
                    y, x = cy + v, cx + u
                else:                                              # the character keeps its shape, turned onto the arc
                    t = along / radius
                    y = cy - radius + (radius + v) * np.cos(t) - (u - along) * np.sin(t)
                    x = cx + (radius + v) * np.sin(t) + (u - along) * np.cos(t)
                quads[m, corner] = turn(y, x)
        lines.append(quads)
        pts = quads.reshape(-1, 2)
        if radius is None:
            for corner, (a, d) in enumerate(((-1, -1), (1, -1), (1, 1), (-1, 1))):
                rects[k, corner] = turn(cy + d * ht / 2, cx + a * ln / 2)
        else:                                                      # the chord's rectangle around all corners
            A = (quads[-1].mean(axis=0) - quads[0].mean(axis=0))
            A /= np.hypot(*A)
            D = np.array([A[1], -A[0]])
            a, d = pts @ A, pts @ D
            for corner, (ua, ud) in enumerate(((a.min(), d.min()), (a.max(), d.min()), (a.max(), d.max()), (a.min(), d.max()))):
                rects[k, corner] = ua * A + ud * D
    return lines, rects


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--log', default=None, help='also append the lines to this file')
    a = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def replayed(fn):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        return graph.replay

    dev = torch.device('cuda', 0)
    g = np.random.default_rng(1)
    for name, angle, radius in (('straight, 0.05 rad', 0.05, None), ('bent to 400 px, 0.05 rad', 0.05, 400.0),
                                ('straight, 0.8 rad', 0.8, None)):
        for B in (1, 8):
            images = [g.integers(0, 256, (SIDE, SIDE, 3), dtype=np.uint8) for _ in range(B)]
            arena, sources, d_sources = ops.image_arena(images, dev)
            scene = [char_lines(angle, 600.0, 40.0, radius, 10 + b) for b in range(B)]
            spine = spine_rows([s[0] for s in scene], HEIGHT)
            check_spine_rows(spine.rows, spine.knots, sources, HEIGHT, spine.out_bytes, spine.columns)
            quad = strip_rows([s[1] for s in scene], HEIGHT)
            check_strip_rows(quad.rows, sources, HEIGHT, quad.out_bytes)
            assert len(spine.rows) == len(quad.rows) == B * LINES
            n, T = len(spine.rows), len(spine.knots)
            d_spine = torch.from_numpy(spine_table(spine.rows, spine.knots, HEIGHT)).to(dev)
            d_quad = torch.from_numpy(strip_table(quad.rows, HEIGHT)).to(dev)
            runs = {'spine': lambda: ops.spine_strips_u8(arena, d_sources, d_spine, n, T, HEIGHT, spine.out_bytes, validate=False),
                    'columns alone': lambda: ops.spine_columns(d_spine, n, T, HEIGHT, spine.columns, validate=False),
                    'straight': lambda: ops.quad_strips_u8(arena, d_sources, d_quad, HEIGHT, quad.out_bytes, validate=False)}
            graphs = {k: replayed(fn) for k, fn in runs.items()}
            times = {k: [] for k in list(runs) + [k + ', replayed' for k in runs]}
            for _ in range(3):  # in alternation: the spread of the rounds is the noise
                for k in runs:
                    times[k].append(event_time(runs[k], a.iters))
                    times[k + ', replayed'].append(event_time(graphs[k], a.iters))
            us = lambda k: f'{min(times[k]) * 1e6:.1f} us (rounds {", ".join(f"{t * 1e6:.1f}" for t in times[k])})'
            ratio = min(times['spine, replayed']) / min(times['straight, replayed'])
            say(f'{name}, {B} x {LINES} lines of {CHARS} characters, {T} knots, log2n {sorted(set(spine.rows[:, 7].tolist()))}, spine '
                f'widths {int(spine.rows[:, 3].min())}..{int(spine.rows[:, 3].max())} in slots {sorted(set(spine.rows[:, 2].tolist()))}, '
                f'{spine.out_bytes / 1e6:.2f} MB; straight widths {int(quad.rows[:, 3].min())}..{int(quad.rows[:, 3].max())} in slots '
                f'{sorted(set(quad.rows[:, 2].tolist()))}, log2n {sorted(set(quad.rows[:, 10].tolist()))}, {quad.out_bytes / 1e6:.2f} MB')
            for k in times:
                say(f'    {k}: {us(k)}')
            say(f'    spine route / straight route, replayed: {ratio:.2f}')
            if radius is None and np.array_equal(spine.rows[:, 1:4], quad.rows[:, 1:4]):
                worst = 0.0  # where the two routes put the centre of each column (host arithmetic on the two tables)
                for sr, qr in zip(spine.rows[:LINES].tolist(), quad.rows[:LINES].tolist()):
                    c = spine_columns_host(spine.knots[sr[4]:sr[4] + sr[5]], sr[3], HEIGHT).astype(np.float64)
                    j, mid = np.arange(sr[3]), (HEIGHT - 1) / 2
                    dy = c[:, 0] + mid * c[:, 2] - (qr[4] + mid * qr[6] + j * qr[7])
                    dx = c[:, 1] + mid * c[:, 4] - (qr[5] + mid * qr[8] + j * qr[9])
                    worst = max(worst, float(np.hypot(dy, dx).max()) / 65536)
                say(f'    same slots and widths; a column centre of the spine route lies at most {worst:.2f} px from the straight '
                    f"route's (a knot sits on the nearest whole column, a column is about 1.4 px)")
    if a.log:
        with open(a.log, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
