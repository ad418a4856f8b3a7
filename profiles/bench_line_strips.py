"""Text lines cut into upright strips (ops.quad_strips_u8, csrc/strips.hip): 1 and 8 images of 1024 x 1024 with
64 line rectangles each of about 600 x 40 px, cut to height 32 with the default parameters -

* turned by 0.05 rad (horizontal text);
* the same layout turned by 1.57 rad (vertical text);
* with 80 px high lines (2.5 source pixels per strip pixel, 4 x 4 sub-samples: log2n = 2).

For every workload: the one launch for all strips of all images, eager and replayed; the only route the tree had before for
the same rows - one ops.warp_pack_u8 call per image into a page that holds that image's slots one below the other (the
page's zero columns are not written there, which favours that route) -, eager and replayed; and the byte floor: the slot
bytes written plus the source bytes under the rectangles, with the rate the one launch reaches against it.

Device times are HIP-event times after warm-up.  No figure of this script is quoted anywhere until a log of it exists.

    python profiles/bench_line_strips.py [--iters N] [--log PATH]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from profiles.bench_region_pack import event_time  # noqa: E402
from vkit_ocr_model_adaptive_scaling_amd import ops  # noqa: E402
from vkit_ocr_model_adaptive_scaling_amd.inferencing.strips import check_strip_rows, strip_rows, strip_table  # noqa: E402

SIDE, LINES, HEIGHT = 1024, 64, 32


def line_quads(angle, length, height, seed):
    """64 rectangles of about ``length`` x ``height`` px: a page of lines 14 px apart (they overlap, as a cut may), the whole
    page turned by ``angle`` about the image's centre."""
    g = np.random.default_rng(seed)
    quads = np.zeros((LINES, 4, 2))
    c, s = np.cos(angle), np.sin(angle)
    for k in range(LINES):
        ln, ht = length * g.uniform(0.95, 1.05), height * g.uniform(0.95, 1.05)
        cy, cx = (k - (LINES - 1) / 2) * 14.0 + g.uniform(-2, 2), g.uniform(-40, 40)
        for corner, (a, d) in enumerate(((-1, -1), (1, -1), (1, 1), (-1, 1))):
            y, x = cy + d * ht / 2, cx + a * ln / 2          # upright page coordinates about the centre
            quads[k, corner] = (SIDE / 2 + y * c + x * s, SIDE / 2 - y * s + x * c)
    return quads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--log', default=None, help='also append the lines to this file')
    a = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def eager_and_replayed(fn):
        eager = event_time(fn, a.iters)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        return eager, event_time(graph.replay, a.iters)

    dev = torch.device('cuda', 0)
    g = np.random.default_rng(1)
    for name, angle, length, height in (('0.05 rad', 0.05, 600.0, 40.0), ('1.57 rad', 1.57, 600.0, 40.0),
                                        ('0.05 rad, 80 px lines', 0.05, 600.0, 80.0)):
        for B in (1, 8):
            images = [g.integers(0, 256, (SIDE, SIDE, 3), dtype=np.uint8) for _ in range(B)]
            arena, sources, d_sources = ops.image_arena(images, dev)
            quads = [line_quads(angle, length, height, 10 + b) for b in range(B)]
            layout = strip_rows(quads, HEIGHT)
            rows = check_strip_rows(layout.rows, sources, HEIGHT, layout.out_bytes)
            assert len(rows) == B * LINES
            d_table = torch.from_numpy(strip_table(rows, HEIGHT)).to(dev)
            one = lambda: ops.quad_strips_u8(arena, d_sources, d_table, HEIGHT, layout.out_bytes, validate=False)
            e, r = eager_and_replayed(one)
            # the route of the parent: per image one warp_pack_u8 into a page of that image's slots, one below the other
            srcs, tables, pages = [], [], []
            for b in range(B):
                mine = rows[rows[:, 0] == b]
                wmax = int(mine[:, 2].max())
                warps = np.zeros((len(mine), 12), np.int64)
                warps[:, 0] = np.arange(len(mine)) * HEIGHT
                warps[:, 2], warps[:, 3], warps[:, 4:] = HEIGHT, mine[:, 3], mine[:, 4:]
                off = int(sources[b, 0])
                srcs.append(arena[off:off + SIDE * SIDE * 3].view(SIDE, SIDE, 3))
                tables.append(torch.from_numpy(warps).to(dev))
                pages.append(torch.zeros((len(mine) * HEIGHT, wmax, 3), dtype=torch.uint8, device=dev))

            def per_image():
                for src, table, page in zip(srcs, tables, pages):
                    ops.warp_pack_u8(src, table, page, validate=False)

            pe, pr = eager_and_replayed(per_image)
            # every strip is the same by both routes
            out = one()
            for b in range(B):
                mine = rows[rows[:, 0] == b]
                for k, (_, offset, slot_w, w, *_rest) in enumerate(mine.tolist()):
                    got = out[offset:offset + HEIGHT * slot_w * 3].view(HEIGHT, slot_w, 3)[:, :w]
                    assert torch.equal(got, pages[b][k * HEIGHT:(k + 1) * HEIGHT, :w]), (name, b, k)
            written = int(layout.out_bytes)
            under = int(sum(3 * np.hypot(*(q[:, 1] - q[:, 0]).T) * np.hypot(*(q[:, 3] - q[:, 0]).T) for q in quads).sum())
            say(f'{name}, {B} x {LINES} lines, log2n {sorted(set(rows[:, 10].tolist()))}, widths {int(rows[:, 3].min())}..'
                f'{int(rows[:, 3].max())} in slots {sorted(set(rows[:, 2].tolist()))}: one launch {e * 1e6:.1f} us eager, '
                f'{r * 1e6:.1f} us replayed; per image (warp_pack_u8 x {B}) {pe * 1e6:.1f} us eager, {pr * 1e6:.1f} us replayed; '
                f'floor {written / 1e6:.2f} MB written + {under / 1e6:.2f} MB under the rectangles = '
                f'{(written + under) / max(r, 1e-9) / 1e9:.1f} GB/s at the replayed time')
    if a.log:
        with open(a.log, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
