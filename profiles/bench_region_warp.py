"""Oriented text regions at the reference's page size: a 2048 x 1536 source and a synthetic table of a few hundred slanted
text-line-like regions that fill one stacked page.  Figures:

* the orientation kernels (ops.region_moments / ops.region_extents, csrc/orient.hip) on a label map of the rough pass's size
  for such a page, eager and replayed;
* the device warp (ops.warp_pack_u8, csrc/respack.hip) after the zero-fill of ops.resample_pack_u8, eager and replayed, at
  one, 2 x 2 and 4 x 4 sub-samples, with page pixels per second;
* the same regions by their axis-aligned boxes (ops.resample_pack_u8): the page area and the time the oriented path saves
  or costs.

Device times are HIP-event times after warm-up.  No figure of this script is quoted anywhere until a log of it exists.

    python profiles/bench_region_warp.py [--iters N] [--log PATH]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from profiles.bench_region_pack import event_time  # noqa: E402
from vkit_ocr_model_adaptive_scaling_amd import ops  # noqa: E402
from vkit_ocr_model_adaptive_scaling_amd.inferencing import stack_regions  # noqa: E402

H, W = 1536, 2048


def slanted_lines(seed, log2n):
    """Words of slanted text lines: centre, length, height and angle (up to 30 degrees either way) of each; the oriented
    destination (35 px high) and the destination of its axis-aligned box at the same scale."""
    g = np.random.default_rng(seed)
    rows = []
    for _ in range(300):
        length, hgt = float(g.uniform(60, 400)), float(g.uniform(12, 80)) * (1 << log2n) / 2
        t = math.radians(float(g.uniform(-30, 30)))
        rows.append((float(g.uniform(100, H - 100)), float(g.uniform(250, W - 250)), length, hgt, t))
    rows = np.array(rows)
    scale = 35.0 / rows[:, 3]
    cos, sin = np.cos(rows[:, 4]), np.abs(np.sin(rows[:, 4]))
    oriented = np.stack([np.round(rows[:, 3] * scale), np.round(rows[:, 2] * scale)], axis=1).astype(np.int64)
    boxed = np.stack([np.round((rows[:, 3] * cos + rows[:, 2] * sin) * scale),
                      np.round((rows[:, 2] * cos + rows[:, 3] * sin) * scale)], axis=1).astype(np.int64)
    return rows, scale, oriented, boxed


def warp_table(rows, scale, boxes, log2n):
    out = np.zeros((len(rows), 12), np.int64)
    for k, ((yc, xc, length, hgt, t), s, (dy, dx, dh, dw)) in enumerate(zip(rows.tolist(), scale.tolist(), boxes.tolist())):
        myy, myx = round(65536 * math.cos(t) * hgt / dh), round(65536 * math.sin(t) * length / dw)
        mxy, mxx = round(-65536 * math.sin(t) * hgt / dh), round(65536 * math.cos(t) * length / dw)
        ay = round(65536 * yc - ((dh - 1) * myy + (dw - 1) * myx) / 2)
        ax = round(65536 * xc - ((dh - 1) * mxy + (dw - 1) * mxx) / 2)
        out[k] = (dy, dx, dh, dw, ay, ax, myy, myx, mxy, mxx, log2n, 0)
    return out


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
    image = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    d_src = torch.from_numpy(image).to(dev)

    # a rough label map of a 720-rule page at 1/2 resolution: a few hundred regions of some thousand pixels each
    lab = np.repeat(np.repeat(g.integers(0, 400, (12, 20)), 30, axis=0), 24, axis=1).astype(np.int32)
    d_lab = torch.from_numpy(lab[None]).to(dev)
    R = 4096
    theta = g.uniform(-np.pi / 4, np.pi / 4, R)
    d_dirs = torch.from_numpy(np.stack([np.round(np.cos(theta) * 16384), np.round(np.sin(theta) * 16384)], axis=1)
                              .astype(np.int32)[None]).to(dev)
    e, r = eager_and_replayed(lambda: ops.region_moments(d_lab, R))
    say(f'region_moments on a {lab.shape[0]} x {lab.shape[1]} label map, {R} rows: {e * 1e6:.1f} us eager, {r * 1e6:.1f} us replayed')
    e, r = eager_and_replayed(lambda: ops.region_extents(d_lab, d_dirs, validate=False))
    say(f'region_extents, same map: {e * 1e6:.1f} us eager, {r * 1e6:.1f} us replayed')

    empty = torch.zeros((0, 8), dtype=torch.int32, device=dev)
    for log2n in (0, 1, 2):
        rows, scale, oriented, boxed = slanted_lines(2, log2n)
        page_o, boxes_o, packed_o, _ = stack_regions(oriented, 10, 2, 2048, 256)
        page_b, boxes_b, packed_b, _ = stack_regions(boxed, 10, 2, 2048, 256)
        table = warp_table(rows[packed_o], scale[packed_o], boxes_o[packed_o], log2n)
        d_table = torch.from_numpy(table).to(dev)
        d_page = torch.empty(page_o + (3,), dtype=torch.uint8, device=dev)
        pixels = int((table[:, 2] * table[:, 3]).sum())

        def warp():
            ops.resample_pack_u8(d_src, empty, page_o, validate=False, out=d_page)
            ops.warp_pack_u8(d_src, d_table, d_page, validate=False)

        e, r = eager_and_replayed(warp)
        e0, r0 = eager_and_replayed(lambda: ops.resample_pack_u8(d_src, empty, page_o, validate=False, out=d_page))
        say(f'{1 << log2n} x {1 << log2n} sub-samples (scales {scale.min():.2f} .. {scale.max():.2f}): {len(table)} warps, '
            f'{pixels / 1e6:.2f} Mpx on a {page_o[0]} x {page_o[1]} page: zero-fill + warp {e * 1e6:.1f} us eager, {r * 1e6:.1f} us '
            f'replayed (zero-fill alone {r0 * 1e6:.1f} us) = {pixels / max(r - r0, 1e-9) / 1e9:.2f} Gpx/s')
        # the same regions by their boxes: the source rectangle of a box, clipped to the image
        half_h = (rows[:, 3] * np.cos(rows[:, 4]) + rows[:, 2] * np.abs(np.sin(rows[:, 4]))) / 2
        half_w = (rows[:, 2] * np.cos(rows[:, 4]) + rows[:, 3] * np.abs(np.sin(rows[:, 4]))) / 2
        sy, sx = np.clip(rows[:, 0] - half_h, 0, H - 2).astype(np.int64), np.clip(rows[:, 1] - half_w, 0, W - 2).astype(np.int64)
        sh = np.minimum(np.maximum(2 * half_h, 1).astype(np.int64), H - sy)
        sw = np.minimum(np.maximum(2 * half_w, 1).astype(np.int64), W - sx)
        placements = np.concatenate([np.stack([sy, sx, sh, sw], axis=1)[packed_b], boxes_b[packed_b]], axis=1).astype(np.int32)
        d_pl = torch.from_numpy(placements).to(dev)
        d_page_b = torch.empty(page_b + (3,), dtype=torch.uint8, device=dev)
        eb, rb = eager_and_replayed(lambda: ops.resample_pack_u8(d_src, d_pl, page_b, validate=False, out=d_page_b))
        say(f'    by their boxes: {len(placements)} placements on a {page_b[0]} x {page_b[1]} page '
            f'({page_b[0] * page_b[1] / (page_o[0] * page_o[1]):.2f} x the oriented page): {eb * 1e6:.1f} us eager, {rb * 1e6:.1f} us '
            f'replayed')
    if a.log:
        with open(a.log, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
