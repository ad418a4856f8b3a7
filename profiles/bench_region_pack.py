"""Cropping, rescaling and packing text regions at the reference's page size: a 2048 x 1536 source and a synthetic table of a
few hundred text-line-like regions that fill one stacked page.  Three figures:

* the device pack (ops.resample_pack_u8, csrc/respack.hip), eager and replayed from a captured graph, with its achieved
  bytes per second - page bytes written plus source bytes read (the source rectangles' bytes, each counted once) - beside the
  achievable HBM rate;
* the host route it replaces: the image from the device, a vectorised CPU resampler per region (torch ``interpolate``, area
  for a shrink and bilinear otherwise - NOT this package's integer rule: it only stands for what a host implementation
  costs), the page to the device;
* ``infer`` end to end against the two calls a user had before it (``rough_infer_text_regions``, the host route above on the
  host image, ``precise_infer_char_polygons`` on the host page), with a randomly initialised Tiny model.

Device times are HIP-event times after warm-up; host times are wall times around a synchronise.

    python profiles/bench_region_pack.py [--iters N] [--log PATH]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vkit_ocr_model_adaptive_scaling_amd import ops  # noqa: E402
from vkit_ocr_model_adaptive_scaling_amd.inferencing import (  # noqa: E402
    AdaptiveScalingInferencing, AdaptiveScalingInferencingConfig, region_crops, stack_regions)

HBM_ACHIEVABLE = 6.3e12  # bytes per second: what a streaming kernel reaches on this part
H, W = 1536, 2048


def synthetic_table(seed, n_lines=24):
    """Text lines of random pitch cut into words: source rectangles on the page, each rescaled so that its height becomes
    35 px (factors from about 0.4 to 3), stacked with the package's own shelf packing."""
    g = np.random.default_rng(seed)
    rows = []
    y = 8
    while y < H - 80:
        hgt = int(g.integers(12, 80))
        x = int(g.integers(4, 40))
        while x < W - 40:
            w = min(int(g.integers(40, 400)), W - 4 - x)
            rows.append((y, x, hgt, w))
            x += w + int(g.integers(6, 30))
        y += hgt + int(g.integers(4, 24))
    src = np.array(rows, np.int64)
    scale = 35.0 / src[:, 2]
    shapes = np.stack([np.round(src[:, 2] * scale), np.round(src[:, 3] * scale)], axis=1).astype(np.int64)
    page, boxes, packed, too_large = stack_regions(shapes, 10, 2, 2048, 256)
    table = np.concatenate([src[packed], boxes[packed]], axis=1).astype(np.int32)
    return table, page, int(too_large.sum())


def host_resample(image, table, page_shape):
    """The vectorised CPU route: torch interpolate per region (area for a shrink on both axes, bilinear otherwise)."""
    page = np.zeros(page_shape + (3,), np.uint8)
    t = torch.from_numpy(image).permute(2, 0, 1)[None].float()
    for sy, sx, sh, sw, dy, dx, dh, dw in table.tolist():
        crop = t[:, :, sy:sy + sh, sx:sx + sw]
        if dh < sh and dw < sw:
            out = torch.nn.functional.interpolate(crop, size=(dh, dw), mode='area')
        else:
            out = torch.nn.functional.interpolate(crop, size=(dh, dw), mode='bilinear', align_corners=False)
        page[dy:dy + dh, dx:dx + dw] = out[0].permute(1, 2, 0).round().clamp(0, 255).byte().numpy()
    return page


def event_time(fn, iters):
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


def wall_time(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--log', default=None, help='also append the lines to this file')
    a = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    dev = torch.device('cuda', 0)
    image = np.random.default_rng(1).integers(0, 256, (H, W, 3), dtype=np.uint8)
    table, page_shape, dropped = synthetic_table(2)
    n = len(table)
    page_bytes = page_shape[0] * page_shape[1] * 3
    src_bytes = int((table[:, 2].astype(np.int64) * table[:, 3]).sum()) * 3
    ratios = table[:, 6] / table[:, 2]
    say(f'source {H} x {W}, {n} regions (ratios {ratios.min():.2f} .. {ratios.max():.2f}, {dropped} too large) on a '
        f'{page_shape[0]} x {page_shape[1]} page: {page_bytes / 1e6:.2f} MB written + {src_bytes / 1e6:.2f} MB read')
    d_src = torch.from_numpy(image).to(dev)
    d_table = torch.from_numpy(table).to(dev)
    d_page = torch.empty(page_shape + (3,), dtype=torch.uint8, device=dev)
    pack = lambda: ops.resample_pack_u8(d_src, d_table, page_shape, validate=False, out=d_page)
    eager = event_time(pack, a.iters)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pack()
    replay = event_time(graph.replay, a.iters)
    rate = (page_bytes + src_bytes) / replay
    say(f'device pack: {eager * 1e6:.1f} us eager, {replay * 1e6:.1f} us replayed = {rate / 1e12:.3f} TB/s of page + source '
        f'bytes, {100 * rate / HBM_ACHIEVABLE:.1f} % of the achievable HBM rate ({HBM_ACHIEVABLE / 1e12:.1f} TB/s)')
    validated = wall_time(lambda: ops.resample_pack_u8(d_src, table, page_shape, out=d_page), 10)
    say(f'device pack from a host table (validation of {n} rows + upload + launch): {validated * 1e3:.2f} ms wall')

    def host_route():
        h_img = d_src.cpu().numpy()
        page = host_resample(h_img, table, page_shape)
        return torch.from_numpy(page).to(dev)

    host = wall_time(host_route, 3)
    d2h = wall_time(lambda: d_src.cpu(), 5)
    say(f'host route: image D2H {d2h * 1e3:.2f} ms, D2H + torch-CPU interpolate per region + H2D {host * 1e3:.1f} ms '
        f'({torch.get_num_threads()} CPU threads) = {host / replay:.0f} x the replayed device pack')

    # ---- end to end, Tiny model with random weights: regions come from whatever its rough maps hold
    from vkit_ocr_model_adaptive_scaling_amd.model import (AdaptiveScaling, AdaptiveScalingConfig, AdaptiveScalingSize,
                                                           AdaptiveScalingNeckHeadType)
    torch.manual_seed(0)
    model = AdaptiveScaling(AdaptiveScalingConfig(AdaptiveScalingSize.TINY, AdaptiveScalingNeckHeadType.UPERNEXT))
    inf = AdaptiveScalingInferencing(AdaptiveScalingInferencingConfig(
        model_jit=model, rough_valid_char_height_min=0.0, precise_flattened_text_region_resized_char_height_median=2,
        precise_build_polygons_positive_char_prob_thr=0.5))
    c = inf.config

    def two_calls():
        r = inf.rough_infer_text_regions(image, resize_fn='device', return_labels=False)
        crops = region_crops(r.boxes, image.shape[:2], r.resized_shape)
        shape, boxes, packed, _ = stack_regions(r.resized_shapes, c.precise_stack_flattened_text_regions_page_pad,
                                                c.precise_stack_flattened_text_regions_pad, c.precise_page_width_max,
                                                c.precise_page_height_step, keep=r.keep)
        tab = np.concatenate([crops[packed], boxes[packed]], axis=1).astype(np.int32)
        return inf.precise_infer_char_polygons(host_resample(image, tab, shape)), len(tab), shape

    res = inf.infer(image)
    _, m, shape = two_calls()
    t_infer = wall_time(lambda: inf.infer(image), 10)
    t_two = wall_time(two_calls, 3)
    say(f'end to end (Tiny, random weights; {res.regions.num_regions} regions, {m} packed on a {shape[0]} x {shape[1]} page): '
        f'infer {t_infer * 1e3:.1f} ms; rough_infer_text_regions + host resample + precise_infer_char_polygons '
        f'{t_two * 1e3:.1f} ms')
    if a.log:
        with open(a.log, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
