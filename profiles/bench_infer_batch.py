"""``infer_batch`` against a loop of ``infer`` over the same images (the baseline: what a user with a folder of images had),
with a randomly initialised Tiny model, on three workloads: 8 and 32 synthetic 720 x 1280 images with text-line-like bars,
and 8 images of 360 x 640.  Per workload:

* images per second of both routes, the first (eager) call of ``infer_batch`` and its replayed calls;
* the pages and page rows each route puts through the precise pass: a loop pads every image's page up to the next
  ``precise_page_height_step``, the batch fills shared pages of ``precise_page_height_max`` rows;
* the two multi pack kernels alone (ops.resample_pack_u8_multi / ops.pack_region_labels_multi on the batch's own tables),
  with their achieved bytes per second - page and label bytes written plus source bytes read (the source rectangles'
  bytes, each counted once) - beside the achievable HBM rate.

Device times are HIP-event times after warm-up; end-to-end times are wall times around a synchronise.  Every workload runs
in a child process of its own under a time limit, and a workload that fails ends the run: nothing more is started.

    python profiles/bench_infer_batch.py [--iters N] [--log [PATH]] [--limit SECONDS]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE = 6.3e12  # bytes per second: what a streaming kernel reaches on this part
WORKLOADS = {'8x720x1280': (8, 720, 1280), '32x720x1280': (32, 720, 1280), '8x360x640': (8, 360, 640)}
DEFAULT_LOG = os.path.join(ROOT, 'profiles', 'infer_batch.log')


def synthetic_image(seed, H, W):
    """Light noise with dark text-line-like bars: lines of random pitch cut into words."""
    import numpy as np
    g = np.random.default_rng(seed)
    img = g.integers(160, 256, (H, W, 3), dtype=np.uint8)
    y = int(g.integers(8, 40))
    while y < H - 60:
        hgt = int(g.integers(10, 48))
        x = int(g.integers(4, 60))
        while x < W - 40:
            w = min(int(g.integers(30, 300)), W - 4 - x)
            img[y:y + hgt, x:x + w] //= 6
            x += w + int(g.integers(8, 40))
        y += hgt + int(g.integers(6, 40))
    return img


def wall_time(fn, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


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


def run_workload(name, iters, say):
    import numpy as np
    import torch
    from vkit_ocr_model_adaptive_scaling_amd import ops
    from vkit_ocr_model_adaptive_scaling_amd.inferencing import AdaptiveScalingInferencing, AdaptiveScalingInferencingConfig
    from vkit_ocr_model_adaptive_scaling_amd.model import (AdaptiveScaling, AdaptiveScalingConfig, AdaptiveScalingSize,
                                                           AdaptiveScalingNeckHeadType)
    n, H, W = WORKLOADS[name]
    images = [synthetic_image(100 + k, H, W) for k in range(n)]
    torch.manual_seed(0)
    model = AdaptiveScaling(AdaptiveScalingConfig(AdaptiveScalingSize.TINY, AdaptiveScalingNeckHeadType.UPERNEXT))
    # as profiles/bench_region_pack.py: regions come from whatever the random model's rough maps hold
    inf = AdaptiveScalingInferencing(AdaptiveScalingInferencingConfig(
        model_jit=model, rough_valid_char_height_min=0.0, precise_flattened_text_region_resized_char_height_median=2,
        precise_build_polygons_positive_char_prob_thr=0.5))
    c = inf.config
    loop = lambda: [inf.infer(img) for img in images]
    t_loop_first = wall_time(loop, 1)
    singles = loop()  # the second call of every signature captures its graph
    t0 = time.perf_counter()
    batch = inf.infer_batch(images)
    torch.cuda.synchronize()
    t_batch_first = time.perf_counter() - t0
    inf.infer_batch(images)  # captures
    t_loop = wall_time(loop, iters)
    t_batch = wall_time(lambda: inf.infer_batch(images), iters)
    # alternate once more, so that a drift of the machine shows
    t_loop2 = wall_time(loop, iters)
    t_batch2 = wall_time(lambda: inf.infer_batch(images), iters)
    loop_rows = sum(r.page_shape[0] for r in singles if len(r.placements))
    loop_pages = sum(1 for r in singles if len(r.placements))
    batch_rows = sum(h for h, _ in batch.page_shapes) if len(batch.rows) else 0
    chars = sum(len(p) for r in batch.results for p in r.points)
    say(f'[{name}] {n} images of {H} x {W}: {sum(r.regions.num_regions for r in batch.results)} regions, {len(batch.rows)} '
        f'packed, {chars} characters')
    say(f'[{name}] precise pass: loop of infer {loop_pages} pages, {loop_rows} page rows (widths '
        f'{sorted(set(r.page_shape[1] for r in singles))}); infer_batch {len(batch.page_shapes)} pages {batch.page_shapes}, '
        f'{batch_rows} page rows')
    say(f'[{name}] first calls (eager): loop of infer {n / t_loop_first:.1f} images/s, infer_batch {n / t_batch_first:.1f} images/s')
    say(f'[{name}] replayed, {iters} iterations, twice in alternation: loop of infer {n / t_loop:.1f} and {n / t_loop2:.1f} '
        f'images/s ({t_loop * 1e3:.1f} and {t_loop2 * 1e3:.1f} ms per batch); infer_batch {n / t_batch:.1f} and '
        f'{n / t_batch2:.1f} images/s ({t_batch * 1e3:.1f} and {t_batch2 * 1e3:.1f} ms per batch)')
    if not len(batch.rows):
        return
    # the multi pack kernels alone, on the tables of this batch (all pages taken at the first page's shape)
    mats, arena, sources, d_sources = inf._image_arena(images)
    _, label_arena, label_sources = inf._rough_text_regions_batch(mats, arena, sources, d_sources, False, False, True)
    fdf = 4 // c.precise_head_upsampling_factor
    Q, (Hp, Wp) = len(batch.page_shapes), batch.page_shapes[0]
    d_rows = torch.from_numpy(batch.rows).cuda()
    d_start = torch.from_numpy(np.searchsorted(batch.rows[:, 1], np.arange(Q + 1)).astype(np.int32)).cuda()
    d_label_sources = torch.from_numpy(label_sources).cuda()
    d_pages = torch.empty((Q, Hp, Wp, 3), dtype=torch.uint8, device='cuda')
    d_out = torch.empty((Q, Hp // fdf, Wp // fdf), dtype=torch.int32, device='cuda')
    pack = lambda: ops.resample_pack_u8_multi(arena, d_sources, d_rows, Q, (Hp, Wp), page_start=d_start, validate=False,
                                              out=d_pages)
    labels = lambda: ops.pack_region_labels_multi(label_arena, d_label_sources, d_rows, Q, (Hp // fdf, Wp // fdf), fdf,
                                                  page_start=d_start, validate=False, out=d_out)
    src_bytes = int((batch.rows[:, 4].astype(np.int64) * batch.rows[:, 5]).sum()) * 3
    for what, fn, nbytes in (('resample_pack_u8_multi', pack, d_pages.numel() + src_bytes),
                             ('pack_region_labels_multi', labels, d_out.numel() * 4)):
        eager = event_time(fn, iters)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        replay = event_time(graph.replay, iters)
        rate = nbytes / replay
        say(f'[{name}] {what}: {eager * 1e6:.1f} us eager, {replay * 1e6:.1f} us replayed for {nbytes / 1e6:.2f} MB = '
            f'{rate / 1e12:.3f} TB/s, {100 * rate / HBM_ACHIEVABLE:.1f} % of the achievable HBM rate '
            f'({HBM_ACHIEVABLE / 1e12:.1f} TB/s)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--log', nargs='?', const=DEFAULT_LOG, default=None, help='also append the lines to this file')
    ap.add_argument('--limit', type=int, default=240, help='seconds per workload')
    ap.add_argument('--workload', choices=sorted(WORKLOADS), default=None, help='run this one here (what the parent starts)')
    a = ap.parse_args()
    if a.workload:
        lines = []

        def say(line):
            print(line, flush=True)
            lines.append(line)

        run_workload(a.workload, a.iters, say)
        if a.log:
            with open(a.log, 'a') as f:
                f.write('\n'.join(lines) + '\n')
        return
    for name in WORKLOADS:  # the parent never touches the GPU: a fresh child per workload, each under its own limit
        cmd = ['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--workload', name, '--iters',
               str(a.iters)] + (['--log', a.log] if a.log else [])
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f'[{name}] ended with status {rc}: nothing more is started', flush=True)
            sys.exit(rc)


if __name__ == '__main__':
    main()
