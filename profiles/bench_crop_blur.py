"""Blurred training crops at the train step's size: B = 8 crops of 1024 x 1024 out of one page of 2048 x 1536, at scales 1 and
1/2 (log2n 0 and 1), turned by 3 degrees, photometric jitter and noise on - the rows of profiles/bench_crops.py.  Per scale,
four blur tables: all radii 0 (on device tables, so that the two launches run), all 2, all 7, and a mix drawn at prob = 0.3.
Per table:

* ops.crop_warp_blur (the blur kernels of csrc/crops.hip), eager and replayed from a captured graph, beside ops.crop_warp on
  the same rows - the sharp crops, the kernel this one is added to - and the difference, the cost of the blur;
* the two bounds of the call beside the time: the bytes it must move - the page bytes under the crops and their halo read
  once, the uint8 planes written and read once, the float32 crops written - over the achievable HBM rate, and its integer
  multiply-adds - 3 B H W (2R + 1)^2 - over the full vector rate;
* the host route (dataset/blur.py::crop_blur_host, plain numpy) for ONE of the eight crops, times eight (not at radius 0).

Device times are HIP-event times after warm-up; host times are wall times.  Every workload runs in a child process of its
own under its own time limit; after a child that fails or runs out of time nothing more is started.

    python profiles/bench_crop_blur.py [--iters N] [--log PATH] [--limit SECONDS] [--no-host]
"""
import argparse
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from profiles.bench_crops import B, HBM_ACHIEVABLE, SIZE, event_time, rows_for  # noqa: E402

PAGE = (2048, 1536)
SCALES = (1.0, 0.5)
VALU_RATE = 256 * 4 * 16 * 2.4e9  # lane operations per second: 256 CUs, 4 SIMDs of 16 lanes, 2.4 GHz - a 24-bit multiply-add each
TABLES = ('radius 0', 'radius 2', 'radius 7', 'mix p=0.3')


def blur_for(name):
    from vkit_ocr_model_adaptive_scaling_amd.dataset import (AnnotatedPage, BlurConfig, CropConfig, blur_row, gaussian_blur_row,
                                                             identity_blur_row)
    if name == 'radius 0':
        return np.stack([identity_blur_row()] * B)
    if name == 'radius 2':
        return np.stack([gaussian_blur_row(0.6)] * B)
    if name == 'radius 7':
        return np.stack([gaussian_blur_row(2.3)] * B)
    cfg = CropConfig(size=SIZE, blur=BlurConfig(prob=0.3))
    page = np.zeros((8, 8, 3), np.uint8)
    return np.stack([blur_row('rough', AnnotatedPage(page, np.zeros((0, 4, 2)), b), cfg, 5) for b in range(B)])


def bounds(blur, scale, radius_max):
    """-> (bytes moved at the least, multiply-adds)"""
    H, W = SIZE
    Hw, pitch = H + 2 * radius_max, -(-(W + 2 * radius_max) // 16) * 16
    planes = B * 3 * Hw * pitch
    page = sum(3 * min((H + 2 * r) / scale, PAGE[0]) * min((W + 2 * r) / scale, PAGE[1]) for r in blur[:, 0].tolist())
    return page + 2 * planes + B * 3 * H * W * 4, sum(3 * H * W * (2 * r + 1) ** 2 for r in blur[:, 0].tolist())


def workload(kind, iters):
    import torch
    from vkit_ocr_model_adaptive_scaling_amd import ops
    from vkit_ocr_model_adaptive_scaling_amd.dataset import crop_blur_host
    dev = torch.device('cuda', 0)
    torch.zeros((1 << 20,), device=dev).cpu()  # the context and both copy directions exist before anything is timed
    torch.cuda.synchronize()
    page = np.random.default_rng(0).integers(0, 256, PAGE + (3,), dtype=np.uint8)
    tag = f'blurred crops {B} x {SIZE[0]} x {SIZE[1]} of a {PAGE[0]} x {PAGE[1]} page'
    if kind == 'device':
        arena, table, d_table = ops.image_arena([page], dev)
        out = torch.empty((B, 3) + SIZE, dtype=torch.float32, device=dev)
        for scale in SCALES:
            rows = rows_for(PAGE, scale)
            d_rows = torch.from_numpy(rows).to(dev)
            ops.crop_warp(arena, table, rows, SIZE)  # the tables, checked once on the host
            sharp = lambda: ops.crop_warp(arena, d_table, d_rows, SIZE, validate=False, out=out)
            for name in TABLES:
                blur = blur_for(name)
                radius_max = int(blur[:, 0].max())
                d_blur = torch.from_numpy(blur).to(dev)
                work = torch.empty((ops.crop_blur_work_bytes(B, SIZE, radius_max),), dtype=torch.uint8, device=dev)
                call = lambda: ops.crop_warp_blur(arena, d_table, d_rows, d_blur, SIZE, validate=False, out=out, work=work,
                                                  radius_max=radius_max)
                times = {}
                for what, fn in (('sharp', sharp), ('blur', call)):  # alternating, so that both see the same machine
                    eager = event_time(fn, iters)
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        fn()
                    times[what] = (eager, event_time(graph.replay, iters))
                nbytes, mads = bounds(blur, scale, radius_max)
                best, base = min(times['blur']), min(times['sharp'])
                t_bytes, t_mads = nbytes / HBM_ACHIEVABLE, mads / VALU_RATE
                print(f'{tag}, scale {scale:g} (log2n {int(rows[0, 7])}), {name} (radii {blur[:, 0].tolist()}): '
                      f'crop_warp_blur {times["blur"][0] * 1e6:.1f} us eager, {times["blur"][1] * 1e6:.1f} us replayed; '
                      f'crop_warp {times["sharp"][0] * 1e6:.1f} us eager, {times["sharp"][1] * 1e6:.1f} us replayed; '
                      f'the blur costs {(best - base) * 1e6:.1f} us; bounds: {nbytes / 1e6:.1f} MB = {t_bytes * 1e6:.1f} us at '
                      f'{HBM_ACHIEVABLE / 1e12:.1f} TB/s, {mads / 1e9:.2f} G multiply-adds = {t_mads * 1e6:.1f} us at '
                      f'{VALU_RATE / 1e12:.1f} T/s: {100 * max(t_bytes, t_mads) / best:.1f} % of the '
                      f'{"multiply-add" if t_mads > t_bytes else "byte"} bound', flush=True)
    else:
        for scale in SCALES:
            rows = rows_for(PAGE, scale)
            for name in TABLES[1:3]:
                blur = blur_for(name)
                t0 = time.perf_counter()
                crop_blur_host([page], rows[:1], blur[:1], SIZE)
                t_host = time.perf_counter() - t0
                print(f'{tag}, scale {scale:g}, {name}: host route {t_host * 1e3:.0f} ms for one crop = {B * t_host * 1e3:.0f} ms '
                      f'for {B}', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--log', default=None, help='also append the lines to this file')
    ap.add_argument('--limit', type=int, default=240, help='seconds per workload')
    ap.add_argument('--no-host', action='store_true', help='skip the host route')
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        workload(a.child, a.iters)
        return
    lines = []
    for kind in ('device',) if a.no_host else ('device', 'host'):
        cmd = [sys.executable, os.path.abspath(__file__), '--iters', str(a.iters), '--child', kind]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f'{kind}: no result within {a.limit} s; stopping', flush=True)
            sys.exit(1)
        print(r.stdout, end='', flush=True)
        if r.returncode != 0:
            print(f'{kind}: exit status {r.returncode}; stopping', flush=True)
            sys.exit(1)
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith('blurred crops ')]
    if a.log:
        with open(a.log, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
