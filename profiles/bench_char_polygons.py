"""Character quadrilaterals from the precise maps at config #5's precise map size (page 2048 x 1536, precise head at
factor 2: 1024 x 768 maps), B = 1 and B = 8, two peak densities: the device step (ops.char_polygons, csrc/charpoly.hip)
against the reference's host path (inferencing/adaptive_scaling.py:399-465,481-491: download the four maps, scipy
maximum_filter + threshold, one precise_build_polygon per peak in a Python loop), and the PCIe bytes the device step
avoids.  Device times are HIP-event times after warm-up; host times are wall times.

    python profiles/bench_char_polygons.py [--iters N] [--loop-points N]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vkit_ocr_model_adaptive_scaling_amd import ops  # noqa: E402

THR, SIZE, FDF = 0.7, 5, 2.0


def synthetic_maps(B, H, W, pitch, seed):
    """One bump per pitch x pitch cell (a character every ``pitch`` map pixels) on a noisy background below the threshold."""
    g = np.random.default_rng(seed)
    y = np.arange(H, dtype=np.float32)[:, None]
    x = np.arange(W, dtype=np.float32)[None, :]
    bump = (0.5 + 0.5 * np.cos(2 * np.pi * y / pitch)) * (0.5 + 0.5 * np.cos(2 * np.pi * x / pitch))
    prob = np.clip(0.95 * bump[None] + 0.02 * g.standard_normal((B, H, W)), 0, 1).astype(np.float32)
    offset = (g.standard_normal((B, H, W, 2)) * 6).astype(np.float32)
    logits = g.standard_normal((B, H, W, 4)).astype(np.float32)
    angle = (np.exp(logits) / np.exp(logits).sum(-1, keepdims=True)).astype(np.float32)
    dist = (g.random((B, H, W, 4)) * 12).astype(np.float32)
    return prob, offset, angle, dist


def build_polygon(offset, angle, dist, y, x):
    """precise_build_polygon (:399-465) for one point, numpy scalar arithmetic as the reference does it."""
    py, px = y * FDF, x * FDF
    oy, ox = offset[y][x]
    up_left = (py + oy, px + ox)
    a = angle[y][x]
    _, d1, d2, d3 = dist[y][x]
    two_pi = 2 * np.pi
    theta = np.arctan2(oy, ox) % two_pi
    theta = (theta + a[0] * two_pi) % two_pi
    up_right = (py + np.sin(theta) * d1, px + np.cos(theta) * d1)
    theta = (theta + a[1] * two_pi) % two_pi
    down_right = (py + np.sin(theta) * d2, px + np.cos(theta) * d2)
    theta = (theta + a[2] * two_pi) % two_pi
    down_left = (py + np.sin(theta) * d3, px + np.cos(theta) * d3)
    return [up_left, up_right, down_right, down_left]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--loop-points', type=int, default=3000, help='per-point loop: points timed per case (then scaled)')
    a = ap.parse_args()
    try:
        from scipy.ndimage import maximum_filter
        have_scipy = True
    except ImportError:
        maximum_filter, have_scipy = None, False
    dev = torch.device('cuda', 0)
    H, W = 1024, 768
    print(f'maps {H} x {W} (page 2048 x 1536, precise head factor 2), thr {THR}, maximum filter size {SIZE}', flush=True)
    for B in (1, 8):
        for pitch in (16, 32):
            maps = synthetic_maps(B, H, W, pitch, seed=B * 100 + pitch)
            d = [torch.from_numpy(m).to(dev) for m in maps]
            for _ in range(3):
                out = ops.char_polygons(*d, THR, SIZE, FDF, FDF)
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.iters):
                out = ops.char_polygons(*d, THR, SIZE, FDF, FDF)
            e.record()
            torch.cuda.synchronize()
            dev_ms = s.elapsed_time(e) / a.iters
            t0 = time.perf_counter()
            count, points, probs, quads = out
            n = int(count.item())
            rows = [t[:n].cpu() for t in (points, probs, quads)]
            fetch_ms = (time.perf_counter() - t0) * 1e3
            # the reference's path: all four maps to the host, then scipy and the per-point loop
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = [t.cpu().numpy() for t in d]
            d2h_ms = (time.perf_counter() - t0) * 1e3
            map_bytes = sum(h.nbytes for h in host)
            row_bytes = 4 + sum(r.numel() * r.element_size() for r in rows)
            line = (f'B={B} pitch={pitch}: {n} peaks ({n / B:.0f} per page); device char_polygons {dev_ms * 1e3:.1f} us '
                    f'per call (HIP events, {a.iters} calls); count + rows to host {fetch_ms:.2f} ms; '
                    f'D2H {row_bytes / 2**20:.2f} MiB instead of {map_bytes / 2**20:.1f} MiB of maps '
                    f'({(map_bytes - row_bytes) / 2**20:.1f} MiB avoided; maps D2H took {d2h_ms:.1f} ms)')
            if have_scipy:
                t0 = time.perf_counter()
                peaks = []
                for b in range(B):
                    mat = host[0][b]
                    mask = maximum_filter(mat, size=SIZE) == mat
                    mask[mat < THR] = 0
                    peaks.append(np.nonzero(mask))
                filt_ms = (time.perf_counter() - t0) * 1e3
                n_host = sum(len(p[0]) for p in peaks)
                todo = [(b, y, x) for b, (ys, xs) in enumerate(peaks) for y, x in zip(ys, xs)][:a.loop_points]
                t0 = time.perf_counter()
                for b, y, x in todo:
                    build_polygon(host[1][b], host[2][b], host[3][b], y, x)
                loop_ms = (time.perf_counter() - t0) * 1e3 * (n_host / max(1, len(todo)))
                line += (f'; host: maximum_filter + threshold {filt_ms:.1f} ms, per-point loop {loop_ms:.1f} ms '
                         f'({n_host} peaks, {len(todo)} timed), host path total {d2h_ms + filt_ms + loop_ms:.1f} ms')
                assert n_host == n, (n_host, n)
            else:
                line += '; host path: not measured (scipy is not installed here)'
            print(line, flush=True)
            del out, d, rows
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
