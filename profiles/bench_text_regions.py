"""Text regions of the rough maps at a 360 x 640 map (a 720 x 1280 page, rough head at factor 2): the device step
(ops.text_regions, csrc/regions.hip), eager and replayed from a captured graph, against the host route a user had before
it: copy the mask and the height map to the host, then label and take the per-region medians there (scipy ``label`` +
np.median per region where scipy is installed; the package's own ``text_regions_host`` as well).  Device times are HIP-event
times after warm-up; host times are wall times.  The synthetic pages hold text-line-like blobs: rows of rounded boxes.

    python profiles/bench_text_regions.py [--iters N] [--log PATH]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vkit_ocr_model_adaptive_scaling_amd import ops  # noqa: E402
from vkit_ocr_model_adaptive_scaling_amd.inferencing import text_regions_host  # noqa: E402

CAP = 4096


def synthetic_page(H, W, line_pitch, seed):
    """Text lines every ``line_pitch`` rows, each a run of words of random length with ragged edges; heights near 60 % of
    the pitch with noise, 20 % of the pixels without a valid height."""
    g = np.random.default_rng(seed)
    mask = np.zeros((H, W), np.uint8)
    th = max(2, int(line_pitch * 0.6))
    for y0 in range(line_pitch // 2, H - th, line_pitch):
        x = int(g.integers(4, 24))
        while x < W - 8:
            w = int(g.integers(12, 90))
            mask[y0:y0 + th, x:min(W - 4, x + w)] = 1
            x += w + int(g.integers(3, 14))
    mask &= (g.random((H, W)) > 0.03).astype(np.uint8)  # pinholes and ragged edges
    height = (th + g.standard_normal((H, W)) * 1.5).astype(np.float32)
    height[height < 3.0] = 0
    height[g.random((H, W)) < 0.2] = 0
    height[mask == 0] = 0
    return mask, height


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--log', default=None, help='also append the lines to this file')
    a = ap.parse_args()
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    dev = torch.device('cuda', 0)
    H, W = 360, 640
    say(f'maps {H} x {W} (page 720 x 1280, rough head factor 2), table of {CAP} rows, {a.iters} timed calls per figure')
    cases = [('text lines, pitch 12', synthetic_page(H, W, 12, 1)), ('text lines, pitch 24', synthetic_page(H, W, 24, 2)),
             ('random, density 0.5', ((np.random.default_rng(3).random((H, W)) < 0.5).astype(np.uint8),
                                      np.random.default_rng(4).uniform(3, 60, (H, W)).astype(np.float32))),
             ('full mask (one region)', (np.ones((H, W), np.uint8),
                                         np.random.default_rng(5).uniform(3, 60, (H, W)).astype(np.float32)))]
    for name, (mask, height) in cases:
        d_mask, d_height = torch.from_numpy(mask[None]).to(dev), torch.from_numpy(height[None]).to(dev)
        for _ in range(3):
            out = ops.text_regions(d_mask, d_height, CAP)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            out = ops.text_regions(d_mask, d_height, CAP)
        e.record()
        torch.cuda.synchronize()
        eager_us = s.elapsed_time(e) / a.iters * 1e3
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            g_out = ops.text_regions(d_mask, d_height, CAP)
        graph.replay()
        torch.cuda.synchronize()
        s.record()
        for _ in range(a.iters):
            graph.replay()
        e.record()
        torch.cuda.synchronize()
        replay_us = s.elapsed_time(e) / a.iters * 1e3
        for u, v in zip(out, g_out):
            assert torch.equal(u, v)
        t0 = time.perf_counter()
        n = int(g_out[0][0].item())
        rows = [t[0, :min(n, CAP)].cpu() for t in g_out[2:]]
        rows_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        labels = g_out[1][0].cpu().numpy()
        labels_ms = (time.perf_counter() - t0) * 1e3
        # the host route: both maps to the host, then labelling and medians there
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h_mask, h_height = d_mask[0].cpu().numpy(), d_height[0].cpu().numpy()
        d2h_ms = (time.perf_counter() - t0) * 1e3
        line = (f'{name}: {n} regions; device text_regions {eager_us:.1f} us eager, {replay_us:.1f} us replayed; count + '
                f'{min(n, CAP)} rows to host {rows_ms:.2f} ms, label map {labels_ms:.2f} ms; host route: maps D2H {d2h_ms:.2f} ms')
        if ndimage is not None:
            t0 = time.perf_counter()
            ref, k = ndimage.label(h_mask, structure=np.ones((3, 3)))
            label_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            sel = (ref > 0) & (h_height > 0)
            of, hs = ref[sel], h_height[sel]
            order = np.argsort(of, kind='stable')
            of, hs = of[order], hs[order]
            bounds = np.searchsorted(of, np.arange(1, k + 2))
            med = np.array([np.median(hs[bounds[r]:bounds[r + 1]]) if bounds[r + 1] > bounds[r] else 0 for r in range(k)],
                           np.float32)
            slices = ndimage.find_objects(ref)
            median_ms = (time.perf_counter() - t0) * 1e3
            assert k == n and len(slices) == n and (ref > 0).sum() == (labels > 0).sum()
            assert n > CAP or np.array_equal(np.sort(med), np.sort(rows[3].numpy()))
            line += (f', scipy label {label_ms:.1f} ms, boxes + np.median per region {median_ms:.1f} ms, total '
                     f'{d2h_ms + label_ms + median_ms:.1f} ms')
        else:
            line += ', scipy: not installed here'
        t0 = time.perf_counter()
        host = text_regions_host(h_mask, h_height)
        own_ms = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(host[0], labels) and host[4][:CAP].tobytes() == rows[3].numpy().tobytes()
        line += f'; text_regions_host (the plain oracle) {own_ms:.0f} ms'
        say(line)
        del out, g_out, graph
    if a.log:
        with open(a.log, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
