"""FpnHead 5x5 smoothing at factor 4, forward + backward of the packed convolution of two rough heads (B = 8, neck 256 x 256 x
384, 2 x 192 output channels): the folded kernels (ops.UpConv5) against the materialised composite (ops.Resize nearest x4 +
ops.Conv 5x5).  Run under rocprofv3 --kernel-trace --stats for per-kernel times; prints wall times from HIP events.

    python profiles/bench_upconv5.py [--iters N] [--only folded|composite]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vkit_ocr_model_adaptive_scaling_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--only', choices=['folded', 'composite'], default=None)
    a = ap.parse_args()
    B, H, W, C, N, f = 8, 256, 256, 384, 384, 4
    dev = torch.device('cuda', 0)
    g = torch.Generator(device='cpu').manual_seed(0)
    x = torch.randn(B, H, W, C, generator=g).to(dev, torch.bfloat16).requires_grad_(True)
    w = (0.02 * torch.randn(N, C, 5, 5, generator=g)).to(dev).requires_grad_(True)
    b = torch.zeros(N, device=dev, requires_grad=True)
    dy = torch.randn(B, f * H, f * W, N, device=dev, dtype=torch.bfloat16)
    variants = {'folded': lambda: ops.UpConv5.apply(x, w, b, f),
                'composite': lambda: ops.Conv.apply(ops.Resize.apply(x, (f * H, f * W), 1), w, b, 1, 2)}
    for name, fn in variants.items():
        if a.only and name != a.only:
            continue
        for it in range(a.iters + 1):
            x.grad = w.grad = b.grad = None
            s, m, e = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            s.record()
            y = fn()
            m.record()
            y.backward(dy)
            e.record()
            torch.cuda.synchronize()
            del y
            if it:
                print(f'{name}: forward {s.elapsed_time(m):.2f} ms, backward {m.elapsed_time(e):.2f} ms, '
                      f'peak {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB', flush=True)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()


if __name__ == '__main__':
    main()
