#!/usr/bin/env python3
"""Time the pooled branches of the pyramid-pooling block alone (PpmBlock.branches_cat: everything in front of the final 3x3
block), forward without grad and forward + backward, on the fused kernels (csrc/ppm.hip) against the unfused ops
(VKAS_PPM_UNFUSED=1) in ONE process: three rounds in alternation, HIP-event times, microseconds per call.

Shapes: the train step's block (B = 8, 32 x 32, C = 768, Cb = 96, bf16) and config 5's largest page (B = 1, 64 x 48,
ConvNeXt-Base widths C = 1024, Cb = 128, fp16).  Log: profiles/ppm_fused.log."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from vkit_ocr_model_adaptive_scaling_amd.model.upernext import PpmBlock  # noqa: E402
from vkit_ocr_model_adaptive_scaling_amd.training import FlatBuffers  # noqa: E402

SHAPES = [('train B=8 32x32 C=768 Cb=96 bf16', 8, 32, 32, 768, 96, torch.bfloat16),
          ('config5 B=1 64x48 C=1024 Cb=128 fp16', 1, 64, 48, 1024, 128, torch.float16)]
ROUNDS, ITERS = 3, 20


def timed(fn):
    fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(ITERS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / ITERS * 1e3


def main():
    dev = torch.device('cuda:0')
    g = torch.Generator(device='cuda').manual_seed(0)
    for name, B, H, W, C, Cb, dtype in SHAPES:
        blk = PpmBlock((1, 2, 3, 6), C, Cb).to(dev)
        FlatBuffers(blk.named_parameters())  # the training harness' flat gradient views: parameter gradients are added in place
        x = torch.randn((B, H, W, C), generator=g, device=dev).to(dtype)
        dcat = torch.randn((B, H, W, C + 4 * Cb), generator=g, device=dev).to(dtype)

        def fwd():
            with torch.no_grad():
                blk.branches_cat(x)

        def fwd_bwd():
            xin = x.detach().requires_grad_(True)
            blk.branches_cat(xin).backward(dcat)

        for what, fn in (('forward (no grad)', fwd), ('forward + backward', fwd_bwd)):
            rows = {'fused': [], 'unfused': []}
            for _ in range(ROUNDS):
                for route in ('unfused', 'fused'):
                    if route == 'unfused':
                        os.environ['VKAS_PPM_UNFUSED'] = '1'
                    else:
                        os.environ.pop('VKAS_PPM_UNFUSED', None)
                    rows[route].append(timed(fn))
            os.environ.pop('VKAS_PPM_UNFUSED', None)
            fmt = lambda v: ' / '.join('%7.1f' % t for t in v)
            print(f'{name:38s} {what:18s} unfused {fmt(rows["unfused"])} us   fused {fmt(rows["fused"])} us   '
                  f'x{min(rows["unfused"]) / max(rows["fused"]):.2f}', flush=True)


if __name__ == '__main__':
    main()
