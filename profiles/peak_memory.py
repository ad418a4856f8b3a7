#!/usr/bin/env python3
"""Peak device memory of the headline train step: runs bench.py's default configuration in this process (2 warm-up + 3 timed
steps unless other bench.py arguments are given) and prints torch.cuda.max_memory_allocated() / max_memory_reserved() behind
the bench line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402

if __name__ == '__main__':
    sys.argv = [os.path.join(ROOT, 'bench.py')] + (sys.argv[1:] or ['--gpus', '1', '--steps', '3', '--warmup', '2'])
    bench.main()
    torch.cuda.synchronize()
    print(json.dumps({'max_memory_allocated_MiB': round(torch.cuda.max_memory_allocated() / 2**20, 1),
                      'max_memory_reserved_MiB': round(torch.cuda.max_memory_reserved() / 2**20, 1)}))
