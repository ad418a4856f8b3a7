"""bench.py --dump-outputs on the host: the seeded sample is the same on every run, and the files keep the float types and
stay within the byte budget (small arrays whole, large ones sampled)."""
import os

import numpy as np
import torch

import bench


def test_dump_positions_fixed_sorted_distinct():
    a, b = bench.dump_positions(10 ** 6, 1000), bench.dump_positions(10 ** 6, 1000)
    assert np.array_equal(a, b)
    assert len(np.unique(a)) == 1000 and (np.diff(a) > 0).all() and a[-1] < 10 ** 6
    assert bench.dump_positions(10, 10) is None


def test_write_dump_types_and_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 1 << 20)
    big = torch.arange(1 << 20, dtype=torch.float32)
    bench.write_dump(str(tmp_path), [('loss', torch.tensor(1.5, dtype=torch.float64)),
                                     ('feat', torch.ones(2, 3, dtype=torch.bfloat16)),
                                     ('mask', torch.tensor([0, 1], dtype=torch.uint8)), ('big', big)])
    files = {f[:-4]: np.load(os.path.join(str(tmp_path), f)) for f in os.listdir(str(tmp_path))}
    assert sorted(files) == ['big', 'feat', 'loss', 'mask']
    assert files['loss'].dtype == np.float64 and files['loss'].shape == () and float(files['loss']) == 1.5
    assert files['feat'].dtype == np.float32 and files['feat'].shape == (2, 3)
    assert files['mask'].dtype == np.float32 and files['mask'].tolist() == [0.0, 1.0]
    s = files['big']
    assert s.dtype == np.float32 and 0 < s.size < big.numel()
    assert np.array_equal(s, big.numpy()[bench.dump_positions(big.numel(), s.size)])
    assert sum(os.path.getsize(os.path.join(str(tmp_path), f)) for f in os.listdir(str(tmp_path))) <= 1 << 20
