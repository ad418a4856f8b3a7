"""bench.py end to end at a small size, each run in a fresh child process: a plain run prints the headline line without the
side measurements, ``--full`` adds them (config 3: ``cpu_baseline`` and ``config.per_pass``; config 2: ``cpu_baseline`` and
the ``roofline`` of the eager kernel-timing pass)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', *args], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-4000:]
    out = json.loads(lines[0])
    assert all(k in out for k in HEADLINE) and out['value'] > 0 and out['ms_per_step'] > 0
    return out


SMALL_TRAIN = ('--size', '256', '--batch', '2', '--steps', '2', '--warmup', '1')


def test_plain_train_step_line_without_side_measurements():
    out = _bench(*SMALL_TRAIN)
    assert out['config']['full'] is False
    assert 'cpu_baseline' not in out and out['config']['per_pass'] is None
    assert out['roofline']['kernel'] != 'none'  # from the launch timer of the timed steps, no run of its own


def test_full_train_step_line_with_side_measurements():
    out = _bench(*SMALL_TRAIN, '--full')
    assert out['config']['full'] is True
    assert out['cpu_baseline']['value'] > 0
    pp = out['config']['per_pass']
    for k in ('rough_only_ms', 'precise_only_ms', 'two_pass_ms_per_step', 'dense_point_backward_ms_per_step',
              'label_point_forward_ms_per_step'):
        assert pp[k] > 0, k


def test_forward_config_plain_and_full():
    plain = _bench('--config', '2', '--steps', '1', '--warmup', '0')
    assert 'cpu_baseline' not in plain and plain['roofline'] is None and plain['config']['eager_ms_per_step'] is None
    full = _bench('--config', '2', '--steps', '1', '--warmup', '0', '--full')
    assert full['cpu_baseline']['value'] > 0 and full['config']['eager_ms_per_step'] > 0
    assert full['roofline']['kernel'] != 'none'
