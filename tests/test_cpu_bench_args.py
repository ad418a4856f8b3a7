"""bench.py's command line on the host: a plain run leaves the side measurements out, ``--full`` asks for them, and the
options that trim a full run are still accepted."""
import pytest

import bench


def test_plain_run_is_not_full():
    a = bench.parse_args(['--gpus', '1', '--steps', '3', '--warmup', '1'])
    assert (a.gpus, a.steps, a.warmup, a.config) == (1, 3, 1, 3)
    assert a.full is False and a.dump_outputs is None


def test_full_and_its_trims():
    a = bench.parse_args(['--full', '--no-cpu-baseline', '--no-per-pass', '--config', '2'])
    assert a.full and a.no_cpu_baseline and a.no_per_pass and a.config == 2


def test_steps_and_warmup_bounds():
    with pytest.raises(SystemExit):
        bench.parse_args(['--steps', '0'])
    with pytest.raises(SystemExit):
        bench.parse_args(['--warmup', '-1'])
