"""bench.py's host side without a GPU: the argument checks and the --dump-outputs writer."""
import os

import numpy as np
import pytest
import torch

import bench


def test_steps_must_be_positive():
    assert bench.parse_args(['--steps', '7', '--warmup', '0']).steps == 7
    with pytest.raises(SystemExit):
        bench.parse_args(['--steps', '0'])
    with pytest.raises(SystemExit):
        bench.parse_args(['--warmup', '-1'])


def test_only_full_makes_the_extra_runs():
    plain = bench.parse_args([])
    assert not plain.full and plain.no_alt and plain.no_cpu_baseline
    full = bench.parse_args(['--full'])
    assert full.full and not full.no_alt and not full.no_cpu_baseline
    assert bench.parse_args(['--full', '--timed-only']).no_alt
    assert bench.parse_args(['--full', '--no-cpu-baseline']).no_cpu_baseline


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample_of_large_ones(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_SAMPLE', 1000)
    big = torch.arange(6000, dtype=torch.float32).reshape(2, 3000)
    arrays = {'big': big, 'counts': [5000, 4321], 'ints': torch.tensor([3, 4]), 'f64': torch.ones(3, dtype=torch.float64)}
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), arrays)
    assert sorted(os.listdir(tmp_path / 'a')) == ['big_sample.npy', 'counts.npy', 'f64.npy', 'ints.npy']
    a = {n[:-4]: np.load(str(tmp_path / 'a' / n)) for n in os.listdir(tmp_path / 'a')}
    b = {n[:-4]: np.load(str(tmp_path / 'b' / n)) for n in os.listdir(tmp_path / 'b')}
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k       # same arguments, same sample
    s = a['big_sample']
    assert s.dtype == np.float32 and s.shape == (1000,) and np.all(np.diff(s) > 0)  # distinct elements, in index order
    assert np.array_equal(s, big.reshape(-1).numpy()[s.astype(np.int64)])
    assert a['counts'].dtype == np.float64 and a['counts'].tolist() == [5000.0, 4321.0]
    assert a['ints'].dtype == np.float64 and a['f64'].dtype == np.float64


def test_dump_outputs_refuses_more_than_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 1024)
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path), {'x': torch.zeros(100), 'y': torch.zeros(200)})
