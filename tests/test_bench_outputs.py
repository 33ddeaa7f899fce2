"""bench.py's plain run and `--dump-outputs DIR`: the timed steps only, and what one more step from the seeded starting state handed
its caller, written as DIR/<name>.npy (float32 / float64, at most 64 MB in all: a fixed sample of each array past that)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench                                                            # noqa: E402


def test_write_outputs_keeps_float_types_and_samples_past_the_limit(tmp_path):
    g = torch.Generator().manual_seed(1)
    arrays = {'big': torch.rand(4000, 3, generator=g), 'half': torch.rand(100, generator=g).half(), 'f64': torch.rand(10, generator=g).double(),
              'scalar': torch.tensor(0.25)}
    bench.write_outputs(str(tmp_path / 'all'), arrays)
    for k, v in arrays.items():
        a = np.load(tmp_path / 'all' / f'{k}.npy')
        assert a.dtype == (np.float64 if k == 'f64' else np.float32) and a.shape == tuple(v.shape)
        assert np.array_equal(a, v.double().numpy() if k == 'f64' else v.float().numpy())
    limit = 20000
    for run in ('a', 'b'):
        bench.write_outputs(str(tmp_path / run), arrays, limit=limit)
        assert sum(os.path.getsize(tmp_path / run / f) for f in os.listdir(tmp_path / run)) <= limit
    for k in arrays:
        a, b = np.load(tmp_path / 'a' / f'{k}.npy'), np.load(tmp_path / 'b' / f'{k}.npy')
        assert np.array_equal(a, b)                                     # the same sample every time
    big = np.load(tmp_path / 'a' / 'big.npy')
    assert 0 < big.size < arrays['big'].numel() and np.isin(big, arrays['big'].numpy()).all()


def _plain_run(out, steps):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '2', '--views', '3', '--H', '96',
           '--W', '128', '--txt', '64', '--dump-outputs', str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_only_the_steps_and_dumps_a_reproducible_step(tmp_path):
    """Two processes, different numbers of timed steps: the dumped step starts from the same seeded state in both, so its outputs agree to
    rounding (unordered fp32 atomic sums; the state after the timed steps does not: chained steps grow those differences)."""
    d = _plain_run(tmp_path / 'a', 4)
    assert d['steps'] == 4 and d['warmup'] == 2 and d['ms_per_step'] > 0 and d['unit'] == 'views/s' and d['higher_is_better'] is True
    assert abs(d['value'] - 3 / (d['ms_per_step'] * 1e-3)) < 1e-6 * d['value']
    assert d['roofline'] is None and d['phases'] is None and 'cpu_baseline' not in d and 'batch4' not in d and d['sync_timeouts'] == 0
    assert _plain_run(tmp_path / 'b', 7)['steps'] == 7
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == sorted(os.listdir(tmp_path / 'b'))
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in files) <= bench.DUMP_LIMIT_BYTES
    a = {f[:-4]: np.load(tmp_path / 'a' / f) for f in files}
    b = {f[:-4]: np.load(tmp_path / 'b' / f) for f in files}
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
    assert a['param_textures'].shape == (10, 64, 64, 3) and a['grad_textures'].shape == (10, 64, 64, 3)
    assert np.abs(a['grad_textures']).max() > 0 and float(a['loss_total']) > 0
    # the first step from the seeded state: Adam's moments are (1 - beta1) g and (1 - beta2) g^2 of the dumped gradient (betas 0.9, 0.999)
    for name in ('textures', 'S', 'T'):
        g = a[f'grad_{name}'].astype(np.float64)
        assert np.abs(a[f'exp_avg_{name}'] - 0.1 * g).max() <= 1e-5 * np.abs(0.1 * g).max(), name
        assert np.abs(a[f'exp_avg_sq_{name}'] - 0.001 * g * g).max() <= 1e-4 * np.abs(0.001 * g * g).max(), name
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert np.abs(a[k].astype(np.float64) - b[k]).max() <= 1e-4 * max(float(np.abs(a[k]).max()), 1e-30), k
