"""bench.py: the --dump-outputs writer (CPU), and plain runs of both branches -- the result line, no --full figures, dumps
that are finite and the same in every run (GPU)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')
SMALL = ['--items', '200001', '--users', '20001', '--neg', '64', '--steps', '3', '--warmup', '1']
CONTRACT = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')


def test_dump_outputs_budget_sample_and_dtypes(tmp_path):
    import bench
    M, n = 1000, 64
    g = torch.Generator().manual_seed(0)
    out = {'neg_ids': torch.randint(1, 10 ** 7, (M, n), generator=g), 'neg_score': torch.randn(M, n, generator=g),
           'pos_score': torch.randn(M, generator=g), 'loss': torch.tensor(0.5), 'note': 'not an array'}
    bench.dump_outputs(tmp_path / 'whole', out)
    assert sorted(os.listdir(tmp_path / 'whole')) == ['loss.npy', 'neg_ids.npy', 'neg_score.npy', 'pos_score.npy']
    ids = np.load(tmp_path / 'whole' / 'neg_ids.npy')
    assert ids.dtype == np.float64 and np.array_equal(ids, out['neg_ids'].numpy())          # ids exact as float64
    assert np.load(tmp_path / 'whole' / 'neg_score.npy').dtype == np.float32
    assert np.load(tmp_path / 'whole' / 'loss.npy').shape == ()
    # over the budget: every per-row array cut to the SAME seeded rows (sorted, listed in sample_rows.npy); data <= budget
    per_row = n * 8 + n * 4 + 4 + 8                      # neg_ids, neg_score, pos_score, the row index
    budget = 4 + 200 * per_row
    for name in ('cut', 'cut_again'):
        bench.dump_outputs(tmp_path / name, out, budget=budget)
    rows = np.load(tmp_path / 'cut' / 'sample_rows.npy')
    assert rows.dtype == np.float64 and len(rows) == 200 and np.all(np.diff(rows) > 0)
    r = rows.astype(np.int64)
    data = 0
    for f in ('neg_ids', 'neg_score', 'pos_score', 'loss', 'sample_rows'):
        a, b = np.load(tmp_path / 'cut' / f'{f}.npy'), np.load(tmp_path / 'cut_again' / f'{f}.npy')
        assert np.array_equal(a, b), f                   # seeded: the same sample every time
        data += a.nbytes
        if f in out and out[f].dim():
            assert np.array_equal(a, out[f].numpy()[r].astype(a.dtype)), f
    assert data <= budget


def _line(cmd, env=None):
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def _same_finite_dumps(a, b):
    names = sorted(os.listdir(a))
    assert names and names == sorted(os.listdir(b))
    for f in names:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert x.dtype in (np.float32, np.float64), f
        assert np.isfinite(x).all(), f
        assert np.array_equal(x, y), f
    return names


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_dumps_the_same_outputs(tmp_path):
    """A plain single-GPU run: the contract's keys, no --full figure, a whole-step roofline under its own keys, and the
    last timed step's outputs -- finite, and the same in two runs (the headline restarts its batches and generator after
    the time-based pre-warm)."""
    lines = [_line([sys.executable, BENCH, '--gpus', '1', '--batch', '4096'] + SMALL + ['--dump-outputs', str(tmp_path / r)])
             for r in ('a', 'b')]
    for line in lines:
        assert all(k in line for k in CONTRACT)
        assert line['steps'] == 3 and line['warmup'] == 1 and line['ms_per_step'] > 0
        assert line['value'] == pytest.approx(4096 * 64 / line['ms_per_step'] / 1e3, rel=5e-3)
        assert not {'cpu_baseline', 'train_step', 'sweep', 'fullscore', 'unfused_loss_ms_per_step'} & set(line)
        assert 'step_frac' in line['roofline'] and 'frac' not in line['roofline']
    names = _same_finite_dumps(tmp_path / 'a', tmp_path / 'b')
    assert {'neg_ids.npy', 'neg_score.npy', 'pos_score.npy', 'pos_logp.npy', 'dneg.npy', 'loss.npy'} <= set(names)


@pytest.mark.gpu
def test_plain_multi_rank_branch_staged_world2(tmp_path):
    """The --gpus N > 1 branch without --full (two STAGED ranks on the one test GPU, as in
    test_bench_multi_rank_branch_runs_staged_world2): one line without the world-1 reference or side figures, and each
    rank's outputs of its last timed step, finite and the same in two runs."""
    env = dict(os.environ, RSA_BENCH_STAGED='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    lines = []
    for r in ('a', 'b'):
        with socket.socket() as s:
            s.bind(('127.0.0.1', 0))
            port = s.getsockname()[1]
        lines.append(_line([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
                            '--master-addr', '127.0.0.1', '--master-port', str(port), BENCH, '--gpus', '2', '--batch', '512']
                           + SMALL + ['--dump-outputs', str(tmp_path / r)], env=env))
    for line in lines:
        assert all(k in line for k in CONTRACT) and line['n_gpus'] == 2 and line['steps'] == 3
        assert not {'world1_reference', 'efficiency_vs_world1', 'train_step', 'one_batch_ahead'} & set(line)
    names = _same_finite_dumps(tmp_path / 'a', tmp_path / 'b')
    assert any(f.endswith('_rank1.npy') for f in names) and any(not f.endswith('_rank1.npy') for f in names)
