"""bench.py's command line: a plain run does only what the headline figure needs
(--full adds the CPU baseline and the nested configs[2] line), and --dump-outputs
writes the last timed step's outputs so that two builds can be compared."""
import json
import sys

import numpy as np
import pytest
import torch

import bench


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, 'argv', ['bench.py'] + list(argv))
    return bench.parse()


def test_full_and_dump_outputs_are_off_by_default(monkeypatch):
    a = _args(monkeypatch, '--gpus', '1', '--steps', '3', '--warmup', '1')
    assert a.full is False and a.dump_outputs is None and a.steps == 3 and a.warmup == 1
    a = _args(monkeypatch, '--full', '--dump-outputs', 'somewhere')
    assert a.full is True and a.dump_outputs == 'somewhere'


def test_dump_outputs_writes_float32_and_samples_large_arrays(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_SAMPLE', 64)
    small = torch.arange(60, dtype=torch.int32).reshape(3, 20)
    flags = torch.tensor([True, False, True])
    large = torch.arange(1000, dtype=torch.int64).reshape(10, 100)
    for _ in range(2):  # a second run overwrites with the same values: the sample is fixed
        bench._dump_outputs(str(tmp_path / 'd'), [('small', small), ('flags', flags), ('large', large)])
        got = {n: np.load(str(tmp_path / 'd' / (n + '.npy'))) for n in ('small', 'flags', 'large')}
        assert all(v.dtype == np.float32 for v in got.values())
        assert got['small'].shape == (3, 20) and np.array_equal(got['small'], small.numpy())
        assert np.array_equal(got['flags'], [1.0, 0.0, 1.0])
        idx = np.random.default_rng(20240607).integers(0, 1000, 64)
        assert got['large'].shape == (64,) and np.array_equal(got['large'], idx.astype(np.float32))


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_reproducible_outputs(lib, cuda, tmp_path, monkeypatch, capsys):
    """Two plain runs with the same arguments: no CPU baseline, no nested configs[2]
    run; the dumped rollout batch and parameters are bit-identical between the runs
    (seeded envs, weights and sampler; the kernels' reductions have a fixed order)."""
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    N, T, K = 16, 20, 3
    runs = []
    for name in ('a', 'b'):
        d = tmp_path / name
        bench.run(_args(monkeypatch, '--gpus', '1', '--steps', str(K), '--warmup', '1', '--envs-per-gpu', str(N),
                        '--dump-outputs', str(d)))
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')]
        assert len(lines) == 1
        out = json.loads(lines[0])
        # --steps is the number of timed iterations: the global step starts at 30, the
        # one warm-up iteration and each timed one advance it by one
        from actorcritic import session as sess
        assert out['steps'] == K and sess.get_or_create_global_step().value == 30 + 1 + K
        assert out['cpu_baseline'] is None and out['configs2'] is None
        assert out['ms_per_step'] > 0
        assert out['value'] == pytest.approx(N * T / (out['ms_per_step'] * 1e-3), rel=1e-9)
        runs.append({p.name[:-4]: np.load(str(p)) for p in sorted(d.glob('*.npy'))})
    a, b = runs
    shapes = {'observations': (bench.DUMP_SAMPLE,), 'actions': (N, T), 'rewards': (N, T), 'terminals': (N, T),
              'next_observations': (N, 84, 84, 4), 'params': (865413,)}
    assert {k: v.shape for k, v in a.items()} == shapes
    for k in shapes:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k], b[k]), k
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert 0 < a['observations'].max() <= 255 and set(np.unique(a['actions'])) <= {0.0, 1.0, 2.0, 3.0}
