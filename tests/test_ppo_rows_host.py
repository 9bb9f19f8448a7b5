"""CPU tests of PPO's row minibatches: the host row order, the argument checks of
``optimize_shared(minibatch=...)`` / ``normalize_advantages='minibatch'``, and
acmi_gather_rows' host-side argument checks (fake device addresses: every check fails,
or rows == 0 returns, before anything is enqueued)."""
import ctypes
import os
import re

import numpy as np
import pytest

from actorcritic import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBS_BYTES = 84 * 84 * 4
ERR_ARG = -1  # ACMI_ERR_ARG


def test_row_order_is_a_seeded_int32_permutation_per_epoch():
    from actorcritic.objectives import ppo_row_order
    M, epochs, seed, step = 60, 3, 7, 11
    a = ppo_row_order(seed, step, epochs, M)
    assert len(a) == epochs
    for p in a:
        assert isinstance(p, np.ndarray) and p.dtype == np.int32 and p.shape == (M,)
        assert np.array_equal(np.sort(p), np.arange(M))
    assert not all(np.array_equal(a[0], p) for p in a[1:])  # (one draw per epoch)
    b = ppo_row_order(seed, step, epochs, M)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    c = ppo_row_order(seed, step + 1, epochs, M)
    assert not any(np.array_equal(x, y) for x, y in zip(a, c))
    # nmb equal slices partition range(M)
    for nmb in (1, 4, 5, 60):
        parts = np.split(a[0], nmb)
        assert all(len(q) == M // nmb for q in parts)
        assert sorted(int(i) for q in parts for i in q) == list(range(M))
    # the literal restatement
    rng = np.random.default_rng([seed, step])
    for p in a:
        assert np.array_equal(p, rng.permutation(M))


def test_minibatch_mode_argument_checks():
    from actorcritic.objectives import PPOObjective, PPOOptimizeOp
    obj = PPOObjective(object())
    op = obj.optimize_shared(object())
    assert isinstance(op, PPOOptimizeOp) and op.minibatch == 'envs'
    assert op.last_order is None and op.last_rows is None
    assert obj.optimize_shared(object(), minibatch='rows').minibatch == 'rows'
    for bad in ('cols', None, 'ROWS'):
        with pytest.raises(ValueError):
            obj.optimize_shared(object(), minibatch=bad)
    with pytest.raises(ValueError):
        PPOOptimizeOp(obj, object(), 1, 1, 0, None, None, 'cols')

    per_mb = PPOObjective(object(), normalize_advantages='minibatch')
    with pytest.raises(ValueError):
        per_mb.optimize_shared(object())
    with pytest.raises(ValueError):
        per_mb.optimize_shared(object(), minibatch='envs')
    assert per_mb.optimize_shared(object(), minibatch='rows').minibatch == 'rows'
    assert not per_mb._normalize  # (no batch-level normalisation on top)
    with pytest.raises(ValueError):
        PPOObjective(object(), normalize_advantages='batch')
    assert PPOObjective(object())._normalize and not PPOObjective(object(), normalize_advantages=False)._normalize


def test_example_passes_the_mode_through():
    import inspect

    import actorcritic.examples.atari.ppo as ppo
    assert inspect.signature(ppo.train_ppo).parameters['minibatch'].default == 'envs'


def test_gather_rows_is_declared_bound_and_exported(lib):
    src = open(os.path.join(ROOT, 'include', 'acmi.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    assert 'acmi_gather_rows' in set(re.findall(r'\b(acmi_[a-z0-9_]+)\s*\(', src))
    assert 'acmi_gather_rows' in _lib.EXPORTED and hasattr(lib, 'acmi_gather_rows')
    assert lib.acmi_abi_version() == 4


def test_gather_rows_argument_checks_fail_before_any_launch(lib):
    fake = lambda k: ctypes.c_void_p(0x100000 * k)
    nv = 5
    src = (ctypes.c_void_p * 9)(*[0x100000 * (10 + k) for k in range(9)])
    dst = (ctypes.c_void_p * 9)(*[0x100000 * (30 + k) for k in range(9)])

    def status(obs=fake(1), img_stride=OBS_BYTES, src_rows=8, index=fake(2), rows=4, obs_out=fake(3),
               out_stride=OBS_BYTES, nvec=nv, vec_src=src, vec_dst=dst):
        return lib.acmi_gather_rows(obs, img_stride, src_rows, index, rows, obs_out, out_stride, nvec, vec_src,
                                    vec_dst, None, None)

    assert status(nvec=9) == ERR_ARG and b'acmi_gather_rows' in lib.acmi_last_error()
    assert status(nvec=-1) == ERR_ARG
    assert status(rows=-1) == ERR_ARG
    assert status(src_rows=-1) == ERR_ARG
    assert status(out_stride=OBS_BYTES + 1) == ERR_ARG
    assert status(img_stride=OBS_BYTES + 8) == ERR_ARG
    assert status(out_stride=OBS_BYTES - 16) == ERR_ARG  # (output rows would overlap)
    assert status(index=None) == ERR_ARG
    assert status(obs_out=None) == ERR_ARG
    assert status(obs=ctypes.c_void_p(0x100004)) == ERR_ARG
    assert status(obs_out=ctypes.c_void_p(0x300008)) == ERR_ARG
    assert status(vec_src=None) == ERR_ARG and status(vec_dst=None) == ERR_ARG
    hole = (ctypes.c_void_p * 9)(*[0x100000 * (10 + k) if k != 3 else None for k in range(9)])
    assert status(vec_src=hole) == ERR_ARG and status(vec_dst=hole) == ERR_ARG
    # rows == 0: ACMI_OK without a launch (also with no image, and with no vectors)
    assert status(rows=0) == 0
    assert status(rows=0, vec_src=hole, nvec=3) == 0  # (the null pointer is past nvec)
    assert status(rows=0, obs=None, obs_out=None) == 0
    assert status(rows=0, nvec=0, vec_src=None, vec_dst=None) == 0
    # ... but the other arguments are still checked
    assert status(rows=0, nvec=9) == ERR_ARG and status(rows=0, index=None) == ERR_ARG
