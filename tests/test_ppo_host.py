"""CPU tests of the PPO feature's host side: the three entry points are declared in
include/acmi.h, bound in actorcritic/_lib.py and exported by libacmi.so; argument
checks that need no GPU; the example imports."""
import os
import re

import pytest

from actorcritic import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('acmi_ppo_loss_ws_floats', 'acmi_ppo_loss', 'acmi_adam_apply')


def test_new_entry_points_are_declared_bound_and_exported(lib):
    src = open(os.path.join(ROOT, 'include', 'acmi.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(acmi_[a-z0-9_]+)\s*\(', src))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.EXPORTED, name
        assert hasattr(lib, name), name
    assert lib.acmi_abi_version() == 4
    for M in (1, 37, 1000, 10240):
        assert lib.acmi_ppo_loss_ws_floats(M) > 0
    # five partial sums per block of 256 rows
    assert lib.acmi_ppo_loss_ws_floats(1000) >= 5 * 4


def test_minibatches_must_divide_the_envs():
    from actorcritic.objectives import ppo_minibatch_rows
    assert ppo_minibatch_rows(4, 5, 2) == [(0, 10), (10, 10)]
    assert ppo_minibatch_rows(4, 5, 1) == [(0, 20)]
    for bad in (3, 8, 0):
        with pytest.raises(ValueError):
            ppo_minibatch_rows(4, 5, bad)


def test_minibatch_order_is_a_seeded_permutation_per_epoch():
    from actorcritic.objectives import ppo_minibatch_order
    a = ppo_minibatch_order(7, 3, 4, 8)
    assert a == ppo_minibatch_order(7, 3, 4, 8)
    assert all(sorted(p) == list(range(8)) for p in a) and len(a) == 4
    assert a != ppo_minibatch_order(7, 4, 4, 8) and a != ppo_minibatch_order(8, 3, 4, 8)


def test_objective_argument_checks():
    from actorcritic.objectives import ActorCriticObjective, PPOObjective
    for bad in (0.0, -0.1):
        with pytest.raises(ValueError):
            PPOObjective(object(), clip_range=bad)
    with pytest.raises(ValueError):
        PPOObjective(object(), value_clip_range=0.0)
    with pytest.raises(ValueError):
        PPOObjective(object(), gae_lambda=1.5)
    obj = PPOObjective(object())
    assert isinstance(obj, ActorCriticObjective)
    for name in ('policy_loss', 'baseline_loss', 'mean_entropy', 'approx_kl', 'clip_fraction', 'target_values',
                 'advantage'):
        assert getattr(obj, name) is not None
    with pytest.raises(ValueError):
        obj.optimize_shared(object(), num_epochs=0)


def test_kfac_optimizer_is_refused():
    from actorcritic.kfac_utils import KfacOptimizer
    from actorcritic.objectives import PPOObjective
    opt = KfacOptimizer.__new__(KfacOptimizer)  # (no engine behind it: only its type matters)
    with pytest.raises(NotImplementedError, match='first-order'):
        PPOObjective(object()).optimize_shared(opt)


def test_adam_slots_and_example_import():
    from actorcritic.nn import AdamOptimizer, ClipGlobalNormOptimizer
    opt = AdamOptimizer(2.5e-4, epsilon=1e-5)
    assert opt._slot_names == ('_m', '_v', '_t') and opt.slots() == {}
    assert ClipGlobalNormOptimizer(opt, 0.5).slots() == {}
    import actorcritic.examples.atari.ppo as ppo
    assert callable(ppo.train_ppo)
    wrapped = ppo.create_optimizer(2.5e-4)
    assert isinstance(wrapped.optimizer, AdamOptimizer) and wrapped.clip_norm == 0.5
