"""CPU tests of the legal-action masks' host side: the six *_masked
entry points are exported with ctypes signatures, their argument errors are reported
before any launch, the mask words of wrappers.action_mask_bits / the Atari-57 table,
and the mask-count check of a forward."""
import ctypes

import numpy as np
import pytest

MASKED = ('acmi_sample_actions_masked', 'acmi_categorical_masked', 'acmi_a2c_loss_masked', 'acmi_ppo_loss_masked',
          'acmi_kfac_output_stats_masked', 'acmi_rollout_step_masked')
ERR_ARG = -1


def fake(k):
    return ctypes.c_void_p(0x100000 * k)  # a device address no argument check touches


def test_masked_symbols_are_exported_with_signatures(lib):
    from actorcritic import _lib
    for name in MASKED:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTED, 'no ctypes signature for ' + name
        assert getattr(lib, name).argtypes is not None
    assert lib.acmi_abi_version() == 4


def _calls(lib, A, legal):
    """Every masked entry point with otherwise valid arguments -> [(name, status, message)]."""
    from actorcritic import _lib
    B, ld, ldh = 8, A + 3, A + 4
    net = _lib.Net(A, 32, fake(1).value, fake(2).value)
    acts = _lib.Acts(*[fake(3 + i).value for i in range(6)], A)
    bwd = _lib.Bwd(*[fake(10 + i).value for i in range(5)], 36)
    io = _lib.RolloutIO(1, 0, 0, None, 0, fake(30).value, fake(31).value,
                        _lib.EnvState(*[fake(32 + i).value for i in range(5)], None), 0, 1, fake(40).value,
                        84 * 84 * 4, fake(41).value, fake(42).value, fake(43).value, 1, 0, None, 1, None)
    out = []

    def run(name, *args):
        rc = getattr(lib, name)(*args)
        out.append((name, rc, lib.acmi_last_error()))

    run('acmi_sample_actions_masked', fake(20), ld, B, A, 1, 0, None, 0, 0, None, 0, legal, fake(21), fake(22), None)
    run('acmi_categorical_masked', fake(20), ld, B, A, fake(21), legal, fake(22), fake(23), None)
    run('acmi_a2c_loss_masked', fake(20), ld, fake(21), fake(22), fake(23), fake(24), B, A, 0.01, 0.5, 1.0, fake(25),
        ldh, fake(26), fake(27), legal, None, None)
    run('acmi_ppo_loss_masked', fake(20), ld, fake(21), fake(22), fake(23), fake(24), fake(25), fake(26), B, A, 0.1,
        0.0, 0.01, 0.5, 1.0, fake(27), ldh, fake(28), fake(29), None, legal, None, None)
    run('acmi_kfac_output_stats_masked', ctypes.byref(net), B, ctypes.byref(acts), ctypes.byref(bwd), 7, 0, 3, legal,
        fake(22), fake(23), 1 << 40, None)
    run('acmi_rollout_step_masked', ctypes.byref(net), fake(20), 84 * 84 * 4, B, ctypes.byref(acts), 1,
        ctypes.byref(io), legal, None)
    return out


def test_more_than_32_actions_with_a_mask_is_an_argument_error(lib):
    for name, rc, msg in _calls(lib, 33, fake(50)):
        assert rc == ERR_ARG, name
        assert name.encode() in msg and b'32' in msg, (name, msg)


def test_null_mask_is_an_argument_error(lib):
    for name, rc, msg in _calls(lib, 18, None):
        assert rc == ERR_ARG, name
        assert name.encode() in msg and b'legal' in msg, (name, msg)


def test_action_mask_bits():
    from actorcritic.envs.atari.wrappers import action_mask_bits
    assert action_mask_bits([0, 1, 3, 4], 18) == 0b11011
    assert action_mask_bits(range(32), 32) == 0xFFFFFFFF
    with pytest.raises(ValueError):
        action_mask_bits([], 18)
    with pytest.raises(ValueError):
        action_mask_bits([0, 18], 18)
    with pytest.raises(ValueError):
        action_mask_bits([-1], 18)
    with pytest.raises(ValueError):
        action_mask_bits([0], 33)


def test_per_game_words_are_the_minimal_action_sets():
    from actorcritic.envs.atari import wrappers
    words = wrappers.game_action_masks(wrappers.ATARI57)
    assert len(words) == 57
    assert words == [(1 << n) - 1 for n in wrappers.ATARI57_ACTIONS]
    # the stepper's table (csrc/stepper.hpp kGameActions; Breakout's n_legal is 4) is this one
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'actor-critic_amd', 'csrc',
                            'stepper.hpp')).read()
    table = re.search(r'kGameActions\[kNumGames\] = \{([^}]*)\}', src).group(1)
    assert tuple(int(x) for x in table.split(',')) == wrappers.ATARI57_ACTIONS
    assert wrappers.ATARI57_ACTIONS[wrappers.game_index('Breakout')] == 4
    assert re.search(r'g == kGameBreakout\) p\.n_legal = 4u', src)
    assert wrappers.game_action_masks(['Freeway', 'Breakout', 'Pong', 'Seaquest']) == [0b111, 0b1111, 0x3F, 0x3FFFF]


def test_host_masks_are_validated():
    from actorcritic._engine import host_action_masks
    assert host_action_masks([0b11011, 1], 18).dtype == np.uint32
    assert list(host_action_masks(np.array([0xFFFFFFFF], np.uint32), 32)) == [0xFFFFFFFF]
    with pytest.raises(ValueError, match='empty'):
        host_action_masks([3, 0], 18)
    with pytest.raises(ValueError, match='at or above'):
        host_action_masks([1 << 18], 18)
    with pytest.raises(ValueError, match='32'):
        host_action_masks([1], 33)
    with pytest.raises(ValueError):
        host_action_masks([], 18)


def test_mask_count_mismatch_raises_naming_both_numbers():
    import torch
    from actorcritic._engine import NetEngine, check_mask_count
    check_mask_count(8, 8)
    with pytest.raises(ValueError, match=r'8 envs.* 6'):
        check_mask_count(8, 6)
    # the engine's per-row expansion of the words checks the env count first
    eng = object.__new__(NetEngine)
    eng.masks, eng._mask_rows = torch.tensor([7, 15, 63], dtype=torch.int32), {}
    assert eng.row_masks(3, 2).tolist() == [7, 7, 15, 15, 63, 63]
    assert eng.row_masks(3, 2) is eng.row_masks(3, 2)  # cached
    with pytest.raises(ValueError, match=r'3 envs.* 4'):
        eng.row_masks(4, 2)
