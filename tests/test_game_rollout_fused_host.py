"""The fused rollout step of the device games, host side ("Fused step"):
acmi_rollout_step_games' declaration, binding and struct mirror, the unchanged ABI, the
pending entry's size, every argument error (nothing is enqueued, so no GPU is needed) and
the opt-in default.  The GPU half is tests/test_gpu_game_rollout_fused.py."""
import ctypes
import os
import re

import pytest

from actorcritic import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('acmi_game_pend_ints', 'acmi_rollout_game_io_bytes', 'acmi_rollout_step_games')
ONE = ctypes.c_void_p(16)     # a non-null, 16-byte aligned pointer no call gets as far as using
ODD = ctypes.c_void_p(16 + 4)  # a pending area that is not 16-byte aligned


def test_header_declares_the_struct_and_the_three_functions(lib):
    src = open(os.path.join(ROOT, 'include', 'acmi.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    flat = re.sub(r'\s+', ' ', src)
    declared = set(re.findall(r'\b(acmi_[a-z0-9_]+)\s*\(', src))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED and hasattr(lib, name), name
    assert ('typedef struct acmi_rollout_game_io { acmi_rollout_io_t io; acmi_game_state_t state; '
            'const uint8_t* games; acmi_game_rules_t rules; uint8_t* truncated; int32_t* bad_envs; int32_t* pend; } '
            'acmi_rollout_game_io_t;') in flat
    assert 'int acmi_game_pend_ints(void);' in flat and 'int64_t acmi_rollout_game_io_bytes(void);' in flat
    assert ('int acmi_rollout_step_games(const acmi_net_t* net, const uint8_t* obs, int64_t img_stride, int B, '
            'const acmi_acts_t* acts, int64_t act_img_stride, const acmi_rollout_game_io_t* io, '
            'const uint32_t* legal, acmi_stream_t stream);') in flat
    assert len(_lib._SIGS['acmi_rollout_step_games'][1]) == 9


def test_struct_mirror_abi_and_pending_entry(lib):
    assert ctypes.sizeof(_lib.RolloutGameIO) == lib.acmi_rollout_game_io_bytes()
    assert [f[0] for f in _lib.RolloutGameIO._fields_] == ['io', 'state', 'games', 'rules', 'truncated', 'bad_envs',
                                                           'pend']
    # ABI 4 and its five struct sizes: nothing that existed has moved
    assert lib.acmi_abi_version() == 4
    sizes = (ctypes.c_int64 * 6)()
    assert lib.acmi_abi_struct_sizes(ctypes.cast(sizes, ctypes.c_void_p), 6) == 5
    assert list(sizes[:5]) == [ctypes.sizeof(c) for c in (_lib.Net, _lib.Acts, _lib.Bwd, _lib.EnvState,
                                                          _lib.RolloutIO)]
    assert lib.acmi_game_state_bytes() == ctypes.sizeof(_lib.GameState) == 48
    # episode, step, total, done, 12 vars, the flag -- in whole 16-byte words
    ints = lib.acmi_game_pend_ints()
    assert ints >= 17 and (4 * ints) % 16 == 0
    # the pending area is the caller's: the forward workspace is what it was (B * 8 floats at B <= 64)
    for B, nz in ((1, 16), (64, 16)):
        assert lib.acmi_forward_ws_floats(B) == nz * (B + 1) * 512 + 8 * B
    assert lib.acmi_forward_ws_floats(65) == 16 * 66 * 512


def _call(lib, B=1, A=4, net=True, gio=True, state=None, rules=(0, 0), games=ONE, trunc=ONE, bad=ONE, pend=ONE,
          legal=None, next_acts=False, tower_done=0, img_stride=28224, **io_kw):
    """acmi_rollout_step_games on pointers nothing dereferences before the checks are through."""
    acts = _lib.Acts(ONE, ONE, ONE, ONE, ONE, ONE, max(A, 1), None, 0, None, None, None)
    nxt = _lib.Acts(ONE, ONE, ONE, ONE, ONE, ONE, max(A, 1), None, 0, None, None, None)
    f = dict(actions=ONE, bad_rows=ONE, obs_out=ONE, out_stride=28224, rewards=ONE, terminals=ONE,
             episode_rewards=ONE, ld=1, row_offset=0, env_offset=0)
    f.update(io_kw)
    io = _lib.RolloutIO(0, 0, 0, None, f['row_offset'], f['actions'], f['bad_rows'], _lib.EnvState(),
                        f['env_offset'], 0, f['obs_out'], f['out_stride'], f['rewards'], f['terminals'],
                        f['episode_rewards'], f['ld'], tower_done, ctypes.addressof(nxt) if next_acts else None, 1,
                        None)
    st = state if state is not None else _lib.GameState(ONE, ONE, ONE, ONE, ONE, 0)
    g = _lib.RolloutGameIO(io, st, games, _lib.GameRules(*rules), trunc, bad, pend)
    n = _lib.Net(A, 32, ONE, None, 0, 0, 0)
    return lib.acmi_rollout_step_games(ctypes.byref(n) if net else None, ONE, img_stride, B, ctypes.byref(acts), 1,
                                       ctypes.byref(g) if gio else None, legal, None)


def test_argument_errors_enqueue_nothing(lib):
    E = _lib.ERR_ARG
    # null net / io, and every required pointer of the io
    assert _call(lib, net=False) == E and _call(lib, gio=False) == E
    assert b'acmi_rollout_step_games' in lib.acmi_last_error()
    for name in ('actions', 'bad_rows', 'obs_out', 'rewards', 'terminals', 'episode_rewards'):
        assert _call(lib, **{name: None}) == E, name
    assert _call(lib, ld=0) == E and _call(lib, out_stride=28224 + 8) == E and _call(lib, img_stride=28224 + 8) == E
    assert _call(lib, row_offset=-1) == E and _call(lib, env_offset=-1) == E
    # the game state: a null array, a state.game too large (or negative) -- with or without a games array
    for i in range(5):
        p = [ONE] * 5
        p[i] = None
        assert _call(lib, state=_lib.GameState(*p, 0)) == E, i
    for game in (2, 7, -1):
        for games in (ONE, None):
            assert _call(lib, state=_lib.GameState(ONE, ONE, ONE, ONE, ONE, game), games=games) == E
    # rules out of range
    for rules in ((0, -1), (0, 2001), (2, 0), (-1, 0)):
        assert _call(lib, rules=rules) == E, rules
        assert _call(lib, rules=rules, B=0) == E  # checked before "nothing to do"
    # the head limit: A <= 31, masked or not
    assert _call(lib, A=32) == E and _call(lib, A=40) == E and _call(lib, A=32, legal=ONE) == E
    assert b'num_actions=32' in lib.acmi_last_error()
    # the split form (B <= 64) with step fusion needs the pending area, 16-byte aligned
    for B in (1, 64):
        assert _call(lib, B=B, next_acts=True, pend=None) == E
        assert _call(lib, B=B, tower_done=1, pend=None) == E
    assert b'pending' in lib.acmi_last_error()
    assert _call(lib, B=1, next_acts=True, pend=ODD) == E and _call(lib, B=0, pend=ODD) == E
    assert b'aligned' in lib.acmi_last_error()


def test_nothing_to_do_is_not_an_error(lib):
    # B = 0 launches nothing; games, truncated, bad_envs, legal and (without step fusion) pend may be null
    for games in (ONE, None):
        for rules in ((0, 0), (1, 2000), (1, 1)):
            assert _call(lib, B=0, games=games, rules=rules) == 0
            assert _call(lib, B=0, games=games, rules=rules, trunc=None, bad=None, pend=None) == 0
    assert _call(lib, B=0, legal=ONE) == 0 and _call(lib, B=0, A=31) == 0
    assert _call(lib, B=0, next_acts=True) == 0 and _call(lib, B=0, tower_done=1) == 0


def test_the_fused_step_is_opt_in():
    """The class attribute stays False (the default rollout is the three-call chain); the
    keyword exists and defaults to off, here and in the training functions."""
    import inspect
    from actorcritic.envs.games import DeviceGameEnvs
    from actorcritic.examples.atari.a2c_acktr import create_game_environments, train_a2c_acktr
    from actorcritic.examples.atari.ppo import train_ppo
    assert DeviceGameEnvs.fused_step is False
    assert inspect.signature(DeviceGameEnvs.__init__).parameters['fused_step'].default is False
    assert inspect.signature(create_game_environments).parameters['fused_step'].default is False
    for fn in (train_a2c_acktr, train_ppo):
        assert inspect.signature(fn).parameters['fused_games'].default is False
    assert callable(DeviceGameEnvs.rollout_step)


@pytest.mark.parametrize('fn', ['a2c', 'ppo'])
def test_fused_games_needs_a_device_game(fn):
    from actorcritic.examples.atari.a2c_acktr import train_a2c_acktr
    from actorcritic.examples.atari.ppo import train_ppo
    with pytest.raises(ValueError, match='fused_games'):
        if fn == 'a2c':
            train_a2c_acktr(False, 'x', 2, 2, None, 'x', fused_games=True)
        else:
            train_ppo('x', 2, 2, None, 'x', fused_games=True)
