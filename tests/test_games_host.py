"""CPU tests of the device games' host side: the rule book
actorcritic/envs/games/host.py (HostGame: Catch and Breakout), the list path over it,
and the C-ABI of the stepper (declared, bound, exported; argument errors; the ctypes
mirror's size)."""
import ctypes
import os
import re

import numpy as np
import pytest

from actorcritic import _lib
from actorcritic.envs.games import host
from actorcritic.envs.games.host import HostGame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('acmi_game_reset', 'acmi_game_step', 'acmi_game_state_ints', 'acmi_game_state_bytes')
BX, BY, VX, VY, PX, LIVES, B0 = range(7)


def _placed(game, **kw):
    """A freshly reset game with some state entries replaced."""
    g = HostGame(game, seed=1, env_id=0)
    g.reset()
    s = g.state
    for k, v in kw.items():
        s[{'bx': BX, 'by': BY, 'vx': VX, 'vy': VY, 'px': PX, 'lives': LIVES}[k]] = v
    g.set_state(s)
    return g


# -- Catch ----------------------------------------------------------------------
def test_catch_frame_and_spaces():
    g = HostGame('catch', seed=3, env_id=2)
    f = g.reset()
    assert f.shape == (84, 84, 1) and f.dtype == np.uint8
    assert g.action_space.n == 3 and tuple(g.observation_space.shape) == (84, 84, 1)
    s = g.state
    assert s.dtype == np.int32 and s.shape == (host.STATE_INTS,)
    assert s[BY] == 0 and s[PX] == 36 and s[BX] % 4 == 0 and 0 <= s[BX] <= 80 and s[VX] in (-4, 0, 4)
    want = np.zeros((84, 84), np.uint8)
    want[80:84, 36:48] = 200
    want[0:4, s[BX]:s[BX] + 4] = 255
    assert np.array_equal(f[..., 0], want)
    assert sorted(np.unique(f)) == [0, 200, 255]


def test_catch_paddle_clamps_at_both_walls():
    g = _placed('catch', vx=0)
    for _ in range(12):
        g.step(1)
    assert g.state[PX] == 72
    g = _placed('catch', vx=0)
    for _ in range(12):
        g.step(2)
    assert g.state[PX] == 0
    g = _placed('catch', vx=0)
    for a in (0, 3, 17, -1):  # NOOP and out-of-range actions leave the paddle
        g.step(a)
    assert g.state[PX] == 36


def test_catch_ball_bounces_off_the_walls():
    g = _placed('catch', bx=76, vx=4)
    xs = []
    for _ in range(4):
        g.step(0)
        xs.append((int(g.state[BX]), int(g.state[VX])))
    assert xs == [(80, 4), (76, -4), (72, -4), (68, -4)]
    g = _placed('catch', bx=4, vx=-4)
    xs = []
    for _ in range(3):
        g.step(0)
        xs.append((int(g.state[BX]), int(g.state[VX])))
    assert xs == [(0, -4), (4, 4), (8, 4)]


def test_catch_ends_exactly_at_step_19():
    g = HostGame('catch', seed=5, env_id=1)
    g.reset()
    for t in range(1, 20):
        f, r, term, info = g.step(0)
        assert term == (t == 19)
        if t < 19:
            assert r == 0.0
        assert g.state[BY] == 4 * t
    assert r in (-1.0, 1.0)
    assert np.array_equal(f[76:80, g.state[BX]:g.state[BX] + 4, 0], np.full((4, 4), 255))


@pytest.mark.parametrize('offset,reward', [(-4, -1.0), (0, 1.0), (4, 1.0), (8, 1.0), (12, -1.0)])
def test_catch_reward_columns(offset, reward):
    """The ball lands at x = 40 with the paddle at 40 - offset."""
    g = _placed('catch', bx=40, vx=0, by=72, px=40 - offset)
    _, r, term, _ = g.step(0)
    assert term and r == reward


def test_catch_start_is_a_pure_function_of_seed_env_episode():
    def starts(seed, env_id, n=12):
        g = HostGame('catch', seed=seed, env_id=env_id)
        out = []
        for _ in range(n):
            g.reset()
            out.append((int(g.state[BX]), int(g.state[VX])))
        return out
    a = starts(7, 3)
    assert a == starts(7, 3)
    assert len(set(a)) > 3  # differs across episodes
    assert a != starts(8, 3) and a != starts(7, 4)
    h = host.key4(7, 3, 2, host.CATCH_TAG)
    assert a[2] == (4 * (h % 21), 4 * ((h >> 8) % 3 - 1))
    # the hash is csrc/common.hpp's, as the oracle restates it
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import oracle
    for args in ((0, 0, 0, 0), (7, 3, 2, host.CATCH_TAG), (0xFFFFFFFF, 12345, 99, host.BREAKOUT_TAG + 3)):
        assert host.key4(*args) == int(oracle.key4(*args))


def test_catch_is_always_winnable():
    for e in range(20):
        g = HostGame('catch', seed=0, env_id=e)
        g.reset()
        probe = HostGame('catch', seed=0, env_id=e)
        probe.reset()
        for _ in range(19):
            probe.step(0)
        target = int(probe.state[BX])  # the ball's landing column does not depend on the actions
        r = term = None
        for _ in range(19):
            px = int(g.state[PX])
            _, r, term, _ = g.step(1 if px + 4 < target else (2 if px + 4 > target + 4 else 0))
        assert term and r == 1.0


# -- Breakout -------------------------------------------------------------------
def test_breakout_frame():
    g = HostGame('breakout', seed=2, env_id=0)
    f = g.reset()[..., 0]
    s = g.state
    assert g.action_space.n == 4
    assert s[LIVES] == 3 and s[BY] == 40 and s[VY] == 2 and s[VX] in (-2, -1, 1, 2) and s[BX] % 2 == 0
    assert list(s[B0:B0 + 3]) == [0xFFFFFF] * 3 and list(s[9:]) == [0, 0, 0]
    for r in range(6):
        assert (f[12 + 3 * r:15 + 3 * r] == 100 + 20 * r).all()
    assert (f[80:82, 36:48] == 200).all() and (f[82:] == 0).all() and (f[:12] == 0).all()
    assert (f[40:42, s[BX]:s[BX] + 2] == 255).all()


def test_breakout_brick_hit_clears_one_bit_rewards_and_flips_vy():
    g = _placed('breakout', bx=30, by=32, vx=1, vy=-2)
    before = g.state
    _, r, term, _ = g.step(0)
    assert r == 0.0 and g.state[BY] == 30  # the probe pixel (31, 30) is below the bricks
    _, r, term, _ = g.step(1)  # FIRE acts as NOOP
    s = g.state
    assert r == 1.0 and not term
    assert s[VY] == 2 and s[BY] == 28 and s[BX] == 32
    gone = [int(a) ^ int(b) for a, b in zip(before[B0:B0 + 3], s[B0:B0 + 3])]
    # row 5 (y 27..29), column 32 // 7 = 4: bit 12 + 4 of the third word
    assert gone == [0, 0, 1 << 16]
    f = g.render()[..., 0]
    assert (f[27:30, 28:35] == 0).sum() == 21 - 4 and (f[28:30, 32:34] == 255).all()
    _, r, _, _ = g.step(0)
    assert r == 0.0 and g.state[BY] == 30


def test_breakout_paddle_sets_vx_from_the_hit_offset():
    for off, vx in ((-1, -2), (2, -2), (3, -1), (5, -1), (6, 1), (8, 1), (9, 2), (11, 2)):
        g = _placed('breakout', bx=40 + off - 1, by=76, vx=1, vy=2, px=40)
        g.step(0)
        assert (g.state[BY], g.state[VY], g.state[VX]) == (78, -2, vx), off
    g = _placed('breakout', bx=40 + 12 - 1, by=76, vx=1, vy=2, px=40)  # one past the paddle
    g.step(0)
    assert g.state[VY] == 2


def test_breakout_life_loss_respawns_without_a_terminal_and_ends_at_zero_lives():
    g = _placed('breakout', bx=0, by=76, vx=1, vy=2, px=60)
    k = g.episode
    _, r, term, _ = g.step(0)
    assert not term and g.state[LIVES] == 3 and g.state[BY] == 78
    _, r, term, _ = g.step(0)
    s = g.state
    assert r == 0.0 and not term and s[LIVES] == 2 and s[PX] == 60
    h = host.key4(1, 0, k, host.BREAKOUT_TAG + 2)
    assert (s[BX], s[BY], s[VX], s[VY]) == (2 * (h % 42), 40, (-2, -1, 1, 2)[(h >> 8) & 3], 2)
    g = _placed('breakout', bx=0, by=78, vx=1, vy=2, px=60, lives=1)
    _, r, term, _ = g.step(0)
    assert term and g.state[LIVES] == 0 and r == 0.0
    # the last brick ends the game as well
    g = _placed('breakout', bx=30, by=30, vx=1, vy=-2)
    s = g.state
    s[B0:B0 + 3] = (0, 0, 1 << 16)
    g.set_state(s)
    _, r, term, _ = g.step(0)
    assert r == 1.0 and term and g.state[LIVES] == 3


def test_breakout_is_deterministic_and_bounces_off_walls_and_ceiling():
    rng = np.random.RandomState(0)
    script = rng.randint(0, 6, size=400)
    def run():
        g = HostGame('breakout', seed=9, env_id=4)
        out = [g.reset().tobytes()]
        for a in script:
            f, r, term, _ = g.step(a)
            out.append((f.tobytes(), r, term, g.state.tobytes()))
            if term:
                out.append(g.reset().tobytes())
        return out
    assert run() == run()
    g = _placed('breakout', bx=1, by=2, vx=-2, vy=-2)
    s = g.state
    s[B0:B0 + 3] = (1, 0, 0)
    g.set_state(s)
    g.step(0)
    assert (g.state[BX], g.state[VX], g.state[BY], g.state[VY]) == (3, 2, 0, -2)
    g.step(0)
    assert (g.state[BY], g.state[VY]) == (2, 2)
    g = _placed('breakout', bx=82, by=50, vx=1, vy=-2)
    g.step(0)
    assert (g.state[BX], g.state[VX]) == (81, -1)


def test_breakout_step_cap():
    """With lives and bricks left the game ends at step 2000, not before."""
    g = _placed('breakout', bx=40, by=60, vx=1, vy=-2)
    g.steps = host.BREAKOUT_MAX_STEPS - 2
    _, _, term, _ = g.step(0)
    assert not term and g.steps == 1999
    _, _, term, _ = g.step(0)
    assert term and g.steps == 2000 and g.state[LIVES] == 3 and g.state[B0] == 0xFFFFFF
    # and a paddle that follows the ball keeps a game going for hundreds of steps
    g = HostGame('breakout', seed=4, env_id=0)
    g.reset()
    total = 0.0
    for t in range(600):
        s = g.state
        _, r, term, _ = g.step(2 if s[PX] + 5 < s[BX] else (3 if s[PX] + 5 > s[BX] else 0))
        total += r
        if term:
            break
    assert g.state[LIVES] == 3 and total >= 10


# -- the list path ----------------------------------------------------------------
def test_list_path_steps_and_auto_resets():
    from actorcritic.envs.atari.wrappers import EpisodeInfoWrapper, FrameStackWrapper
    from actorcritic.multi_env import MultiEnv
    envs = MultiEnv([FrameStackWrapper(EpisodeInfoWrapper(HostGame('catch', seed=0, env_id=i)), 4) for i in range(2)])
    try:
        assert envs.batched is None and envs.num_envs == 2 and envs.action_space.n == 3
        assert tuple(envs.observation_space.shape) == (84, 84, 4)
        obs = envs.reset()
        assert obs[0].shape == (84, 84, 4) and all((obs[0][..., c] == obs[0][..., 0]).all() for c in range(4))
        totals = []
        for t in range(1, 41):
            obs, rew, term, infos = envs.step([1, 2])
            assert term == [t in (19, 38)] * 2
            if term[0]:
                assert all((o[..., :3] == 0).all() for o in obs)  # zero-filled on a terminal
                totals.append([info['episode']['total_reward'] for info in infos])
                assert totals[-1] == rew
            elif t in (20, 39):  # the reset step: [f0, f0, f0, f1]
                assert all((o[..., 0] == o[..., 2]).all() and o[0:4, :, 0].max() == 255 for o in obs)
                assert all(o[4:8, :, 3].max() == 255 and o[0:4, :, 3].max() == 0 for o in obs)
            else:
                assert all('episode' not in info for info in infos)
        assert len(totals) == 2
    finally:
        envs.close()


# -- the C-ABI ----------------------------------------------------------------------
def test_new_entry_points_are_declared_bound_and_exported(lib):
    src = open(os.path.join(ROOT, 'include', 'acmi.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(acmi_[a-z0-9_]+)\s*\(', src))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.EXPORTED, name
        assert hasattr(lib, name), name
    assert lib.acmi_abi_version() == 4
    sizes = (ctypes.c_int64 * 6)()
    assert lib.acmi_abi_struct_sizes(ctypes.cast(sizes, ctypes.c_void_p), 6) == 5


def test_state_mirror_size_and_ints(lib):
    assert lib.acmi_game_state_bytes() == ctypes.sizeof(_lib.GameState)
    assert lib.acmi_game_state_ints() == host.STATE_INTS == 12


def test_argument_errors(lib):
    one = ctypes.c_void_p(16)  # a non-null pointer no call gets as far as using
    def state(game=0, vars_=one):
        return _lib.GameState(one, one, one, one, vars_, game)
    step = lambda st, N=1, in_stride=28224, out_stride=28224, ld=1, actions=one: lib.acmi_game_step(
        ctypes.byref(st), N, 0, 0, actions, one, in_stride, one, out_stride, one, one, one, ld, None)
    reset = lambda st, N=1, stride=28224, obs=one: lib.acmi_game_reset(ctypes.byref(st), N, 0, 0, obs, stride, None)
    for bad in (state(game=2), state(game=-1), state(vars_=None)):
        assert step(bad) == _lib.ERR_ARG
        assert reset(bad) == _lib.ERR_ARG
    assert b'acmi_game_reset' in lib.acmi_last_error()
    ok = state()
    assert step(ok, N=-1) == _lib.ERR_ARG
    assert step(ok, in_stride=28224 + 8) == _lib.ERR_ARG
    assert step(ok, out_stride=28208) == _lib.ERR_ARG
    assert step(ok, ld=0) == _lib.ERR_ARG
    assert step(ok, actions=None) == _lib.ERR_ARG
    assert b'acmi_game_step' in lib.acmi_last_error()
    assert reset(ok, N=-1) == _lib.ERR_ARG
    assert reset(ok, stride=28224 - 16) == _lib.ERR_ARG
    assert reset(ok, obs=None) == _lib.ERR_ARG
    assert lib.acmi_game_step(None, 1, 0, 0, one, one, 28224, one, 28224, one, one, one, 1, None) == _lib.ERR_ARG
    # nothing to do is not an error (and launches nothing)
    assert step(ok, N=0) == 0 and reset(ok, N=0) == 0


def test_device_envs_argument_checks_need_no_library_call():
    from actorcritic.envs import games
    assert games.GAME_ACTIONS == {'catch': 3, 'breakout': 4}
    assert host.game_id('catch') == 0 and host.game_id('breakout') == 1 and host.game_id(1) == 1
    with pytest.raises(ValueError):
        host.game_id('pong')
    assert games.DeviceGameEnvs.fused_step is False


def test_examples_take_the_game_keyword():
    import inspect
    from actorcritic.examples.atari import a2c_acktr, ppo
    assert inspect.signature(a2c_acktr.train_a2c_acktr).parameters['game'].default is None
    assert inspect.signature(ppo.train_ppo).parameters['game'].default is None
