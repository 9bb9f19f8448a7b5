"""CPU tests of mixed device-game batches ("Mixed batches"): game_pattern,
the C-ABI of acmi_game_count / acmi_game_actions / acmi_game_reset_mixed /
acmi_game_step_mixed (declared, bound, exported, argument errors), and the host replay
of a batch of different games with the coverage of the scripts that
tests/test_gpu_games_mixed.py runs on the device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from actorcritic import _lib
from actorcritic.envs.games import host
from actorcritic.envs.games.host import HostGame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('acmi_game_count', 'acmi_game_actions', 'acmi_game_reset_mixed', 'acmi_game_step_mixed')
NAN_BITS = 0x7fc00000
B, C = 'breakout', 'catch'

# the GPU bit-exactness test's run
MIXED_SEED, MIXED_OFFSET, MIXED_MAX_STEPS = 11, 5, 600
MIXED_ACTIONS = np.random.RandomState(3).randint(-1, 7, size=(MIXED_MAX_STEPS, 3)).astype(np.int32)
MIXED_PATTERNS = {'BCB': ((B, C, B), 124), 'CBC': ((C, B, C), 104)}  # -> the steps each needs


class MixedReplay(object):
    """N HostGame of per-env games (with or without cuts) behind the lazy auto-reset, the
    4-frame stack (roll, zero-fill on a terminal, the reset frame 4x) and the whole-game
    episode total: what acmi_game_step_mixed must produce.  done holds the stepper's codes
    (0 running, 1 game over, 2 life lost)."""

    def __init__(self, games, seed=0, env_offset=0, episodic_life=False, max_episode_steps=None):
        self.games = [HostGame(g, seed=seed, env_id=env_offset + n, episodic_life=episodic_life,
                               max_episode_steps=max_episode_steps) for n, g in enumerate(games)]
        N = len(self.games)
        self.stacks = np.stack([np.repeat(g.reset(), 4, axis=-1) for g in self.games])
        self.done = np.zeros(N, np.uint8)
        self.total = np.zeros(N, np.float32)
        self.events = [dict(brick=0, life=0, terminal=0, reset=0, life_cut=0, restack=0, truncation=0, game_over=0)
                       for _ in range(N)]

    def step(self, actions):
        N = len(self.games)
        rew, term, trunc = np.zeros(N, np.float32), np.zeros(N, np.uint8), np.zeros(N, np.uint8)
        ep = np.full(N, NAN_BITS, np.uint32)
        for n, g in enumerate(self.games):
            ev = self.events[n]
            if self.done[n]:
                self.stacks[n] = np.repeat(g.reset(), 4, axis=-1)
                if self.done[n] == 1:
                    self.total[n] = 0
                    ev['reset'] += 1
                else:
                    ev['restack'] += 1
            lives = g.lives
            frame, r, t, info = g.step(int(actions[n]))
            over = info.get('game_over', t)
            self.stacks[n] = np.roll(self.stacks[n], -1, axis=-1)
            if t:
                self.stacks[n].fill(0)
            self.stacks[n][..., -1:] = frame
            self.total[n] += np.float32(r)
            rew[n], term[n], trunc[n] = r, t, info.get('truncated', False)
            if over:
                ep[n] = self.total[n:n + 1].view(np.uint32)[0]
            self.done[n] = 1 if over else (2 if t else 0)
            ev['brick'] += r > 0 and g.game == 'breakout'
            ev['life'] += g.lives < lives
            ev['terminal'] += bool(t)
            ev['life_cut'] += bool(t and not over)
            ev['truncation'] += int(trunc[n])
            ev['game_over'] += bool(over)
        return self.stacks.copy(), rew, term, trunc, ep

    def state(self):
        g = self.games
        return (np.array([x.episode for x in g], np.int32), np.array([x.steps for x in g], np.int32),
                np.where(self.done == 1, np.float32(0), self.total).astype(np.float32), self.done.copy(),
                np.stack([x.state for x in g]))


def mixed_steps(games):
    """The shortest prefix of MIXED_ACTIONS whose host trace holds, for every Breakout env,
    a brick hit, a life loss, a terminal and the reset step after it -> (steps, events)."""
    ref = MixedReplay(games, seed=MIXED_SEED, env_offset=MIXED_OFFSET)
    need = ('brick', 'life', 'terminal', 'reset')
    for s in range(MIXED_MAX_STEPS):
        ref.step(MIXED_ACTIONS[s])
        if all(min(ev[k] for k in need) >= 1 for g, ev in zip(games, ref.events) if g == B):
            return s + 1, ref.events
    return None, ref.events


# -- game_pattern -------------------------------------------------------------------------
def test_game_pattern_names_ids_strings_and_sequences():
    gp = host.game_pattern
    assert gp('catch', 3) == (C, C, C) and gp(1, 2) == (B, B) and gp(np.int64(0), 1) == (C,)
    assert gp('catch+breakout', 4) == (C, B, C, B)
    assert gp('breakout+catch', 3) == (B, C, B)
    assert gp('catch+catch+breakout', 4) == (C, C, B, C)
    assert gp('breakout', 0) == () and gp('catch+breakout', 0) == ()
    assert gp([C, 1, 'breakout'], 3) == (C, B, B) and gp((0, 0), 2) == (C, C)
    assert gp(np.array([1, 0]), 2) == (B, C)
    assert all(isinstance(g, str) for g in gp([0, 1], 2))


def test_game_pattern_follows_the_global_env_id():
    gp = host.game_pattern
    assert gp('catch+breakout', 3, env_offset=5) == (B, C, B)
    assert gp('catch+breakout', 3, 4) == (C, B, C)
    whole = gp('catch+catch+breakout', 12)
    for rank in range(4):  # four shards of three envs are the whole batch
        assert gp('catch+catch+breakout', 3, env_offset=3 * rank) == whole[3 * rank:3 * rank + 3]
    assert gp('breakout', 2, env_offset=7) == (B, B)


@pytest.mark.parametrize('bad,n', [('pong', 1), ('catch+pong', 2), ('catch+', 2), ('+catch', 2), ('', 1), ('+', 2),
                                   (2, 1), (-1, 1), ([C], 2), ([C, B, C], 2), ([C, 'pong'], 2), ([C, 2], 2),
                                   (None, 1), (1.5, 1), ({C: 1}, 1), ('Catch', 1)])
def test_game_pattern_errors(bad, n):
    with pytest.raises(ValueError):
        host.game_pattern(bad, n)


def test_game_pattern_leaves_the_registry_alone():
    assert host.GAMES == ('catch', 'breakout') and host.GAME_ACTIONS == {'catch': 3, 'breakout': 4}
    assert host.game_id('catch') == 0 and host.game_id(1) == 1
    with pytest.raises(ValueError):
        host.game_id('pong')
    assert 'Mixed batches' in host.__doc__


# -- the C-ABI ----------------------------------------------------------------------------
def test_new_entry_points_are_declared_bound_and_exported(lib):
    src = open(os.path.join(ROOT, 'include', 'acmi.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(acmi_[a-z0-9_]+)\s*\(', src))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.EXPORTED, name
        assert hasattr(lib, name), name
    # the signatures: games after the state, bad_envs ahead of the stream
    flat = re.sub(r'\s+', ' ', src)
    assert ('int acmi_game_reset_mixed(const acmi_game_state_t* st, const uint8_t* games, int N, int env_offset, '
            'uint32_t seed, uint8_t* obs_out, int64_t out_stride, int32_t* bad_envs, acmi_stream_t stream);') in flat
    assert ('int acmi_game_step_mixed(const acmi_game_state_t* st, const uint8_t* games, '
            'const acmi_game_rules_t* rules, int N, int env_offset, uint32_t seed, const int32_t* actions, '
            'const uint8_t* obs_in, int64_t in_stride, uint8_t* obs_out, int64_t out_stride, float* rewards, '
            'uint8_t* terminals, uint8_t* truncated, float* episode_rewards, int64_t ld, int32_t* bad_envs, '
            'acmi_stream_t stream);') in flat
    assert len(_lib._SIGS['acmi_game_reset_mixed'][1]) == 9 and len(_lib._SIGS['acmi_game_step_mixed'][1]) == 18


def test_game_count_and_actions(lib):
    assert lib.acmi_game_count() == 2 == len(host.GAMES)
    assert [lib.acmi_game_actions(i) for i in range(2)] == [3, 4] == [host.GAME_ACTIONS[g] for g in host.GAMES]
    for bad in (2, -1, 7, 255):
        assert lib.acmi_game_actions(bad) == _lib.ERR_ARG
    assert b'acmi_game_actions' in lib.acmi_last_error()


def test_abi_version_and_struct_sizes_are_unchanged(lib):
    assert lib.acmi_abi_version() == 4
    sizes = (ctypes.c_int64 * 6)()
    assert lib.acmi_abi_struct_sizes(ctypes.cast(sizes, ctypes.c_void_p), 6) == 5
    assert lib.acmi_game_state_bytes() == ctypes.sizeof(_lib.GameState) == 48
    assert ctypes.sizeof(_lib.GameRules) == 8 and lib.acmi_game_state_ints() == 12


def test_mixed_entry_points_argument_errors(lib):
    one = ctypes.c_void_p(16)  # a non-null pointer no call gets as far as using

    def state(game=0, vars_=one):
        return _lib.GameState(one, one, one, one, vars_, game)

    def step(st, rules=(0, 0), games=one, N=1, in_stride=28224, out_stride=28224, ld=1, actions=one, trunc=one,
             bad=one, offset=0):
        r = ctypes.byref(_lib.GameRules(*rules)) if rules is not None else None
        return lib.acmi_game_step_mixed(ctypes.byref(st) if st is not None else None, games, r, N, offset, 0, actions,
                                        one, in_stride, one, out_stride, one, one, trunc, one, ld, bad, None)

    def reset(st, games=one, N=1, stride=28224, obs=one, bad=one, offset=0):
        return lib.acmi_game_reset_mixed(ctypes.byref(st) if st is not None else None, games, N, offset, 0, obs,
                                         stride, bad, None)
    ok = state()
    # the state: null, a null array, st->game invalid even though games is given
    assert step(None) == _lib.ERR_ARG and reset(None) == _lib.ERR_ARG
    for bad in (state(game=2), state(game=-1), state(vars_=None)):
        assert step(bad) == _lib.ERR_ARG and reset(bad) == _lib.ERR_ARG
        assert step(bad, games=None) == _lib.ERR_ARG and reset(bad, games=None) == _lib.ERR_ARG
    assert b'acmi_game_reset_mixed' in lib.acmi_last_error()
    # the rules: required, with acmi_game_step_cuts' checks
    for rules in (None, (0, -1), (0, 2001), (2, 0), (-1, 0)):
        assert step(ok, rules=rules) == _lib.ERR_ARG
        assert step(ok, rules=rules, N=0) == _lib.ERR_ARG  # checked before "nothing to do"
    assert b'acmi_game_step_mixed' in lib.acmi_last_error()
    # strides, ld, counts, pointers
    assert step(ok, in_stride=28224 + 8) == _lib.ERR_ARG and step(ok, out_stride=28208) == _lib.ERR_ARG
    assert step(ok, in_stride=28224 - 16) == _lib.ERR_ARG
    assert step(ok, ld=0) == _lib.ERR_ARG and step(ok, ld=-1) == _lib.ERR_ARG
    assert step(ok, N=-1) == _lib.ERR_ARG and step(ok, offset=-1) == _lib.ERR_ARG
    assert step(ok, actions=None) == _lib.ERR_ARG
    assert reset(ok, N=-1) == _lib.ERR_ARG and reset(ok, offset=-1) == _lib.ERR_ARG
    assert reset(ok, stride=28224 - 16) == _lib.ERR_ARG and reset(ok, stride=28224 + 8) == _lib.ERR_ARG
    assert reset(ok, obs=None) == _lib.ERR_ARG
    # nothing to do is not an error (and launches nothing); games, truncated and bad_envs may be null
    for games in (one, None):
        for bad in (one, None):
            assert reset(ok, games=games, N=0, bad=bad) == 0
            for rules in ((0, 0), (1, 2000), (1, 1)):
                assert step(ok, rules=rules, games=games, N=0, bad=bad) == 0
                assert step(ok, rules=rules, games=games, N=0, bad=bad, trunc=None) == 0


# -- the Python surface ---------------------------------------------------------------------
def test_python_surface_needs_no_gpu():
    from actorcritic.envs import games
    from actorcritic.examples.atari import a2c_acktr
    assert games.game_pattern is host.game_pattern and callable(games.returns_by_game)
    assert 'returns_by_game' in games.__all__ and 'game_pattern' in games.__all__
    assert games.DeviceGameEnvs.fused_step is False
    assert list(inspect.signature(host.game_pattern).parameters) == ['game', 'num_envs', 'env_offset']
    assert inspect.signature(host.game_pattern).parameters['env_offset'].default == 0
    assert list(inspect.signature(games.returns_by_game).parameters) == ['envs', 'returns']
    assert 'env_offset' in inspect.signature(a2c_acktr.create_game_environments).parameters


def test_returns_by_game_on_the_host():
    import torch
    from actorcritic.envs.games import returns_by_game

    class Envs(object):
        num_envs, is_mixed, game = 4, True, 'catch+breakout'
        game_ids = (1, 0, 1, 0)
    r = torch.arange(8.0).reshape(4, 2)
    out = returns_by_game(Envs(), r)
    assert list(out) == ['catch', 'breakout']
    assert out['catch'].tolist() == [[2.0, 3.0], [6.0, 7.0]] and out['breakout'].tolist() == [[0.0, 1.0], [4.0, 5.0]]
    Envs.is_mixed, Envs.game = False, 'breakout'
    assert list(returns_by_game(Envs(), r)) == ['breakout']
    with pytest.raises(ValueError):
        returns_by_game(Envs(), r[:3])


def test_scalar_log_keys_by_game():
    from actorcritic.examples.atari.a2c_acktr import episode_rewards_by_game

    class Envs(object):
        is_mixed, games = True, (C, B, C, B)
    nan = np.nan
    ep = np.array([[nan, 1.0], [nan, nan], [-1.0, nan], [nan, nan]], np.float32)
    out = episode_rewards_by_game(Envs(), ep)
    assert sorted(out) == ['episode_reward/breakout', 'episode_reward/catch']
    assert out['episode_reward/catch'] == 0.0 and np.isnan(out['episode_reward/breakout'])
    ep[3, 1] = 7.0
    assert episode_rewards_by_game(Envs(), ep)['episode_reward/breakout'] == 7.0
    Envs.is_mixed = False
    assert episode_rewards_by_game(Envs(), ep) == {} and episode_rewards_by_game(None, ep) == {}


# -- the replay and the scripts ---------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(MIXED_PATTERNS))
def test_mixed_scripts_cover_the_interesting_steps(name):
    """(host only) every Breakout env of the pattern sees a brick hit, a life loss, a
    terminal and the reset step within the stated steps, the Catch envs several episodes."""
    games, stated = MIXED_PATTERNS[name]
    assert host.game_pattern('catch+breakout', 3, MIXED_OFFSET) == (B, C, B)
    assert MIXED_ACTIONS.min() == -1 and MIXED_ACTIONS.max() == 6  # out-of-range actions included
    S, events = mixed_steps(games)
    assert S is not None and S <= MIXED_MAX_STEPS, events
    assert S == stated, (S, events)
    for g, ev in zip(games, events):
        if g == C:
            assert ev['terminal'] == S // 19 and ev['reset'] == (S - 1) // 19, ev
    if name == 'BCB':
        assert events[1]['terminal'] == 6


def test_an_envs_trace_does_not_depend_on_its_neighbours():
    """The replay of (B, C, B) at offset 5 is, env by env, the single-game replay of that
    env's game at the same global id."""
    S = 60
    mixed = MixedReplay((B, C, B), seed=MIXED_SEED, env_offset=MIXED_OFFSET)
    alone = [MixedReplay((g,), seed=MIXED_SEED, env_offset=MIXED_OFFSET + n) for n, g in enumerate((B, C, B))]
    for s in range(S):
        got = mixed.step(MIXED_ACTIONS[s])
        for n, one in enumerate(alone):
            want = one.step(MIXED_ACTIONS[s, n:n + 1])
            for a, b in zip(got, want):
                assert np.array_equal(a[n:n + 1], b), (s, n)
    for n, one in enumerate(alone):
        for a, b in zip(mixed.state(), one.state()):
            assert np.array_equal(a[n:n + 1], b)


def test_cuts_trace_of_the_mixed_batch_holds_every_kind_of_cut():
    """(host only) the GPU cuts test's run: (B, C, B), episodic life, a 60-step cap."""
    ref = MixedReplay((B, C, B), seed=MIXED_SEED, env_offset=MIXED_OFFSET, episodic_life=True, max_episode_steps=60)
    for s in range(200):
        ref.step(MIXED_ACTIONS[s])
    for kind in ('life_cut', 'restack', 'truncation', 'game_over', 'reset'):
        assert sum(ev[kind] for ev in ref.events) >= 1, (kind, ref.events)
    assert ref.events[1]['life_cut'] == 0 and ref.events[1]['truncation'] == 0  # Catch: one life, 19 steps
