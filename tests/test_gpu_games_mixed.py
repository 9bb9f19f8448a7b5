"""Mixed device-game batches on the GPU ("Mixed batches"): Catch and Breakout
envs side by side under one launch of the stepper, against the rule book (HostGame per env)
bit for bit; the identity of acmi_game_*_mixed with the old entry points on one-game
batches; cuts, env ranges, the rollout (masked and not), evaluate(), the bad-id
contract, and the end-to-end check that A2C on the mixed batch learns Catch."""
import ctypes
import math

import numpy as np
import pytest

from actorcritic import _lib
from actorcritic.envs.games.host import GAME_ACTIONS, HostGame, game_id

pytestmark = pytest.mark.gpu

OBS = 84 * 84 * 4
NAN_BITS = 0x7fc00000
B, C = 'breakout', 'catch'
MIXED_SEED, MIXED_OFFSET, MIXED_MAX_STEPS = 11, 5, 600
MIXED_ACTIONS = np.random.RandomState(3).randint(-1, 7, size=(MIXED_MAX_STEPS, 3)).astype(np.int32)
# the seed of the masked rollout test's model: with it a Breakout env draws action 3
# within the 15 steps on an MI355X (the draw is deterministic in the seed)
MASKED_MODEL_SEED = 3

# A2C updates of the learning test, by the rule of tests/test_gpu_games.py: the smallest
# multiple of 250 at which three seeds all cleared the bar on Catch when trained on 16 Catch
# + 16 Breakout envs on an MI355X (1000: trained +0.47, -0.20, +0.36 against uniform -0.72,
# -0.77, -0.73 with bounds 0.28-0.30; at 750 seeds 2 and 3 did not: -0.65, -0.64), doubled
# ("Mixed batches", has the curves)
MIXED_LEARN_UPDATES = 2000


class MixedReplay(object):
    """N HostGame of per-env games (with or without cuts) behind the lazy auto-reset, the
    4-frame stack (roll, zero-fill on a terminal, the reset frame 4x) and the whole-game
    episode total, restated on arrays: step(actions) -> what the device must produce.
    done holds the stepper's codes (0 running, 1 game over, 2 life lost)."""

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
    a brick hit, a life loss, a terminal and the reset step after it (124 for (B, C, B),
    104 for (C, B, C): tests/test_games_mixed_host.py pins them)."""
    ref = MixedReplay(games, seed=MIXED_SEED, env_offset=MIXED_OFFSET)
    for s in range(MIXED_MAX_STEPS):
        ref.step(MIXED_ACTIONS[s])
        if all(min(ev[k] for k in ('brick', 'life', 'terminal', 'reset')) >= 1
               for g, ev in zip(games, ref.events) if g == B):
            return s + 1
    return None


def _assert_state(env, ref, s):
    for a, b in zip(env.state_arrays(), ref.state()):
        assert a.dtype == b.dtype and np.array_equal(a, b), s


# -- the stepper ----------------------------------------------------------------------------
@pytest.mark.parametrize('games,layout', [((B, C, B), 'in_place'), ((C, B, C), 'in_place'), ((B, C, B), 'strided')])
def test_mixed_stepper_matches_the_host_games_bit_for_bit(cuda, games, layout):
    """Per step: the whole stack, reward, terminal, the episode reward by its bits (the
    NaN's too) and the five state arrays, at env_offset 5.  Strided: two [N, 2, 28224]
    buffers ping-pong, the per-step outputs [N, 2]; the slots in between keep their
    sentinel."""
    import torch
    from actorcritic.envs.games import DeviceGameEnvs
    N, strided = 3, layout == 'strided'
    S = mixed_steps(games)
    assert S is not None and S <= MIXED_MAX_STEPS
    ref = MixedReplay(games, seed=MIXED_SEED, env_offset=MIXED_OFFSET)
    spelled = 'catch+breakout' if games == (B, C, B) else list(games)  # (offset 5: the pattern starts with breakout)
    env = DeviceGameEnvs(spelled, N, seed=MIXED_SEED, env_offset=MIXED_OFFSET, device=cuda)
    assert env.is_mixed and env.games == games and env.game == 'catch+breakout' and env.game_id is None
    assert env.emits_truncations is False and env.fused_step is False
    k = 2 if strided else 1
    bufs = [torch.full((N, k, OBS), 0xAB, dtype=torch.uint8, device=cuda) for _ in range(k)]
    rew = torch.full((N, k), -7.0, dtype=torch.float32, device=cuda)
    term = torch.full((N, k), 9, dtype=torch.uint8, device=cuda)
    ep = torch.full((N, k), -7.0, dtype=torch.float32, device=cuda)
    env.reset_into(bufs[0].data_ptr(), k * OBS)
    assert np.array_equal(bufs[0][:, 0].cpu().numpy().reshape(N, 84, 84, 4), ref.stacks)
    _assert_state(env, ref, -1)
    dev_actions = torch.from_numpy(MIXED_ACTIONS[:S]).to(cuda)
    for s in range(S):
        src, dst = bufs[s % k], bufs[(s + 1) % k]
        env.step_into(dev_actions[s].data_ptr(), src.data_ptr(), k * OBS, dst.data_ptr(), k * OBS, rew.data_ptr(),
                      term.data_ptr(), ep.data_ptr(), k)
        want_obs, want_rew, want_term, _, want_ep = ref.step(MIXED_ACTIONS[s])
        assert np.array_equal(dst[:, 0].cpu().numpy().reshape(N, 84, 84, 4), want_obs), s
        assert np.array_equal(rew[:, 0].cpu().numpy(), want_rew), s
        assert np.array_equal(term[:, 0].cpu().numpy(), want_term), s
        assert np.array_equal(ep[:, 0].cpu().numpy().view(np.uint32), want_ep), s
        _assert_state(env, ref, s)
    if strided:
        for b in bufs:
            assert bool((b[:, 1] == 0xAB).all())
        assert bool((rew[:, 1] == -7.0).all()) and bool((term[:, 1] == 9).all()) and bool((ep[:, 1] == -7.0).all())
    for g, ev in zip(games, ref.events):
        if g == B:
            assert min(ev['brick'], ev['life'], ev['terminal'], ev['reset']) >= 1
        else:
            assert ev['terminal'] == S // 19 >= 5
    assert int(env.bad_envs.item()) == 0


def _drive(cuda, game, N, S, actions, entry):
    """The trace of a one-game batch (seed 11, offset 5) under one entry point: 'old' (acmi_game_reset /
    acmi_game_step through DeviceGameEnvs), 'games' (the mixed entry points with an all-one-game array)
    or 'null' (the mixed entry points with games = NULL and st->game)."""
    import torch
    from actorcritic.envs.games import DeviceGameEnvs
    env = DeviceGameEnvs(game, N, seed=11, env_offset=5, device=cuda)
    assert env.is_mixed is False and not hasattr(env, 'games_tensor') and env.game == game
    ids = torch.full((N,), game_id(game), dtype=torch.uint8, device=cuda)
    gp = None if entry == 'null' else _lib.ptr(ids)
    # with an array the state's own id is ignored: give it the other game's
    st = env.state if entry != 'games' else _lib.GameState(env.state.episode, env.state.step, env.state.total,
                                                           env.state.done, env.state.vars, 1 - game_id(game))
    rules = _lib.GameRules(0, 0)
    bad = torch.zeros(1, dtype=torch.int32, device=cuda)
    obs = torch.full((N, OBS), 0xAB, dtype=torch.uint8, device=cuda)
    rew = torch.zeros((S, N), dtype=torch.float32, device=cuda)
    term = torch.zeros((S, N), dtype=torch.uint8, device=cuda)
    ep = torch.zeros((S, N), dtype=torch.float32, device=cuda)
    stream = _lib.stream_handle(cuda)
    if entry == 'old':
        env.reset_into(obs.data_ptr())
    else:
        _lib.call('acmi_game_reset_mixed', ctypes.byref(st), gp, N, env.env_offset, env.seed, _lib.ptr(obs), OBS,
                  _lib.ptr(bad), stream)
    trace = [obs.clone()]
    first_state = env.state_arrays()
    for s in range(S):
        if entry == 'old':
            env.step_into(actions[s].data_ptr(), obs.data_ptr(), OBS, obs.data_ptr(), OBS, rew[s].data_ptr(),
                          term[s].data_ptr(), ep[s].data_ptr(), 1)
        else:
            _lib.call('acmi_game_step_mixed', ctypes.byref(st), gp, ctypes.byref(rules), N, env.env_offset, env.seed,
                      _lib.ptr(actions[s]), _lib.ptr(obs), OBS, _lib.ptr(obs), OBS, _lib.ptr(rew[s]),
                      _lib.ptr(term[s]), None, _lib.ptr(ep[s]), 1, _lib.ptr(bad), stream)
        trace.append(obs.clone())
    assert int(bad.item()) == 0
    return [torch.stack(trace).cpu().numpy(), rew.cpu().numpy(), term.cpu().numpy(),
            ep.cpu().numpy().view(np.uint32)] + list(first_state) + list(env.state_arrays())


@pytest.mark.parametrize('game', [C, B])
def test_one_game_through_the_mixed_entry_points_is_todays_bytes(cuda, game):
    """A games array that is all one game, and NULL games with st->game, through
    acmi_game_reset_mixed / acmi_game_step_mixed: the bytes of DeviceGameEnvs(<that game>)
    on the old entry points -- reset stack, every step's stack, rewards, terminals, episode
    rewards, state after the reset and at the end.  Catch 45 steps, Breakout the 124-step script."""
    import torch
    N = 3
    S = 45 if game == C else mixed_steps((B, C, B))
    assert S == (45 if game == C else 124)
    actions = torch.from_numpy(MIXED_ACTIONS[:S]).to(cuda)
    want = _drive(cuda, game, N, S, actions, 'old')
    assert want[2].sum() >= (2 * N if game == C else 1)
    for entry in ('games', 'null'):
        got = _drive(cuda, game, N, S, actions, entry)
        for a, b in zip(want, got):
            assert a.dtype == b.dtype and np.array_equal(a, b), entry


def test_cuts_in_a_mixed_batch(cuda):
    """(B, C, B) at offset 5, episodic life under a 60-step cap, 200 steps: stacks, rewards,
    terminals, truncations, episode rewards and the state with its done codes are those of
    HostGame(..., episodic_life, max_episode_steps) behind the wrappers, per env."""
    import torch
    from actorcritic.envs.games import DeviceGameEnvs
    games, N, S = (B, C, B), 3, 200
    rules = dict(episodic_life=True, max_episode_steps=60)
    probe = MixedReplay(games, seed=MIXED_SEED, env_offset=MIXED_OFFSET, **rules)
    for s in range(S):
        probe.step(MIXED_ACTIONS[s])
    for kind in ('life_cut', 'truncation', 'game_over'):  # first, on the host: the trace holds them all
        assert sum(ev[kind] for ev in probe.events) >= 1, (kind, probe.events)
    ref = MixedReplay(games, seed=MIXED_SEED, env_offset=MIXED_OFFSET, **rules)
    env = DeviceGameEnvs(games, N, seed=MIXED_SEED, env_offset=MIXED_OFFSET, device=cuda, **rules)
    assert env.is_mixed and env.emits_truncations is True
    obs = torch.zeros((N, OBS), dtype=torch.uint8, device=cuda)
    rew = torch.full((N,), -7.0, dtype=torch.float32, device=cuda)
    term = torch.full((N,), 9, dtype=torch.uint8, device=cuda)
    trunc = torch.full((N,), 9, dtype=torch.uint8, device=cuda)
    ep = torch.full((N,), -7.0, dtype=torch.float32, device=cuda)
    env.reset_into(obs.data_ptr())
    dev_actions = torch.from_numpy(MIXED_ACTIONS[:S]).to(cuda)
    for s in range(S):
        env.step_into(dev_actions[s].data_ptr(), obs.data_ptr(), OBS, obs.data_ptr(), OBS, rew.data_ptr(),
                      term.data_ptr(), ep.data_ptr(), 1, trunc_ptr=trunc.data_ptr())
        want_obs, want_rew, want_term, want_trunc, want_ep = ref.step(MIXED_ACTIONS[s])
        assert np.array_equal(obs.cpu().numpy().reshape(N, 84, 84, 4), want_obs), s
        assert np.array_equal(rew.cpu().numpy(), want_rew), s
        assert np.array_equal(term.cpu().numpy(), want_term), s
        assert np.array_equal(trunc.cpu().numpy(), want_trunc), s
        assert np.array_equal(ep.cpu().numpy().view(np.uint32), want_ep), s
        _assert_state(env, ref, s)


def test_env_ranges_of_a_mixed_batch_equal_the_whole_batch(cuda):
    """N = 4 (C, B, B, C), 25 steps: step_range_into over the halves at n0 = 0 and n0 = 2 =
    step_into over all = the host games.  The halves start with different games, so a
    games pointer that did not move with the state would play (C, B) twice."""
    import torch
    from actorcritic.envs.games import DeviceGameEnvs
    N, S, h = 4, 25, 2
    games = (C, B, B, C)  # the halves start with different games
    actions = torch.from_numpy(np.random.RandomState(2).randint(-1, 7, size=(S, N)).astype(np.int32)).to(cuda)
    out = []
    for halves in (False, True):
        env = DeviceGameEnvs(games, N, seed=4, env_offset=3, device=cuda)
        obs = torch.zeros((N, OBS), dtype=torch.uint8, device=cuda)
        rew = torch.zeros((S, N), dtype=torch.float32, device=cuda)
        term = torch.zeros((S, N), dtype=torch.uint8, device=cuda)
        ep = torch.zeros((S, N), dtype=torch.float32, device=cuda)
        env.reset_into(obs.data_ptr())
        trace = []
        for s in range(S):
            p = obs.data_ptr()
            if halves:
                for n0 in (0, h):
                    env.step_range_into(n0, h, actions[s].data_ptr() + 4 * n0, p + n0 * OBS, OBS, p + n0 * OBS, OBS,
                                        rew[s].data_ptr() + 4 * n0, term[s].data_ptr() + n0,
                                        ep[s].data_ptr() + 4 * n0, 1)
            else:
                env.step_into(actions[s].data_ptr(), p, OBS, p, OBS, rew[s].data_ptr(), term[s].data_ptr(),
                              ep[s].data_ptr(), 1)
            trace.append(obs.clone())
        out.append([torch.stack(trace).cpu().numpy(), rew.cpu().numpy(), term.cpu().numpy(),
                    ep.cpu().numpy().view(np.uint32)] + list(env.state_arrays()))
    assert out[0][2][:, [0, 3]].sum() == 2  # one terminal per Catch env in 25 steps
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    # and both are the host games
    ref = MixedReplay(games, seed=4, env_offset=3)
    host_actions = actions.cpu().numpy()
    for s in range(S):
        want_obs, want_rew, _, _, _ = ref.step(host_actions[s])
        assert np.array_equal(out[1][0][s].reshape(N, 84, 84, 4), want_obs) and np.array_equal(out[1][1][s], want_rew)
    with pytest.raises(ValueError):
        env.step_range_into(3, 2, 0, 0, OBS, 0, OBS, 0, 0, 0, 1)


def test_alternating_ranges_of_the_pattern(cuda):
    """The pattern's own layout, (C, B, C, B) in halves of two: equal to the whole batch too."""
    import torch
    from actorcritic.envs.games import DeviceGameEnvs
    N, S, h = 4, 25, 2
    actions = torch.from_numpy(np.random.RandomState(2).randint(-1, 7, size=(S, N)).astype(np.int32)).to(cuda)
    out = []
    for halves in (False, True):
        env = DeviceGameEnvs('catch+breakout', N, seed=4, device=cuda)
        assert env.games == (C, B, C, B)
        obs = torch.zeros((N, OBS), dtype=torch.uint8, device=cuda)
        rew = torch.zeros((S, N), dtype=torch.float32, device=cuda)
        term = torch.zeros((S, N), dtype=torch.uint8, device=cuda)
        ep = torch.zeros((S, N), dtype=torch.float32, device=cuda)
        env.reset_into(obs.data_ptr())
        for s in range(S):
            p = obs.data_ptr()
            for n0, n in ((0, h), (h, h)) if halves else ((0, N),):
                env.step_range_into(n0, n, actions[s].data_ptr() + 4 * n0, p + n0 * OBS, OBS, p + n0 * OBS, OBS,
                                    rew[s].data_ptr() + 4 * n0, term[s].data_ptr() + n0, ep[s].data_ptr() + 4 * n0, 1)
        out.append([obs.cpu().numpy(), rew.cpu().numpy(), term.cpu().numpy(), ep.cpu().numpy().view(np.uint32)] +
                   list(env.state_arrays()))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# -- the rollout ------------------------------------------------------------------------------
@pytest.mark.parametrize('masked', [False, True])
def test_mixed_rollout_replays_through_the_host_games(cuda, masked):
    """MultiEnvAgent over DeviceGameEnvs('catch+breakout', 4), 3 x 5 steps: every batch is
    what the four host games give for the returned actions, on the unfused device path.
    Unmasked under the 4-action head; masked under an 18-action head, where no Catch env
    leaves {0, 1, 2}, no Breakout env leaves {0..3}, and some Breakout env draws action 3
    (which no Catch env may)."""
    from actorcritic import session as sess
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.envs.games import DeviceGameEnvs
    from actorcritic.multi_env import MultiEnv
    N, T, rounds = 4, 5, 3
    games = (C, B, C, B)
    sess.reset_default_graph()
    envs = DeviceGameEnvs('catch+breakout', N, num_actions=18 if masked else None, seed=6, device=cuda)
    assert envs.games == games and envs.num_own_actions == 4 and list(envs.own_action_counts) == [3, 4, 3, 4]
    assert envs.legal_action_masks.cpu().numpy().tolist() == [0b0111, 0b1111, 0b0111, 0b1111]
    env = MultiEnv(envs)
    assert env.batched is envs and env.action_space.n == (18 if masked else 4)
    model = AtariModel(env.observation_space, env.action_space, 32, random_seed=MASKED_MODEL_SEED)
    agent = MultiEnvAgent(env, model, T, copy_batches=True, mask_actions=masked)
    ref = MixedReplay(games, seed=6)
    seen = []
    prev_next = ref.stacks.copy()
    with sess.Session() as s:
        for _ in range(rounds):
            obs, actions, rewards, terminals, next_obs, infos = agent.interact(s)
            obs, actions, next_obs = obs.cpu().numpy(), actions.cpu().numpy(), next_obs.cpu().numpy()
            rewards, terminals = rewards.cpu().numpy(), terminals.cpu().numpy()
            ep = infos.episode_rewards.cpu().numpy().view(np.uint32)
            assert obs.shape == (N, T, 84, 84, 4) and actions.shape == (N, T)
            assert np.array_equal(obs[:, 0], prev_next)
            for t in range(T):
                want_obs, want_rew, want_term, _, want_ep = ref.step(actions[:, t])
                assert np.array_equal(obs[:, t + 1] if t + 1 < T else next_obs, want_obs)
                assert np.array_equal(rewards[:, t], want_rew)
                assert np.array_equal(terminals[:, t], want_term.astype(bool))
                assert np.array_equal(ep[:, t], want_ep)
            prev_next = next_obs
            seen.append(actions)
    assert agent._bufs.fused is False
    actions = np.concatenate(seen, axis=1)
    assert actions.shape == (N, rounds * T) and actions.min() >= 0
    if masked:
        assert actions[[0, 2]].max() <= 2 and actions[[1, 3]].max() <= 3
        print('masked mixed rollout, model seed {}: breakout actions {}'.format(
            MASKED_MODEL_SEED, np.bincount(actions[[1, 3]].ravel(), minlength=4).tolist()))
        assert (actions[[1, 3]] == 3).any()
    else:
        assert actions.max() <= 3


# -- evaluate -----------------------------------------------------------------------------------
def test_evaluate_uniform_on_a_mixed_batch(cuda):
    """N = 4 (C, B, C, B), E = 2, a 100-step cap: the returns are the host replay of the
    returned actions, every env's actions stay in its own set, returns_by_game groups them."""
    from actorcritic.envs.games import DeviceGameEnvs, evaluate, returns_by_game
    N, E = 4, 2
    games = (C, B, C, B)
    envs = DeviceGameEnvs('catch+breakout', N, seed=2, device=cuda, max_episode_steps=100)
    returns, actions = evaluate(None, envs, E, uniform=True, seed=5, return_actions=True)
    by_game = returns_by_game(envs, returns)
    returns, actions = returns.cpu().numpy(), actions.cpu().numpy()
    assert returns.shape == (N, E) and actions.shape[1] == N and actions.shape[0] <= 200
    assert actions.min() >= 0 and actions[:, [0, 2]].max() == 2 and actions[:, [1, 3]].max() == 3
    ref = MixedReplay(games, seed=2, max_episode_steps=100)
    want = [[] for _ in range(N)]
    for a in actions:
        _, _, term, _, ep = ref.step(a)
        for n in np.nonzero(term)[0]:
            want[n].append(ep[n:n + 1].view(np.float32)[0])
    assert all(len(w) >= E for w in want) and min(len(want[1]), len(want[3])) == E
    assert len(want[0]) > E  # the Catch envs played on past their count
    assert np.array_equal(returns, np.array([w[:E] for w in want], np.float32))
    assert list(by_game) == [C, B]
    assert np.array_equal(by_game[C].cpu().numpy(), returns[[0, 2]])
    assert np.array_equal(by_game[B].cpu().numpy(), returns[[1, 3]])


@pytest.mark.parametrize('game', [C, B])
def test_evaluate_uniform_on_one_game_draws_what_it_drew(cuda, game):
    """A single-game batch, however spelled, draws RandomState(seed).randint(0, own, size=N)
    per step: the actions of the commit before mixed batches."""
    from actorcritic.envs.games import DeviceGameEnvs, evaluate, returns_by_game
    N, seed = 4, 5
    envs = DeviceGameEnvs([game] * N, N, seed=2, device=cuda, max_episode_steps=100)
    assert envs.is_mixed is False and envs.game == game and envs.game_id == game_id(game)
    returns, actions = evaluate(None, envs, 1, uniform=True, seed=seed, return_actions=True)
    actions = actions.cpu().numpy()
    rng = np.random.RandomState(seed)
    want = np.stack([rng.randint(0, GAME_ACTIONS[game], size=N) for _ in range(len(actions))])
    assert np.array_equal(actions, want)
    assert list(returns_by_game(envs, returns)) == [game]


def test_evaluate_refuses_masks_of_another_composition(cuda):
    from actorcritic import session as sess
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.envs.games import DeviceGameEnvs, evaluate
    N = 4
    sess.reset_default_graph()
    made_for = DeviceGameEnvs('catch+breakout', N, num_actions=18, seed=1, device=cuda)
    other = DeviceGameEnvs('breakout+catch', N, num_actions=18, seed=1, device=cuda, max_episode_steps=30)
    assert made_for.games == (C, B, C, B) and other.games == (B, C, B, C)
    model = AtariModel(made_for.observation_space, made_for.action_space, 32, random_seed=3)
    model.set_action_masks(made_for.legal_action_masks)
    with pytest.raises(ValueError, match='mixed batch'):
        evaluate(model, other, 1)
    same = DeviceGameEnvs('catch+breakout', N, num_actions=18, seed=9, device=cuda, max_episode_steps=30)
    returns, actions = evaluate(model, same, 1, greedy=False, seed=4, return_actions=True)
    actions = actions.cpu().numpy()
    assert tuple(returns.shape) == (N, 1) and actions[:, [0, 2]].max() <= 2 and actions[:, [1, 3]].max() <= 3


# -- a bad id --------------------------------------------------------------------------------------
def test_a_bad_game_id_is_a_defined_result(cuda):
    """One env, id 7, one step and one reset through the mixed entry points (the Python layer
    never produces such an id): the state is untouched, the stack zero, reward and terminal
    and truncated 0, the episode reward the quiet NaN, and bad_envs counts the env once per
    call."""
    import torch
    from actorcritic.envs.games import DeviceGameEnvs
    env = DeviceGameEnvs(C, 1, seed=3, device=cuda)
    obs = torch.full((1, OBS), 0xAB, dtype=torch.uint8, device=cuda)
    env.reset_into(obs.data_ptr())
    before = env.state_arrays()
    ids = torch.tensor([7], dtype=torch.uint8, device=cuda)
    bad = torch.zeros(1, dtype=torch.int32, device=cuda)
    rew = torch.full((1,), -7.0, dtype=torch.float32, device=cuda)
    term = torch.full((1,), 9, dtype=torch.uint8, device=cuda)
    trunc = torch.full((1,), 9, dtype=torch.uint8, device=cuda)
    ep = torch.full((1,), -7.0, dtype=torch.float32, device=cuda)
    action = torch.ones(1, dtype=torch.int32, device=cuda)
    rules = _lib.GameRules(0, 0)
    stream = _lib.stream_handle(cuda)
    _lib.call('acmi_game_step_mixed', ctypes.byref(env.state), _lib.ptr(ids), ctypes.byref(rules), 1, 0, env.seed,
              _lib.ptr(action), _lib.ptr(obs), OBS, _lib.ptr(obs), OBS, _lib.ptr(rew), _lib.ptr(term),
              _lib.ptr(trunc), _lib.ptr(ep), 1, _lib.ptr(bad), stream)
    assert int(bad.item()) == 1
    assert not obs.any()
    assert rew.item() == 0.0 and term.item() == 0 and trunc.item() == 0
    assert ep.cpu().numpy().view(np.uint32)[0] == NAN_BITS
    for a, b in zip(env.state_arrays(), before):
        assert np.array_equal(a, b)
    obs.fill_(0xAB)
    _lib.call('acmi_game_reset_mixed', ctypes.byref(env.state), _lib.ptr(ids), 1, 0, env.seed, _lib.ptr(obs), OBS,
              _lib.ptr(bad), stream)
    assert int(bad.item()) == 2 and not obs.any()  # (the counter accumulates)
    for a, b in zip(env.state_arrays(), before):
        assert np.array_equal(a, b)


# -- learning -----------------------------------------------------------------------------------------
def test_a2c_on_the_mixed_batch_learns_catch(cuda):
    """The example's A2C on 'catch+breakout' (16 + 16 envs x 5 steps, one unmasked 4-action
    head): after MIXED_LEARN_UPDATES updates the greedy policy, played on a fresh batch of
    Catch alone, beats the uniform policy's mean return over 256 episodes by more than 4
    standard errors of the difference -- the bar of test_a2c_learns_catch.  Breakout's
    progress in the mix is in DESIGN.md, not asserted."""
    import torch
    from actorcritic import session as sess
    from actorcritic.envs.games import DeviceGameEnvs, evaluate
    from actorcritic.examples.atari.a2c_acktr import train_a2c_acktr
    sess.reset_default_graph()
    model, _ = train_a2c_acktr(False, 'catch+breakout', 32, 5, None, 'catch+breakout', max_updates=MIXED_LEARN_UPDATES,
                               seed=1, game='catch+breakout')
    assert model.engine.A == 4 and model.engine.masks is None
    trained = evaluate(model, DeviceGameEnvs('catch', 32, num_actions=4, seed=1001, device=cuda), 8,
                       greedy=True).double().flatten()
    random = evaluate(None, DeviceGameEnvs('catch', 32, seed=1001, device=cuda), 8, uniform=True,
                      seed=7).double().flatten()
    assert trained.numel() == random.numel() == 256
    mt, mr = float(trained.mean()), float(random.mean())
    bound = 4.0 * math.sqrt(float(trained.var(unbiased=True)) / 256 + float(random.var(unbiased=True)) / 256)
    print('catch after {} A2C updates on catch+breakout: trained {:+.3f}, uniform {:+.3f}, bound {:.3f}'.format(
        MIXED_LEARN_UPDATES, mt, mr, bound))
    assert torch.isfinite(model.params).all()
    assert mt - mr > bound
