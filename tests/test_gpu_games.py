"""The device games on the GPU: acmi_game_step against the rule book
(HostGame) bit for bit, the env ranges, the rollout through MultiEnvAgent replayed on
the host, evaluate(), and the end-to-end check that A2C learns Catch."""
import math

import numpy as np
import pytest

from actorcritic.envs.games.host import HostGame

pytestmark = pytest.mark.gpu

OBS = 84 * 84 * 4
NAN_BITS = 0x7fc00000
BREAKOUT_SCRIPT_SEED = 3  # (104 steps for N = 1, 124 for N = 3 at env_offset 5)
MAX_BREAKOUT_STEPS = 600

# A2C updates of the learning test: the smallest round number at which three seeds all
# cleared the bar on an MI355X (750: trained +0.44, +0.53, +0.92 against uniform -0.72,
# -0.77, -0.73; at 500 none did), doubled, since learning speed varies with the seed
# (DESIGN.md 7d has the curves)
LEARN_UPDATES = 1500


class HostReplay(object):
    """N HostGame behind the reference's wrappers, restated on arrays: the lazy
    auto-reset, the 4-frame stack (roll, zero-fill on a terminal, reset frame 4x) and
    the episode total.  step(actions) -> what the device must produce."""

    def __init__(self, game, N, seed=0, env_offset=0):
        self.games = [HostGame(game, seed=seed, env_id=env_offset + n) for n in range(N)]
        self.stacks = np.stack([np.repeat(g.reset(), 4, axis=-1) for g in self.games])
        self.done = np.zeros(N, bool)
        self.total = np.zeros(N, np.float32)
        self.events = [dict(brick=0, life=0, terminal=0, reset=0) for _ in range(N)]

    def step(self, actions):
        N = len(self.games)
        rew = np.zeros(N, np.float32)
        term = np.zeros(N, bool)
        ep = np.full(N, NAN_BITS, np.uint32)
        for n, g in enumerate(self.games):
            if self.done[n]:
                self.stacks[n] = np.repeat(g.reset(), 4, axis=-1)
                self.total[n] = 0
                self.events[n]['reset'] += 1
            lives = g.lives
            frame, r, t, _ = g.step(int(actions[n]))
            self.stacks[n] = np.roll(self.stacks[n], -1, axis=-1)
            if t:
                self.stacks[n].fill(0)
            self.stacks[n][..., -1:] = frame
            self.total[n] += np.float32(r)
            rew[n], term[n] = r, t
            if t:
                ep[n] = self.total[n:n + 1].view(np.uint32)[0]
            self.events[n]['brick'] += r > 0 and g.game == 'breakout'
            self.events[n]['life'] += g.lives < lives
            self.events[n]['terminal'] += bool(t)
            self.done[n] = t
        return self.stacks.copy(), rew, term, ep

    def state(self):
        g = self.games
        return (np.array([x.episode for x in g], np.int32), np.array([x.steps for x in g], np.int32),
                np.where(self.done, np.float32(0), self.total).astype(np.float32), self.done.astype(np.uint8),
                np.stack([x.state for x in g]))


def script(game, steps, N, seed):
    """Seeded actions, out-of-range ones (-1 and past the own count) included."""
    own = 3 if game == 'catch' else 4
    return np.random.RandomState(seed).randint(-1, own + 3, size=(steps, N)).astype(np.int32)


def breakout_steps(N, env_offset):
    """The shortest prefix of the breakout script whose host trace holds, for every env,
    a brick hit, a life loss, a terminal and the reset step after it."""
    actions = script('breakout', MAX_BREAKOUT_STEPS, N, BREAKOUT_SCRIPT_SEED)
    ref = HostReplay('breakout', N, seed=11, env_offset=env_offset)
    for s in range(MAX_BREAKOUT_STEPS):
        ref.step(actions[s])
        if all(min(ev.values()) >= 1 for ev in ref.events):
            return s + 1, ref.events
    return None, ref.events


@pytest.mark.parametrize('N,env_offset', [(1, 0), (3, 5)])
def test_breakout_script_covers_the_interesting_steps(N, env_offset):
    """(host only) the script of the bit-exactness test is long enough within the cap."""
    S, events = breakout_steps(N, env_offset)
    assert S is not None and S <= MAX_BREAKOUT_STEPS, events


@pytest.mark.parametrize('layout', ['one_in_place', 'three_in_place', 'three_strided'])
@pytest.mark.parametrize('game', ['catch', 'breakout'])
def test_stepper_matches_the_host_game_bit_for_bit(cuda, game, layout):
    """Per step: the whole stack, reward, terminal, episode reward (the NaN's bits too)
    and the five state arrays.  Strided: two [N, 2, 28224] buffers ping-pong, rewards
    [N, 2]; the slots in between keep their sentinel."""
    import torch
    from actorcritic.envs.games import DeviceGameEnvs
    N, env_offset = (1, 0) if layout == 'one_in_place' else (3, 5)
    strided = layout == 'three_strided'
    if game == 'catch':
        S = 45
    else:
        S, events = breakout_steps(N, env_offset)
        assert S is not None, 'the script covers too little: {}'.format(events)
    actions = script(game, S, N, BREAKOUT_SCRIPT_SEED if game == 'breakout' else 1)
    ref = HostReplay(game, N, seed=11, env_offset=env_offset)
    env = DeviceGameEnvs(game, N, seed=11, env_offset=env_offset, device=cuda)
    k = 2 if strided else 1
    bufs = [torch.full((N, k, OBS), 0xAB, dtype=torch.uint8, device=cuda) for _ in range(k)]
    rew = torch.full((N, k), -7.0, dtype=torch.float32, device=cuda)
    term = torch.full((N, k), 9, dtype=torch.uint8, device=cuda)
    ep = torch.full((N, k), -7.0, dtype=torch.float32, device=cuda)
    env.reset_into(bufs[0].data_ptr(), k * OBS)
    assert np.array_equal(bufs[0][:, 0].cpu().numpy().reshape(N, 84, 84, 4), ref.stacks)
    for a, b in zip(env.state_arrays(), ref.state()):
        assert np.array_equal(a, b)
    dev_actions = torch.from_numpy(actions).to(cuda)
    for s in range(S):
        src, dst = bufs[s % k], bufs[(s + 1) % k]
        env.step_into(dev_actions[s].data_ptr(), src.data_ptr(), k * OBS, dst.data_ptr(), k * OBS, rew.data_ptr(),
                      term.data_ptr(), ep.data_ptr(), k)
        want_obs, want_rew, want_term, want_ep = ref.step(actions[s])
        assert np.array_equal(dst[:, 0].cpu().numpy().reshape(N, 84, 84, 4), want_obs), s
        assert np.array_equal(rew[:, 0].cpu().numpy(), want_rew), s
        assert np.array_equal(term[:, 0].cpu().numpy(), want_term.astype(np.uint8)), s
        assert np.array_equal(ep[:, 0].cpu().numpy().view(np.uint32), want_ep), s
        for a, b in zip(env.state_arrays(), ref.state()):
            assert a.dtype == b.dtype and np.array_equal(a, b), s
    if strided:
        for b in bufs:
            assert bool((b[:, 1] == 0xAB).all())
        assert bool((rew[:, 1] == -7.0).all()) and bool((term[:, 1] == 9).all()) and bool((ep[:, 1] == -7.0).all())
    for ev in ref.events:
        if game == 'catch':
            assert ev['terminal'] == 2 and ev['reset'] == 2
        else:
            assert min(ev.values()) >= 1


def test_env_ranges_equal_the_whole_batch(cuda):
    """step_range_into over the two halves = step_into over all (N = 4, 25 steps)."""
    import torch
    from actorcritic.envs.games import DeviceGameEnvs
    N, S, h = 4, 25, 2
    actions = torch.from_numpy(script('catch', S, N, 2)).to(cuda)
    out = []
    for halves in (False, True):
        env = DeviceGameEnvs('catch', N, seed=4, env_offset=3, device=cuda)
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
    assert out[0][2].sum() == N  # one terminal per env in 25 steps, and the steps after it
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        env.step_range_into(3, 2, 0, 0, OBS, 0, OBS, 0, 0, 0, 1)


def _replay_rollouts(agent, s, ref, rounds, N, T):
    """interact() `rounds` times; every batch equals the host replay of its actions."""
    actions_seen = []
    prev_next = ref.stacks.copy()
    for _ in range(rounds):
        obs, actions, rewards, terminals, next_obs, infos = agent.interact(s)
        obs, actions, next_obs = obs.cpu().numpy(), actions.cpu().numpy(), next_obs.cpu().numpy()
        rewards, terminals = rewards.cpu().numpy(), terminals.cpu().numpy()
        ep = infos.episode_rewards.cpu().numpy().view(np.uint32)
        assert obs.shape == (N, T, 84, 84, 4) and actions.shape == (N, T)
        assert np.array_equal(obs[:, 0], prev_next)
        for t in range(T):
            want_obs, want_rew, want_term, want_ep = ref.step(actions[:, t])
            got = obs[:, t + 1] if t + 1 < T else next_obs
            assert np.array_equal(got, want_obs)
            assert np.array_equal(rewards[:, t], want_rew)
            assert np.array_equal(terminals[:, t], want_term)
            assert np.array_equal(ep[:, t], want_ep)
        prev_next = next_obs
        actions_seen.append(actions)
    return np.concatenate(actions_seen, axis=1)


@pytest.mark.parametrize('masked', [False, True])
def test_rollout_replays_through_the_host_games(cuda, masked):
    """MultiEnvAgent over DeviceGameEnvs('catch', 4), 3 x 5 steps: the batch is what four
    HostGame behind a host frame stack and auto-reset give for the returned actions, on
    the unfused device path.  Under an 18-action head with mask_actions=True no action
    leaves the own set (unmasked, 5 in 6 draws of the fresh policy would)."""
    from actorcritic import session as sess
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.envs.games import DeviceGameEnvs
    from actorcritic.multi_env import MultiEnv
    N, T = 4, 5
    sess.reset_default_graph()
    envs = DeviceGameEnvs('catch', N, num_actions=18 if masked else None, seed=6, device=cuda)
    env = MultiEnv(envs)
    assert env.batched is envs and env.action_space.n == (18 if masked else 3)
    model = AtariModel(env.observation_space, env.action_space, 32, random_seed=3)
    agent = MultiEnvAgent(env, model, T, copy_batches=True, mask_actions=masked)
    ref = HostReplay('catch', N, seed=6)
    with sess.Session() as s:
        actions = _replay_rollouts(agent, s, ref, 3, N, T)
    assert agent._bufs.fused is False and agent._bufs.fuse_steps is False
    assert actions.min() >= 0 and actions.max() < 3
    if masked:
        assert len(np.unique(actions)) > 1


def test_wide_head_without_masks_steps_extra_actions_as_noop(cuda):
    from actorcritic.envs.games import DeviceGameEnvs
    assert DeviceGameEnvs('breakout', 2, num_actions=64, device=cuda).legal_action_masks is None
    m = DeviceGameEnvs('breakout', 2, num_actions=32, device=cuda).legal_action_masks
    assert m.cpu().numpy().tolist() == [15, 15]
    assert DeviceGameEnvs('catch', 1, device=cuda).legal_action_masks.cpu().numpy().tolist() == [7]
    for bad in (2, 65):
        with pytest.raises(ValueError):
            DeviceGameEnvs('catch', 1, num_actions=bad, device=cuda)


def test_evaluate_uniform_counts_the_first_episodes_of_every_env(cuda):
    from actorcritic.envs.games import DeviceGameEnvs, evaluate
    N, E = 8, 4
    envs = DeviceGameEnvs('catch', N, seed=2, device=cuda)
    returns, actions = evaluate(None, envs, E, uniform=True, seed=5, return_actions=True)
    returns, actions = returns.cpu().numpy(), actions.cpu().numpy()
    assert returns.shape == (N, E) and returns.size == 32
    assert set(np.unique(returns)) <= {-1.0, 1.0}
    assert actions.shape == (19 * E, N) and actions.min() >= 0 and actions.max() <= 2
    ref = HostReplay('catch', N, seed=2)
    want = [[] for _ in range(N)]
    for a in actions:
        _, _, term, ep = ref.step(a)
        for n in np.nonzero(term)[0]:
            want[n].append(ep[n:n + 1].view(np.float32)[0])
    assert np.array_equal(returns, np.array(want, np.float32))
    # the same seed draws the same actions
    again = evaluate(None, DeviceGameEnvs('catch', N, seed=2, device=cuda), E, uniform=True, seed=5)
    assert np.array_equal(again.cpu().numpy(), returns)


def test_a2c_learns_catch(cuda):
    """The whole loop -- rollout, targets, loss, backward, RMSProp, next rollout -- makes
    the return go up: after LEARN_UPDATES updates of the example's A2C on 32 envs x 5
    steps, the greedy policy's mean return over 256 episodes beats the uniform policy's
    by more than 4 standard errors of the difference."""
    import torch
    from actorcritic import session as sess
    from actorcritic.envs.games import DeviceGameEnvs, evaluate
    from actorcritic.examples.atari.a2c_acktr import train_a2c_acktr
    sess.reset_default_graph()
    model, _ = train_a2c_acktr(False, 'catch', 32, 5, None, 'catch', max_updates=LEARN_UPDATES, seed=1, game='catch')
    trained = evaluate(model, DeviceGameEnvs('catch', 32, seed=1001, device=cuda), 8, greedy=True).double().flatten()
    random = evaluate(None, DeviceGameEnvs('catch', 32, seed=1001, device=cuda), 8, uniform=True,
                      seed=7).double().flatten()
    assert trained.numel() == random.numel() == 256
    mt, mr = float(trained.mean()), float(random.mean())
    bound = 4.0 * math.sqrt(float(trained.var(unbiased=True)) / 256 + float(random.var(unbiased=True)) / 256)
    print('catch after {} A2C updates: trained {:+.3f}, uniform {:+.3f}, bound {:.3f}'.format(
        LEARN_UPDATES, mt, mr, bound))
    assert torch.isfinite(model.params).all()
    assert mt - mr > bound
