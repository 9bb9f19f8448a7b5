"""Episode statistics on the GPU: acmi_epstats_update against the numpy
restatement (actorcritic.episode_stats.host_episode_stats), the agent's update on every device
rollout path against numpy over the fetched infos and against the envs' own step counters,
and the example loops: the option changes nothing it does not log, logs what the host path
logged, and resumes from a run state bit for bit."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

pytestmark = pytest.mark.gpu

NAN_WORDS = (0x7fc00000, 0xffc00000, 0x7f800001)
GUARD = 64


def _bits(t):
    return t.contiguous().view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


# -- 1. the kernel ------------------------------------------------------------------------------
def _batch(N, T, seed, p=0.4, floats=False):
    """[N][T] f32: about ``p`` of the steps end an episode (integer-valued returns, or floats);
    everywhere else one of the three NaN patterns in turn."""
    rng = np.random.RandomState(seed)
    ret = rng.randn(N, T) * 37.5 if floats else rng.randint(-21, 400, (N, T))
    words = np.array(NAN_WORDS, np.uint32)[rng.randint(0, 3, (N, T))].view(np.float32)
    return np.where(rng.rand(N, T) < p, ret.astype(np.float32), words).astype(np.float32)


def _device_update(lib, ep, grp, G, carry, acc, bad):
    """One acmi_epstats_update on copies with guards behind ws and acc -> (carry, acc, bad) numpy."""
    from actorcritic import _lib
    N, T = ep.shape
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    need = int(lib.acmi_epstats_ws_doubles(N))
    assert need >= 8 * N
    ws = torch.full((need + GUARD,), float('nan'), dtype=torch.float64, device='cuda')
    acc_d = torch.cat([dev(acc).reshape(-1), torch.full((GUARD,), 12345.0, dtype=torch.float64, device='cuda')])
    ep_d, grp_d, carry_d, bad_d = dev(ep), dev(np.asarray(grp, np.uint8)), dev(carry), dev(bad)
    _lib.call('acmi_epstats_update', _lib.ptr(ep_d), _lib.ptr(grp_d), N, T, G, _lib.ptr(carry_d), _lib.ptr(ws),
              _lib.ptr(acc_d), _lib.ptr(bad_d), _lib.stream_handle())
    torch.cuda.synchronize()
    assert torch.isnan(ws[need:]).all() and not torch.isnan(ws[:8 * N]).any()  # written: all of ws[N][8], no more
    assert bool((acc_d[8 * G:] == 12345.0).all())
    assert np.array_equal(ep_d.cpu().numpy().view(np.uint32), ep.view(np.uint32))  # the input is only read
    return carry_d.cpu().numpy(), acc_d[:8 * G].reshape(G, 8).cpu().numpy(), bad_d.cpu().numpy()


SHAPES = [(1, 1, 1), (3, 5, 2), (64, 1, 64), (65, 5, 2), (257, 3, 57)]


@pytest.mark.parametrize('N,T,G', SHAPES, ids=['{}x{}x{}'.format(*s) for s in SHAPES])
def test_kernel_equals_the_oracle_bit_for_bit_over_three_calls(lib, cuda, N, T, G):
    """Integer-valued returns: sums and squares below 2^53 are exact in any order, so all eight
    columns and the carry are the oracle's bytes.  Three successive calls accumulate; the NaN
    patterns are the steppers' 0x7fc00000 and two others; where N >= 3 two envs carry group ids
    >= G (counted once per call each, their carry advancing)."""
    from actorcritic import episode_stats as es
    rng = np.random.RandomState(N)
    grp = rng.randint(0, G, N).astype(np.uint8)
    grp[:min(N, G)] = rng.permutation(G)[:min(N, G)]
    nbad = 0
    if N >= 3:
        grp[1], grp[N - 1], nbad = G, 255, 2
    carry, acc, bad = np.zeros(N, np.int32), es.cleared_acc(G), np.zeros(1, np.int32)
    want_carry, want_acc = carry.copy(), acc.copy()
    seen = set()
    for call in range(3):
        ep = _batch(N, T, seed=100 * N + call, p=0.5 if N == 1 else 0.4)
        seen |= set(ep.view(np.uint32)[es.is_nan_bits(ep)].tolist())
        carry, acc, bad = _device_update(lib, ep, grp, G, carry, acc, bad)
        want_carry, want_acc = es.host_episode_stats(ep, grp, G, want_carry, want_acc)
        assert carry.dtype == np.int32 and np.array_equal(carry, want_carry), call
        assert np.array_equal(acc.view(np.uint64), want_acc.view(np.uint64)), (call, acc, want_acc)
        assert bad.tolist() == [nbad * (call + 1)]
    if N * T >= 15:
        assert seen == set(NAN_WORDS) and want_acc[:, 0].sum() >= 3
    # the same bytes in, the same bytes out
    again = _device_update(lib, ep, grp, G, want_carry * 0, es.cleared_acc(G), np.zeros(1, np.int32))
    once = _device_update(lib, ep, grp, G, want_carry * 0, es.cleared_acc(G), np.zeros(1, np.int32))
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(again, once))


@pytest.mark.parametrize('N,T,G', SHAPES[1:], ids=['{}x{}x{}'.format(*s) for s in SHAPES[1:]])
def test_kernel_with_float_returns_is_within_the_summation_bound(lib, cuda, N, T, G):
    """Columns 1 and 2 within (n - 1) 2^-53 sum|x| of the oracle (n terms x; x^2 for column 2): the
    worst case of a double-precision sum in any order.  The other six columns are exact."""
    from actorcritic import episode_stats as es
    grp = (np.arange(N) % G).astype(np.uint8)
    ep = _batch(N, T, seed=7 * N, p=0.6, floats=True)
    carry0 = np.random.RandomState(N).randint(0, 50, N).astype(np.int32)
    carry, acc, _ = _device_update(lib, ep, grp, G, carry0, es.cleared_acc(G), np.zeros(1, np.int32))
    want_carry, want = es.host_episode_stats(ep, grp, G, carry0)
    assert np.array_equal(carry, want_carry)
    exact = [0, 3, 4, 5, 6, 7]
    assert np.array_equal(acc[:, exact].view(np.uint64), want[:, exact].view(np.uint64))
    samples, _ = es.host_samples(ep, carry0)
    for g in range(G):
        x = np.array([np.float64(r) for n, row in enumerate(samples) if grp[n] == g for r, _ in row])
        assert x.size == want[g, 0]
        for col, terms in ((1, x), (2, x * x)):
            bound = max(x.size - 1, 0) * 2.0 ** -53 * np.abs(terms).sum()
            err = abs(acc[g, col] - want[g, col])
            print('N={} g={} col={} n={} err={:.3e} bound={:.3e}'.format(N, g, col, x.size, err, bound))
            assert err <= bound, (g, col, err, bound)


def test_class_update_moves_to_the_device_and_reads_back(lib, cuda):
    from actorcritic import episode_stats as es
    N, T, G = 65, 5, 2
    grp = (np.arange(N) % G).tolist()
    ep = _batch(N, T, seed=5)
    stats, host = es.EpisodeStats(grp, group_names=('a', 'b')), es.EpisodeStats(grp, group_names=('a', 'b'))
    assert stats.device.type == 'cpu'
    stats.update(torch.from_numpy(ep).cuda())
    stats.update(torch.from_numpy(ep).cuda())
    assert stats.device.type == 'cuda' and stats.length_carry.is_cuda and stats.bad_envs.is_cuda
    host.update(ep)
    host.update(ep)
    assert torch.equal(_bits(stats.acc.cpu()), _bits(host.acc))
    assert torch.equal(stats.length_carry.cpu(), host.length_carry) and int(stats.bad_envs.item()) == 0
    got, want = stats.read(), host.read()
    assert repr(got) == repr(want) and got['all']['episodes'] > 50
    assert torch.equal(_bits(stats.acc.cpu()), _bits(torch.from_numpy(es.cleared_acc(G))))
    assert torch.equal(stats.length_carry.cpu(), host.length_carry)  # read() keeps the carry
    with pytest.raises(ValueError, match='envs'):
        stats.update(torch.zeros((3, 2), device='cuda'))
    sd = stats.state_dict()
    assert all(v.device.type == 'cpu' for v in sd.values() if torch.is_tensor(v))
    stats.load_state_dict(host.state_dict())
    assert stats.acc.is_cuda and torch.equal(stats.acc.cpu(), host.acc)


# -- 2. the rollout paths -------------------------------------------------------------------------
def _rollout_form(monkeypatch, fused=True):
    monkeypatch.setenv('ACMI_ROLLOUT_SPLIT', '0')
    monkeypatch.setenv('ACMI_ROLLOUT_GRAPH', '0')
    monkeypatch.setenv('ACMI_ROLLOUT_FUSED', '1' if fused else '0')
    monkeypatch.setenv('ACMI_ROLLOUT_FUSE_STEPS', '1')


def _agent(benv, T, episode_stats=True):
    from actorcritic import session as sess
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.multi_env import MultiEnv
    sess.reset_default_graph()
    env = MultiEnv(benv)
    model = AtariModel(env.observation_space, env.action_space, 32, random_seed=3, init_seed=1)
    return env, MultiEnvAgent(env, model, T, episode_stats=episode_stats)


def _roll(agent, rollouts, benv=None):
    """``rollouts`` x interact() -> (episode rewards [N][rollouts * T] numpy, the envs' step counters
    after every rollout [N][rollouts] numpy or None); nothing is read from the device until the end."""
    from actorcritic import session as sess
    eps, steps = [], []
    with sess.Session() as s:
        for _ in range(rollouts):
            infos = agent.interact(s)[5]
            eps.append(infos.episode_rewards.clone())
            if benv is not None:
                steps.append(benv._step.clone())
    torch.cuda.synchronize()
    ep = torch.cat(eps, dim=1).cpu().numpy()
    return ep, (torch.stack(steps, dim=1).cpu().numpy() if steps else None)


def _numpy_stats(ep, rows=None):
    """mean / min / max / count of the episode rewards of ``rows`` by plain numpy (float64)."""
    r = (ep if rows is None else ep[rows])
    r = r[~np.isnan(r)].astype(np.float64)
    return dict(episodes=r.size, mean=r.sum() / r.size, min=r.min(), max=r.max())


def _assert_returns(got, want):
    assert got['episodes'] == want['episodes']
    assert (got['mean'], got['min'], got['max']) == (want['mean'], want['min'], want['max'])


def test_catch_on_the_chain(lib, cuda, monkeypatch):
    from actorcritic.envs.games import DeviceGameEnvs
    _rollout_form(monkeypatch)
    env, agent = _agent(DeviceGameEnvs('catch', 4, seed=11), 5)
    ep, _ = _roll(agent, 8)
    stats = agent.episode_stats
    assert stats.device.type == 'cuda' and stats.group_names == ('catch', 'breakout')
    assert stats.length_carry.tolist() == [2] * 4 and int(stats.bad_envs.item()) == 0
    got = stats.read()
    assert got['all']['episodes'] == 8 and got['catch']['episodes'] == 8 and got['breakout']['episodes'] == 0
    assert got['all']['mean_length'] == got['all']['min_length'] == got['all']['max_length'] == 19
    _assert_returns(got['all'], _numpy_stats(ep))
    assert got['all']['std'] == np.sqrt(max(1.0 - got['all']['mean'] ** 2, 0.0))  # returns of +-1
    assert np.isnan(got['breakout']['mean'])


def _cap_run(monkeypatch, fused_step):
    from actorcritic.envs.games import DeviceGameEnvs
    _rollout_form(monkeypatch)
    benv = DeviceGameEnvs('catch+breakout', 4, seed=11, max_episode_steps=7, fused_step=fused_step)
    env, agent = _agent(benv, 5)
    ep, _ = _roll(agent, 3)
    stats = agent.episode_stats
    return ep, stats.acc.cpu().clone(), stats.length_carry.cpu().clone(), stats


def test_step_cap_on_the_chain_and_on_the_fused_step(lib, cuda, monkeypatch):
    """catch+breakout under max_episode_steps=7, 15 steps: every env ends an episode at steps 7 and
    14, so each game has 4 episodes of length 7; the fused step leaves the chain's bytes."""
    ep, acc, carry, stats = _cap_run(monkeypatch, fused_step=False)
    assert carry.tolist() == [1] * 4
    got = stats.read()
    for name, rows in (('catch', [0, 2]), ('breakout', [1, 3])):
        assert got[name]['episodes'] == 4
        assert got[name]['mean_length'] == got[name]['min_length'] == got[name]['max_length'] == 7
        _assert_returns(got[name], _numpy_stats(ep, rows))
    _assert_returns(got['all'], _numpy_stats(ep))
    ep_f, acc_f, carry_f, _ = _cap_run(monkeypatch, fused_step=True)
    assert np.array_equal(ep_f.view(np.uint32), ep.view(np.uint32))
    assert torch.equal(_bits(acc_f), _bits(acc)) and torch.equal(carry_f, carry)


def _assert_lengths_are_the_step_counters(agent, ep, steps, grp, G):
    """T = 1: wherever an episode reward appeared, the sample's length is the env's own step counter
    after that step (the reset is lazy) -- the oracle's samples say so, and the device's
    accumulators are the oracle's over the whole run."""
    from actorcritic import episode_stats as es
    samples, carry = es.host_samples(ep)
    ended = ~np.isnan(ep)
    for n, row in enumerate(samples):
        assert [l for _, l in row] == steps[n][ended[n]].tolist(), n
    stats = agent.episode_stats
    want_carry, want = es.host_episode_stats(ep, grp, G)
    assert torch.equal(_bits(stats.acc.cpu()), _bits(torch.from_numpy(want)))
    assert np.array_equal(stats.length_carry.cpu().numpy(), want_carry)
    lengths = steps[ended].astype(np.float64)
    got = stats.read()['all']
    assert got['episodes'] == lengths.size
    assert (got['mean_length'], got['min_length'], got['max_length']) == (lengths.sum() / lengths.size,
                                                                          lengths.min(), lengths.max())
    return ended


def test_episodic_life_lengths_are_the_envs_step_counters(lib, cuda, monkeypatch):
    """Breakout with episodic_life, rollouts of T = 1: a life-loss terminal produces no sample and
    does not restart the length; a game over produces one whose length is the env's step counter."""
    from actorcritic import session as sess
    from actorcritic.envs.games import DeviceGameEnvs
    _rollout_form(monkeypatch)
    N = 4
    benv = DeviceGameEnvs('breakout', N, seed=11, episodic_life=True)
    env, agent = _agent(benv, 1)
    eps, steps, terms = [], [], []
    with sess.Session() as s:
        for _ in range(150):
            data = agent.interact(s)
            eps.append(data[5].episode_rewards.clone())
            terms.append(data[3].clone())
            steps.append(benv._step.clone())
    torch.cuda.synchronize()
    ep, step = torch.cat(eps, dim=1).cpu().numpy(), torch.stack(steps, dim=1).cpu().numpy()
    term = torch.cat(terms, dim=1).cpu().numpy()
    ended = _assert_lengths_are_the_step_counters(agent, ep, step, [1] * N, 2)
    assert ended.sum() >= 1                     # a game over: the ball is lost at step 20 of a life
    assert (term & ~ended).sum() >= 2           # life-loss terminals: no sample there
    assert not (ended & ~term).any()
    assert step[ended].min() > 40               # a sample spans the lives before it


def test_synthetic_stepper_lengths_are_the_envs_step_counters(lib, cuda, monkeypatch):
    """T = 1 on the synthetic stepper (fused rollout step), until every env has finished an episode
    (its episodes last 50..500 steps)."""
    from actorcritic.envs.atari.wrappers import SyntheticAtariEnvs
    _rollout_form(monkeypatch)
    N = 3
    benv = SyntheticAtariEnvs(N, num_actions=4, seed=5)
    env, agent = _agent(benv, 1)
    ep, step = _roll(agent, 500, benv)
    ended = _assert_lengths_are_the_step_counters(agent, ep, step, [0] * N, 1)
    assert ended.any(axis=1).all()


def test_host_stepped_envs(lib, cuda):
    """HostAtariEnvs over oracle.FakeALE chains (as tests/test_gpu_host_envs.py builds them): the
    update runs after the upload of the pinned episode rewards."""
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import oracle
    from actorcritic import episode_stats as es
    from actorcritic import spaces
    from actorcritic.envs.atari import wrappers

    class ALE(oracle.FakeALE):
        action_space = spaces.Discrete(4)
        observation_space = spaces.Box(low=0, high=255, shape=(210, 160, 3), dtype=np.uint8)

    N, T = 4, 5
    env, agent = _agent(wrappers.HostAtariEnvs([wrappers.wrap_atari_env(ALE(100 + i), preprocess=False)
                                                for i in range(N)]), T)
    try:
        ep, _ = _roll(agent, 8)
    finally:
        env.close()
    stats = agent.episode_stats
    assert stats.num_groups == 1 and stats.device.type == 'cuda'
    want_carry, want = es.host_episode_stats(ep, [0] * N, 1)
    assert torch.equal(_bits(stats.acc.cpu()), _bits(torch.from_numpy(want)))
    assert np.array_equal(stats.length_carry.cpu().numpy(), want_carry)
    got = stats.read()['all']
    assert got['episodes'] >= 1
    _assert_returns(got, _numpy_stats(ep))


def test_graph_and_two_halves_forms_update_once_per_rollout(lib, cuda, monkeypatch):
    """The captured rollout (the update stays outside the graph) and the two-halves form (N = 256:
    the update follows the join of the side stream) leave the one-chain bytes."""
    from actorcritic import episode_stats as es
    from actorcritic.envs.atari.wrappers import SyntheticAtariEnvs
    N, T, rollouts = 256, 2, 4
    results = []
    for split, graph in ((0, 0), (1, 0), (0, 1)):
        _rollout_form(monkeypatch)
        monkeypatch.setenv('ACMI_ROLLOUT_SPLIT', str(split))
        monkeypatch.setenv('ACMI_ROLLOUT_GRAPH', str(graph))
        env, agent = _agent(SyntheticAtariEnvs(N, num_actions=4, seed=5), T)
        ep, _ = _roll(agent, rollouts)
        stats = agent.episode_stats
        want_carry, want = es.host_episode_stats(ep, [0] * N, 1)
        assert torch.equal(_bits(stats.acc.cpu()), _bits(torch.from_numpy(want))), (split, graph)
        assert np.array_equal(stats.length_carry.cpu().numpy(), want_carry)
        results.append(ep)
    assert all(np.array_equal(r.view(np.uint32), results[0].view(np.uint32)) for r in results)
    assert results[0].shape == (N, T * rollouts)


def test_no_statistics_nothing_allocated(lib, cuda, monkeypatch):
    from actorcritic.envs.games import DeviceGameEnvs
    _rollout_form(monkeypatch)
    env, agent = _agent(DeviceGameEnvs('catch', 4, seed=11), 5, episode_stats=None)
    _roll(agent, 1)
    assert agent.episode_stats is None and 'episode_stats' not in agent.run_state()


# -- 3. through the example -----------------------------------------------------------------------
def _train(directory=None, max_updates=6, summary=None, game='catch', **kw):
    from actorcritic import session as sess
    from actorcritic.examples.atari.a2c_acktr import train_a2c_acktr
    sess.reset_default_graph()
    return train_a2c_acktr(False, 'DeviceGame', 4, 5, None if directory is None else str(directory), 'Run',
                           summary_path=None if summary is None else str(summary), max_updates=max_updates, seed=2,
                           game=game, **kw)


def _single_process(monkeypatch):
    _rollout_form(monkeypatch)
    for var in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        monkeypatch.delenv(var, raising=False)


def test_statistics_are_passive(lib, cuda, monkeypatch):
    """Two A2C runs of 6 updates on catch, with and without: bit-identical parameters."""
    _single_process(monkeypatch)
    off, _ = _train(max_updates=6)
    params_off = off.params.clone()
    on, _ = _train(max_updates=6, episode_stats=True)
    assert torch.equal(_bits(on.params), _bits(params_off))


def _lines(directory):
    with open(os.path.join(str(directory), 'scalars.jsonl')) as f:
        return [json.loads(line) for line in f]


def test_log_lines_hold_the_host_paths_episode_reward(lib, cuda, tmp_path, monkeypatch):
    """log_every=1: the interval is one rollout, so float32(episode_reward) of every line is the
    option-off line's (both the correctly rounded quotient of the same two small integers).  The
    other keys of the option-off lines are untouched; the new ones appear with the option only."""
    _single_process(monkeypatch)
    _train(summary=tmp_path / 'off', max_updates=8, log_every=1)
    _train(summary=tmp_path / 'on', max_updates=8, log_every=1, episode_stats=True)
    off, on = _lines(tmp_path / 'off'), _lines(tmp_path / 'on')
    assert len(off) == len(on) == 8
    f32 = lambda v: None if v is None else float(np.float32(v))
    for a, b in zip(off, on):
        assert list(a) == ['step', 'policy_loss', 'baseline_loss', 'policy_entropy', 'episode_reward']
        assert list(b) == list(a) + ['episode_reward_std', 'episode_reward_min', 'episode_reward_max',
                                     'episode_length', 'episode_length_max', 'episodes']
        assert all(a[k] == b[k] for k in ('step', 'policy_loss', 'baseline_loss', 'policy_entropy'))
        assert f32(a['episode_reward']) == f32(b['episode_reward'])
        assert (b['episodes'] == 0) == (b['episode_reward'] is None)
    ended = [b for b in on if b['episodes']]
    assert [b['step'] for b in ended] == [4, 8] and all(b['episodes'] == 4 for b in ended)  # catch: steps 19, 38
    assert all(b['episode_length'] == b['episode_length_max'] == 19 for b in ended)


def test_interval_covers_every_rollout_since_the_last_line(lib, cuda, tmp_path, monkeypatch):
    """log_every=4 on catch+breakout capped at 7 steps: the lines at steps 1, 5 and 9 hold the episodes
    of 1, 4 and 4 rollouts (0, then those that ended at env-steps 7 and 14 with step 21 of the next
    interval: per env (5 + 20) // 7 = 3 and (45 // 7) - 3 = 3)."""
    _single_process(monkeypatch)
    _train(summary=tmp_path / 's', max_updates=9, log_every=4, episode_stats=True, game='catch+breakout',
           max_episode_steps=7)
    lines = _lines(tmp_path / 's')
    assert [l['step'] for l in lines] == [1, 5, 9]
    assert [l['episodes'] for l in lines] == [0, 12, 12]
    assert [l['episodes/catch'] for l in lines] == [0, 6, 6] and [l['episodes/breakout'] for l in lines] == [0, 6, 6]
    assert all(l['episode_length'] == l['episode_length_max'] == l['episode_length/breakout'] == 7 for l in lines[1:])


def test_ppo_example_logs_the_interval(lib, cuda, tmp_path, monkeypatch):
    from actorcritic import session as sess
    from actorcritic.examples.atari.ppo import train_ppo
    _single_process(monkeypatch)
    sess.reset_default_graph()
    train_ppo('DeviceGame', 4, 5, None, 'Run', summary_path=str(tmp_path), max_updates=4, seed=2, log_every=1,
              num_epochs=2, num_minibatches=2, game='catch', episode_stats=True)
    lines = _lines(tmp_path)
    assert [l['step'] for l in lines] == [1, 2, 3, 4] and [l['episodes'] for l in lines] == [0, 0, 0, 4]
    assert list(lines[3])[:8] == ['step', 'policy_loss', 'baseline_loss', 'policy_entropy', 'approx_kl',
                                  'clip_fraction', 'episode_reward', 'episode_reward_std']
    assert lines[3]['episode_length'] == 19 and lines[0]['episode_reward'] is None
    assert -1.0 <= lines[3]['episode_reward_min'] <= lines[3]['episode_reward'] <= lines[3]['episode_reward_max'] <= 1.0


def _load(path):
    return torch.load(str(path), map_location='cpu', weights_only=True)


def test_resumed_run_reads_the_uninterrupted_runs_statistics(lib, cuda, tmp_path, monkeypatch):
    """2 + 2 updates of catch+breakout capped at 7 steps with a run-state checkpoint at 2 (env-step 10:
    every env is 3 steps into its second episode): the resumed run's accumulators and length carry
    at step 4 are the straight run's bytes, with the episode that ran across the cut at length 7."""
    from actorcritic import episode_stats as es
    _single_process(monkeypatch)
    straight, cut = tmp_path / 'straight', tmp_path / 'cut'
    straight.mkdir()
    cut.mkdir()
    opts = dict(run_state=True, checkpoint_every=2, episode_stats=True, game='catch+breakout', max_episode_steps=7)
    _train(straight, 4, **opts)
    _train(cut, 2, **opts)
    mid = _load(cut / 'Run-2.run0.pt')['episode_stats']
    assert set(mid) == {'acc', 'length_carry', 'num_groups', 'groups'}
    assert mid['length_carry'].tolist() == [3] * 4 and mid['acc'][:, 0].tolist() == [2.0, 2.0]
    _train(cut, 2, **opts)  # resumes
    a, b = _load(straight / 'Run-4.run0.pt')['episode_stats'], _load(cut / 'Run-4.run0.pt')['episode_stats']
    for k in ('acc', 'length_carry', 'groups'):
        assert a[k].dtype == b[k].dtype and torch.equal(_bits(a[k]), _bits(b[k])), k
    assert a['num_groups'] == b['num_groups'] == 2
    assert b['acc'][:, 0].tolist() == [4.0, 4.0] and b['acc'][:, 3].tolist() == [28.0, 28.0]  # 4 episodes x 7 steps
    assert b['acc'][:, 6].tolist() == [7.0, 7.0] and b['acc'][:, 7].tolist() == [-7.0, -7.0]
    assert b['length_carry'].tolist() == [6] * 4
    # the next read of both is the same log line
    ra, rb = es.EpisodeStats([0, 1, 0, 1], group_names=('catch', 'breakout')), \
        es.EpisodeStats([0, 1, 0, 1], group_names=('catch', 'breakout'))
    ra.load_state_dict(a)
    rb.load_state_dict(b)
    assert repr(ra.log_scalars(ra.read())) == repr(rb.log_scalars(rb.read()))
    # a run state written without statistics is refused, not silently restarted
    bare = tmp_path / 'bare'
    bare.mkdir()
    _train(bare, 2, **dict(opts, episode_stats=False))
    assert 'episode_stats' not in _load(bare / 'Run-2.run0.pt')
    with pytest.raises(ValueError, match='episode_stats'):
        _train(bare, 2, **opts)
