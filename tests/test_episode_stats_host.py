"""CPU tests of the episode statistics (actorcritic/episode_stats.py): the numpy
restatement host_episode_stats on hand-written cases, its algebra over time, read()'s arithmetic
against numpy over the (ret, len) samples, the C-ABI of acmi_epstats_update (declared, bound,
exported, argument errors), the state_dict round trip, the run-state file, the list path of
MultiEnvAgent, and read() as a collective over two gloo ranks."""
import ctypes
import inspect
import os
import re
import socket
import sys
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from actorcritic import _lib, checkpoint
from actorcritic import episode_stats as es

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('acmi_epstats_ws_doubles', 'acmi_epstats_update')
NAN, INF = np.nan, np.inf


def f32_bits(*words):
    return np.array(words, np.uint32).view(np.float32)


def direct(samples):
    """read()'s dict from a list of (ret, len), by plain numpy."""
    if not samples:
        return dict({k: NAN for k in es.STAT_KEYS}, episodes=0)
    r = np.array([s[0] for s in samples], np.float64)
    l = np.array([s[1] for s in samples], np.float64)
    mean = r.sum() / r.size
    return {'episodes': r.size, 'mean': mean, 'std': np.sqrt(max((r * r).sum() / r.size - mean * mean, 0.0)),
            'min': r.min(), 'max': r.max(), 'mean_length': l.sum() / l.size, 'min_length': l.min(),
            'max_length': l.max()}


def same_stats(got, want):
    assert set(got) == set(want) == set(es.STAT_KEYS)
    assert type(got['episodes']) is int and got['episodes'] == want['episodes']
    for k in es.STAT_KEYS[1:]:
        assert np.array_equal(np.float64(got[k]), np.float64(want[k]), equal_nan=True), (k, got[k], want[k])


def random_batch(N, T, seed, p=0.3):
    """Episode rewards with about ``p`` of the steps ending an episode, integer-valued returns."""
    rng = np.random.RandomState(seed)
    ep = np.where(rng.rand(N, T) < p, rng.randint(-5, 30, (N, T)).astype(np.float32), np.float32(NAN))
    return ep.astype(np.float32)


# -- the oracle on hand-written cases ---------------------------------------------------------
def test_a_row_without_an_episode_only_advances_the_carry():
    carry, acc = es.host_episode_stats(np.full((1, 4), NAN, np.float32), [0], 1)
    assert carry.dtype == np.int32 and carry.tolist() == [4]
    assert acc.dtype == np.float64 and np.array_equal(acc, es.cleared_acc(1))
    assert acc[0].tolist() == [0, 0, 0, 0, -INF, -INF, -INF, -INF]
    carry, acc = es.host_episode_stats(np.full((1, 3), NAN, np.float32), [0], 1, carry, acc)
    assert carry.tolist() == [7] and np.array_equal(acc, es.cleared_acc(1))


def test_a_row_where_every_step_ends_an_episode_has_lengths_of_one():
    carry, acc = es.host_episode_stats(np.array([[2, 3, 5]], np.float32), [0], 1)
    assert carry.tolist() == [0]
    assert acc[0].tolist() == [3, 10, 38, 3, 5, -2, 1, -1]
    # a carry of 6 lengthens the first episode alone
    carry, acc = es.host_episode_stats(np.array([[2, 3, 5]], np.float32), [0], 1, [6])
    assert acc[0].tolist() == [3, 10, 38, 9, 5, -2, 7, -1]


def test_several_episodes_negative_zero_and_infinite_returns():
    ep = np.array([[NAN, -4, NAN, NAN, -0.0, 1, NAN],
                   [INF, NAN, NAN, 2, NAN, NAN, NAN],
                   [NAN, NAN, -INF, NAN, NAN, NAN, 7]], np.float32)
    carry, acc = es.host_episode_stats(ep, [0, 1, 2], 3, [1, 0, 0])
    assert carry.tolist() == [1, 3, 0]
    assert acc[0].tolist() == [3, -3, 17, 7, 1, 4, 3, -1]  # lengths 3 (carry 1 + 2), 3, 1; -0.0 counts as 0
    assert acc[1].tolist() == [2, INF, INF, 4, INF, -2, 3, -1]
    assert acc[2].tolist() == [2, -INF, INF, 7, 7, INF, 4, -3]
    one = es.host_episode_stats(ep, [0, 0, 0], 1)[1]
    assert one[0, 0] == 7 and np.isnan(one[0, 1]) and one[0, 2] == INF  # +inf and -inf in one group
    assert one[0, 4:].tolist() == [INF, INF, 4, -1]


def test_every_nan_payload_means_no_episode():
    nans = f32_bits(0x7fc00000, 0xffc00000, 0x7f800001)
    assert es.is_nan_bits(nans).all()
    assert not es.is_nan_bits(f32_bits(0x7f800000, 0xff800000, 0x7f7fffff, 0x80000000, 0)).any()
    ep = np.stack([nans, f32_bits(0x7f800001, 0x40400000, 0xffc00000)])
    carry, acc = es.host_episode_stats(ep, [0, 0], 1)
    assert carry.tolist() == [3, 1] and acc[0].tolist() == [1, 3, 9, 2, 3, -3, 2, -2]


def test_a_bad_group_id_joins_no_group_and_its_carry_advances():
    ep = np.array([[NAN, 1], [5, NAN], [NAN, 2], [9, NAN]], np.float32)
    carry, acc = es.host_episode_stats(ep, [0, 2, 1, 255], 2)
    assert carry.tolist() == [0, 1, 0, 1]
    keep = [0, 2]
    ref_carry, ref = es.host_episode_stats(ep[keep], [0, 1], 2)
    assert np.array_equal(acc, ref) and acc[:, 0].tolist() == [1, 1]


# -- over time --------------------------------------------------------------------------------
def test_two_calls_over_time_are_one_call_over_the_concatenation():
    N, G = 6, 3
    ep = random_batch(N, 7, seed=1)
    grp = np.arange(N) % G
    c1, a1 = es.host_episode_stats(ep[:, :3], grp, G)
    c2, a2 = es.host_episode_stats(ep[:, 3:], grp, G, c1, a1)
    call, aall = es.host_episode_stats(ep, grp, G)
    assert np.array_equal(c2, call) and np.array_equal(a2, aall) and aall[:, 0].sum() > 4
    # the arguments are not written
    assert np.array_equal(a1, es.host_episode_stats(ep[:, :3], grp, G)[1])


def test_read_resets_the_accumulators_and_keeps_the_carry():
    N, G = 6, 2
    ep = random_batch(N, 9, seed=2, p=0.25)
    grp = (np.arange(N) % G).tolist()
    stats = es.EpisodeStats(grp)
    stats.update(ep[:, :4])
    first, again = stats.read(reset=False), stats.read()
    for name in first:  # (reset=False left everything in place)
        same_stats(again[name], first[name])
    assert torch.equal(stats.acc, torch.from_numpy(es.cleared_acc(G)))
    carry = stats.length_carry.clone()
    assert carry.any()
    stats.update(torch.from_numpy(ep[:, 4:]))  # a CPU tensor takes the host path too
    samples, want_carry = es.host_samples(ep)
    late = [row[int(np.isfinite(ep[n, :4]).sum()):] for n, row in enumerate(samples)]  # those after the read
    got = stats.read()
    assert np.array_equal(stats.length_carry.numpy(), want_carry)
    same_stats(got['all'], direct([s for row in late for s in row]))
    assert any(l > 5 for row in late for _, l in row)  # an episode that ran across the read


# -- read() -----------------------------------------------------------------------------------
def test_read_arithmetic_against_numpy_over_the_samples():
    N, T, G = 9, 40, 3
    rng = np.random.RandomState(3)
    ep = np.where(rng.rand(N, T) < 0.2, (rng.randn(N, T) * 10).astype(np.float32), np.float32(NAN)).astype(np.float32)
    grp = [0, 2, 0, 2, 0, 2, 0, 2, 0]  # group 1 stays empty
    stats = es.EpisodeStats(grp, num_groups=G, group_names=('a', 'empty', 'c'))
    stats.update(ep)
    got = stats.read(reset=False)
    assert list(got) == ['a', 'empty', 'c', 'all']
    samples, _ = es.host_samples(ep)
    by = lambda g: [s for n, row in enumerate(samples) if grp[n] == g for s in row]
    for name, g in (('a', 0), ('c', 2)):
        want = direct(by(g))
        assert got[name]['episodes'] == want['episodes'] > 10
        for k in ('min', 'max', 'mean_length', 'min_length', 'max_length'):
            assert got[name][k] == want[k], (name, k)
        assert abs(got[name]['mean'] - want['mean']) <= 1e-12 * abs(want['mean']) + 1e-12
        assert abs(got[name]['std'] - want['std']) <= 1e-12 * want['std']
    same_stats(got['empty'], direct([]))
    assert got['empty']['episodes'] == 0 and all(np.isnan(got['empty'][k]) for k in es.STAT_KEYS[1:])
    want = direct(by(0) + by(2))
    assert got['all']['episodes'] == want['episodes'] and got['all']['max'] == want['max']
    assert got['all']['min'] == want['min'] and got['all']['max_length'] == want['max_length']
    assert abs(got['all']['mean'] - want['mean']) <= 1e-12 and abs(got['all']['std'] - want['std']) <= 1e-11
    # integer-valued returns: every figure exactly numpy's
    ints = es.EpisodeStats([0, 1, 0, 1])
    ep = random_batch(4, 30, seed=4)
    ints.update(ep)
    s, _ = es.host_samples(ep)
    out = ints.read()
    same_stats(out['0'], direct(s[0] + s[2]))
    same_stats(out['1'], direct(s[1] + s[3]))
    same_stats(out['all'], direct(s[0] + s[1] + s[2] + s[3]))
    # unnamed groups: '0', '1', ...; a variance that rounds below zero is clamped
    const = es.EpisodeStats([0])
    const.update(np.full((1, 3), 0.1, np.float32))
    assert const.read()['all']['std'] >= 0.0


def test_log_scalars_keys():
    stats = es.EpisodeStats([0, 1], group_names=('catch', 'breakout'))
    stats.update(np.array([[NAN, 1.0], [NAN, NAN]], np.float32))
    out = stats.log_scalars(stats.read())
    base = ['episode_reward', 'episode_reward_std', 'episode_reward_min', 'episode_reward_max', 'episode_length',
            'episode_length_max', 'episodes']
    assert list(out) == base + [k + '/catch' for k in base] + [k + '/breakout' for k in base]
    assert out['episode_reward'] == 1.0 and out['episode_length'] == 2.0 and out['episodes'] == 1
    assert out['episodes/breakout'] == 0 and np.isnan(out['episode_reward/breakout'])
    single = es.EpisodeStats([1, 1], num_groups=2, group_names=('catch', 'breakout'))
    assert list(single.log_scalars(single.read())) == base  # one game: no per-game keys
    assert list(es.EpisodeStats([0, 1]).log_scalars(es.EpisodeStats([0, 1]).read())) == base  # no names


@pytest.mark.parametrize('kw', [dict(groups=[]), dict(groups=[0, 2], num_groups=2), dict(groups=[0], num_groups=65),
                                dict(groups=[-1]), dict(groups=[0], group_names=['a', 'b']), dict(groups=[64])])
def test_argument_errors_of_the_class(kw):
    with pytest.raises(ValueError):
        es.EpisodeStats(**kw)


def test_update_refuses_another_number_of_envs():
    with pytest.raises(ValueError, match='envs'):
        es.EpisodeStats([0, 0]).update(np.zeros((3, 2), np.float32))


def test_groups_come_from_return_norm():
    from actorcritic import return_norm
    from actorcritic.envs.games import host
    assert es.groups_for_envs is return_norm.groups_for_envs
    envs = types.SimpleNamespace(num_envs=4, env_game_ids=host.env_game_ids('catch+breakout', 4, 1))
    stats = es.EpisodeStats.for_envs(types.SimpleNamespace(batched=envs))
    assert stats.groups.tolist() == [1, 0, 1, 0] and stats.groups.dtype == torch.uint8
    assert stats.num_groups == 2 and stats.group_names == ('catch', 'breakout')
    assert stats.acc.shape == (2, 8) and stats.acc.dtype == torch.float64
    assert stats.length_carry.shape == (4,) and stats.length_carry.dtype == torch.int32
    assert stats.acc.device.type == 'cpu' and stats.bad_envs.tolist() == [0]


# -- the C-ABI --------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported(lib):
    src = open(os.path.join(ROOT, 'include', 'acmi.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(acmi_[a-z0-9_]+)\s*\(', src))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.EXPORTED, name
        assert hasattr(lib, name), name
    flat = re.sub(r'\s+', ' ', src)
    assert 'int64_t acmi_epstats_ws_doubles(int64_t N);' in flat
    assert ('int acmi_epstats_update(const float* episode_rewards, const uint8_t* groups, int N, int T, int G, '
            'int32_t* length_carry, double* ws, double* acc, int32_t* bad_envs, acmi_stream_t stream);') in flat
    assert len(_lib._SIGS['acmi_epstats_update'][1]) == 10
    assert lib.acmi_abi_version() == 4
    assert lib.acmi_epstats_ws_doubles(1) >= 8 and lib.acmi_epstats_ws_doubles(257) >= 8 * 257


def test_argument_errors_come_before_any_launch(lib):
    one = ctypes.c_void_p(16)  # a non-null pointer no call gets as far as using

    def update(ep=one, grp=one, N=1, T=1, G=1, carry=one, ws=one, acc=one, bad=one):
        return lib.acmi_epstats_update(ep, grp, N, T, G, carry, ws, acc, bad, None)

    for name in ('ep', 'grp', 'carry', 'ws', 'acc'):
        assert update(**{name: None}) == _lib.ERR_ARG, name
    for kw in (dict(N=0), dict(N=-1), dict(T=0), dict(T=-3), dict(G=0), dict(G=65), dict(G=-1), dict(G=255)):
        assert update(**kw) == _lib.ERR_ARG, kw
        assert update(bad=None, **kw) == _lib.ERR_ARG, kw
    assert b'acmi_epstats_update' in lib.acmi_last_error()
    assert lib.acmi_epstats_ws_doubles(0) == 0 and lib.acmi_epstats_ws_doubles(-5) == 0


# -- state ------------------------------------------------------------------------------------
def _filled(groups=(0, 1, 0, 1), **kw):
    stats = es.EpisodeStats(list(groups), **kw)
    stats.update(random_batch(len(groups), 11, seed=6))
    return stats


def test_state_dict_round_trip_and_refusals():
    a = _filled()
    sd = a.state_dict()
    assert set(sd) == {'acc', 'length_carry', 'num_groups', 'groups'} and sd['num_groups'] == 2
    assert all(torch.is_tensor(sd[k]) and sd[k].device.type == 'cpu' for k in ('acc', 'length_carry', 'groups'))
    assert a.length_carry.any() and a.acc[:, 0].sum() > 0
    b = es.EpisodeStats([0, 1, 0, 1])
    b.load_state_dict(sd)
    assert torch.equal(b.acc, a.acc) and torch.equal(b.length_carry, a.length_carry)
    a.reset()  # (copies: what was saved does not follow the object)
    assert sd['acc'][:, 0].sum() > 0 and a.length_carry.any()
    for field, other in (('num_groups', es.EpisodeStats([0, 1, 0, 1], num_groups=3)),
                         ('groups', es.EpisodeStats([1, 0, 1, 0])),
                         ('length_carry', es.EpisodeStats([0, 1, 0, 1, 0])),
                         ('length_carry', es.EpisodeStats([0, 1]))):
        before = other.acc.clone()
        with pytest.raises(ValueError, match=field):
            other.load_state_dict(sd)
        assert torch.equal(other.acc, before) and not other.length_carry.any()


class _Agent(object):
    """What checkpoint.save_run_state / load_run_state touch of a MultiEnvAgent."""

    def __init__(self, stats=None):
        self.episode_stats = stats
        self.loaded = None

    def run_state(self):
        state = {'next_obs': torch.zeros((4, 84, 84, 4), dtype=torch.uint8), 'sample_counter': 12,
                 'env': {'kind': 2, 'num_envs': 4}}
        if self.episode_stats is not None:
            state['episode_stats'] = self.episode_stats.state_dict()
        return state

    def load_run_state(self, state):
        self.loaded = state


def test_run_state_file_carries_the_statistics(tmp_path):
    stats = _filled()
    path = checkpoint.save_run_state(str(tmp_path / 'm'), 7, _Agent(stats))
    blob = torch.load(path, map_location='cpu', weights_only=True)
    assert set(blob['episode_stats']) == {'acc', 'length_carry', 'num_groups', 'groups'}
    agent = _Agent(es.EpisodeStats([0, 1, 0, 1]))
    checkpoint.load_run_state(path, agent)
    assert set(agent.loaded) == {'next_obs', 'sample_counter', 'env', 'episode_stats'}
    agent.episode_stats.load_state_dict(agent.loaded['episode_stats'])
    assert torch.equal(agent.episode_stats.acc, stats.acc)
    assert torch.equal(agent.episode_stats.length_carry, stats.length_carry)
    # an agent without statistics reads the same file as before
    plain = _Agent()
    checkpoint.load_run_state(path, plain)
    assert set(plain.loaded) == {'next_obs', 'sample_counter', 'env'}
    # a file without them for an agent that has them: never a silent reset
    bare = checkpoint.save_run_state(str(tmp_path / 'bare'), 7, _Agent())
    assert 'episode_stats' not in torch.load(bare, map_location='cpu', weights_only=True)
    agent = _Agent(es.EpisodeStats([0, 1, 0, 1]))
    with pytest.raises(ValueError, match='episode_stats'):
        checkpoint.load_run_state(bare, agent)
    assert agent.loaded is None


def test_agent_and_examples_take_the_argument():
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.examples.atari import a2c_acktr, ppo
    assert inspect.signature(MultiEnvAgent.__init__).parameters['episode_stats'].default is None
    for fn in (a2c_acktr.train_a2c_acktr, ppo.train_ppo):
        assert inspect.signature(fn).parameters['episode_stats'].default is False
    from actorcritic import parallel
    assert parallel.allreduce_max_(torch.tensor([1.0, -2.0])).tolist() == [1.0, -2.0]  # one process: untouched
    envs = types.SimpleNamespace(num_envs=2, batched=None)
    assert MultiEnvAgent(envs, None, 5).episode_stats is None
    with pytest.raises(ValueError, match='envs'):
        MultiEnvAgent(envs, None, 5, episode_stats=es.EpisodeStats([0, 0, 0]))
    with pytest.raises(TypeError):
        MultiEnvAgent(envs, None, 5, episode_stats='yes')


# -- the list path ----------------------------------------------------------------------------
def test_list_path_agent_counts_catch_episodes_of_length_19():
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari.wrappers import EpisodeInfoWrapper, FrameStackWrapper
    from actorcritic.envs.games.host import HostGame
    from actorcritic.multi_env import MultiEnv
    N, T = 3, 5
    envs = MultiEnv([FrameStackWrapper(EpisodeInfoWrapper(HostGame('catch', seed=0, env_id=i)), 4) for i in range(N)])
    rng = np.random.RandomState(0)
    model = types.SimpleNamespace(sample_actions=lambda obs, session: rng.randint(0, 3, N).tolist())
    try:
        agent = MultiEnvAgent(envs, model, T, episode_stats=True)
        assert isinstance(agent.episode_stats, es.EpisodeStats) and agent.episode_stats.num_groups == 1
        infos = [agent.interact(None)[5] for _ in range(8)]
    finally:
        envs.close()
    ep = np.concatenate([EpisodeInfoWrapper.get_episode_rewards_from_info_batch(i) for i in infos], axis=1)
    assert ep.shape == (N, 40) and np.isfinite(ep).sum() == 2 * N
    got = agent.episode_stats.read()
    r = ep[np.isfinite(ep)].astype(np.float64)
    assert got['all']['episodes'] == 2 * N and got['all']['mean'] == r.sum() / r.size
    assert got['all']['min'] == r.min() and got['all']['max'] == r.max()
    assert got['all']['mean_length'] == got['all']['min_length'] == got['all']['max_length'] == 19
    assert agent.episode_stats.length_carry.tolist() == [2] * N  # 40 steps = 19 + 19 + 2
    assert list(got) == ['0', 'all']


# -- two ranks ----------------------------------------------------------------------------------
def _two_rank_samples():
    """4 envs x 6 steps; the largest return and the shortest episode on rank 0's envs, the
    smallest return and the longest episode on rank 1's."""
    ep = np.full((4, 6), NAN, np.float32)
    ep[0, 0], ep[0, 3] = 50.0, 2.0   # lengths 1, 3
    ep[1, 4] = 3.0                   # length 5
    ep[2, 5] = -7.0                  # length 6
    ep[3, 2], ep[3, 4] = 4.0, 1.0    # lengths 3, 2
    return ep, [0, 1, 0, 1]


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, os.path.join(ROOT, 'actor-critic_amd'))
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from actorcritic import episode_stats, parallel
    parallel.init_from_env(backend='gloo')
    assert parallel.world_size() == world and parallel.rank() == rank
    ep, grp = _two_rank_samples()
    mine = slice(2 * rank, 2 * rank + 2)
    stats = episode_stats.EpisodeStats(grp[mine], num_groups=2, group_names=('catch', 'breakout'))
    stats.update(ep[mine])
    local = stats.acc.clone()
    got = stats.read(reset=False)
    assert torch.equal(stats.acc, local)  # the all-reduces ran on copies
    again = stats.read()
    assert repr(again) == repr(got) and torch.equal(stats.acc, torch.from_numpy(episode_stats.cleared_acc(2)))
    torch.save(got, os.path.join(out_dir, 'rank{}.pt'.format(rank)))
    parallel.barrier()
    parallel.destroy()


def test_read_over_two_gloo_ranks_is_the_single_process_result(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    ep, grp = _two_rank_samples()
    single = es.EpisodeStats(grp, num_groups=2, group_names=('catch', 'breakout'))
    single.update(ep)
    want = single.read()
    assert (want['all']['max'], want['all']['min']) == (50.0, -7.0)
    assert (want['all']['min_length'], want['all']['max_length'], want['all']['episodes']) == (1.0, 6.0, 6)
    for rank in range(world):
        got = torch.load(str(tmp_path / 'rank{}.pt'.format(rank)))
        assert list(got) == list(want)
        for name in want:
            same_stats(got[name], want[name])
    # the extremes come from different ranks
    halves = []
    for rank in range(world):
        part = es.EpisodeStats(grp[2 * rank:2 * rank + 2], num_groups=2)
        part.update(ep[2 * rank:2 * rank + 2])
        halves.append(part.read()['all'])
    assert halves[0]['max'] == 50.0 and halves[1]['max'] < 50.0 and halves[1]['min'] == -7.0 < halves[0]['min']
    assert halves[0]['min_length'] == 1.0 < halves[1]['min_length'] and halves[1]['max_length'] == 6.0
