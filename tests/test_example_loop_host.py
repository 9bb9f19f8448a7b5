"""The schedule of the examples' training loop, without a GPU.

``train_a2c_acktr`` and ``train_ppo`` run here over fakes (envs, model, agent, objective, optimizer, checkpoint
files, ranks) that append to one trace; the session, the global step, the placeholders and the scalar log are the
real ones.  What is asserted is the order and the conditions of the loop's steps: which updates log, what every
rank must call although rank 0 alone writes, what is saved when, and what a stop request leaves behind.
"""
import importlib
import json
import os
import types

import numpy as np
import pytest

from actorcritic import checkpoint, parallel
from actorcritic import session as sess
from actorcritic.episode_stats import EpisodeStats
from actorcritic.examples.atari import a2c_acktr, ppo
from actorcritic.update_diag import UpdateDiagnostics

try:  # the module of the shared loop, where there is one
    _loop = importlib.import_module('actorcritic.examples.atari.loop')
except ImportError:
    _loop = None
MODULES = [m for m in (a2c_acktr, ppo, _loop) if m is not None]

ALGOS = ('a2c', 'ppo')
FEEDS = ['observations', 'bootstrap_observations', 'actions', 'rewards', 'terminals']
LOSS_KEYS = {'a2c': ['policy_loss', 'baseline_loss', 'policy_entropy'],
             'ppo': ['policy_loss', 'baseline_loss', 'policy_entropy', 'approx_kl', 'clip_fraction']}
LOSS_EVALS = {'a2c': ['eval:policy_loss', 'eval:baseline_loss', 'eval:mean_entropy'],
              'ppo': ['eval:policy_loss', 'eval:baseline_loss', 'eval:mean_entropy', 'eval:approx_kl',
                      'eval:clip_fraction']}


class _Node(sess.Node):
    def __init__(self, h, name, value):
        self.h, self.name, self.value = h, name, value

    def _eval(self, ctx):
        self.h.trace.append('eval:' + self.name)
        return self.value


class _OptimizeOp(sess.Node):
    """One update: the real global step moves by one."""

    def __init__(self, h, global_step):
        self.h, self.global_step = h, global_step

    def _eval(self, ctx):
        self.h.trace.append('eval:optimize')
        self.global_step.assign(self.global_step.value + 1)


class _Stats(EpisodeStats):
    def __init__(self, h, num_envs):
        self.h, self.num_envs = h, num_envs

    def read(self):
        self.h.trace.append('stats.read')
        return 'interval'

    def log_scalars(self, interval):
        assert interval == 'interval'
        return {'episode_reward': 1.5, 'episodes': 2.0}


class _Diag(UpdateDiagnostics):
    def __init__(self, h):
        self.h = h

    def request(self):
        self.h.trace.append('diag.request')

    def read(self):
        self.h.trace.append('diag.read')
        return {'explained_variance': 0.25, 'grad_norm': 2.0}


class Harness(object):
    """The fakes of one run and what they recorded."""

    def __init__(self, monkeypatch, tmp_path, rank=0, world_size=1, latest=None, loaded_step=4, blob_step=4,
                 interrupt_at=None, truncations=None, host_envs=3):
        self.trace, self.runs, self.made, self.on_updates = [], [], {}, []
        self.tmp_path, self.rank = tmp_path, rank
        self.interrupt_at, self.truncations = interrupt_at, truncations
        h = self
        sess.reset_default_graph()

        def patch(name, value):
            """On every module of the examples that has the name."""
            hit = [m for m in MODULES if hasattr(m, name)]
            assert hit, name
            for m in hit:
                monkeypatch.setattr(m, name, value)

        class FakeMultiEnv(object):
            observation_space = action_space = None

            def __init__(self, batched):
                self.batched, self.num_envs = batched, batched.num_envs

            def close(self):
                h.trace.append('env.close')

        def batched(kind):
            def create(*args, **kwargs):
                h.made[kind] = (args, kwargs)
                return types.SimpleNamespace(num_envs=args[1], is_mixed=False)
            return create

        def create_host(env_fns):
            h.made['host'] = ((env_fns,), {})
            return FakeMultiEnv(types.SimpleNamespace(num_envs=host_envs, is_mixed=False))

        class FakeModel(object):
            def __init__(self, observation_space, action_space, conv3_num_filters, random_seed=None):
                h.model = self
                self.conv3_num_filters, self.random_seed = conv3_num_filters, random_seed
                for name in FEEDS + ['truncations']:
                    setattr(self, name + '_placeholder', sess.Placeholder(np.float32, [None], name))

        class FakeAgent(object):
            def __init__(self, multi_env, model, num_steps, mask_actions=False, episode_stats=None):
                h.agent = self
                self.multi_env, self.num_steps, self.mask_actions = multi_env, num_steps, mask_actions
                self.episode_stats = episode_stats
                self.last_truncations = h.truncations
                self.interacts = 0

            def interact(self, session):
                self.interacts += 1
                h.trace.append('interact')
                if self.interacts == h.interrupt_at:
                    raise KeyboardInterrupt
                infos = [[{'episode': {'total_reward': 3.0}}, {}], [{}, {}]]  # one episode ended, of return 3
                return 'obs', 'act', 'rew', 'term', 'next', infos

        class FakeObjective(object):
            def __init__(self, model, **kwargs):
                h.objective, self.kwargs = self, kwargs
                self.diagnostics = kwargs.get('diagnostics')
                self.policy_loss, self.baseline_loss = _Node(h, 'policy_loss', 0.5), _Node(h, 'baseline_loss', 0.25)
                self.mean_entropy = _Node(h, 'mean_entropy', 1.0)
                self.approx_kl, self.clip_fraction = _Node(h, 'approx_kl', 0.125), _Node(h, 'clip_fraction', 0.75)

            def optimize_shared(self, optimizer, **kwargs):
                self.optimize_kwargs = kwargs
                return _OptimizeOp(h, kwargs['global_step'])

        class RecordingSession(sess.Session):
            def __init__(self):
                super(RecordingSession, self).__init__(device='cpu')

            def run(self, fetches, feed_dict=None, host=True):
                h.trace.append('run')
                h.runs.append(dict(fed=[k.name for k in feed_dict], host=host, fetches=len(fetches)))
                return super(RecordingSession, self).run(fetches, feed_dict=feed_dict, host=host)

        class TracedLog(checkpoint.ScalarLog):
            def add(self, step, **scalars):
                h.trace.append('add:{}'.format(step))
                super(TracedLog, self).add(step, **scalars)

            def close(self):
                h.trace.append('log.close')
                super(TracedLog, self).close()

        def load(path, model, optimizer=None, global_step=None, objective=None):
            h.trace.append('load')
            global_step.assign(loaded_step)

        def save(prefix, step, model, optimizer=None, objective=None):
            h.trace.append('save:{}'.format(step))

        def save_run_state(prefix, step, agent, objective=None):
            assert agent is h.agent
            h.trace.append('save_run_state:{}'.format(step))

        def load_run_state(path, agent, objective=None):
            h.trace.append('load_run_state')
            return {'global_step': blob_step}

        patch('MultiEnv', FakeMultiEnv)
        patch('create_environments', batched('synthetic'))
        patch('create_game_environments', batched('game'))
        patch('create_host_environments', create_host)
        patch('AtariModel', FakeModel)
        patch('MultiEnvAgent', FakeAgent)
        patch('A2CObjective', FakeObjective)
        patch('PPOObjective', FakeObjective)
        patch('create_optimizer', lambda *args: 'optimizer')
        patch('Session', RecordingSession)
        monkeypatch.setattr(checkpoint, 'ScalarLog', TracedLog)
        monkeypatch.setattr(checkpoint, 'latest', lambda directory: latest)
        monkeypatch.setattr(checkpoint, 'load', load)
        monkeypatch.setattr(checkpoint, 'save', save)
        monkeypatch.setattr(checkpoint, 'save_run_state', save_run_state)
        monkeypatch.setattr(checkpoint, 'load_run_state', load_run_state)
        monkeypatch.setattr(parallel, 'init_from_env', lambda *args: None)
        monkeypatch.setattr(parallel, 'rank', lambda: rank)
        monkeypatch.setattr(parallel, 'world_size', lambda: world_size)

    def train(self, algo, num_envs=2, num_steps=2, checkpoint_path='ckpt', **kwargs):
        """``checkpoint_path``: under tmp_path, or None; ``summary=True`` for the summary path."""
        if checkpoint_path is not None:
            checkpoint_path = str(self.tmp_path / checkpoint_path)
        if kwargs.pop('summary', False):
            kwargs['summary_path'] = str(self.tmp_path / 'summaries')
        if kwargs.pop('count_updates', True):
            kwargs['on_update'] = lambda n, model: (self.trace.append('on_update:{}'.format(n)),
                                                    self.on_updates.append(model))
        if algo == 'ppo':
            return ppo.train_ppo('Env-v0', num_envs, num_steps, checkpoint_path, 'model', **kwargs)
        return a2c_acktr.train_a2c_acktr(algo == 'acktr', 'Env-v0', num_envs, num_steps, checkpoint_path, 'model',
                                         **kwargs)

    def lines(self):
        with open(str(self.tmp_path / 'summaries' / 'scalars.jsonl')) as f:
            return [json.loads(line) for line in f]

    def only(self, *prefixes):
        return [t for t in self.trace if t.startswith(prefixes)]


def _update(algo, n, log, save=None, run_state=False):
    """The trace of update ``n`` (the step after it)."""
    return (['interact', 'run', 'eval:optimize'] + (LOSS_EVALS[algo] + ['add:{}'.format(n)] if log else [])
            + ['on_update:{}'.format(n)] + (['save_run_state:{}'.format(save)] if save and run_state else [])
            + (['save:{}'.format(save)] if save else []))


# -- 1: a plain run ---------------------------------------------------------------------------
@pytest.mark.parametrize('algo', ALGOS)
def test_plain_run_logs_every_second_update_and_saves_at_even_steps(monkeypatch, tmp_path, algo):
    h = Harness(monkeypatch, tmp_path)
    model, optimizer = h.train(algo, summary=True, log_every=2, checkpoint_every=2, max_updates=5)
    assert model is h.model and optimizer == 'optimizer'
    # log_now is taken from the step BEFORE the update: the lines are those of steps 1, 3, 5
    assert h.trace == (_update(algo, 1, True) + _update(algo, 2, False, save=2) + _update(algo, 3, True)
                       + _update(algo, 4, False, save=4) + _update(algo, 5, True) + ['env.close', 'log.close'])
    assert h.on_updates == [h.model] * 5
    lines = h.lines()
    assert [line['step'] for line in lines] == [1, 3, 5]
    assert list(lines[0]) == ['step'] + LOSS_KEYS[algo] + ['episode_reward']
    assert lines[0]['policy_loss'] == 0.5 and lines[0]['baseline_loss'] == 0.25 and lines[0]['policy_entropy'] == 1.0
    assert lines[0]['episode_reward'] == 3.0  # (the rollout's infos, copied on the rank that writes)
    if algo == 'ppo':
        assert lines[0]['approx_kl'] == 0.125 and lines[0]['clip_fraction'] == 0.75
    # the loss scalars are fetched, and the results copied to the host, on the logging updates alone
    assert [r['host'] for r in h.runs] == [True, False, True, False, True]
    assert [r['fetches'] for r in h.runs] == [3 + len(LOSS_KEYS[algo]), 3] * 2 + [3 + len(LOSS_KEYS[algo])]
    assert all(r['fed'] == FEEDS for r in h.runs)


def test_what_the_algorithms_build(monkeypatch, tmp_path):
    h = Harness(monkeypatch, tmp_path)
    h.train('a2c', max_updates=1, seed=7, mask_actions=True)
    assert (h.model.conv3_num_filters, h.model.random_seed) == (64, 7)
    assert (h.agent.num_steps, h.agent.mask_actions, h.agent.episode_stats) == (2, True, None)
    assert h.objective.kwargs == dict(discount_factor=0.99, entropy_regularization_strength=0.01,
                                      normalize_returns=None, diagnostics=None)
    assert set(h.objective.optimize_kwargs) == {'baseline_loss_weight', 'global_step'}
    h = Harness(monkeypatch, tmp_path)
    h.train('acktr', max_updates=1)
    assert h.model.conv3_num_filters == 32
    h = Harness(monkeypatch, tmp_path)
    h.train('ppo', max_updates=1, seed=7, num_epochs=3, num_minibatches=2, clip_range=0.2, value_clip_range=0.3,
            minibatch='rows')
    assert (h.model.conv3_num_filters, h.model.random_seed) == (64, 7)
    assert h.objective.kwargs == dict(discount_factor=0.99, entropy_regularization_strength=0.01, clip_range=0.2,
                                      value_clip_range=0.3, gae_lambda=0.95, normalize_advantages=True,
                                      normalize_returns=None, diagnostics=None)
    kwargs = dict(h.objective.optimize_kwargs)
    assert kwargs.pop('global_step') is sess.get_or_create_global_step()
    assert kwargs == dict(baseline_loss_weight=0.5, num_epochs=3, num_minibatches=2, shuffle_seed=7, minibatch='rows')


# -- 2: the caller's own objects and no summary path ---------------------------------------------
@pytest.mark.parametrize('algo', ALGOS)
def test_without_a_summary_path_the_loop_never_requests_or_reads(monkeypatch, tmp_path, algo):
    h = Harness(monkeypatch, tmp_path)
    stats, diag = _Stats(h, 2), _Diag(h)
    h.train(algo, log_every=1, max_updates=3, episode_stats=stats, diagnostics=diag)
    assert h.agent.episode_stats is stats and h.objective.diagnostics is diag
    assert h.trace == sum((_update(algo, n, False) for n in (1, 2, 3)), []) + ['env.close']
    assert [r['host'] for r in h.runs] == [False] * 3


# -- 3: episode statistics and diagnostics on rank 0 -------------------------------------------
@pytest.mark.parametrize('algo', ALGOS)
def test_rank0_arms_runs_reads_both_and_writes(monkeypatch, tmp_path, algo):
    h = Harness(monkeypatch, tmp_path)
    h.train(algo, summary=True, log_every=2, max_updates=3, episode_stats=_Stats(h, 2), diagnostics=_Diag(h),
            count_updates=False)
    logging = ['interact', 'diag.request', 'run', 'eval:optimize'] + LOSS_EVALS[algo] + ['diag.read', 'stats.read']
    assert h.trace == (logging + ['add:1'] + ['interact', 'run', 'eval:optimize'] + logging + ['add:3']
                       + ['env.close', 'log.close'])
    assert [r['host'] for r in h.runs] == [True, False, True]
    # loss scalars in list order, then the episode scalars, then the diagnostics
    assert list(h.lines()[0]) == ['step'] + LOSS_KEYS[algo] + ['episode_reward', 'episodes', 'explained_variance',
                                                               'grad_norm']
    assert h.lines()[1]['step'] == 3 and h.lines()[1]['episodes'] == 2.0 and h.lines()[1]['grad_norm'] == 2.0


# -- 4: the same on rank 1 of 2 ------------------------------------------------------------------
@pytest.mark.parametrize('algo', ALGOS)
@pytest.mark.parametrize('run_state', (False, True))
def test_rank1_joins_the_collectives_and_writes_its_run_state_alone(monkeypatch, tmp_path, algo, run_state):
    h = Harness(monkeypatch, tmp_path, rank=1, world_size=2)
    h.train(algo, summary=True, log_every=2, checkpoint_every=2, max_updates=3, episode_stats=_Stats(h, 2),
            diagnostics=_Diag(h), run_state=run_state, count_updates=False)
    logging = ['interact', 'diag.request', 'run', 'eval:optimize', 'diag.read', 'stats.read']
    saves = [['save_run_state:2'], ['save_run_state:3']] if run_state else [[], []]
    assert h.trace == logging + ['interact', 'run', 'eval:optimize'] + saves[0] + logging + saves[1] + ['env.close']
    assert [r['host'] for r in h.runs] == [False] * 3 and [r['fetches'] for r in h.runs] == [3] * 3
    assert not os.path.exists(str(tmp_path / 'summaries' / 'scalars.jsonl'))


# -- 5: run-state pairs ----------------------------------------------------------------------------
@pytest.mark.parametrize('algo', ALGOS)
@pytest.mark.parametrize('max_updates, pairs', [(3, [2, 3]), (4, [2, 4])])
def test_run_state_pairs_at_the_schedule_and_once_at_the_end(monkeypatch, tmp_path, algo, max_updates, pairs):
    h = Harness(monkeypatch, tmp_path)
    h.train(algo, run_state=True, checkpoint_every=2, max_updates=max_updates)
    # every rank's run state BEFORE rank 0's model checkpoint; no second pair for a step already saved
    assert h.only('save') == sum((['save_run_state:{}'.format(s), 'save:{}'.format(s)] for s in pairs), [])
    assert h.trace[-3:] == ['save_run_state:{}'.format(pairs[-1]), 'save:{}'.format(pairs[-1]), 'env.close']


@pytest.mark.parametrize('algo', ALGOS)
def test_without_run_state_the_end_of_the_loop_saves_nothing(monkeypatch, tmp_path, algo):
    h = Harness(monkeypatch, tmp_path)
    h.train(algo, checkpoint_every=2, max_updates=3)
    assert h.only('save') == ['save:2']
    h = Harness(monkeypatch, tmp_path)
    h.train(algo, checkpoint_every=1, max_updates=2, run_state=True, checkpoint_path=None)
    assert h.only('save', 'load') == []


# -- 6: a stop request -----------------------------------------------------------------------------
@pytest.mark.parametrize('algo', ALGOS)
@pytest.mark.parametrize('rank, run_state, saved', [(0, False, ['save:2']), (0, True, []), (1, False, [])])
def test_stop_request_saves_the_model_only_on_rank0_without_run_state(monkeypatch, tmp_path, capsys, algo, rank,
                                                                       run_state, saved):
    h = Harness(monkeypatch, tmp_path, rank=rank, world_size=2, interrupt_at=3)
    h.train(algo, summary=True, run_state=run_state, max_updates=10)
    assert h.only('save') == saved
    assert h.only('on_update') == ['on_update:1', 'on_update:2']
    closes = ['env.close', 'log.close'] if rank == 0 else ['env.close']  # (rank 0 alone has a log)
    assert h.trace[-1 - len(saved) - len(closes):] == ['interact'] + saved + closes
    out = capsys.readouterr().out
    assert 'Stop requested' in out and ('Saved model (step 2)' in out) == bool(saved)


# -- 7: resume -------------------------------------------------------------------------------------
@pytest.mark.parametrize('algo', ALGOS)
@pytest.mark.parametrize('run_state', (False, True))
def test_resume_counts_on_from_the_loaded_step(monkeypatch, tmp_path, capsys, algo, run_state):
    h = Harness(monkeypatch, tmp_path, latest='ckpt/model-4.pt')
    os.makedirs(str(tmp_path / 'ckpt'))
    open(checkpoint.run_state_path(str(tmp_path / 'ckpt' / 'model'), 4, 0), 'w').close()
    h.train(algo, summary=True, log_every=2, checkpoint_every=2, max_updates=2, run_state=run_state)
    rs = ['save_run_state:6'] if run_state else []
    assert h.trace == (['load'] + (['load_run_state'] if run_state else [])
                       + ['interact', 'run', 'eval:optimize'] + LOSS_EVALS[algo] + ['add:5', 'on_update:1']
                       + ['interact', 'run', 'eval:optimize', 'on_update:2'] + rs + ['save:6']
                       + ['env.close', 'log.close'])
    out = capsys.readouterr().out
    assert 'Loaded model' in out and ('Loaded run state' in out) == run_state and 'Saved model (step 6)' in out


@pytest.mark.parametrize('algo', ALGOS)
def test_resume_without_a_checkpoint_starts_at_zero(monkeypatch, tmp_path, capsys, algo):
    h = Harness(monkeypatch, tmp_path, latest=None)
    h.train(algo, max_updates=1, run_state=True)
    assert h.only('load') == [] and h.only('save') == ['save_run_state:1', 'save:1']
    assert 'No model loaded' in capsys.readouterr().out


@pytest.mark.parametrize('algo', ALGOS)
def test_resume_refuses_a_missing_or_foreign_run_state(monkeypatch, tmp_path, algo):
    h = Harness(monkeypatch, tmp_path, latest='ckpt/model-4.pt')
    with pytest.raises(ValueError, match='no run state for rank 0'):
        h.train(algo, max_updates=1, run_state=True)
    assert h.only('load', 'interact') == ['load']
    h = Harness(monkeypatch, tmp_path, latest='ckpt/model-4.pt', blob_step=3)
    os.makedirs(str(tmp_path / 'ckpt'))
    open(checkpoint.run_state_path(str(tmp_path / 'ckpt' / 'model'), 4, 0), 'w').close()
    with pytest.raises(ValueError, match='saved at step 3, the model checkpoint at 4'):
        h.train(algo, max_updates=1, run_state=True)
    assert h.only('load', 'interact') == ['load', 'load_run_state']


# -- 8: truncations --------------------------------------------------------------------------------
@pytest.mark.parametrize('algo', ALGOS)
def test_truncations_are_fed_when_the_agent_has_them(monkeypatch, tmp_path, algo):
    h = Harness(monkeypatch, tmp_path, truncations='cuts')
    h.train(algo, max_updates=2)
    assert [r['fed'] for r in h.runs] == [FEEDS + ['truncations']] * 2
    h = Harness(monkeypatch, tmp_path, truncations=None)
    h.train(algo, max_updates=2)
    assert [r['fed'] for r in h.runs] == [FEEDS] * 2


# -- 9: the choice of envs ---------------------------------------------------------------------------
@pytest.mark.parametrize('algo', ALGOS)
def test_env_choice(monkeypatch, tmp_path, algo):
    h = Harness(monkeypatch, tmp_path)
    h.train(algo, num_envs=6, max_updates=1, seed=3, game='catch+breakout', mask_actions=True, episodic_life=True,
            max_episode_steps=50, fused_games=True)
    assert list(h.made) == ['game']
    assert h.made['game'] == (('catch+breakout', 6), dict(seed=3, full_action_set=True, episodic_life=True,
                                                          max_episode_steps=50, fused_step=True))
    assert h.agent.multi_env.num_envs == 6
    h = Harness(monkeypatch, tmp_path)
    h.train(algo, num_envs=6, max_updates=1, seed=3, mask_actions=True)
    assert list(h.made) == ['synthetic']
    assert h.made['synthetic'] == (('Env-v0', 6), dict(seed=3, full_action_set=True))
    # env_fns: their number (3) replaces num_envs (7): 1e7 / (3 * 1e6) = 3.33 -> four updates, not two
    fns = [object()] * 3
    h = Harness(monkeypatch, tmp_path, host_envs=3)
    h.train(algo, num_envs=7, num_steps=1000000, env_fns=fns)
    assert list(h.made) == ['host'] and h.made['host'][0][0] is fns
    assert h.agent.multi_env.num_envs == 3 and h.only('on_update') == ['on_update:{}'.format(n) for n in (1, 2, 3, 4)]


@pytest.mark.parametrize('algo', ALGOS)
def test_env_arguments_are_checked_before_anything_is_built(monkeypatch, tmp_path, algo):
    for bad in (dict(episodic_life=True), dict(max_episode_steps=5), dict(fused_games=True)):
        h = Harness(monkeypatch, tmp_path)
        with pytest.raises(ValueError, match='need a device game'):
            h.train(algo, max_updates=1, **bad)
        assert h.made == {} and h.trace == []
    h = Harness(monkeypatch, tmp_path)
    with pytest.raises(ValueError, match='checkpoint_every must be at least 1'):
        h.train(algo, max_updates=1, checkpoint_every=0)
    with pytest.raises(ValueError, match='run_state needs device envs'):
        h.train(algo, max_updates=1, run_state=True, env_fns=[object()])
    assert h.made == {} and h.trace == []


# -- 10: the bound of the whole job -------------------------------------------------------------------
def test_a2c_ends_after_ten_million_env_steps(monkeypatch, tmp_path):
    h = Harness(monkeypatch, tmp_path)
    h.train('a2c', num_envs=1000000, num_steps=5, max_updates=None)  # 1e7 / (1e6 * 5) = 2
    assert h.only('on_update') == ['on_update:1', 'on_update:2']
    h = Harness(monkeypatch, tmp_path, world_size=2)  # the bound is the whole job's: two ranks, one update each
    h.train('a2c', num_envs=1000000, num_steps=5, max_updates=None)
    assert h.only('on_update') == ['on_update:1']
