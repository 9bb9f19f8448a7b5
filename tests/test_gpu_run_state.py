"""Run-state checkpoints on the GPU: a run that is saved between two updates
(checkpoint.save + checkpoint.save_run_state), thrown away, rebuilt from the same constructor
arguments and loaded (checkpoint.load, then checkpoint.load_run_state) continues as the
uninterrupted run, bit for bit.

The pattern is one comparison.  Run A does 2K updates straight; run B does K, saves, is
rebuilt, loads and does K more.  After the last update everything is compared with
torch.equal (floats by their bits: episode rewards hold NaN): parameters, optimizer slots
and K-FAC state, every env state array, next_obs and the sample counter, the normaliser's
stats and carry, and the last rollout's actions, rewards, terminals and truncations.  A
straight run is computed once per configuration and shared by the tests that need it.
"""
import os
import socket
import sys
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

pytestmark = pytest.mark.gpu

ENV_SEED = 11


def _case(algo='a2c', game=None, N=4, T=3, K=2, mask=False, norm=False, gs0=None, env_seed=ENV_SEED, **rules):
    return types.SimpleNamespace(algo=algo, game=game, N=N, T=T, K=K, mask=mask, norm=norm, gs0=gs0,
                                 env_seed=env_seed, rules=rules)


MIXED = dict(game='catch+breakout', mask=True, norm=True)
# (breakout-life: a ball that misses the paddle is lost at step 20 of its life (by = 40 + 2*20), the end of
# the fourth of the six T = 5 rollouts -- in the resumed half.  ENV_SEED gave life-loss terminals there.)
CASES = {
    'synthetic': _case(),
    'catch-cap5': _case(game='catch', max_episode_steps=5),
    'breakout-cap5': _case(game='breakout', max_episode_steps=5),
    'breakout-life': _case(game='breakout', T=5, K=3, episodic_life=True),
    'mixed-a2c': _case(**MIXED),
    'mixed-ppo-envs': _case(algo='ppo-envs', **MIXED),
    'mixed-ppo-rows': _case(algo='ppo-rows', **MIXED),
    'catch-acktr': _case(algo='acktr', game='catch', gs0=38),
    'synthetic-65': _case(N=65, T=2, K=1),
    'catch-65': _case(game='catch', N=65, T=2, K=1),
}
GAME_CASES = [k for k, c in CASES.items() if c.game is not None and c.N == 4]


def _rollout_form(monkeypatch, fused):
    """The synthetic stepper's rollout: the fused step with step fusion, or the three-call chain."""
    monkeypatch.setenv('ACMI_ROLLOUT_SPLIT', '0')
    monkeypatch.setenv('ACMI_ROLLOUT_GRAPH', '0')
    monkeypatch.setenv('ACMI_ROLLOUT_FUSED', '1' if fused else '0')
    monkeypatch.setenv('ACMI_ROLLOUT_FUSE_STEPS', '1')


def _build(case, fused_step=False, env_offset=0, device=None):
    """A fresh graph, envs, model, agent, objective and optimizer."""
    from actorcritic import session as sess
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.envs.atari.wrappers import SyntheticAtariEnvs
    from actorcritic.envs.games import DeviceGameEnvs
    from actorcritic.examples.atari import a2c_acktr, ppo
    from actorcritic.multi_env import MultiEnv
    from actorcritic.nn import linear_decay
    from actorcritic.objectives import A2CObjective, PPOObjective
    from actorcritic.return_norm import ReturnNormalizer
    sess.reset_default_graph()
    if case.game is None:
        benv = SyntheticAtariEnvs(case.N, num_actions=4, seed=case.env_seed, env_offset=env_offset, device=device)
    else:
        benv = DeviceGameEnvs(case.game, case.N, num_actions=18 if case.mask else None, seed=case.env_seed,
                              env_offset=env_offset, fused_step=fused_step, device=device, **case.rules)
    env = MultiEnv(benv)
    acktr = case.algo == 'acktr'
    model = AtariModel(env.observation_space, env.action_space, 32 if acktr else 64, random_seed=3, init_seed=1,
                       device=device)
    agent = MultiEnvAgent(env, model, case.T, mask_actions=case.mask)
    norm = ReturnNormalizer.for_envs(env) if case.norm else None
    gs = sess.get_or_create_global_step()
    if case.algo.startswith('ppo'):
        obj = PPOObjective(model, normalize_returns=norm)
        opt = ppo.create_optimizer(2.5e-4)
        op = obj.optimize_shared(opt, 0.5, num_epochs=2, num_minibatches=2, shuffle_seed=9, global_step=gs,
                                 minibatch=case.algo[4:])
    else:
        obj = A2CObjective(model, normalize_returns=norm)
        opt = a2c_acktr.create_optimizer(acktr, model, linear_decay(0.25, 0.025, gs, 1000) if acktr else 7e-4)
        op = obj.optimize_shared(opt, 0.5, global_step=gs)
    if case.gs0 is not None:
        gs.assign(case.gs0)
    return types.SimpleNamespace(benv=benv, env=env, model=model, agent=agent, norm=norm, gs=gs, obj=obj, opt=opt,
                                 op=op, device=device)


def _run(r, updates, log):
    """``updates`` x (rollout, update); per rollout ``log`` gains its terminals, truncations, episode
    rewards, the envs' done codes after it and the K-FAC schedule flags of its update."""
    from actorcritic import session as sess
    with sess.Session(*(() if r.device is None else (r.device,))) as s:
        for _ in range(updates):
            obs, act, rew, term, nxt, infos = r.agent.interact(s)
            feed = {r.model.observations_placeholder: obs, r.model.bootstrap_observations_placeholder: nxt,
                    r.model.actions_placeholder: act, r.model.rewards_placeholder: rew,
                    r.model.terminals_placeholder: term}
            trunc = r.agent.last_truncations
            if trunc is not None:
                feed[r.model.truncations_placeholder] = trunc
            rec = dict(terminals=term.cpu().clone(), truncations=None if trunc is None else trunc.cpu().clone(),
                       done=r.benv._done.cpu().clone())
            s.run(r.op, feed_dict=feed)
            rec['flags'] = getattr(r.opt, 'last_flags', None)
            log.append(rec)
    torch.cuda.synchronize()


def _snapshot(r):
    """Everything the comparison covers, on the host."""
    from actorcritic import checkpoint
    out = {'params': r.model.params.cpu().clone(), 'global_step': int(r.gs.value)}
    for k, v in checkpoint._optimizer_state(r.opt).items():
        out['optimizer/' + k] = v.clone()
    rs = r.agent.run_state()
    out['next_obs'], out['sample_counter'] = rs['next_obs'], rs['sample_counter']
    for k, v in rs['env'].items():
        out['env/' + k] = v
    if r.norm is not None:
        out['retnorm/stats'], out['retnorm/carry'] = r.norm.stats.cpu().clone(), r.norm.carry_state()
    rb = r.agent._bufs
    for k in ('actions', 'rewards', 'terminals', 'truncations', 'episode_rewards'):
        out['rollout/' + k] = getattr(rb, k).cpu().clone()
    return out


def _bits(t):
    if t.is_floating_point():
        return t.contiguous().view({4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def _assert_same(got, want):
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k]
        if torch.is_tensor(w):
            assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(_bits(g), _bits(w)), k
        else:
            assert type(g) is type(w) and g == w, (k, g, w)


_STRAIGHT = {}


def _straight(name, form=None):
    """Run A of a case: 2K updates straight -> (snapshot, log); made once per (case, form)."""
    key = (name, form)
    if key not in _STRAIGHT:
        case = CASES[name]
        r = _build(case, fused_step=bool(form) and case.game is not None)
        log = []
        _run(r, 2 * case.K, log)
        _STRAIGHT[key] = (_snapshot(r), log)
    return _STRAIGHT[key]


def _resumed(name, tmp_path, fused_save=False, fused_resume=False, with_run_state=True, log=None):
    """Run B: K updates, the two saves, everything rebuilt, the two loads, K updates -> snapshot."""
    from actorcritic import checkpoint
    case = CASES[name]
    prefix = str(tmp_path / 'Run')
    r = _build(case, fused_step=fused_save)
    _run(r, case.K, [] if log is None else log)
    step = r.gs.value
    model_path = checkpoint.save(prefix, step, r.model, r.opt, objective=r.obj)
    state_path = checkpoint.save_run_state(prefix, step, r.agent, r.obj)
    assert state_path == checkpoint.run_state_path(prefix, step, 0) and os.path.exists(state_path)
    del r
    r = _build(case, fused_step=fused_resume)
    checkpoint.load(model_path, r.model, r.opt, r.gs, objective=r.obj)
    if with_run_state:
        blob = checkpoint.load_run_state(state_path, r.agent, r.obj)
        assert int(blob['global_step']) == step == r.gs.value
    _run(r, case.K, [] if log is None else log)
    return _snapshot(r)


def _check_events(name, log):
    """The run held what the case is about, on both sides of the save point."""
    case = CASES[name]
    halves = (log[:case.K], log[case.K:])
    if 'max_episode_steps' in case.rules:
        for half in halves:  # every env is capped, truncated and reset on both sides
            assert any(rec['terminals'].any() for rec in half)
            assert any(rec['truncations'].any() for rec in half)
    if case.rules.get('episodic_life'):
        assert any((rec['done'] == 2).any() for rec in log)  # a life-loss terminal (games.hpp: done code 2)
    if case.algo == 'acktr':  # (cold, cov, inv): the resumed half holds a factor-inverse update
        assert [rec['flags'] for rec in halves[1]][0] == (False, True, True)
        assert all(rec['flags'][2] is False for rec in halves[0])


# -- 1. the matrix ------------------------------------------------------------------------------
@pytest.mark.parametrize('fused', [False, True], ids=['three-calls', 'fused-step'])
def test_synthetic_run_resumes_bit_for_bit(lib, cuda, tmp_path, monkeypatch, fused):
    """The synthetic stepper under ACMI_ROLLOUT_FUSED=0 and 1; N = 4 is the split form, whose
    pending area (the tail of the forward workspace) is not saved: nothing stays pending."""
    _rollout_form(monkeypatch, fused)
    want, log = _straight('synthetic', form=fused)
    got = _resumed('synthetic', tmp_path)
    _assert_same(got, want)
    assert got['sample_counter'] == 4 * 3 and got['global_step'] == 4 and len(log) == 4


@pytest.mark.parametrize('fused', [False, True], ids=['three-calls', 'fused-step'])
@pytest.mark.parametrize('name', GAME_CASES)
def test_game_run_resumes_bit_for_bit(lib, cuda, tmp_path, monkeypatch, name, fused):
    """Every game case with fused_step=False and True (N = 4: the split form, so also the proof
    that no game state stays pending between two rollouts: ``_pend`` is not saved)."""
    _rollout_form(monkeypatch, True)
    want, log = _straight(name, form=fused)
    _check_events(name, log)
    got = _resumed(name, tmp_path, fused_save=fused, fused_resume=fused)
    _assert_same(got, want)
    case = CASES[name]
    assert got['global_step'] == (case.gs0 or 0) + 2 * case.K


# -- 2. across the forms ------------------------------------------------------------------------
@pytest.mark.parametrize('fused_save', [True, False], ids=['fused-to-chain', 'chain-to-fused'])
def test_state_saved_under_one_form_resumes_under_the_other(lib, cuda, tmp_path, monkeypatch, fused_save):
    _rollout_form(monkeypatch, True)
    want, _ = _straight('mixed-a2c', form=True)
    got = _resumed('mixed-a2c', tmp_path, fused_save=fused_save, fused_resume=not fused_save)
    _assert_same(got, want)


# -- 3. the one-block form ----------------------------------------------------------------------
@pytest.mark.parametrize('name', ['synthetic-65', 'catch-65'])
def test_one_block_form_resumes_bit_for_bit(lib, cuda, tmp_path, monkeypatch, name):
    """N = 65, just above the split form's bound of 64 (catch: fused_step=True)."""
    _rollout_form(monkeypatch, True)
    want, _ = _straight(name, form=True)
    _assert_same(_resumed(name, tmp_path, fused_save=name == 'catch-65', fused_resume=name == 'catch-65'), want)


# -- 4. teeth -----------------------------------------------------------------------------------
def test_model_checkpoint_alone_does_not_continue_the_run(lib, cuda, tmp_path, monkeypatch):
    """The same comparison without load_run_state: the envs start afresh and the run is another."""
    _rollout_form(monkeypatch, True)
    want, _ = _straight('mixed-a2c', form=False)
    got = _resumed('mixed-a2c', tmp_path, with_run_state=False)
    assert got['global_step'] == want['global_step']
    assert not torch.equal(got['params'], want['params'])
    assert not torch.equal(got['next_obs'], want['next_obs'])
    assert got['sample_counter'] != want['sample_counter']


# -- 5. the env round trip ----------------------------------------------------------------------
def test_env_state_round_trip_through_the_gym_api(lib, cuda):
    """reset() + 3 step() on a mixed batch, state_dict() into a fresh instance: the fourth step
    (the reset after the step-3 truncation) is the same, output by output."""
    from actorcritic.envs.games import DeviceGameEnvs
    make = lambda: DeviceGameEnvs('catch+breakout', 4, seed=5, max_episode_steps=3)
    actions = np.array([[1, 2, 0, 3], [2, 2, 1, 0], [0, 3, 2, 2], [1, 0, 2, 3]])
    a = make()
    a.reset()
    for t in range(3):
        a.step(actions[t])
    assert bool(a.last_truncations.all())
    state = a.state_dict()
    assert all(torch.is_tensor(v) and v.device.type == 'cpu' or type(v) is int for v in state.values())
    b = make()
    b.load_state_dict(state)
    for x, y in zip(a.state_arrays(), b.state_arrays()):
        assert np.array_equal(x, y)
    oa, ra, da, ia = a.step(actions[3])
    ob, rb, db, ib = b.step(actions[3])
    assert torch.equal(oa, ob) and torch.equal(_bits(ra), _bits(rb)) and torch.equal(da, db)
    assert torch.equal(a.last_truncations, b.last_truncations)
    assert torch.equal(_bits(ia.episode_rewards), _bits(ib.episode_rewards))
    assert not torch.equal(oa.cpu(), state['obs'])  # (the step drew new frames)


# -- 6. refusals --------------------------------------------------------------------------------
@pytest.mark.parametrize('field,kwargs', [
    ('num_envs', dict(num_envs=5)), ('seed', dict(seed=6)), ('env_offset', dict(env_offset=1)),
    ('game_ids', dict(game='breakout+catch')), ('episodic_life', dict(episodic_life=True)),
    ('max_episode_steps', dict(max_episode_steps=7)), ('num_actions', dict(num_actions=18))])
def test_load_state_dict_names_the_mismatched_field(lib, cuda, field, kwargs):
    from actorcritic.envs.games import DeviceGameEnvs
    base = dict(game='catch+breakout', num_envs=4, seed=5, max_episode_steps=3)
    a = DeviceGameEnvs(**base)
    a.reset()
    state = a.state_dict()
    b = DeviceGameEnvs(**dict(base, **kwargs))
    before = [x.copy() for x in b.state_arrays()]
    with pytest.raises(ValueError, match=field):
        b.load_state_dict(state)
    for x, y in zip(before, b.state_arrays()):
        assert np.array_equal(x, y)  # refused before anything was written
    DeviceGameEnvs(fused_step=True, **base).load_state_dict(state)  # fused_step is free to differ


def test_env_kinds_do_not_mix(lib, cuda):
    from actorcritic.envs.atari.wrappers import SyntheticAtariEnvs
    from actorcritic.envs.games import DeviceGameEnvs
    synth, games = SyntheticAtariEnvs(4, seed=5), DeviceGameEnvs('breakout', 4, seed=5)
    with pytest.raises(ValueError, match='kind'):
        games.load_state_dict(synth.state_dict())
    with pytest.raises(ValueError, match='kind'):
        synth.load_state_dict(games.state_dict())
    with pytest.raises(ValueError, match='seed'):
        SyntheticAtariEnvs(4, seed=6).load_state_dict(synth.state_dict())


def test_run_state_before_the_first_interact_raises(lib, cuda):
    r = _build(CASES['catch-cap5'])
    with pytest.raises(ValueError, match='interact'):
        r.agent.run_state()


def test_a_rollout_length_of_its_own_is_fine_and_other_envs_are_refused(lib, cuda, monkeypatch):
    """Nothing saved depends on T: a state saved at T = 3 loads into an agent of T = 2, which then
    steps the saved envs; an agent over other envs refuses it."""
    _rollout_form(monkeypatch, True)
    r = _build(CASES['catch-cap5'])
    _run(r, 1, [])
    state = r.agent.run_state()
    assert state['sample_counter'] == 3
    short = _build(_case(game='catch', T=2, max_episode_steps=5))
    short.agent.load_run_state(state)
    log = []
    _run(short, 1, log)
    assert short.model.engine.sample_counter == 5
    assert bool(log[0]['truncations'][:, 1].all())  # steps 4 and 5 of the saved episodes: the cap at 5
    other = _build(_case(game='catch', max_episode_steps=5, env_seed=ENV_SEED + 1))
    with pytest.raises(ValueError, match='seed'):
        other.agent.load_run_state(state)


def test_host_stepped_envs_have_no_run_state(lib, cuda):
    """A HostAtariEnvs agent (fake host envs, as tests/test_gpu_host_envs.py builds them)."""
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import oracle
    from actorcritic import session as sess
    from actorcritic import spaces
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari import wrappers
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.multi_env import MultiEnv

    class ALE(oracle.FakeALE):
        action_space = spaces.Discrete(4)
        observation_space = spaces.Box(low=0, high=255, shape=(210, 160, 3), dtype=np.uint8)

    sess.reset_default_graph()
    env = MultiEnv(wrappers.HostAtariEnvs([wrappers.wrap_atari_env(ALE(100 + i), preprocess=False)
                                           for i in range(2)]))
    try:
        model = AtariModel(env.observation_space, env.action_space, 32, random_seed=3, init_seed=1)
        agent = MultiEnvAgent(env, model, 2)
        with sess.Session() as s:
            agent.interact(s)
        with pytest.raises(ValueError, match='host'):
            agent.run_state()
        with pytest.raises(ValueError, match='host'):
            agent.load_run_state({})
        with pytest.raises(ValueError, match='host'):
            env.batched.state_dict()
    finally:
        env.close()


def test_a_pending_game_state_is_refused_and_loading_clears_it(lib, cuda):
    from actorcritic.envs.games import DeviceGameEnvs
    env = DeviceGameEnvs('catch', 4, seed=5, fused_step=True)
    env.reset()
    state = env.state_dict()
    env._pend[2, env._pend_flag] = 1
    with pytest.raises(RuntimeError, match='pending'):
        env.state_dict()
    env.load_state_dict(state)  # zeroes the pending area, as reset_into does
    assert not env._pend.any()
    env.state_dict()


# -- 7. through the example ---------------------------------------------------------------------
def _train(directory, max_updates, **kw):
    from actorcritic import session as sess
    from actorcritic.examples.atari.a2c_acktr import train_a2c_acktr
    sess.reset_default_graph()
    return train_a2c_acktr(False, 'DeviceGame', 4, 3, str(directory), 'Run', max_updates=max_updates, seed=2,
                           game='catch+breakout', **kw)


def _load(path):
    return torch.load(str(path), map_location='cpu', weights_only=True)


def _assert_blobs_equal(a, b, where=''):
    assert set(a) == set(b), where
    for k, v in a.items():
        if isinstance(v, dict):
            _assert_blobs_equal(v, b[k], where + k + '/')
        elif torch.is_tensor(v):
            assert v.dtype == b[k].dtype and v.shape == b[k].shape and torch.equal(_bits(v), _bits(b[k])), where + k
        else:
            assert v == b[k], where + k


def test_example_resumes_its_own_run(lib, cuda, tmp_path, monkeypatch):
    from actorcritic import checkpoint
    _rollout_form(monkeypatch, True)
    for var in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        monkeypatch.delenv(var, raising=False)
    straight, cut = tmp_path / 'straight', tmp_path / 'cut'
    straight.mkdir()
    cut.mkdir()
    opts = dict(run_state=True, checkpoint_every=2, normalize_returns=True)
    _train(straight, 4, **opts)
    assert sorted(p.name for p in straight.iterdir()) == ['Run-2.pt', 'Run-2.run0.pt', 'Run-4.pt', 'Run-4.run0.pt',
                                                          'checkpoint']
    _train(cut, 2, **opts)
    assert sorted(p.name for p in cut.iterdir()) == ['Run-2.pt', 'Run-2.run0.pt', 'checkpoint']
    _train(cut, 2, **opts)  # resumes
    assert checkpoint.latest(str(cut)) == str(cut / 'Run-4.pt')
    assert checkpoint.latest(str(straight)) == str(straight / 'Run-4.pt')
    for name in ('Run-4.pt', 'Run-4.run0.pt', 'Run-2.pt', 'Run-2.run0.pt'):
        _assert_blobs_equal(_load(cut / name), _load(straight / name), name + ': ')
    assert int(_load(cut / 'Run-4.run0.pt')['sample_counter']) == 4 * 3
    # one more pair when the loop ends off the schedule
    _train(cut, 1, **opts)
    assert {'Run-5.pt', 'Run-5.run0.pt'} <= {p.name for p in cut.iterdir()}
    # run_state=False on that directory: as ever -- the weights resume, the envs start afresh,
    # and only the scheduled model checkpoint is written
    listing = sorted(p.name for p in cut.iterdir())
    model, _ = _train(cut, 1, checkpoint_every=2)
    assert sorted(p.name for p in cut.iterdir()) == sorted(listing + ['Run-6.pt'])
    assert model.engine.sample_counter == 3
    # a model checkpoint without this rank's run state: an error, not a silent reset
    with pytest.raises(ValueError, match='run state'):
        _train(cut, 1, **opts)


def test_ppo_example_resumes_its_own_run(lib, cuda, tmp_path, monkeypatch):
    """The straight-versus-cut core of the test above through train_ppo: the loop is the same one."""
    from actorcritic import checkpoint
    from actorcritic import session as sess
    from actorcritic.examples.atari.ppo import train_ppo
    _rollout_form(monkeypatch, True)
    for var in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        monkeypatch.delenv(var, raising=False)

    def train(directory, max_updates):
        sess.reset_default_graph()
        return train_ppo('DeviceGame', 4, 3, str(directory), 'Run', max_updates=max_updates, seed=2,
                         game='catch+breakout', num_epochs=2, num_minibatches=2, run_state=True, checkpoint_every=2,
                         normalize_returns=True)

    straight, cut = tmp_path / 'straight', tmp_path / 'cut'
    straight.mkdir()
    cut.mkdir()
    train(straight, 4)
    assert sorted(p.name for p in straight.iterdir()) == ['Run-2.pt', 'Run-2.run0.pt', 'Run-4.pt', 'Run-4.run0.pt',
                                                          'checkpoint']
    train(cut, 2)
    assert sorted(p.name for p in cut.iterdir()) == ['Run-2.pt', 'Run-2.run0.pt', 'checkpoint']
    train(cut, 2)  # resumes
    assert checkpoint.latest(str(cut)) == str(cut / 'Run-4.pt')
    assert checkpoint.latest(str(straight)) == str(straight / 'Run-4.pt')
    for name in ('Run-4.pt', 'Run-4.run0.pt', 'Run-2.pt', 'Run-2.run0.pt'):
        _assert_blobs_equal(_load(cut / name), _load(straight / name), name + ': ')


# -- 8. two ranks -------------------------------------------------------------------------------
WORLD = 2


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, port, out_dir):
    sys.path.insert(0, os.path.join(ROOT, 'actor-critic_amd'))
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(WORLD),
                      LOCAL_RANK=str(rank), ACMI_DIST_BACKEND='gloo', ACMI_ROLLOUT_SPLIT='0', ACMI_ROLLOUT_GRAPH='0')
    from actorcritic import checkpoint, parallel
    world, r = parallel.init_from_env()
    assert (world, r) == (WORLD, rank)
    dev = torch.device('cuda', torch.cuda.current_device())
    case = _case(game='catch+breakout', N=2, norm=True, max_episode_steps=5)
    build = lambda: _build(case, env_offset=rank * case.N, device=dev)
    a = build()
    _run(a, 2 * case.K, [])
    straight = _snapshot(a)
    del a
    b = build()
    _run(b, case.K, [])
    prefix = os.path.join(out_dir, 'Run')
    step = b.gs.value
    if rank == 0:
        checkpoint.save(prefix, step, b.model, b.opt, objective=b.obj)
    own = checkpoint.save_run_state(prefix, step, b.agent, b.obj)
    assert own == checkpoint.run_state_path(prefix, step, rank)
    parallel.barrier()
    del b
    b = build()
    checkpoint.load(checkpoint.latest(out_dir), b.model, b.opt, b.gs, objective=b.obj)
    refused = False
    try:
        checkpoint.load_run_state(checkpoint.run_state_path(prefix, step, 1 - rank), b.agent, b.obj)
    except ValueError as e:
        refused = 'rank' in str(e)
    checkpoint.load_run_state(own, b.agent, b.obj)
    _run(b, case.K, [])
    torch.save(dict(straight=straight, resumed=_snapshot(b), refused=refused),
               os.path.join(out_dir, 'rank{}.pt'.format(rank)))
    parallel.barrier()
    parallel.destroy()


def test_two_ranks_resume_each_from_its_own_file(lib, cuda, tmp_path):
    """gloo world 2 on one card (as tests/test_gpu_dp.py), 2 envs a rank of catch+breakout with the
    return normaliser (its moments are summed over the ranks): every rank writes and reads its own
    file, the resumed ranks equal the straight ones, and the other rank's file is refused."""
    ctx = mp.get_context('spawn')
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, port, str(tmp_path))) for r in range(WORLD)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        assert p.exitcode == 0, 'rank failed with exit code {}'.format(p.exitcode)
    assert {'Run-2.pt', 'Run-2.run0.pt', 'Run-2.run1.pt'} <= {p.name for p in tmp_path.iterdir()}
    ranks = [_load(tmp_path / 'rank{}.pt'.format(r)) for r in range(WORLD)]
    for res in ranks:
        assert res['refused'] is True
        _assert_same(res['resumed'], res['straight'])
    assert torch.equal(ranks[0]['resumed']['params'], ranks[1]['resumed']['params'])
    assert not torch.equal(ranks[0]['resumed']['next_obs'], ranks[1]['resumed']['next_obs'])
    files = [_load(tmp_path / 'Run-2.run{}.pt'.format(r)) for r in range(WORLD)]
    assert [(f['rank'], f['world_size'], f['global_step']) for f in files] == [(0, 2, 2), (1, 2, 2)]
    assert [int(f['env']['env_offset']) for f in files] == [0, 2]
