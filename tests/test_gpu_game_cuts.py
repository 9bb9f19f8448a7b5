"""The device games' cuts on the GPU: acmi_game_step_cuts against the rule
book behind the wrappers (test_game_cuts_host.CutsReplay) bit for bit, its identity with
acmi_game_step under rules {0, 0}, the truncation-aware targets against the float32
restatement and the float64 recursion, the rollout's truncations replayed on the host,
the objectives with and without the truncations fed, and evaluate()'s refusal."""
import ctypes

import numpy as np
import pytest

from actorcritic import _lib
from actorcritic.objectives import gamma_tables
from test_game_cuts_host import (CUTS_CAP, CUTS_SCRIPT_SEED, CUTS_SEED, GAMMA, TARGET_SHAPES, CutsReplay,
                                 breakout_cuts_steps, cuts_script, f64_bound, gae_trunc_f32, hand_case, random_case,
                                 returns_trunc_f32, targets_trunc_f64)

pytestmark = pytest.mark.gpu

OBS = 84 * 84 * 4


# -- the stepper --------------------------------------------------------------------------
@pytest.mark.parametrize('layout', ['one_in_place', 'three_in_place', 'three_strided'])
@pytest.mark.parametrize('game', ['catch', 'breakout'])
def test_step_cuts_matches_the_host_game_bit_for_bit(cuda, game, layout):
    """Per step: the whole stack, reward, terminal, truncated, the episode reward by its
    bits and the five state arrays, done codes included.  Breakout: episodic life under a
    60-step cap, as long as its host trace needs to hold, for every env, a life-loss
    terminal, the restack step after it, a truncation and the reset step after that;
    Catch: a 7-step cap over 20 steps.  Strided: two [N, 2, 28224] buffers ping-pong, the
    per-step outputs [N, 2]; the slots in between keep their sentinel."""
    import torch
    from actorcritic.envs.games import DeviceGameEnvs
    N, env_offset = (1, 0) if layout == 'one_in_place' else (3, 5)
    strided = layout == 'three_strided'
    if game == 'catch':
        S, rules = 20, dict(max_episode_steps=7)
    else:
        S, events = breakout_cuts_steps(N, env_offset)
        assert S is not None, 'the script covers too little: {}'.format(events)
        rules = dict(episodic_life=True, max_episode_steps=CUTS_CAP)
    actions = cuts_script(game, S, N, CUTS_SCRIPT_SEED)
    ref = CutsReplay(game, N, seed=CUTS_SEED, env_offset=env_offset, **rules)
    env = DeviceGameEnvs(game, N, seed=CUTS_SEED, env_offset=env_offset, device=cuda, **rules)
    assert env.emits_truncations is True and env.fused_step is False
    k = 2 if strided else 1
    bufs = [torch.full((N, k, OBS), 0xAB, dtype=torch.uint8, device=cuda) for _ in range(k)]
    rew = torch.full((N, k), -7.0, dtype=torch.float32, device=cuda)
    term = torch.full((N, k), 9, dtype=torch.uint8, device=cuda)
    trunc = torch.full((N, k), 9, dtype=torch.uint8, device=cuda)
    ep = torch.full((N, k), -7.0, dtype=torch.float32, device=cuda)
    env.reset_into(bufs[0].data_ptr(), k * OBS)
    assert np.array_equal(bufs[0][:, 0].cpu().numpy().reshape(N, 84, 84, 4), ref.stacks)
    dev_actions = torch.from_numpy(actions).to(cuda)
    for s in range(S):
        src, dst = bufs[s % k], bufs[(s + 1) % k]
        env.step_into(dev_actions[s].data_ptr(), src.data_ptr(), k * OBS, dst.data_ptr(), k * OBS, rew.data_ptr(),
                      term.data_ptr(), ep.data_ptr(), k, trunc_ptr=trunc.data_ptr())
        want_obs, want_rew, want_term, want_trunc, want_ep = ref.step(actions[s])
        assert np.array_equal(dst[:, 0].cpu().numpy().reshape(N, 84, 84, 4), want_obs), s
        assert np.array_equal(rew[:, 0].cpu().numpy(), want_rew), s
        assert np.array_equal(term[:, 0].cpu().numpy(), want_term), s
        assert np.array_equal(trunc[:, 0].cpu().numpy(), want_trunc), s
        assert np.array_equal(ep[:, 0].cpu().numpy().view(np.uint32), want_ep), s
        for a, b in zip(env.state_arrays(), ref.state()):
            assert a.dtype == b.dtype and np.array_equal(a, b), s
    if strided:
        for b in bufs:
            assert bool((b[:, 1] == 0xAB).all())
        assert bool((rew[:, 1] == -7.0).all()) and bool((ep[:, 1] == -7.0).all())
        assert bool((term[:, 1] == 9).all()) and bool((trunc[:, 1] == 9).all())
    for ev in ref.events:
        if game == 'catch':  # truncated at steps 7 and 14, reset at 8 and 15
            assert ev['truncation'] == 2 and ev['reset'] == 2 and ev['life_cut'] == 0
        else:
            assert min(ev['life_cut'], ev['restack'], ev['truncation'], ev['reset']) >= 1


@pytest.mark.parametrize('game,S', [('catch', 45), ('breakout', 130)])
def test_rules_zero_without_truncated_are_acmi_game_step(cuda, game, S):
    """Rules {0, 0} and truncated = NULL: the bytes of acmi_game_step, N = 3 (and with a
    truncated array: the same bytes beside it)."""
    import torch
    from actorcritic.envs.games import DeviceGameEnvs
    N = 3
    actions = torch.from_numpy(cuts_script(game, S, N, 1)).to(cuda)
    rules = _lib.GameRules(0, 0)
    out = []
    for entry in ('old', 'cuts', 'cuts+truncated'):
        env = DeviceGameEnvs(game, N, seed=11, env_offset=5, device=cuda)
        assert env.emits_truncations is False
        obs = torch.zeros((N, OBS), dtype=torch.uint8, device=cuda)
        rew = torch.zeros((S, N), dtype=torch.float32, device=cuda)
        term = torch.zeros((S, N), dtype=torch.uint8, device=cuda)
        trunc = torch.full((S, N), 9, dtype=torch.uint8, device=cuda)
        ep = torch.zeros((S, N), dtype=torch.float32, device=cuda)
        env.reset_into(obs.data_ptr())
        trace = []
        for s in range(S):
            p = ctypes.c_void_p(obs.data_ptr())
            if entry == 'old':
                env.step_into(actions[s].data_ptr(), p.value, OBS, p.value, OBS, rew[s].data_ptr(),
                              term[s].data_ptr(), ep[s].data_ptr(), 1)
            else:
                tp = ctypes.c_void_p(trunc[s].data_ptr()) if entry == 'cuts+truncated' else None
                _lib.call('acmi_game_step_cuts', ctypes.byref(env.state), ctypes.byref(rules), N, env.env_offset,
                          env.seed, _lib.ptr(actions[s]), p, OBS, p, OBS, _lib.ptr(rew[s]), _lib.ptr(term[s]), tp,
                          _lib.ptr(ep[s]), 1, _lib.stream_handle(cuda))
            trace.append(obs.clone())
        out.append([torch.stack(trace).cpu().numpy(), rew.cpu().numpy(), term.cpu().numpy(),
                    ep.cpu().numpy().view(np.uint32)] + list(env.state_arrays()))
        if entry == 'cuts':
            assert bool((trunc == 9).all())
        if entry == 'cuts+truncated':  # no cap within S steps: nothing is truncated
            assert bool((trunc == 0).all())
    assert out[0][2].sum() >= (2 * N if game == 'catch' else 1)  # terminals, and the reset steps after them
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert a.dtype == b.dtype and np.array_equal(a, b)


# -- the targets --------------------------------------------------------------------------
def _targets(cuda, case, lam, trunc):
    """acmi_returns(_trunc) (lam None) or acmi_gae(_trunc) on a case -> (targets, adv);
    trunc None: the entry point without truncations."""
    import torch
    r, d, _, v, vb = case
    N, T = r.shape
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(cuda)
    rd, dd, vd, vbd = dev(r), dev(d), dev(v), dev(vb)
    tg = torch.full((N, T), -9.0, dtype=torch.float32, device=cuda)
    adv = torch.full((N, T), -9.0, dtype=torch.float32, device=cuda)
    trd = None if trunc is None else dev(trunc)
    tr = () if trd is None else (_lib.ptr(trd),)
    if lam is None:
        gp, bp = (dev(x) for x in gamma_tables(GAMMA, T))
        _lib.call('acmi_returns' + ('_trunc' if tr else ''), _lib.ptr(rd), _lib.ptr(dd), *tr, _lib.ptr(vd),
                  _lib.ptr(vbd), N, T, _lib.ptr(gp), _lib.ptr(bp), _lib.ptr(tg), _lib.ptr(adv),
                  _lib.stream_handle(cuda))
    else:
        _lib.call('acmi_gae' + ('_trunc' if tr else ''), _lib.ptr(rd), _lib.ptr(dd), *tr, _lib.ptr(vd),
                  _lib.ptr(vbd), N, T, GAMMA, lam, _lib.ptr(tg), _lib.ptr(adv), _lib.stream_handle(cuda))
    return tg.cpu().numpy(), adv.cpu().numpy()


@pytest.mark.parametrize('lam', [None, 0.95])
@pytest.mark.parametrize('shape', TARGET_SHAPES)
def test_trunc_targets_with_no_truncation_are_the_existing_kernels(cuda, shape, lam):
    case = random_case(*shape, zero_trunc=True)
    assert not case[2].any() and (case[1].any() or shape == (1, 1))
    want = _targets(cuda, case, lam, None)
    got = _targets(cuda, case, lam, case[2])
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('lam', [None, 0.95])
@pytest.mark.parametrize('case', ['hand', 'random-65x20'])
def test_trunc_targets_match_the_restatement_and_float64(cuda, case, lam):
    """Bit for bit against the float32 restatement; against the float64 recursion within
    the float32-vs-float64 tolerance of test_gpu_parity.  'hand': truncation at t = 0 and
    at T-1 (v_boot), two cuts in a row, a plain terminal beside a truncated one, and a
    flag where there is no terminal (test_game_cuts_host.hand_case)."""
    c = hand_case() if case == 'hand' else random_case(*(int(x) for x in case.split('-')[1].split('x')))
    r, d, tr, v, vb = c
    assert (tr & d).any() and (tr & ~d & 1).any() and (d & ~tr & 1).any()
    got_t, got_a = _targets(cuda, c, lam, tr)
    if lam is None:
        want_t, want_a = returns_trunc_f32(r, d, tr, v, vb, GAMMA)
    else:
        want_t, want_a = gae_trunc_f32(r, d, tr, v, vb, GAMMA, lam)
    assert np.array_equal(got_t.view(np.uint32), want_t.view(np.uint32))
    assert np.array_equal(got_a.view(np.uint32), want_a.view(np.uint32))
    t64, a64 = targets_trunc_f64(r, d, tr, v, vb, GAMMA, lam)
    assert np.abs(got_t - t64).max() <= f64_bound(t64)
    assert np.abs(got_a - a64).max() <= f64_bound(a64)
    # and the flags matter: the kernel without them gives other targets
    assert not np.array_equal(got_t, _targets(cuda, c, lam, None)[0])


# -- the rollout ----------------------------------------------------------------------------
def _agent(cuda, game, N, T, seed, **rules):
    from actorcritic import session as sess
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.envs.games import DeviceGameEnvs
    from actorcritic.multi_env import MultiEnv
    sess.reset_default_graph()
    envs = DeviceGameEnvs(game, N, seed=seed, device=cuda, **rules)
    env = MultiEnv(envs)
    assert env.batched is envs
    model = AtariModel(env.observation_space, env.action_space, 32, random_seed=3)
    return model, MultiEnvAgent(env, model, T, copy_batches=True)


@pytest.mark.parametrize('form', ['loop', 'graph'])
def test_rollout_truncations_replay_through_the_host_games(cuda, monkeypatch, form):
    """MultiEnvAgent over DeviceGameEnvs('breakout', 4, episodic_life=True,
    max_episode_steps=25), 12 rollouts of 5 steps: observations, rewards, terminals, episode
    rewards and last_truncations are what four HostGame chains give for the returned
    actions, and the trace holds both kinds of cut.  'loop': the plain unfused loop;
    'graph': the _half_step chain, eager once and then captured and replayed."""
    from actorcritic import session as sess
    monkeypatch.setenv('ACMI_ROLLOUT_SPLIT', '0')
    monkeypatch.setenv('ACMI_ROLLOUT_GRAPH', '1' if form == 'graph' else '0')
    N, T, rounds = 4, 5, 12
    model, agent = _agent(cuda, 'breakout', N, T, 6, episodic_life=True, max_episode_steps=25)
    ref = CutsReplay('breakout', N, seed=6, episodic_life=True, max_episode_steps=25)
    prev_next = ref.stacks.copy()
    with sess.Session() as s:
        for _ in range(rounds):
            obs, actions, rewards, terminals, next_obs, infos = agent.interact(s)
            trunc = agent.last_truncations
            assert trunc is not None and tuple(trunc.shape) == (N, T) and trunc.is_cuda
            obs, actions, next_obs = obs.cpu().numpy(), actions.cpu().numpy(), next_obs.cpu().numpy()
            rewards, terminals, trunc = rewards.cpu().numpy(), terminals.cpu().numpy(), trunc.cpu().numpy()
            ep = infos.episode_rewards.cpu().numpy().view(np.uint32)
            assert trunc.dtype == np.bool_ and np.array_equal(obs[:, 0], prev_next)
            for t in range(T):
                want_obs, want_rew, want_term, want_trunc, want_ep = ref.step(actions[:, t])
                assert np.array_equal(obs[:, t + 1] if t + 1 < T else next_obs, want_obs)
                assert np.array_equal(rewards[:, t], want_rew)
                assert np.array_equal(terminals[:, t], want_term.astype(bool))
                assert np.array_equal(trunc[:, t], want_trunc.astype(bool))
                assert np.array_equal(ep[:, t], want_ep)
            prev_next = next_obs
    rb = agent._bufs
    assert rb.fused is False and rb.use_graph is (form == 'graph') and (rb.graph is not None) is (form == 'graph')
    # both kinds of cut, and the step after each, somewhere in the trace (which env holds
    # which depends on the actions the policy drew)
    for kind in ('life_cut', 'restack', 'truncation', 'reset'):
        assert sum(ev[kind] for ev in ref.events) >= 1, ref.events


def test_plain_envs_emit_no_truncations(cuda):
    from actorcritic import session as sess
    model, agent = _agent(cuda, 'catch', 4, 5, 6)
    assert agent.last_truncations is None
    with sess.Session() as s:
        agent.interact(s)
    assert agent.last_truncations is None and agent._env.batched.emits_truncations is False
    obs, rew, term, info = agent._env.batched.step([0, 1, 2, 0])
    assert agent._env.batched.last_truncations is None


def test_batched_step_leaves_the_truncations_in_an_attribute(cuda):
    from actorcritic.envs.games import DeviceGameEnvs
    envs = DeviceGameEnvs('catch', 2, seed=1, device=cuda, max_episode_steps=3)
    envs.reset()
    seen = []
    for _ in range(4):
        _, _, term, _ = envs.step([0, 0])
        assert np.array_equal(term.cpu().numpy(), envs.last_truncations.cpu().numpy())
        seen.append(envs.last_truncations.cpu().numpy().tolist())
    assert seen == [[False, False], [False, False], [True, True], [False, False]]


# -- the objectives ---------------------------------------------------------------------------
@pytest.mark.parametrize('objective,lam', [('a2c', None), ('a2c', 0.95), ('ppo', 0.95)])
def test_objectives_use_the_truncations_only_when_fed(cuda, objective, lam):
    """target_values and advantage over a (3, 5) batch with hand-placed rewards, terminals
    and truncations (hand_case) and the model's own values.  Fed: the float32 restatement,
    bit for bit.  Unfed: acmi_returns / acmi_gae called directly on the same batch."""
    from actorcritic import session as sess
    from actorcritic.objectives import A2CObjective, PPOObjective
    N, T = 3, 5
    model, agent = _agent(cuda, 'catch', N, T, 2)
    if objective == 'a2c':
        obj = A2CObjective(model, discount_factor=GAMMA, gae_lambda=lam)
    else:
        obj = PPOObjective(model, discount_factor=GAMMA, gae_lambda=lam, normalize_advantages=False)
    r, d, tr, _, _ = hand_case()
    with sess.Session() as s:
        obs, actions, _, _, next_obs, _ = agent.interact(s)
        feed = {model.observations_placeholder: obs, model.bootstrap_observations_placeholder: next_obs,
                model.actions_placeholder: actions, model.rewards_placeholder: r,
                model.terminals_placeholder: d.astype(bool)}
        fetches = [obj.target_values, obj.advantage, model.baseline.value, model.bootstrap_values]
        unfed = s.run(fetches, feed_dict=feed)
        feed[model.truncations_placeholder] = tr.astype(bool)
        fed = s.run(fetches, feed_dict=feed)
    v, vb = np.asarray(fed[2], np.float32).reshape(N, T), np.asarray(fed[3], np.float32).reshape(N)
    assert np.array_equal(v, np.asarray(unfed[2]).reshape(N, T))
    if lam is None:
        want_t, want_a = returns_trunc_f32(r, d, tr, v, vb, GAMMA)
    else:
        want_t, want_a = gae_trunc_f32(r, d, tr, v, vb, GAMMA, lam)
    assert np.array_equal(np.asarray(fed[0]).view(np.uint32), want_t.view(np.uint32))
    assert np.array_equal(np.asarray(fed[1]).view(np.uint32), want_a.view(np.uint32))
    old_t, old_a = _targets(cuda, (r, d, tr, v, vb), lam, None)
    assert np.array_equal(np.asarray(unfed[0]).view(np.uint32), old_t.view(np.uint32))
    assert np.array_equal(np.asarray(unfed[1]).view(np.uint32), old_a.view(np.uint32))
    assert not np.array_equal(fed[0], unfed[0])


# -- evaluate -----------------------------------------------------------------------------------
def test_evaluate_refuses_episodic_life(cuda):
    from actorcritic.envs.games import DeviceGameEnvs, evaluate
    with pytest.raises(ValueError):
        evaluate(None, DeviceGameEnvs('breakout', 2, device=cuda, episodic_life=True), 1, uniform=True)
    # a step cap alone is fine: a truncated game is over and reports its total
    returns = evaluate(None, DeviceGameEnvs('catch', 2, device=cuda, max_episode_steps=7), 2, uniform=True)
    assert returns.cpu().numpy().tolist() == [[0.0, 0.0], [0.0, 0.0]]
