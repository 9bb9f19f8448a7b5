"""Update diagnostics on the GPU, end to end on Catch with conv3 = 32: an armed run
stays bit for bit the run without diagnostics (parameters, optimizer slots, K-FAC state, env state,
next observations, sample counter, the engine's version), and every logged scalar equals the numpy
restatement (actorcritic.update_diag.host_*) fed with tensors the test captures itself -- the values,
targets and logits the loss read, a forward of the same observations in the same chunks after the
update, the gradient and parameter buffers -- within the kernel tests' tolerances: 2 (M - 1) 2^-53
sum|term| for the value and segment sums, 1e-12 per row for KL and H."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ROW_TOL = 1e-12
OBS_BYTES = 84 * 84 * 4


def _bits(t):
    if not t.is_floating_point():
        return t
    return t.contiguous().view({4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _single_process(monkeypatch):
    monkeypatch.setenv('ACMI_ROLLOUT_SPLIT', '0')
    monkeypatch.setenv('ACMI_ROLLOUT_GRAPH', '0')
    for var in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        monkeypatch.delenv(var, raising=False)


def _rmsprop(lr):
    from actorcritic.nn import ClipGlobalNormOptimizer, RMSPropOptimizer
    return ClipGlobalNormOptimizer(RMSPropOptimizer(learning_rate=lr), clip_norm=0.5)


def _acktr(model, lr=0.25):
    from actorcritic.kfac_utils import ColdStartPeriodicInvUpdateKfacOpt, LayerCollection
    from actorcritic.nn import ClipGlobalNormOptimizer, MomentumOptimizer
    lc = LayerCollection()
    model.register_layers(lc)
    model.register_predictive_distributions(lc)
    cold = ClipGlobalNormOptimizer(MomentumOptimizer(learning_rate=0.0003, momentum=0.9), clip_norm=0.5)
    return ColdStartPeriodicInvUpdateKfacOpt(num_cold_updates=1, cold_optimizer=cold, invert_every=2,
                                             learning_rate=lr, cov_ema_decay=0.99, damping=0.01,
                                             layer_collection=lc, momentum=0.9, norm_constraint=0.0001)


def _sum_close(got, terms, what):
    """|got - sum(terms)| within 2 (M - 1) 2^-53 sum|terms| (terms: float64, any shape)."""
    terms = np.asarray(terms, np.float64).ravel()
    bound = 2 * max(terms.size - 1, 0) * U * np.abs(terms).sum()
    err = abs(got - terms.sum())
    print('{}: M={} err={:.3e} bound={:.3e}'.format(what, terms.size, err, bound))
    assert err <= bound, (what, got, terms.sum(), err, bound)


def _check_update(diag, scal, cap, kfac=None):
    """One armed update's accumulators (``diag.last_acc``) and scalars against the restatement on the
    captured tensors ``cap``."""
    from actorcritic import update_diag as ud
    acc = diag.last_acc
    N, T, A = cap['N'], cap['T'], cap['A']
    grp, G = diag.groups.numpy(), diag.num_groups
    g_rows = np.repeat(grp.astype(np.int64), T)
    # value
    v64, y64 = cap['values'].astype(np.float64).ravel(), cap['targets'].astype(np.float64).ravel()
    e = y64 - v64
    for g in range(G):
        sel = g_rows == g
        assert acc['value'][g, 0] == sel.sum()
        for col, terms in ((1, v64[sel]), (2, y64[sel]), (3, y64[sel] ** 2), (4, e[sel]), (5, e[sel] * e[sel])):
            _sum_close(acc['value'][g, col], terms, 'value g={} col={}'.format(g, col))
    want_v, _ = ud.host_value_diag(cap['values'].reshape(N, T), cap['targets'].reshape(N, T), grp, G)
    for k, v in ud.value_scalars(want_v.sum(axis=0)).items():
        assert abs(scal[k] - v) <= 1e-11 * max(1.0, abs(v)), (k, scal[k], v)
    # policy: per row 1e-12
    want_p, bad_envs, bad_rows = ud.host_policy_diag(cap['logits_old'], cap['logits_new'], cap['legal'], grp, G, T, A)
    assert (bad_envs, bad_rows) == (0, 0) and np.array_equal(acc['policy'][:, 0], want_p[:, 0])
    for g in range(G):
        n = want_p[g, 0]
        if n == 0:
            assert acc['policy'][g].tolist() == want_p[g].tolist()
            continue
        for col in (1, 2, 3):
            err = abs(acc['policy'][g, col] - want_p[g, col])
            print('policy g={} col={} n={:.0f} err={:.3e}'.format(g, col, n, err))
            assert err <= ROW_TOL * (1 if col == 3 else n), (g, col, err)
    allp = ud.reduce_policy_groups(want_p)
    assert allp[0] == N * T
    assert abs(scal['policy_kl'] - allp[1] / allp[0]) <= ROW_TOL
    assert abs(scal['policy_kl_max'] - allp[3]) <= ROW_TOL
    assert abs(scal['policy_entropy_after'] - allp[2] / allp[0]) <= ROW_TOL
    # norms: float64 over the captured buffers, per segment
    off = cap['offsets']
    g64, w1, w0 = (cap[k].astype(np.float64) for k in ('grads', 'params_after', 'params_before'))
    p64 = None if kfac is None else cap['precon'].astype(np.float64)
    d = w1 - w0
    for s in range(12):
        sl = slice(off[s], off[s + 1])
        _sum_close(acc['grad'][s, 0], g64[sl] ** 2, 'grad^2 s={}'.format(s))
        _sum_close(acc['step'][s, 0], w1[sl] ** 2, 'param^2 s={}'.format(s))
        _sum_close(acc['step'][s, 1], w0[sl] ** 2, 'before^2 s={}'.format(s))
        _sum_close(acc['step'][s, 3], d[sl] * d[sl], 'step^2 s={}'.format(s))
        if p64 is not None:
            _sum_close(acc['grad'][s, 1], p64[sl] ** 2, 'precon^2 s={}'.format(s))
            _sum_close(acc['grad'][s, 2], g64[sl] * p64[sl], 'grad.precon s={}'.format(s))
    rel = lambda a, b: abs(a - b) <= 1e-12 * max(abs(b), 1e-300)
    assert rel(scal['grad_norm'], np.linalg.norm(g64)) and rel(scal['step_norm'], np.linalg.norm(d))
    assert rel(scal['param_norm'], np.linalg.norm(w1))
    for l, name in enumerate(ud.LAYERS):
        sl = slice(off[2 * l], off[2 * l + 2])
        assert rel(scal['grad_norm/' + name], np.linalg.norm(g64[sl])), name
        assert rel(scal['step_norm/' + name], np.linalg.norm(d[sl])), name
        if p64 is not None:
            assert rel(scal['precon_norm/' + name], np.linalg.norm(p64[sl])), name
            cos = g64[sl] @ p64[sl] / (np.linalg.norm(g64[sl]) * np.linalg.norm(p64[sl]))
            assert abs(scal['precon_cos/' + name] - cos) <= 1e-11, (name, scal['precon_cos/' + name], cos)
    if kfac is None:
        assert not any(k.startswith('precon') or k == 'kfac_coeff' for k in scal)
    else:
        assert scal['kfac_coeff'] == float(kfac.last_coeff.item())


def _run(algo, armed, updates, N=8, T=5, game='catch', mask=False, lr=0.0007, check=True, forward_rows=1024,
         **ppo_kw):
    """``updates`` rollouts + updates by hand (the example loop's feeds).  ``armed``: None (no object),
    False (an object that is never armed) or True (armed on every update; with ``check`` every update's
    scalars are checked against the restatement).  -> (final state dict of tensors, list of scalar dicts)."""
    from actorcritic import session as sess
    from actorcritic import update_diag as ud
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.examples.atari.a2c_acktr import create_game_environments
    from actorcritic.multi_env import MultiEnv
    from actorcritic.objectives import A2CObjective, PPOObjective
    sess.reset_default_graph()
    env = MultiEnv(create_game_environments(game, N, seed=4, full_action_set=mask, env_offset=0))
    model = AtariModel(env.observation_space, env.action_space, 32, random_seed=3, init_seed=1)
    agent = MultiEnvAgent(env, model, T, mask_actions=mask)
    diag = None if armed is None else ud.UpdateDiagnostics.for_envs(env, forward_rows=forward_rows)
    eng = model.engine
    gs = sess.get_or_create_global_step()
    if algo == 'ppo':
        objective = PPOObjective(model, diagnostics=diag)
        opt = _rmsprop(lr)
        op = objective.optimize_shared(opt, 0.5, global_step=gs, shuffle_seed=5, **ppo_kw)
    else:
        objective = A2CObjective(model, diagnostics=diag)
        opt = _acktr(model) if algo == 'acktr' else _rmsprop(lr)
        op = objective.optimize_shared(opt, 0.5, global_step=gs)
    kfac = opt if algo == 'acktr' else None
    scalars = []
    M = N * T
    off = list(eng.layout.offsets) + [eng.layout.nparams]
    with sess.Session() as s:
        for _ in range(updates):
            obs, actions, rewards, terminals, next_obs, infos = agent.interact(s)
            feed = {model.observations_placeholder: obs, model.bootstrap_observations_placeholder: next_obs,
                    model.actions_placeholder: actions, model.rewards_placeholder: rewards,
                    model.terminals_placeholder: terminals}
            if agent.last_truncations is not None:
                feed[model.truncations_placeholder] = agent.last_truncations
            before = eng.params.clone()
            if armed:
                diag.request()
            s.run([op], feed_dict=feed, host=False)
            if not armed:
                continue
            assert not diag.armed
            scal = diag.read()
            scalars.append(scal)
            if not check:
                continue
            st = eng.update_state(M)
            fwd = st.fwd
            assert fwd.M == M
            grads = (st if algo != 'ppo' else eng.update_state(M // ppo_kw['num_minibatches'])).grads
            new = torch.zeros(M, eng.A, device=eng.device)
            flat = fwd.obs.reshape(M, 84, 84, 4)
            for r0 in range(0, M, forward_rows):  # the same chunks through activations of the test's own
                rows = min(forward_rows, M - r0)
                acts = eng.activations(rows, 'test')
                eng.forward(flat.data_ptr() + r0 * OBS_BYTES, rows, acts.struct, want_value=False)
                new[r0:r0 + rows] = acts.logits[:rows]
            legal = None if eng.masks is None else eng.row_masks(N, T).cpu().numpy().view(np.uint32)
            cap = dict(N=N, T=T, A=eng.A, offsets=off, legal=legal,
                       values=fwd.flat_value.cpu().numpy(), targets=st.targets[:M].cpu().numpy(),
                       logits_old=fwd.flat_logits.cpu().numpy(), logits_new=new.cpu().numpy(),
                       grads=grads.cpu().numpy(), params_after=eng.params.cpu().numpy(),
                       params_before=before.cpu().numpy(),
                       precon=None if kfac is None else kfac.state['precon'].cpu().numpy())
            assert _same(diag._dev['logits'], new)  # what the hook gathered: bit-identical
            _check_update(diag, scal, cap, kfac)
        torch.cuda.synchronize()
        state = {'params': eng.params.clone(), 'version': torch.tensor(eng.version),
                 'global_step': torch.tensor(gs.value)}
        state.update({'slot.' + k: v.clone() for k, v in opt.slots().items()})
        if kfac is not None:
            state.update({'kfac.' + k: kfac.state[k].clone() for k in ('velocity', 'factors', 'inv', 'biased')})
            state.update({'cold.' + k: v.clone() for k, v in kfac._cold_optimizer.slots().items()})
        rs = agent.run_state()
        state['next_obs'], state['sample_counter'] = rs['next_obs'], torch.tensor(rs['sample_counter'])
        state.update({'env.' + k: v for k, v in rs['env'].items() if torch.is_tensor(v)})
        # the rollout cache (dead since the update bumped the version) and the rollout's activations
        state['rollout_cache_alive'] = torch.tensor(eng.lookup_rollout(obs) is not None)
        acts = eng.update_state(M).fwd.acts
        state.update({'rollout.' + k: getattr(acts, k).clone() for k in ('logits', 'value', 'a4', 'a1')})
    env.close()
    return state, scalars


def _assert_passive(on, off):
    assert set(on) == set(off)
    for k in off:
        assert _same(on[k].cpu(), off[k].cpu()), k
    assert {'params', 'next_obs', 'sample_counter', 'env.vars', 'env.obs', 'version'} <= set(off)


def test_a2c_armed_on_every_update_is_passive_and_matches_the_restatement(lib, cuda, monkeypatch):
    _single_process(monkeypatch)
    off, _ = _run('a2c', None, 3)
    on, scalars = _run('a2c', True, 3)
    _assert_passive(on, off)
    assert {'slot._ms', 'slot._mom'} <= set(off) and len(scalars) == 3
    from actorcritic import update_diag as ud
    keys = list(ud.VALUE_KEYS + ud.POLICY_KEYS) + ['grad_norm', 'step_norm', 'param_norm'] + \
        ['grad_norm/' + l for l in ud.LAYERS] + ['step_norm/' + l for l in ud.LAYERS]
    assert all(list(s) == keys for s in scalars)  # one game, a first-order optimizer
    assert all(s['step_norm'] > 0 and s['policy_kl'] > 0 and s['policy_kl_max'] >= s['policy_kl'] for s in scalars)
    # an object that is never armed launches nothing and changes nothing; chunks of 16 rows change no scalar's check
    idle, none = _run('a2c', False, 3)
    _assert_passive(idle, off)
    assert none == []
    chunked, _ = _run('a2c', True, 2, forward_rows=16)
    assert _same(chunked['params'], _run('a2c', None, 2)[0]['params'])


def test_a2c_learning_rate_zero_has_a_step_of_exactly_zero(lib, cuda, monkeypatch):
    _single_process(monkeypatch)
    _, scalars = _run('a2c', True, 2, lr=0.0)
    assert all(s['step_norm'] == 0.0 and all(s['step_norm/' + l] == 0.0 for l in ('conv1', 'fc_policy'))
               for s in scalars)
    assert all(abs(s['policy_kl']) <= 1e-9 and s['grad_norm'] > 0 for s in scalars)  # (last bits of two forwards)


def test_acktr_is_passive_with_kfac_state_and_logs_the_preconditioner(lib, cuda, monkeypatch):
    _single_process(monkeypatch)
    off, _ = _run('acktr', None, 4, T=20)
    on, scalars = _run('acktr', True, 4, T=20)
    _assert_passive(on, off)
    assert {'kfac.velocity', 'kfac.factors', 'kfac.inv', 'cold._accum'} <= set(off) and len(scalars) == 4
    assert all('kfac_coeff' in s and 'precon_cos/conv1' in s and 'precon_norm/fc_baseline' in s for s in scalars)
    assert all(0.0 < s['kfac_coeff'] <= 1.0 for s in scalars)


@pytest.mark.parametrize('mode', ['envs', 'rows'])
def test_ppo_is_passive_and_the_step_is_the_whole_ops(lib, cuda, monkeypatch, mode):
    _single_process(monkeypatch)
    kw = dict(T=16, lr=0.00025, num_epochs=2, num_minibatches=2, minibatch=mode)
    off, _ = _run('ppo', None, 2, **kw)
    on, scalars = _run('ppo', True, 2, **kw)  # (_check_update: step_norm against params after - before the op)
    _assert_passive(on, off)
    assert len(scalars) == 2 and all(s['step_norm'] > 0 for s in scalars)


def test_mixed_masked_batch_has_per_game_keys_that_add_up(lib, cuda, monkeypatch):
    _single_process(monkeypatch)
    kw = dict(game='catch+breakout', mask=True, T=5)
    off, _ = _run('a2c', None, 2, **kw)
    on, scalars = _run('a2c', True, 2, **kw)
    _assert_passive(on, off)
    for s in scalars:
        for k in ('explained_variance', 'policy_kl'):
            assert k + '/catch' in s and k + '/breakout' in s


def test_mixed_per_game_counts_and_sums(lib, cuda, monkeypatch):
    """catch+breakout, 8 envs, masks: each game has n = 4 T rows, and the games' sums add up to ``all``."""
    _single_process(monkeypatch)
    from actorcritic import session as sess
    from actorcritic import update_diag as ud
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.examples.atari.a2c_acktr import create_game_environments
    from actorcritic.multi_env import MultiEnv
    from actorcritic.objectives import A2CObjective
    N, T = 8, 5
    sess.reset_default_graph()
    env = MultiEnv(create_game_environments('catch+breakout', N, seed=4, full_action_set=True, env_offset=0))
    model = AtariModel(env.observation_space, env.action_space, 32, random_seed=3, init_seed=1)
    agent = MultiEnvAgent(env, model, T, mask_actions=True)
    diag = ud.UpdateDiagnostics.for_envs(env)
    assert diag.group_names[:2] == ('catch', 'breakout') and sorted(set(diag.groups.tolist())) == [0, 1]
    objective = A2CObjective(model, diagnostics=diag)
    op = objective.optimize_shared(_rmsprop(0.0007), 0.5, global_step=sess.get_or_create_global_step())
    with sess.Session() as s:
        obs, actions, rewards, terminals, next_obs, _ = agent.interact(s)
        diag.request()
        s.run([op], feed_dict={model.observations_placeholder: obs,
                               model.bootstrap_observations_placeholder: next_obs,
                               model.actions_placeholder: actions, model.rewards_placeholder: rewards,
                               model.terminals_placeholder: terminals}, host=False)
        scal = diag.read()
    env.close()
    acc = diag.last_acc
    assert acc['value'][:2, 0].tolist() == [4.0 * T, 4.0 * T] and acc['policy'][:2, 0].tolist() == [4.0 * T, 4.0 * T]
    assert not acc['value'][2:].any() and not acc['policy'][2:, :3].any()
    both = acc['policy'][:2]
    assert abs(scal['policy_kl'] - both[:, 1].sum() / (8 * T)) <= 1e-15
    assert scal['policy_kl_max'] == both[:, 3].max()
    assert abs(scal['policy_kl/catch'] - both[0, 1] / (4 * T)) <= 1e-15
    assert scal['explained_variance/breakout'] == ud.explained_variance(acc['value'][1])
    assert scal['explained_variance'] == ud.explained_variance(acc['value'].sum(axis=0))
    assert int(diag._dev['bad'].sum()) == 0


# -- through the example --------------------------------------------------------------------------
def _lines(directory):
    with open(os.path.join(str(directory), 'scalars.jsonl')) as f:
        return [json.loads(line) for line in f]


def test_example_logs_the_new_keys_only_with_the_option(lib, cuda, tmp_path, monkeypatch):
    from actorcritic import session as sess
    from actorcritic import update_diag as ud
    from actorcritic.examples.atari.a2c_acktr import train_a2c_acktr
    _single_process(monkeypatch)
    models = {}
    for name, kw in (('off', {}), ('on', dict(diagnostics=True)), ('default', dict(diagnostics=False))):
        sess.reset_default_graph()
        models[name], _ = train_a2c_acktr(False, 'DeviceGame', 4, 5, None, 'Run', summary_path=str(tmp_path / name),
                                          max_updates=4, seed=2, log_every=2, game='catch', **kw)
    off, on, default = (_lines(tmp_path / n) for n in ('off', 'on', 'default'))
    assert [l['step'] for l in off] == [l['step'] for l in on] == [l['step'] for l in default] == [1, 3]
    today = [list(l) for l in off]  # the key set of a run without the option
    assert [list(l) for l in default] == today
    new = {'explained_variance', 'value_mean', 'target_mean', 'target_std', 'policy_kl', 'policy_kl_max',
           'policy_entropy_after', 'grad_norm', 'step_norm', 'param_norm'}
    new |= {k + '/' + l for l in ud.LAYERS for k in ('grad_norm', 'step_norm')}  # (A2C: no K-FAC keys)
    for a, b in zip(off, on):
        assert list(b)[:len(a)] == list(a) and set(b) - set(a) == new
        assert all(a[k] == b[k] for k in a)  # the run is the same run: the old keys hold the same values
        assert b['step_norm'] > 0 and b['policy_kl'] >= 0
    assert _same(models['on'].params, models['off'].params)
