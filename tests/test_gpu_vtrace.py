"""GPU tests of the V-trace feature: acmi_vtrace against its rule book (actorcritic/vtrace.py), the reductions
to acmi_categorical and acmi_gae that hold bit for bit, the edge rules and argument checks, and
VTraceObjective / VTraceOptimizeOp against hand-driven chains of the same launches.

Every (N, T, A) of the shape sets runs in the kernel's four forms (plain, truncating, masked, both).  A case
holds: terminals nowhere (env 0), at step 0 (env 1), at step T-1 (env 2), everywhere (env 3), random beyond;
under truncation the terminal of env 2 at T-1 is a truncation (it boots from v_boot) and so is env 3's
mid-row one; log-ratios spread over [-3, 3] against bars 1.5 > 0.8, so both bind; under masks random legal
sets with the actions drawn inside them, but for one row whose taken action is illegal.

Weight accuracy: the OpenCL accuracy requirement for exp is 3 ulp and the device math library is built to
it; rho = min(rho_bar, expf(D)) adds no rounding, so |rho - min(rho_bar, exp(D))| <= 4 ulp is asserted with
D the float32 difference, the reference in float64.
"""
import functools
import itertools
import os
import sys

import numpy as np
import pytest
import torch

from actorcritic import _lib, _ops
from actorcritic import vtrace as rules

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
import oracle  # noqa: E402

pytestmark = pytest.mark.gpu

NS, TS, AS = (1, 3, 64, 257), (1, 2, 5, 20), (3, 4, 18, 32)
FORMS = ('plain', 'trunc', 'masked', 'masked-trunc')
GAMMA, LAM = 0.99, 0.95
RHO_BAR, C_BAR = 1.5, float(np.float32(0.8))  # (what the C ABI's float receives)
ERR_ARG = -1  # ACMI_ERR_ARG


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def words_of(S):
    A = S.shape[1]
    return (S.astype(np.uint64) << np.arange(A, dtype=np.uint64)).sum(1).astype(np.uint32)


def make_case(N, T, A, form, seed=0):
    """The host arrays of one case (flat rows m = n*T + t), a pure function of its arguments."""
    rng = np.random.default_rng([seed, N, T, A, FORMS.index(form)])
    M = N * T
    c = dict(N=N, T=T, A=A, form=form)
    c['logits'] = (1.5 * rng.standard_normal((M, A))).astype(np.float32)
    S = np.ones((M, A), bool)
    if 'masked' in form:
        S = rng.random((M, A)) < 0.6
        S[np.arange(M), rng.integers(0, A, M)] = True  # non-empty
    actions = np.array([rng.choice(np.flatnonzero(S[m])) for m in range(M)], np.int32)
    c['bad'] = 0
    if 'masked' in form:
        m = M // 2  # one row with an illegal taken action
        S[m, :] = True
        S[m, (actions[m] + 1) % A] = True
        S[m, actions[m]] = False
        c['bad'], c['bad_row'] = 1, m
        c['legal'] = words_of(S).view(np.int32)
    c['S'], c['actions'] = S, actions
    z = np.where(S, c['logits'].astype(np.float64), -np.inf)
    mx = z.max(1, keepdims=True)
    lp = z - (mx + np.log(np.exp(z - mx).sum(1, keepdims=True)))
    with np.errstate(invalid='ignore'):
        c['logp64'] = lp[np.arange(M), actions]  # (-inf at the illegal row)
    finite = np.where(np.isfinite(c['logp64']), c['logp64'], -1.0)
    c['blogp'] = (finite - rng.uniform(-3.0, 3.0, M)).astype(np.float32)
    c['rewards'] = rng.standard_normal((N, T)).astype(np.float32)
    c['values'] = rng.standard_normal((N, T)).astype(np.float32)
    c['v_boot'] = rng.standard_normal(N).astype(np.float32)
    d = rng.random((N, T)) < 0.2
    for n, pat in enumerate(('none', 'first', 'last', 'all')[:N]):
        d[n] = pat == 'all'
        if pat == 'first':
            d[n, 0] = True
        if pat == 'last':
            d[n, T - 1] = True
    c['terminals'] = d
    c['truncated'] = None
    if 'trunc' in form:
        tr = (rng.random((N, T)) < 0.5) & d
        if N > 2:
            tr[2, T - 1] = True  # at T-1: boots from v_boot
        if N > 3:
            tr[3, T // 2] = True  # mid-row (T = 1: the same step)
        c['truncated'] = tr
    return c


def call_vtrace(lib, c, rho_bar=RHO_BAR, c_bar=C_BAR, blogp=None, lam=LAM, want_logp=True, status=False, **over):
    """One acmi_vtrace launch on the case's arrays -> dict of host outputs (and the status, if asked)."""
    N, T, A = (over.get(k, c[k]) for k in ('N', 'T', 'A'))
    M = max(c['N'] * c['T'], 1)
    t = dict(logits=dev(c['logits']), actions=dev(c['actions']),
             blogp=dev(c['blogp']) if blogp is None else blogp, rewards=dev(c['rewards']),
             terminals=dev(c['terminals'].view(np.uint8)), values=dev(c['values']), v_boot=dev(c['v_boot']))
    trunc = None if c['truncated'] is None else dev(c['truncated'].view(np.uint8))
    legal = dev(c['legal']) if 'legal' in c else None
    t.update({k: v for k, v in over.items() if k in t})
    legal = over.get('legal', legal)
    bad = torch.zeros(1, dtype=torch.int32, device='cuda')
    out = {k: torch.full((M,), 7.0, device='cuda') for k in ('targets', 'adv', 'rho', 'logp')}
    st = lib.acmi_vtrace(_lib.ptr(t['logits']), over.get('ld', c['A']), A, _lib.ptr(t['actions']), _lib.ptr(t['blogp']),
                         _lib.ptr(t['rewards']), _lib.ptr(t['terminals']), _lib.ptr(trunc), _lib.ptr(t['values']),
                         _lib.ptr(t['v_boot']), N, T, over.get('gamma', GAMMA), lam, rho_bar, c_bar, _lib.ptr(legal),
                         _lib.ptr(bad), _lib.ptr(over.get('targets', out['targets'])), _lib.ptr(out['adv']),
                         _lib.ptr(out['rho']), _lib.ptr(out['logp']) if want_logp else None, _lib.stream_handle())
    if not status:
        _lib.check(st, 'acmi_vtrace')
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res['bad'] = int(bad.item())
    res['dev'] = out
    return (st, res) if status else res


@functools.lru_cache(maxsize=None)
def solved(lib, N, T, A, form):
    """A case, the kernel's outputs at the bars (1.5, 0.8), its weights at rho_bar = c_bar (the kernel's c),
    and the rule book's scan of the kernel's own weights: computed once, shared by the tests, never changed."""
    c = make_case(N, T, A, form)
    got = call_vtrace(lib, c)
    c_run = call_vtrace(lib, c, rho_bar=C_BAR, c_bar=C_BAR)
    ref = rules.vtrace_f32(got['rho'].reshape(N, T), c_run['rho'].reshape(N, T), c['rewards'], c['terminals'],
                           c['values'], c['v_boot'], GAMMA, LAM, truncated=c['truncated'])
    return c, got, c_run, ref


SHAPES = list(itertools.product(NS, TS, AS))


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('N,T,A', SHAPES)
def test_scan_is_bit_exact(lib, cuda, N, T, A, form):
    c, got, c_run, (tgt, adv) = solved(lib, N, T, A, form)
    assert np.array_equal(bits(c_run['rho']), bits(np.minimum(np.float32(C_BAR), got['rho'])))
    assert np.array_equal(bits(got['targets']), bits(tgt).reshape(-1))
    assert np.array_equal(bits(got['adv']), bits(adv).reshape(-1))
    assert np.isfinite(got['targets']).all() and np.isfinite(got['adv']).all()
    assert got['bad'] == c['bad'] and c_run['bad'] == c['bad']


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('N,T,A', SHAPES)
def test_weights_within_four_ulp(lib, cuda, N, T, A, form):
    c, got, c_run, _ = solved(lib, N, T, A, form)
    M = N * T
    L, AC = dev(c['logits']), dev(c['actions'])
    lp = torch.full((M,), 7.0, device=cuda)
    _ops.categorical(L, A, M, A, AC, None, lp, _lib.stream_handle(), legal=dev(c['legal']) if 'legal' in c else None)
    torch.cuda.synchronize()
    logp = lp.cpu().numpy()
    assert np.array_equal(bits(got['logp']), bits(logp))  # the kernel's log pi(a) is acmi_categorical's
    ok = np.isfinite(c['logp64'])
    assert np.array_equal(np.isneginf(logp), ~ok)
    worst = 0.0
    for bar, run in ((RHO_BAR, got), (C_BAR, c_run)):
        w64 = np.exp((logp - c['blogp']).astype(np.float64))  # (the float32 difference, as the kernel forms it)
        ref = np.minimum(bar, w64)
        ulp = np.spacing(ref.astype(np.float32)).astype(np.float64)
        err = np.abs(run['rho'].astype(np.float64) - ref) / ulp
        worst = max(worst, float(err.max()))
        assert err.max() <= 4.0, (bar, float(err.max()))
        assert (run['rho'] <= np.float32(bar)).all()
        clipped = w64 > bar * (1.0 + 8 * 2.0 ** -23)  # (beyond what 4 ulp of exp could bring back under the bar)
        assert (run['rho'][clipped] == np.float32(bar)).all()
        if M >= 64:
            assert clipped.any() and (~clipped).any()
    print('max ulp error of rho', worst)
    if 'masked' in form:
        assert got['rho'][c['bad_row']] == 0.0  # D = -inf: the illegal action weighs nothing


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('N,T,A', SHAPES)
def test_on_policy_targets_are_gae_bit_for_bit(lib, cuda, N, T, A, form):
    """behaviour_logp = the kernel's own logp and bars >= 1: every weight is exactly 1 and the targets are the
    bytes of acmi_gae / acmi_gae_trunc (the actions all legal: an illegal one weighs 0, which is not GAE)."""
    c = dict(solved(lib, N, T, A, form)[0])
    if c['bad']:
        c['actions'] = c['actions'].copy()
        c['actions'][c['bad_row']] = np.flatnonzero(c['S'][c['bad_row']])[0]
    first = call_vtrace(lib, c)
    assert first['bad'] == 0 and np.isfinite(first['logp']).all()
    r, d, v, vb = dev(c['rewards']), dev(c['terminals'].view(np.uint8)), dev(c['values']), dev(c['v_boot'])
    tg, ad = torch.zeros(N * T, device=cuda), torch.zeros(N * T, device=cuda)
    _ops.targets(r, d, v, vb, N, T, GAMMA, LAM, None, tg, ad, _lib.stream_handle(),
                 truncated=None if c['truncated'] is None else dev(c['truncated'].view(np.uint8)))
    torch.cuda.synchronize()
    for rho_bar, c_bar in ((1.0, 1.0), (2.0, 1.5)):
        got = call_vtrace(lib, c, rho_bar=rho_bar, c_bar=c_bar, blogp=first['dev']['logp'])
        assert (got['rho'] == 1.0).all()
        assert np.array_equal(bits(got['targets']), bits(tg.cpu().numpy()))


def test_edge_rules_and_bad_rows(lib, cuda):
    """D = +inf: the bars; D = -inf: 0; D a NaN: 0 -- and such a row contributes nothing: its target is V, its
    advantage 0.  Illegal taken actions count in bad_rows, once each."""
    N, T, A = 2, 4, 3
    inf = np.float32(np.inf)
    c = make_case(N, T, A, 'masked')
    c['terminals'][:] = False
    S = np.ones((N * T, A), bool)
    c['actions'] = np.zeros(N * T, np.int32)
    S[1, 0] = False  # row 1: illegal action, finite behaviour log-probability -> D = -inf
    S[2, 0] = False  # row 2: illegal action, behaviour -inf                  -> D = NaN
    c['legal'] = words_of(S).view(np.int32)
    c['blogp'] = np.full(N * T, -1.0, np.float32)
    c['blogp'][0] = -inf  # row 0: D = +inf
    c['blogp'][2] = -inf
    c['logits'][5, 0] = -inf  # row 5 (env 1): a legal action of probability 0 -> log pi = -inf, D = -inf
    got = call_vtrace(lib, c, rho_bar=2.0, c_bar=1.5)
    c_run = call_vtrace(lib, c, rho_bar=1.5, c_bar=1.5)
    assert got['bad'] == 2
    assert got['rho'][0] == 2.0 and c_run['rho'][0] == 1.5
    assert got['rho'][1] == 0.0 and got['rho'][2] == 0.0 and got['rho'][5] == 0.0
    assert np.isneginf(got['logp'][[1, 2, 5]]).all() and np.isfinite(got['logp'][[0, 3, 4, 6, 7]]).all()
    v = c['values'].reshape(-1)
    for m in (1, 2, 5):
        assert got['targets'][m] == v[m] and got['adv'][m] == 0.0
    assert np.isfinite(got['targets']).all() and np.isfinite(got['adv']).all()
    tgt, adv = rules.vtrace_f32(got['rho'].reshape(N, T), c_run['rho'].reshape(N, T), c['rewards'], c['terminals'],
                                c['values'], c['v_boot'], GAMMA, LAM)
    assert np.array_equal(bits(got['targets']), bits(tgt).reshape(-1))
    assert np.array_equal(bits(got['adv']), bits(adv).reshape(-1))
    rho, cc = rules.clipped_weights(got['logp'], c['blogp'], 2.0, 1.5, np.float64)
    assert np.array_equal(rho == 0.0, got['rho'] == 0.0) and rho[0] == 2.0 and cc[0] == 1.5
    # without a log_prob output the rest is the same
    again = call_vtrace(lib, c, rho_bar=2.0, c_bar=1.5, want_logp=False)
    assert np.array_equal(bits(again['targets']), bits(got['targets'])) and (again['logp'] == 7.0).all()


def test_empty_batches_and_bad_arguments_launch_nothing(lib, cuda):
    c = make_case(3, 5, 4, 'masked-trunc')
    untouched = lambda res: all((res[k] == 7.0).all() for k in ('targets', 'adv', 'rho', 'logp')) and res['bad'] == 0
    for empty in (dict(N=0), dict(T=0), dict(N=0, T=0)):
        st, res = call_vtrace(lib, c, status=True, **empty)
        assert st == 0 and untouched(res), empty
    bad_calls = [dict(lam=1.5), dict(lam=-0.1), dict(lam=float('nan')), dict(c_bar=0.0), dict(c_bar=-1.0),
                 dict(rho_bar=0.5, c_bar=0.8), dict(rho_bar=float('nan')), dict(N=-1), dict(T=-1), dict(A=0),
                 dict(ld=3), dict(A=33, ld=33)]  # (A = 33 with a mask: a legal-action word holds 32)
    for kw in bad_calls:
        st, res = call_vtrace(lib, c, status=True, **kw)
        assert st == ERR_ARG and untouched(res), kw
        assert b'acmi_vtrace' in lib.acmi_last_error()
    # a NULL required pointer
    args = dict(logits=dev(c['logits']), actions=dev(c['actions']), blogp=dev(c['blogp']), rewards=dev(c['rewards']),
                terminals=dev(c['terminals'].view(np.uint8)), values=dev(c['values']), v_boot=dev(c['v_boot']))
    out = [torch.full((15,), 7.0, device=cuda) for _ in range(3)]

    def status(**null):
        a = dict(args, **null)
        o = [None if null.get('out') == i else out[i] for i in range(3)]
        return lib.acmi_vtrace(_lib.ptr(a['logits']), 4, 4, _lib.ptr(a['actions']), _lib.ptr(a['blogp']),
                               _lib.ptr(a['rewards']), _lib.ptr(a['terminals']), None, _lib.ptr(a['values']),
                               _lib.ptr(a['v_boot']), 3, 5, GAMMA, LAM, RHO_BAR, C_BAR, None, None, _lib.ptr(o[0]),
                               _lib.ptr(o[1]), _lib.ptr(o[2]), None, _lib.stream_handle())

    for k in args:
        assert status(**{k: None}) == ERR_ARG, k
    for i in range(3):
        assert status(out=i) == ERR_ARG
    torch.cuda.synchronize()
    assert all((o == 7.0).all() for o in out)
    assert status() == 0  # (truncated, legal, bad_rows and log_prob are the nullable ones)
    torch.cuda.synchronize()
    assert not any((o == 7.0).any() for o in out)


# ---------------------------------------------------------------------------
# the objective and the update op
# ---------------------------------------------------------------------------
def _build(N=8, T=5, A=4, C3=64, seed=5):
    from actorcritic import session as sess
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.envs.atari.wrappers import SyntheticAtariEnvs
    from actorcritic.multi_env import MultiEnv
    sess.reset_default_graph()
    env = MultiEnv(SyntheticAtariEnvs(N, num_actions=A, seed=seed))
    params = oracle.init_params(A, C3, seed=1)
    model = AtariModel(env.observation_space, env.action_space, C3, params=params, random_seed=3)
    return env, model, MultiEnvAgent(env, model, T), sess.get_or_create_global_step()


def _rmsprop():
    from actorcritic.nn import ClipGlobalNormOptimizer, RMSPropOptimizer
    return ClipGlobalNormOptimizer(RMSPropOptimizer(learning_rate=7e-4), clip_norm=0.5)


def _feed(model, data):
    obs, act, rew, term, nxt, _ = data
    return {model.observations_placeholder: obs, model.bootstrap_observations_placeholder: nxt,
            model.actions_placeholder: act, model.rewards_placeholder: rew, model.terminals_placeholder: term}


def _batch(agent, s):
    """A rollout, copied: the ops then take a fresh batched forward of it, like the hand-driven chains."""
    return tuple(x.clone() if isinstance(x, torch.Tensor) else x for x in agent.interact(s))


def test_objective_with_stale_behaviour_matches_the_rule_book(lib, cuda):
    """8 envs x 5 steps, behaviour log-probabilities fed that are up to 1 off the policy's: the fetched targets,
    advantages and weights are the rule book's for the kernel's own weights, and the loss scalars and dhead are
    acmi_a2c_loss's on those targets, bit for bit."""
    from actorcritic import session as sess
    from actorcritic.objectives import VTraceObjective
    N, T, A = 8, 5, 4
    env, model, agent, gs = _build(N, T, A)
    eng = model.engine
    obj = VTraceObjective(model, 0.99, 0.01, gae_lambda=0.95, rho_bar=1.2, c_bar=0.9)
    M = N * T
    with sess.Session() as s:
        data = _batch(agent, s)
        feed = _feed(model, data)
        logp = s.run(model.policy.log_prob, feed_dict=feed)
        rng = np.random.default_rng(11)
        blogp = (np.asarray(logp, np.float32) - rng.uniform(-1.0, 1.0, (N, T))).astype(np.float32)
        feed[model.behaviour_log_probs_placeholder] = blogp
        pl, bl, ent, tg, adv, rho, vals, vb = s.run(
            [obj.policy_loss, obj.baseline_loss, obj.mean_entropy, obj.target_values, obj.advantage,
             obj.importance_weights, model.baseline.value, model.bootstrap_values], feed_dict=feed)
        st = eng.update_state(M)
        dhead, loss = st.dhead.clone(), st.loss.clone()
        fwd = st.fwd
        logits = fwd.flat_logits.clone()
    obs, act, rew, term, nxt, _ = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in data)
    assert (rho == np.float32(1.2)).any() and (rho < np.float32(0.9)).any()
    w64 = np.minimum(1.2, np.exp((np.asarray(logp, np.float32) - blogp).astype(np.float64)))
    np.testing.assert_allclose(rho, w64, rtol=4 * 2.0 ** -23)
    rtg, radv = rules.vtrace_f32(rho, np.minimum(np.float32(0.9), rho), rew, term, vals, vb, 0.99, 0.95)
    assert np.array_equal(bits(tg), bits(rtg)) and np.array_equal(bits(adv), bits(radv))
    ref_dhead = torch.full((M, eng.ldh), 7.0, device=cuda)
    ref_loss = torch.zeros(4, device=cuda)
    ws = torch.zeros(lib.acmi_a2c_loss_ws_floats(M), device=cuda)
    _ops.a2c_loss(logits, A, dev(vals.reshape(-1)), dev(act.reshape(-1).astype(np.int32)), dev(rtg.reshape(-1)),
                  dev(radv.reshape(-1)), M, A, 0.01, 0.5, 1.0, ref_dhead, eng.ldh, ws, ref_loss, _lib.stream_handle())
    torch.cuda.synchronize()
    assert torch.equal(dhead.view(torch.int32), ref_dhead.view(torch.int32))
    assert torch.equal(loss[:3].view(torch.int32), ref_loss[:3].view(torch.int32))
    assert [pl, bl, ent] == ref_loss[:3].cpu().tolist()


def test_unfed_single_pass_is_on_policy(lib, cuda):
    """Unfed, the batch's own forward is the behaviour policy: all weights are exactly 1 and the targets are
    A2CObjective's GAE(lambda) targets bit for bit; the inherited op updates the parameters."""
    from actorcritic import session as sess
    from actorcritic.nn import OptimizeOp
    from actorcritic.objectives import A2CObjective, VTraceObjective
    env, model, agent, gs = _build()
    vt = VTraceObjective(model, gae_lambda=0.95)
    a2c = A2CObjective(model, gae_lambda=0.95)
    op = vt.optimize_shared(_rmsprop(), 0.5, global_step=gs)
    assert type(op) is OptimizeOp
    with sess.Session() as s:
        data = _batch(agent, s)
        ref = s.run(a2c.target_values, feed_dict=_feed(model, data))
        before = model.params.clone()
        rho, tg, _ = s.run([vt.importance_weights, vt.target_values, op], feed_dict=_feed(model, data))
    assert rho.shape == (8, 5) and (rho == 1.0).all()
    assert np.array_equal(bits(tg), bits(ref))
    assert gs.value == 1 and torch.isfinite(model.params).all() and not torch.equal(model.params, before)


def test_optimize_op_equals_the_hand_driven_chain(lib, cuda):
    """2 epochs x 2 env slices of an 8 x 5 batch (4 gradient steps of 20 rows), behaviour = the batch's forward:
    the parameters after session.run equal, bit for bit, those of the same launches driven by hand through the
    engine's primitives -- slice forward, slice bootstrap forward, acmi_vtrace against the behaviour
    log-probabilities taken once, acmi_a2c_loss, backward, clip-wrapped RMSProp."""
    from actorcritic import session as sess
    from actorcritic.envs.atari.model import ForwardOut
    from actorcritic.objectives import VTraceObjective, ppo_minibatch_order
    N, T, A, epochs, nmb, seed = 8, 5, 4, 2, 2, 9
    env, model, agent, gs = _build(N, T, A)
    eng = model.engine
    obj = VTraceObjective(model, 0.99, 0.01, gae_lambda=0.95, rho_bar=1.5, c_bar=1.0)
    calls, snaps = [], []

    def callback(epoch, pos):
        calls.append((epoch, pos))
        snaps.append(model.params.clone())

    op = obj.optimize_shared(_rmsprop(), 0.5, num_epochs=epochs, num_minibatches=nmb, shuffle_seed=seed,
                             step_callback=callback, global_step=gs)
    with sess.Session() as s:
        data = _batch(agent, s)
        p0 = model.params.clone()
        step0 = gs.value
        out = s.run([op, obj.policy_loss, obj.baseline_loss, obj.mean_entropy, obj.importance_weights],
                    feed_dict=_feed(model, data))
        torch.cuda.synchronize()
        after = model.params.clone()
        last_loss = eng.update_state(N // nmb * T).loss[:3].clone()
    assert gs.value == step0 + 1
    assert calls == [(e, k) for e in range(epochs) for k in range(nmb)]
    order = ppo_minibatch_order(seed, step0, epochs, nmb)
    assert op.last_order == order and sorted(order[0]) == [0, 1]
    assert (out[4] == 1.0).all()  # (the batch's weights at the batch's forward)
    assert list(out[1:4]) == last_loss.cpu().tolist()  # the last gradient step's scalars
    assert not torch.equal(after, p0)

    # by hand, from the same parameters with a fresh optimizer
    model.params.copy_(p0)
    eng.bump_version()
    opt = _rmsprop()
    ctx = sess._RunContext(None, {})
    obs, act, rew, term, nxt, _ = data
    obs = obs.reshape(-1, 84, 84, 4)
    act = act.reshape(-1).to(torch.int32).contiguous()
    rew = rew.reshape(-1).to(torch.float32).contiguous()
    term = term.reshape(-1).to(torch.uint8).contiguous()
    M, envs = N * T, N // nmb
    rows = envs * T
    stream = eng.stream()
    whole = eng.activations(M, 'hand')
    eng.forward(obs.data_ptr(), M, whole.struct, want_value=True)
    blogp = torch.zeros(M, device=cuda)
    _ops.categorical(whole.logits, A, M, A, act, None, blogp, stream)
    rho = torch.zeros(M, device=cuda)
    k = 0
    for perm in order:
        for j in perm:
            sl = slice(j * rows, (j + 1) * rows)
            acts, bacts = eng.activations(rows, 'hand'), eng.activations(envs, 'hand_boot')
            o, b = obs[sl], nxt[j * envs:(j + 1) * envs]
            eng.forward(o.data_ptr(), rows, acts.struct, want_value=True)
            eng.forward(b.data_ptr(), envs, bacts.struct, want_value=True)
            st = eng.update_state(rows)
            _ops.vtrace(acts.logits, A, A, act[sl], blogp[sl], rew[sl], term[sl], acts.value, bacts.value, envs, T,
                        0.99, 0.95, 1.5, 1.0, st.targets, st.adv, rho[sl], stream)
            _ops.a2c_loss(acts.logits, A, acts.value, act[sl], st.targets, st.adv, rows, A, 0.01, 0.5, 1.0, st.dhead,
                          eng.ldh, st.loss_ws, st.loss, stream)
            eng.backward(ForwardOut(eng, acts, envs, T, o), st, with_stats=False)
            opt._apply_dense(ctx, eng, st.grads, 0.0)
            eng.bump_version()
            torch.cuda.synchronize()
            assert torch.equal(model.params, snaps[k]), 'gradient step {}'.format(k)
            if k > 0:
                assert not (rho[sl] == 1.0).all()  # the data are off-policy from the second step on
            k += 1
    assert k == epochs * nmb
    assert torch.equal(model.params, after)

    with pytest.raises(ValueError):  # 3 slices do not divide 8 envs
        with sess.Session() as s:
            s.run(obj.optimize_shared(_rmsprop(), num_minibatches=3, global_step=gs), feed_dict=_feed(model, data))


def test_example_runs_with_the_options_set(lib, cuda):
    from actorcritic import session as sess
    from actorcritic.examples.atari.vtrace import train_vtrace
    sess.reset_default_graph()
    seen = []
    model, _ = train_vtrace('catch', 8, 5, None, 'catch', max_updates=3, seed=1, game='catch', num_epochs=2,
                            num_minibatches=2, rho_bar=1.5, c_bar=1.0, gae_lambda=0.95,
                            on_update=lambda u, m: seen.append(m.params.clone()))
    assert len(seen) == 3 and torch.isfinite(model.params).all()
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    assert model.engine.version == 3 * 4  # four gradient steps an update
    model.engine.check_bad_rows()
