"""GPU tests of the PPO feature: acmi_ppo_loss and acmi_adam_apply against float64
restatements (below; the tower's float64 forward / backward, GAE, normalisation and
RMSProp come from oracle/oracle.py), the reductions to A2C that hold bit for bit, and
the epoch / minibatch update op step by step.  Tolerances are the project's own
(test_gpu_parity.py): loss scalars rel 1e-5, head gradients rtol 1e-4 / 1e-5, the
first-order optimizers' rtol 1e-6 (parameters) and 1e-5 (slots), and the per-element
update bound of test_a2c_update_matches_oracle.
"""
import os
import sys

import numpy as np
import pytest
import torch

from actorcritic import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
import oracle  # noqa: E402

pytestmark = pytest.mark.gpu

F32_EPS = np.finfo(np.float32).eps
MARGIN = 1e-3  # no generated row lies closer than this to a branch boundary


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------
def ppo_ref(logits, values, actions, old_logp, old_values, targets, adv, eps, vclip, beta=0.01, vcoef=0.5):
    """The PPO losses and head gradients of include/acmi.h (acmi_ppo_loss) in float64."""
    z = np.asarray(logits, np.float64)
    M, A = z.shape
    v, tg = np.asarray(values, np.float64), np.asarray(targets, np.float64)
    ad, olp = np.asarray(adv, np.float64), np.asarray(old_logp, np.float64)
    lp = oracle.log_softmax(z)
    p = np.exp(lp)
    H = -(p * lp).sum(-1)
    lpa = lp[np.arange(M), actions]
    r = np.exp(lpa - olp)
    s1, s2 = r * ad, np.clip(r, 1.0 - eps, 1.0 + eps) * ad
    pol_on = s1 <= s2
    e1 = (v - tg) ** 2
    val_on = np.ones(M, bool)
    e = e1
    if vclip > 0:
        vo = np.asarray(old_values, np.float64)
        e2 = (vo + np.clip(v - vo, -vclip, vclip) - tg) ** 2
        val_on = ~((np.abs(v - vo) > vclip) & (e2 > e1))
        e = np.maximum(e1, e2)
    onehot = np.eye(A)[actions]
    ent_term = beta * p * (lp + H[:, None]) / M  # the entropy bonus's share of dL/dlogits
    w = np.where(pol_on, ad * r, 0.0)
    return dict(policy_loss=-(np.mean(np.where(pol_on, s1, s2)) + beta * np.mean(H)), baseline_loss=np.mean(e / 2.0),
                mean_entropy=np.mean(H), approx_kl=np.mean(olp - lpa), clip_frac=np.mean(np.abs(r - 1.0) > eps),
                dlogits=-(w[:, None] * (onehot - p)) / M + ent_term, dvalue=np.where(val_on, vcoef * (v - tg), 0.0) / M,
                ent_term=ent_term, r=r, pol_on=pol_on, val_on=val_on)


def adam_ref(p, m, v, g, lr, t, clip_norm, beta1=0.9, beta2=0.999, eps=1e-8):
    """TF1 AdamOptimizer in float64 (after tf.clip_by_global_norm)."""
    sc = oracle.clip_scale(g, clip_norm)[0] if clip_norm > 0 else 1.0
    g = g * sc
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    lr_t = lr * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t)
    return p - lr_t * m / (np.sqrt(v) + eps), m, v


# ---------------------------------------------------------------------------
# kernel inputs with every branch populated and no row on a boundary
# ---------------------------------------------------------------------------
def _ratio_near_boundary(lpa, old_logp, eps):
    r = np.exp(lpa - old_logp.astype(np.float64))
    return (np.abs(r - (1.0 + eps)) < MARGIN) | (np.abs(r - (1.0 - eps)) < MARGIN)


def _value_near_boundary(values, old_values, targets, vclip):
    """|V - V_old| within MARGIN of vclip, or -- for a row that is clamped; inside the
    range Vc is V and there is no second branch -- the two squared errors within MARGIN."""
    v, vo, tg = (np.asarray(x, np.float64) for x in (values, old_values, targets))
    dv = v - vo
    e1, e2 = (v - tg) ** 2, (vo + np.clip(dv, -vclip, vclip) - tg) ** 2
    return (np.abs(np.abs(dv) - vclip) < MARGIN) | ((np.abs(dv) > vclip) & (np.abs(e1 - e2) < MARGIN))


def make_inputs(M, A, eps, vclip, seed):
    """Random float32 inputs; the old log-probabilities / values of a row that would sit
    within MARGIN of a branch boundary (in float64) are redrawn from the same seeded
    generator until it does not.  The log-ratio is uniform in [-0.25, 0.35]: around a
    third of the rows leave [1 - eps, 1 + eps] = [0.9, 1.1] on either side."""
    rng = np.random.default_rng(seed)
    d = dict(logits=rng.standard_normal((M, A)).astype(np.float32), actions=rng.integers(0, A, M).astype(np.int32),
             adv=rng.standard_normal(M).astype(np.float32), values=rng.standard_normal(M).astype(np.float32),
             targets=rng.standard_normal(M).astype(np.float32))
    lpa = oracle.log_softmax(d['logits'].astype(np.float64))[np.arange(M), d['actions']]
    d['old_logp'], d['old_values'] = np.empty(M, np.float32), np.empty(M, np.float32)
    todo = np.arange(M)
    while todo.size:
        d['old_logp'][todo] = (lpa[todo] - rng.uniform(-0.25, 0.35, todo.size)).astype(np.float32)
        todo = todo[_ratio_near_boundary(lpa[todo], d['old_logp'][todo], eps)]
    todo = np.arange(M)
    while todo.size:
        d['old_values'][todo] = (d['values'][todo] - rng.uniform(-0.5, 0.5, todo.size)).astype(np.float32)
        todo = todo[_value_near_boundary(d['values'][todo], d['old_values'][todo], d['targets'][todo], vclip)]
    d['lpa64'] = lpa
    return d


def run_ppo_loss(lib, cuda, d, A, ldh, eps, vclip, grad_scale=1.0, old_logp=None):
    M = d['logits'].shape[0]
    dhead = torch.full((M, ldh), 7.0, device=cuda)  # (the kernel must write the padding zeros itself)
    ws = torch.zeros(lib.acmi_ppo_loss_ws_floats(M), device=cuda)
    out, cf = torch.zeros(4, device=cuda), torch.zeros(1, device=cuda)
    t = {k: dev(d[k]) for k in ('logits', 'values', 'actions', 'old_values', 'targets', 'adv')}
    olp = dev(d['old_logp']) if old_logp is None else old_logp
    _lib.call('acmi_ppo_loss', _lib.ptr(t['logits']), A, _lib.ptr(t['values']), _lib.ptr(t['actions']), _lib.ptr(olp),
              _lib.ptr(t['old_values']), _lib.ptr(t['targets']), _lib.ptr(t['adv']), M, A, eps, vclip, 0.01, 0.5,
              grad_scale, _lib.ptr(dhead), ldh, _lib.ptr(ws), _lib.ptr(out), _lib.ptr(cf), _lib.stream_handle())
    torch.cuda.synchronize()
    return dhead, out, cf


EPS32, VCLIP32 = float(np.float32(0.1)), float(np.float32(0.2))  # what the C ABI's float receives


@pytest.mark.parametrize('vclip', [0.0, VCLIP32], ids=['vclip-off', 'vclip-0.2'])
@pytest.mark.parametrize('M,A,ldh', [(1000, 18, 20), (37, 4, 8)])
def test_ppo_loss_matches_float64(lib, cuda, M, A, ldh, vclip):
    """All four policy cases and both value branches (>= 50 rows each at M = 1000), no
    row within 1e-3 of a branch boundary, every row compared."""
    d = make_inputs(M, A, EPS32, VCLIP32, seed=21)
    assert not _ratio_near_boundary(d['lpa64'], d['old_logp'], EPS32).any()
    assert not _value_near_boundary(d['values'], d['old_values'], d['targets'], VCLIP32).any()
    ref = ppo_ref(d['logits'], d['values'], d['actions'], d['old_logp'], d['old_values'], d['targets'], d['adv'],
                  EPS32, vclip)
    pos, r = d['adv'] > 0, ref['r']
    cases = [pos & (r > 1 + EPS32), pos & ~(r > 1 + EPS32), ~pos & (r < 1 - EPS32), ~pos & ~(r < 1 - EPS32)]
    assert np.array_equal(ref['pol_on'], cases[1] | cases[3])
    if M == 1000:
        assert min(int(c.sum()) for c in cases) >= 50, [int(c.sum()) for c in cases]
        if vclip > 0:
            assert min(int(ref['val_on'].sum()), int((~ref['val_on']).sum())) >= 50

    dhead, out, cf = run_ppo_loss(lib, cuda, d, A, ldh, EPS32, vclip)
    got, dh = out.cpu().numpy(), dhead.cpu().numpy()
    print('scalars', got, float(cf), [ref[k] for k in ('policy_loss', 'baseline_loss', 'mean_entropy', 'approx_kl',
                                                        'clip_frac')])
    assert got[0] == pytest.approx(ref['policy_loss'], rel=1e-5, abs=1e-7)
    assert got[1] == pytest.approx(ref['baseline_loss'], rel=1e-5)
    assert got[2] == pytest.approx(ref['mean_entropy'], rel=1e-5)
    assert got[3] == pytest.approx(ref['approx_kl'], rel=1e-5)
    assert float(cf) == pytest.approx(ref['clip_frac'], rel=1e-5, abs=1e-7)
    np.testing.assert_allclose(dh[:, :A], ref['dlogits'], rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(dh[:, A], ref['dvalue'], rtol=1e-5, atol=1e-10)
    assert not dh[:, A + 1:].any()
    # a clipped row keeps the entropy bonus's gradient only; a clipped value none
    off = ~ref['pol_on']
    np.testing.assert_allclose(dh[off, :A], ref['ent_term'][off], rtol=1e-4, atol=1e-9)
    assert not dh[~ref['val_on'], A].any()


def test_ppo_loss_reduces_to_a2c_bit_for_bit(lib, cuda):
    """old_logp from acmi_categorical on the same logits, vclip off: r is exactly 1, so
    dhead, the baseline loss and the mean entropy are acmi_a2c_loss's bytes, and the
    approximate KL and the clip fraction are exactly 0.

    The policy-loss scalar cannot be acmi_a2c_loss's: at r = 1 the surrogate
    -(mean(min(r adv, clip(r) adv)) + beta mean(H)) is -(mean(adv) + beta mean(H)), where
    A2C reports -(mean(adv log pi(a)) + beta mean(H)) -- equal gradients, different
    values.  It is checked against float64 at the loss tolerance instead, and must
    not depend on clip_eps."""
    M, A, ldh = 1000, 18, 20
    d = make_inputs(M, A, EPS32, VCLIP32, seed=22)
    L, AC = dev(d['logits']), dev(d['actions'])
    olp = torch.zeros(M, device=cuda)
    _lib.call('acmi_categorical', _lib.ptr(L), A, M, A, _lib.ptr(AC), None, _lib.ptr(olp), _lib.stream_handle())
    dhead, out, cf = run_ppo_loss(lib, cuda, d, A, ldh, EPS32, 0.0, old_logp=olp)

    a2c_dhead = torch.full((M, ldh), 7.0, device=cuda)
    ws = torch.zeros(lib.acmi_a2c_loss_ws_floats(M), device=cuda)
    a2c_out = torch.zeros(4, device=cuda)
    V, TG, AD = dev(d['values']), dev(d['targets']), dev(d['adv'])
    _lib.call('acmi_a2c_loss', _lib.ptr(L), A, _lib.ptr(V), _lib.ptr(AC), _lib.ptr(TG), _lib.ptr(AD), M, A, 0.01, 0.5,
              1.0, _lib.ptr(a2c_dhead), ldh, _lib.ptr(ws), _lib.ptr(a2c_out), _lib.stream_handle())
    torch.cuda.synchronize()
    assert torch.equal(dhead.view(torch.int32), a2c_dhead.view(torch.int32))
    assert torch.equal(out[1:3].view(torch.int32), a2c_out[1:3].view(torch.int32))
    assert float(out[3]) == 0.0 and float(cf) == 0.0
    ad64 = d['adv'].astype(np.float64)
    ref_pl = -(ad64.mean() + 0.01 * oracle.entropy(d['logits'].astype(np.float64)).mean())
    assert float(out[0]) == pytest.approx(ref_pl, rel=1e-5, abs=1e-7)
    _, out2, _ = run_ppo_loss(lib, cuda, d, A, ldh, 0.3, 0.0, old_logp=olp)
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32))


def test_masked_ppo_loss_reduces_to_masked_a2c_bit_for_bit_past_one_block(lib, cuda):
    """The same identity under legal-action masks, one row past the loss kernels' 256-row
    block: random non-empty legal sets, the actions drawn under them, old_logp from
    acmi_categorical_masked on the same logits and masks.  dhead, the baseline loss and
    the mean entropy are acmi_a2c_loss_masked's bits, the approximate KL and the clip
    fraction exactly 0, no row is counted as bad."""
    M, A, ldh = 257, 18, 20
    d = make_inputs(M, A, EPS32, VCLIP32, seed=24)
    rng = np.random.default_rng(25)
    S = rng.random((M, A)) < 0.5
    S[np.arange(M), rng.integers(0, A, M)] = True  # non-empty
    S[0], S[M - 1, :] = True, False
    S[M - 1, A - 1] = True  # a full row, and a single-action row in the second block
    actions = np.array([rng.choice(np.flatnonzero(S[m])) for m in range(M)], np.int32)
    words = (S.astype(np.uint64) << np.arange(A, dtype=np.uint64)).sum(1).astype(np.uint32)
    L, AC, legal = dev(d['logits']), dev(actions), dev(words.view(np.int32))
    V, TG, AD, OV = (dev(d[k]) for k in ('values', 'targets', 'adv', 'old_values'))
    bad = torch.zeros(1, dtype=torch.int32, device=cuda)
    st = _lib.stream_handle()
    olp = torch.zeros(M, device=cuda)
    _lib.call('acmi_categorical_masked', _lib.ptr(L), A, M, A, _lib.ptr(AC), _lib.ptr(legal), None, _lib.ptr(olp), st)

    ppo_dhead, a2c_dhead = (torch.full((M, ldh), 7.0, device=cuda) for _ in range(2))
    ppo_out, a2c_out, cf = torch.zeros(4, device=cuda), torch.zeros(4, device=cuda), torch.ones(1, device=cuda)
    ws = torch.zeros(lib.acmi_ppo_loss_ws_floats(M), device=cuda)
    _lib.call('acmi_ppo_loss_masked', _lib.ptr(L), A, _lib.ptr(V), _lib.ptr(AC), _lib.ptr(olp), _lib.ptr(OV),
              _lib.ptr(TG), _lib.ptr(AD), M, A, EPS32, 0.0, 0.01, 0.5, 1.0, _lib.ptr(ppo_dhead), ldh, _lib.ptr(ws),
              _lib.ptr(ppo_out), _lib.ptr(cf), _lib.ptr(legal), _lib.ptr(bad), st)
    ws2 = torch.zeros(lib.acmi_a2c_loss_ws_floats(M), device=cuda)
    _lib.call('acmi_a2c_loss_masked', _lib.ptr(L), A, _lib.ptr(V), _lib.ptr(AC), _lib.ptr(TG), _lib.ptr(AD), M, A,
              0.01, 0.5, 1.0, _lib.ptr(a2c_dhead), ldh, _lib.ptr(ws2), _lib.ptr(a2c_out), _lib.ptr(legal),
              _lib.ptr(bad), st)
    torch.cuda.synchronize()
    assert int(bad.item()) == 0
    assert torch.isfinite(a2c_dhead).all() and a2c_dhead[:, :A].abs().sum() > 0
    assert torch.equal(ppo_dhead.view(torch.int32), a2c_dhead.view(torch.int32))
    assert torch.equal(ppo_out[1:3].view(torch.int32), a2c_out[1:3].view(torch.int32))
    assert float(ppo_out[3]) == 0.0 and float(cf) == 0.0
    # (the policy-loss scalars differ by construction, see above: PPO's against float64 over the legal sets)
    z = np.where(S, d['logits'].astype(np.float64), -np.inf)
    lp = z - (z.max(1, keepdims=True) + np.log(np.exp(z - z.max(1, keepdims=True)).sum(1, keepdims=True)))
    H = -np.where(S, np.exp(lp) * np.where(S, lp, 0.0), 0.0).sum(1)
    ref_pl = -(d['adv'].astype(np.float64).mean() + 0.01 * H.mean())
    assert float(ppo_out[0]) == pytest.approx(ref_pl, rel=1e-5, abs=1e-7)


def test_ppo_loss_grad_scale_and_argument_errors(lib, cuda):
    M, A, ldh = 1000, 18, 20
    d = make_inputs(M, A, EPS32, VCLIP32, seed=23)
    one = run_ppo_loss(lib, cuda, d, A, ldh, EPS32, VCLIP32, grad_scale=1.0)
    half = run_ppo_loss(lib, cuda, d, A, ldh, EPS32, VCLIP32, grad_scale=0.5)
    for a, b in zip(one, half):
        assert a.abs().sum() > 0
        assert torch.equal((a * 0.5).view(torch.int32), b.view(torch.int32))

    t = {k: dev(d[k]) for k in ('logits', 'values', 'actions', 'old_logp', 'old_values', 'targets', 'adv')}
    dhead = torch.zeros(M, ldh, device=cuda)
    ws = torch.zeros(lib.acmi_ppo_loss_ws_floats(M), device=cuda)
    out, cf = torch.zeros(4, device=cuda), torch.zeros(1, device=cuda)

    def status(ldh_arg=ldh, old_logp=t['old_logp'], old_values=t['old_values'], eps=EPS32, vclip=VCLIP32):
        return lib.acmi_ppo_loss(_lib.ptr(t['logits']), A, _lib.ptr(t['values']), _lib.ptr(t['actions']),
                                 _lib.ptr(old_logp), _lib.ptr(old_values), _lib.ptr(t['targets']), _lib.ptr(t['adv']),
                                 M, A, eps, vclip, 0.01, 0.5, 1.0, _lib.ptr(dhead), ldh_arg, _lib.ptr(ws),
                                 _lib.ptr(out), _lib.ptr(cf), _lib.stream_handle())

    ERR_ARG = -1  # ACMI_ERR_ARG
    assert status() == 0
    assert status(ldh_arg=A) == ERR_ARG
    assert status(old_logp=None) == ERR_ARG
    assert status(eps=0.0) == ERR_ARG and status(eps=-0.1) == ERR_ARG
    assert status(old_values=None) == ERR_ARG  # (needed by vclip > 0 ...)
    assert status(old_values=None, vclip=0.0) == 0  # (... and by nothing else)
    torch.cuda.synchronize()


@pytest.mark.parametrize('clip_norm', [0.0, 0.5], ids=['noclip', 'clip'])
@pytest.mark.parametrize('t', [1, 7])
def test_adam_kernel_matches_float64(lib, cuda, t, clip_norm):
    rng = np.random.default_rng(31)
    n, lr, b1, b2, eps = 100003, 2.5e-4, 0.9, 0.999, 1e-5
    p = rng.standard_normal(n).astype(np.float32)
    g = rng.standard_normal(n).astype(np.float32)
    m = (0.1 * rng.standard_normal(n)).astype(np.float32)
    v = rng.uniform(0.1, 1.1, n).astype(np.float32)
    P, M_, V, G = dev(p), dev(m), dev(v), dev(g)
    ws = torch.zeros(lib.acmi_opt_ws_floats(n), device=cuda)
    norm = torch.zeros(1, device=cuda)
    lr_t = lr * (1.0 - b2 ** t) ** 0.5 / (1.0 - b1 ** t)
    _lib.call('acmi_adam_apply', _lib.ptr(P), _lib.ptr(M_), _lib.ptr(V), _lib.ptr(G), n, lr_t, b1, b2, eps,
              clip_norm, _lib.ptr(ws), _lib.ptr(norm), _lib.stream_handle())
    rp, rm, rv = adam_ref(p.astype(np.float64), m.astype(np.float64), v.astype(np.float64), g.astype(np.float64), lr,
                          t, clip_norm, b1, b2, eps)
    assert not np.array_equal(rp.astype(np.float32), p)
    np.testing.assert_allclose(P.cpu().numpy(), rp, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(M_.cpu().numpy(), rm, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(V.cpu().numpy(), rv, rtol=1e-5)
    assert norm.item() == pytest.approx(np.linalg.norm(g.astype(np.float64)), rel=1e-5)


# ---------------------------------------------------------------------------
# the update op
# ---------------------------------------------------------------------------
def _build(N=4, T=5, A=4, C3=64, seed=5):
    from actorcritic import session as sess
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.envs.atari.wrappers import SyntheticAtariEnvs
    from actorcritic.multi_env import MultiEnv
    sess.reset_default_graph()
    env = MultiEnv(SyntheticAtariEnvs(N, num_actions=A, seed=seed))
    params = oracle.init_params(A, C3, seed=1)
    model = AtariModel(env.observation_space, env.action_space, C3, params=params, random_seed=3)
    return env, model, MultiEnvAgent(env, model, T), sess.get_or_create_global_step(), params


def _rmsprop():
    from actorcritic.nn import ClipGlobalNormOptimizer, RMSPropOptimizer
    return ClipGlobalNormOptimizer(RMSPropOptimizer(learning_rate=7e-4), clip_norm=0.5)


def _feed(model, data):
    obs, act, rew, term, nxt, _ = data
    return {model.observations_placeholder: obs, model.bootstrap_observations_placeholder: nxt,
            model.actions_placeholder: act, model.rewards_placeholder: rew, model.terminals_placeholder: term}


def test_ppo_update_matches_oracle_step_by_step(lib, cuda):
    """2 epochs x 2 env slices of a 4 x 5 batch (4 gradient steps of 10 rows), clip-wrapped
    RMSProp: every step, started from the GPU's parameters before it, matches a float64
    step (tower forward on the slice at those parameters; PPO loss against old
    log-probabilities, values, GAE targets and normalised advantages formed in float64
    at the batch's parameters; backward; RMSProp with the reference's own slot state)
    within test_a2c_update_matches_oracle's per-element bound.

    The ratios stay near 1 over four small steps: this test covers the plumbing
    (slices, pointer offsets, re-forward, slot carry-over, step order, global step);
    test_ppo_loss_matches_float64 covers the clipping branches."""
    from actorcritic import session as sess
    from actorcritic.objectives import PPOObjective
    N, T, A, C3, epochs, nmb, seed = 4, 5, 4, 64, 2, 2, 9
    env, model, agent, gs, params = _build(N, T, A, C3)
    obj = PPOObjective(model)
    snaps, calls = [], []

    def callback(epoch, pos):
        calls.append((epoch, pos))
        snaps.append(model.params.clone())

    op = obj.optimize_shared(_rmsprop(), 0.5, num_epochs=epochs, num_minibatches=nmb, shuffle_seed=seed,
                             step_callback=callback, global_step=gs)
    with sess.Session() as s:
        data = agent.interact(s)
        assert model.engine.lookup_rollout(data[0]) is not None  # (the op takes the rollout's activations)
        snaps.append(model.params.clone())
        step0 = gs.value
        out = s.run([op, obj.policy_loss, obj.baseline_loss, obj.mean_entropy, obj.approx_kl, obj.clip_fraction],
                    feed_dict=_feed(model, data))
    assert gs.value == step0 + 1
    assert calls == [(e, k) for e in range(epochs) for k in range(nmb)]
    rng = np.random.default_rng([seed, step0])
    order = [[int(j) for j in rng.permutation(nmb)] for _ in range(epochs)]
    assert op.last_order == order

    obs, act, rew, term, nxt, _ = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in data)
    obs, act = obs.reshape(-1, 84, 84, 4), act.reshape(-1)
    p0 = snaps[0].cpu().numpy().astype(np.float64)
    full = oracle.forward(p0, obs, A, C3)
    vb = oracle.forward(p0, nxt, A, C3)['value']
    tg, adv = oracle.gae_f64(rew, term, full['value'].reshape(N, T), vb, 0.99, 0.95)
    tg, adv = tg.reshape(-1), oracle.normalize_advantages(adv).reshape(-1)
    old_logp = oracle.log_softmax(full['logits'])[np.arange(N * T), act]
    old_values = full['value']
    ms, mom = np.ones_like(p0), np.zeros_like(p0)
    rows = N // nmb * T
    k, last = 0, None
    for perm in order:
        for j in perm:
            sl = slice(j * rows, (j + 1) * rows)
            pb = snaps[k].cpu().numpy().astype(np.float64)
            got = snaps[k + 1].cpu().numpy().astype(np.float64)
            part = oracle.forward(pb, obs[sl], A, C3)
            last = ppo_ref(part['logits'], part['value'], act[sl], old_logp[sl], old_values[sl], tg[sl], adv[sl],
                           0.1, 0.0)
            grads, _ = oracle.backward(pb, part, last['dlogits'], last['dvalue'], A, C3)
            rp, ms, mom = oracle.rmsprop_apply(pb, ms, mom, grads, 7e-4, 0.5)
            bound = 1e-3 * np.abs(rp - pb) + 2 * F32_EPS * np.abs(pb) + 1e-12
            err = np.abs(got - rp)
            print('step', k, 'slice', j, 'max err/bound', float((err / bound).max()), 'max |r-1|',
                  float(np.abs(last['r'] - 1).max()))
            assert np.all(err <= bound), 'gradient step {}'.format(k)
            k += 1
    assert k == epochs * nmb == len(snaps) - 1
    # the fetched scalars are the last gradient step's
    assert out[1] == pytest.approx(last['policy_loss'], rel=1e-4, abs=1e-6)
    assert out[2] == pytest.approx(last['baseline_loss'], rel=1e-4)
    assert out[3] == pytest.approx(last['mean_entropy'], rel=1e-5)
    assert out[4] == pytest.approx(last['approx_kl'], rel=1e-2, abs=1e-6)
    assert out[5] == pytest.approx(last['clip_frac'], abs=1e-7)

    with pytest.raises(ValueError):  # 3 slices do not divide 4 envs
        with sess.Session() as s:
            s.run(obj.optimize_shared(_rmsprop(), num_minibatches=3, global_step=gs), feed_dict=_feed(model, data))


def test_ppo_single_step_equals_a2c_update(lib, cuda):
    """One epoch of one minibatch without value clipping is the A2C update of the same
    GAE / normalisation options: the parameters come out bit-identical."""
    from actorcritic import session as sess
    from actorcritic.objectives import A2CObjective, PPOObjective
    env, model, agent, gs, params = _build()
    a2c = A2CObjective(model, gae_lambda=0.95, normalize_advantages=True)
    ppo = PPOObjective(model, gae_lambda=0.95, normalize_advantages=True, value_clip_range=None)
    op_a2c = a2c.optimize_shared(_rmsprop(), 0.5, global_step=gs)
    op_ppo = ppo.optimize_shared(_rmsprop(), 0.5, num_epochs=1, num_minibatches=1, global_step=gs)
    with sess.Session() as s:
        # a copy of the batch: both ops take a fresh batched forward of the same inputs
        data = tuple(x.clone() if isinstance(x, torch.Tensor) else x for x in agent.interact(s))
        p0 = model.params.clone()
        s.run(op_a2c, feed_dict=_feed(model, data))
        after_a2c = model.params.clone()
        model.params.copy_(p0)
        model.engine.bump_version()
        kl, cf, _ = s.run([ppo.approx_kl, ppo.clip_fraction, op_ppo], feed_dict=_feed(model, data))
    assert not torch.equal(after_a2c, p0)
    assert torch.equal(model.params, after_a2c)
    assert kl == 0.0 and cf == 0.0 and gs.value == 2


def test_ppo_adam_resume_is_bit_identical(lib, cuda, tmp_path):
    """PPO with clip-wrapped Adam: a checkpoint written between two updates and restored
    into a fresh graph gives the uninterrupted run's second update bit for bit -- the
    Adam moments and the step count come back with the parameters and the global step
    (which also seeds the slice order)."""
    from actorcritic import checkpoint
    from actorcritic import session as sess
    from actorcritic.examples.atari.ppo import create_optimizer
    from actorcritic.objectives import PPOObjective

    def graph():
        env, model, agent, gs, params = _build()
        opt = create_optimizer(2.5e-4)
        op = PPOObjective(model, value_clip_range=0.2).optimize_shared(opt, 0.5, num_epochs=2, num_minibatches=2,
                                                                       shuffle_seed=4, global_step=gs)
        return model, agent, gs, opt, op, params

    model, agent, gs, opt, op, params = graph()
    with sess.Session() as s:
        s.run(op, feed_dict=_feed(model, agent.interact(s)))
        data = tuple(x.clone() if isinstance(x, torch.Tensor) else x for x in agent.interact(s))
        path = checkpoint.save(str(tmp_path / 'Atari'), gs.value, model, opt)
        saved = {k: v.clone() for k, v in opt.slots().items()}
        s.run(op, feed_dict=_feed(model, data))
    torch.cuda.synchronize()
    uninterrupted, gs_after, order = model.params.clone(), gs.value, op.last_order
    assert int(saved['_t'][0]) == 4 and int(opt.slots()['_t'][0]) == 8

    model2, agent2, gs2, opt2, op2, _ = graph()
    checkpoint.load(path, model2, opt2, gs2)
    assert sorted(opt2.slots()) == ['_m', '_t', '_v']
    for k, v in opt2.slots().items():
        assert torch.equal(v.cpu(), saved[k].cpu()), k
    with sess.Session() as s:
        s.run(op2, feed_dict=_feed(model2, data))
    torch.cuda.synchronize()
    assert gs2.value == gs_after and op2.last_order == order
    assert not torch.equal(model2.params, torch.from_numpy(params).cuda())
    assert torch.equal(model2.params, uninterrupted)
