"""GPU tests of the per-game reward scaling ("Return normalisation"):
acmi_retnorm_scan / acmi_retnorm_apply against the numpy reference
(actorcritic.return_norm.host_return_norm) on identical inputs, at the smallest shapes at
which the kernels can still go wrong; determinism, bad group ids, env shards; the objectives'
``normalize_returns``; and the learning test.

Bounds.  carry: bit for bit (float32, fixed operation order).  moments: the count exact; a sum
of n doubles in any order is within n 2^-53 sum|x| of the exact sum (math.fsum here), and
u*u is exact in double.  stats: 1e-12 relative (a dozen double operations) to the reference
merge of the device's own moments.  out: 1 float32 ulp of the reference scale with the
device's own stats (one double sqrt and division rounded to float32, one float32 product).
"""
import math

import numpy as np
import pytest
import torch

from actorcritic import _lib
from actorcritic import return_norm as rn

pytestmark = pytest.mark.gpu

PAD = 8  # canary elements on either side of every buffer
GAMMA = 0.99
RETNORM_LEARN_UPDATES = 3500  # 2 x U, U = 1750: DESIGN.md 7d "Return normalisation"


# -- inputs ---------------------------------------------------------------------------------
def make_case(N, T, G, seed, empty=(), small_m2=None):
    """Rewards from {0, +-1, 3}, about one nonzero in five; terminals about one in seven plus
    the first step of env 0, the last step of env N-1 and (T >= 3) two in a row in env N//2;
    a non-zero incoming carry and non-zero incoming stats.  small_m2: that group's incoming
    statistics are a million samples of variance 0.04, so it scales by about 5 and a reward of 3
    clamps at 10 while a reward of 1 does not."""
    rng = np.random.RandomState(seed)
    r = np.where(rng.rand(N, T) < 0.2, rng.choice([-1.0, 1.0, 3.0], size=(N, T)), 0.0).astype(np.float32)
    d = (rng.rand(N, T) < 1 / 7).astype(np.uint8)
    d[0, 0] = 1
    d[N - 1, T - 1] = 1
    if T >= 3:
        d[N // 2, 1:3] = 1
    live = [g for g in range(G) if g not in empty]
    grp = np.array([live[n % len(live)] for n in range(N)], np.uint8)
    carry = rng.randn(N).astype(np.float32)
    stats = np.stack([rng.randint(5, 50, G).astype(np.float64), rng.randn(G), rng.rand(G) * 20 + 1], axis=1)
    if small_m2 is not None:
        stats[small_m2] = (1e6, 0.1, 0.04e6)
    return dict(N=N, T=T, G=G, r=r, d=d, grp=grp, carry=carry, stats=stats)


CASES = {
    'one': dict(N=1, T=1, G=1, seed=1),
    'empty-group': dict(N=3, T=5, G=2, seed=2, empty=(1,)),
    'crosses-a-wave': dict(N=65, T=5, G=2, seed=3),
    'crosses-a-block': dict(N=257, T=20, G=3, seed=4, small_m2=0),
    'a-group-an-env': dict(N=64, T=1, G=64, seed=5),
}


# -- running the kernels ------------------------------------------------------------------
def padded(values, cuda, canary):
    """(whole buffer, the view the kernel gets): PAD canaries, the values, PAD canaries."""
    v = torch.from_numpy(np.ascontiguousarray(values)).reshape(-1)
    full = torch.full((v.numel() + 2 * PAD,), canary, dtype=v.dtype)
    full[PAD:PAD + v.numel()] = v
    full = full.to(cuda)
    return full, full[PAD:PAD + v.numel()]


def canaries_intact(full, canary):
    ends = torch.cat([full[:PAD], full[-PAD:]]).cpu()
    return bool((ends == canary).all())


def run_device(lib, cuda, c, clip=10.0, eps=1e-8, inplace=False, scan=True, apply=True, G=None, moments_in=None,
               bad_start=0):
    """One scan + apply from the case's state; every output buffer starts as NaN and sits
    between canaries, which are checked here.  -> host arrays."""
    N, T = c['N'], c['T']
    G = c['G'] if G is None else G
    nan = float('nan')
    bufs = {}

    def buf(name, values, canary):
        bufs[name] = (padded(values, cuda, canary), canary)
        return bufs[name][0][1]
    r = buf('r', c['r'], 77.0)
    d = buf('d', c['d'], 9)
    grp = buf('grp', c['grp'], 200)
    carry = buf('carry', c['carry'], 55.0)
    stats = buf('stats', c['stats'], 66.0)
    ws = buf('ws', np.full(int(lib.acmi_retnorm_ws_doubles(N)), nan), 44.0)
    mom = buf('mom', np.full((G, 3), nan) if moments_in is None else moments_in, 33.0)
    out = r if inplace else buf('out', np.full((N, T), nan, np.float32), 22.0)
    inv = buf('inv', np.full(G, nan, np.float32), 11.0)
    bad = buf('bad', np.full(1, bad_start, np.int32), -3)
    stream = _lib.stream_handle(cuda)
    if scan:
        _lib.call('acmi_retnorm_scan', _lib.ptr(r), _lib.ptr(d), _lib.ptr(grp), N, T, G, GAMMA, _lib.ptr(carry),
                  _lib.ptr(ws), _lib.ptr(mom), _lib.ptr(bad), stream)
    if apply:
        _lib.call('acmi_retnorm_apply', _lib.ptr(r), _lib.ptr(grp), N, T, G, _lib.ptr(mom), _lib.ptr(stats), eps,
                  clip, _lib.ptr(out), _lib.ptr(inv), stream)
    torch.cuda.synchronize()
    for name, ((full, _), canary) in bufs.items():
        assert canaries_intact(full, canary), 'canary of ' + name
    if not inplace:  # the inputs are read only
        assert np.array_equal(r.cpu().numpy().reshape(N, T), c['r'])
    assert np.array_equal(d.cpu().numpy().reshape(N, T), c['d']) and np.array_equal(grp.cpu().numpy(), c['grp'])
    return dict(out=out.cpu().numpy().reshape(N, T), carry=carry.cpu().numpy(), stats=stats.cpu().numpy().reshape(G, 3),
                moments=mom.cpu().numpy().reshape(G, 3), inv=inv.cpu().numpy(), bad=int(bad.item()))


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def exact_moments(c, G, keep=None):
    """Per group (count, fsum u, fsum u^2) and the bounds n 2^-53 sum|u|, n 2^-53 sum u^2."""
    u, _ = rn.host_samples(c['r'], c['d'], GAMMA, c['carry'])
    grp = c['grp'].astype(np.int64)
    ref, bound = np.zeros((G, 3)), np.zeros((G, 3))
    for g in range(G):
        rows = (grp == g) if keep is None else ((grp == g) & keep)
        x = [float(v) for v in u[rows].reshape(-1)]
        n = len(x)
        ref[g] = (n, math.fsum(x), math.fsum(v * v for v in x))
        bound[g] = (0.0, n * 2.0 ** -53 * math.fsum(abs(v) for v in x), n * 2.0 ** -53 * ref[g, 2])
    return ref, bound


def stats_close(got, ref, rel=1e-12):
    """Elementwise |got - ref| <= rel |ref| on count, mean and M2 (the counts: equal)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.array_equal(got[:, 0], ref[:, 0]) and bool(np.all(np.abs(got - ref) <= rel * np.abs(ref)))


def within_one_ulp(got, ref):
    return np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref)).astype(np.float64))


def check_against_host(c, got, clip=10.0, eps=1e-8):
    G = c['G']
    ref_out, ref_carry, ref_stats, ref_mom = rn.host_return_norm(c['r'], c['d'], c['grp'], G, GAMMA, carry=c['carry'],
                                                                 stats=c['stats'], epsilon=eps, clip=clip)
    assert np.array_equal(bits(got['carry']), bits(ref_carry))
    exact, bound = exact_moments(c, G)
    assert np.array_equal(got['moments'][:, 0], exact[:, 0]) and np.array_equal(exact[:, 0], ref_mom[:, 0])
    err = np.abs(got['moments'] - exact)
    print('moments: max error / bound', float((err[:, 1:] / np.maximum(bound[:, 1:], 1e-300)).max()))
    assert np.all(err <= bound)
    assert stats_close(got['stats'], rn.host_merge(c['stats'], got['moments']))
    assert stats_close(got['stats'], ref_stats, rel=1e-9)  # (and the reference's own, loosely: other sum orders)
    want = rn.host_scale(c['r'], c['grp'], got['stats'], eps, clip)
    assert not np.isnan(got['out']).any()
    assert within_one_ulp(got['out'], want)
    if clip > 0:
        clamped = np.abs(want) == np.float32(clip)
        assert np.array_equal(got['out'][clamped], want[clamped])
    assert np.all(got['out'][c['r'] == 0] == 0)
    assert within_one_ulp(got['inv'], rn.host_inv(got['stats'], eps))
    return ref_out, want


# -- the kernels against the reference ------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_kernels_match_the_host_reference(lib, cuda, name):
    c = make_case(**CASES[name])
    assert c['d'][0, 0] == 1 and c['d'][-1, -1] == 1 and c['carry'].any() and c['stats'].all()
    if c['T'] >= 3:
        assert c['d'][c['N'] // 2, 1] == 1 and c['d'][c['N'] // 2, 2] == 1
    got = run_device(lib, cuda, c)
    ref_out, want = check_against_host(c, got)
    assert got['bad'] == 0
    if name == 'empty-group':
        assert not got['moments'][1].any() and np.array_equal(got['stats'][1], c['stats'][1])
    if name == 'crosses-a-block':  # the case with a clamp: both kinds of element, on the reference
        g0 = (c['grp'] == 0)[:, None] & (c['r'] != 0)
        assert (np.abs(ref_out[g0]) == 10.0).any() and (np.abs(ref_out[g0]) < 10.0).any()
        assert (np.abs(got['out'][g0]) == 10.0).any()
    # in place: the same bytes
    again = run_device(lib, cuda, c, inplace=True)
    for k in ('out', 'carry', 'stats', 'moments', 'inv'):
        assert np.array_equal(bits(again[k]), bits(got[k])), k


def test_no_clamp_and_epsilon(lib, cuda):
    c = make_case(**CASES['crosses-a-block'])
    got = run_device(lib, cuda, c, clip=0.0, eps=1e-3)
    check_against_host(c, got, clip=0.0, eps=1e-3)
    assert np.abs(got['out']).max() > 10.0


def test_the_same_call_twice_gives_the_same_bytes(lib, cuda):
    c = make_case(N=257, T=20, G=3, seed=6)
    a, b = run_device(lib, cuda, c), run_device(lib, cuda, c)
    for k in ('moments', 'stats', 'out', 'carry', 'inv'):
        assert np.array_equal(bits(a[k]), bits(b[k])), k


def test_zero_moments_freeze_the_stats(lib, cuda):
    c = make_case(N=65, T=5, G=2, seed=7)
    got = run_device(lib, cuda, c, scan=False, moments_in=np.zeros((2, 3)))
    assert np.array_equal(bits(got['stats']), bits(c['stats'])) and np.array_equal(bits(got['carry']), bits(c['carry']))
    assert within_one_ulp(got['out'], rn.host_scale(c['r'], c['grp'], c['stats']))


def test_bad_group_ids_pass_through_and_are_counted(lib, cuda):
    """One env with id G and one with 255 (run once: a defined result, no fault)."""
    c = make_case(N=70, T=5, G=2, seed=8)
    c['grp'][3], c['grp'][68] = 2, 255
    c['r'][3, 0] = 300.0  # past the clip: a pass-through is not clamped either
    got = run_device(lib, cuda, c, bad_start=0)
    assert got['bad'] == 2
    for n in (3, 68):
        assert np.array_equal(bits(got['out'][n]), bits(c['r'][n])), n
    keep = c['grp'] < 2
    exact, bound = exact_moments(c, 2, keep=keep)
    assert exact[:, 0].sum() == 68 * 5
    assert np.array_equal(got['moments'][:, 0], exact[:, 0]) and np.all(np.abs(got['moments'] - exact) <= bound)
    # the batch without the two envs, on the device: other lanes hold the envs, so not the same bytes, but
    # each run is within the bound of the exact sums and the two therefore within twice the bound
    rest = dict(c, N=68, r=c['r'][keep], d=c['d'][keep], grp=c['grp'][keep], carry=c['carry'][keep])
    alone = run_device(lib, cuda, rest)
    assert alone['bad'] == 0 and np.array_equal(alone['moments'][:, 0], got['moments'][:, 0])
    assert np.all(np.abs(alone['moments'] - exact) <= bound)
    assert np.all(np.abs(alone['moments'] - got['moments']) <= 2 * bound)
    assert np.array_equal(bits(alone['carry']), bits(got['carry'][keep]))
    ref = rn.host_return_norm(c['r'], c['d'], c['grp'], 2, GAMMA, carry=c['carry'], stats=c['stats'])
    assert np.array_equal(bits(got['carry']), bits(ref[1]))  # the bad envs' carry advances too
    assert not np.array_equal(got['carry'][[3, 68]], c['carry'][[3, 68]])
    assert stats_close(got['stats'], rn.host_merge(c['stats'], got['moments']))
    assert within_one_ulp(got['out'], rn.host_scale(c['r'], c['grp'], got['stats']))
    # the counter accumulates
    assert run_device(lib, cuda, c, bad_start=5)['bad'] == 7


def test_env_shards_sum_to_the_whole_batch(lib, cuda):
    c = make_case(N=66, T=5, G=2, seed=9)
    whole = run_device(lib, cuda, c)
    h = c['N'] // 2
    halves = [dict(c, N=h, r=c['r'][:h], d=c['d'][:h], grp=c['grp'][:h], carry=c['carry'][:h]),
              dict(c, N=h, r=c['r'][h:], d=c['d'][h:], grp=c['grp'][h:], carry=c['carry'][h:])]
    scans = [run_device(lib, cuda, s, apply=False) for s in halves]
    total = scans[0]['moments'] + scans[1]['moments']  # (the all-reduce)
    applied = [run_device(lib, cuda, s, scan=False, moments_in=total) for s in halves]
    assert np.array_equal(np.concatenate([s['carry'] for s in scans]), whole['carry'])
    for a in applied:
        assert stats_close(a['stats'], whole['stats'])
    assert np.array_equal(bits(applied[0]['stats']), bits(applied[1]['stats']))
    assert within_one_ulp(np.concatenate([a['out'] for a in applied]), whole['out'])


# -- the objectives -----------------------------------------------------------------------------
def _build(N=4, T=5, A=4, C3=64, seed=5):
    from actorcritic import session as sess
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.envs.atari.wrappers import SyntheticAtariEnvs
    from actorcritic.multi_env import MultiEnv
    sess.reset_default_graph()
    env = MultiEnv(SyntheticAtariEnvs(N, num_actions=A, seed=seed))
    model = AtariModel(env.observation_space, env.action_space, C3, random_seed=3, init_seed=1)
    return env, model, MultiEnvAgent(env, model, T), sess.get_or_create_global_step()


def _feed(model, data, rewards, terminals):
    obs, act, _, _, nxt, _ = data
    return {model.observations_placeholder: obs, model.bootstrap_observations_placeholder: nxt,
            model.actions_placeholder: act, model.rewards_placeholder: rewards, model.terminals_placeholder: terminals}


def _batches(N, T, cuda, seed):
    c = make_case(N, T, 2, seed)
    return c, torch.from_numpy(c['r']).to(cuda), torch.from_numpy(c['d']).to(cuda)


@pytest.mark.parametrize('gae', [None, 0.95])
def test_targets_are_those_of_the_scaled_rewards(lib, cuda, gae):
    """target_values with a normalizer == the plain objective's targets (_ops.targets) fed
    host_return_norm's output, bit for bit, n-step and GAE; a second run continues from the
    first's carry and stats; frozen holds them; the fed tensor is not written."""
    from actorcritic import session as sess
    from actorcritic.objectives import A2CObjective
    N, T = 4, 5
    env, model, agent, gs = _build(N, T)
    groups = [0, 1, 0, 1]
    norm = rn.ReturnNormalizer(groups, num_groups=2)
    plain = A2CObjective(model, gae_lambda=gae)
    normed = A2CObjective(model, gae_lambda=gae, normalize_returns=norm)
    carry, stats = np.zeros(N, np.float32), np.zeros((2, 3))
    with sess.Session() as s:
        data = agent.interact(s)
        for run, frozen in enumerate((False, False, True)):
            c, r, d = _batches(N, T, cuda, seed=20 + run)
            fed = r.clone()
            norm.frozen = frozen
            tg, nr, st = s.run([normed.target_values, normed.normalized_rewards, normed.return_stats],
                               feed_dict=_feed(model, data, r, d))
            assert torch.equal(r, fed)
            out, carry2, stats2, _ = rn.host_return_norm(c['r'], c['d'], groups, 2, 0.99, carry=carry, stats=stats,
                                                         frozen=frozen)
            assert np.array_equal(bits(nr), bits(out)), run
            want = s.run(plain.target_values, feed_dict=_feed(model, data, torch.from_numpy(out).to(cuda), d))
            assert np.array_equal(bits(tg), bits(want)), run
            assert not np.array_equal(tg, s.run(plain.target_values, feed_dict=_feed(model, data, r, d)))
            assert np.array_equal(bits(norm.carry.cpu().numpy()), bits(carry2))
            assert stats_close(st, stats2) and np.array_equal(st, norm.stats.cpu().numpy())
            if frozen:
                assert np.array_equal(bits(st), bits(prev)) and np.array_equal(carry2, carry)
            else:
                assert np.array_equal(st[:, 0], stats[:, 0] + 2 * T)
            carry, stats, prev = carry2, stats2, st
    assert int(norm.bad_envs.item()) == 0


def test_ppo_epochs_advance_the_stats_once(lib, cuda):
    """4 epochs x 4 minibatches reuse the run's targets: stats[:, 0] grows by exactly N_g T."""
    from actorcritic import session as sess
    from actorcritic.nn import ClipGlobalNormOptimizer, RMSPropOptimizer
    from actorcritic.objectives import PPOObjective
    N, T = 8, 5
    env, model, agent, gs = _build(N, T)
    norm = rn.ReturnNormalizer([0, 1, 1, 1] * 2, num_groups=2)
    obj = PPOObjective(model, normalize_returns=norm)
    steps = []
    op = obj.optimize_shared(ClipGlobalNormOptimizer(RMSPropOptimizer(learning_rate=7e-4), clip_norm=0.5), 0.5,
                             num_epochs=4, num_minibatches=4, global_step=gs,
                             step_callback=lambda e, k: steps.append((e, k)))
    with sess.Session() as s:
        data = agent.interact(s)
        p0 = model.params.clone()
        for run in range(2):
            c, r, d = _batches(N, T, cuda, seed=30 + run)
            st, _ = s.run([obj.return_stats, op], feed_dict=_feed(model, data, r, d))
            assert st[:, 0].tolist() == [(run + 1) * 2 * T, (run + 1) * 6 * T]
    assert len(steps) == 2 * 16 and not torch.equal(model.params, p0) and torch.isfinite(model.params).all()


def test_without_a_normalizer_the_path_is_todays(lib, cuda):
    """normalize_returns=None: targets are _ops.targets of the fed rewards (called here
    directly on the run's own values), and targets, loss scalars and dhead are, bit for bit,
    those of an objective whose frozen normalizer scales by exactly one (no stats, no clamp)."""
    from actorcritic import _ops
    from actorcritic import session as sess
    from actorcritic.objectives import A2CObjective
    N, T = 4, 5
    env, model, agent, gs = _build(N, T)
    eng = model.engine
    one = rn.ReturnNormalizer([0, 1, 0, 1], num_groups=2, clip=0.0)
    one.frozen = True
    plain, unit = A2CObjective(model), A2CObjective(model, normalize_returns=one)
    assert plain.return_normalizer is None and unit.return_normalizer is one
    c, r, d = _batches(N, T, cuda, seed=40)
    fetch = lambda o: [o.target_values, o.advantage, o.policy_loss, o.baseline_loss, o.mean_entropy]
    with sess.Session() as s:
        data = agent.interact(s)
        feed = _feed(model, data, r, d)
        got = s.run(fetch(plain) + [model._bootstrap_values], feed_dict=feed)
        st = eng.update_state(N * T)
        assert st.norm_rewards is None  # the plain path makes no buffer
        dhead = st.dhead.clone()
        tg, adv = torch.zeros(N * T, device=cuda), torch.zeros(N * T, device=cuda)
        _ops.targets(r, d, st.fwd.flat_value, torch.from_numpy(got[5]).to(cuda), N, T, 0.99, None,
                     plain._tables(T, cuda), tg, adv, eng.stream())
        assert np.array_equal(bits(got[0]), bits(tg.cpu().numpy().reshape(N, T)))
        assert np.array_equal(bits(got[1]), bits(adv.cpu().numpy().reshape(N, T)))
        same = s.run(fetch(unit), feed_dict=feed)
        for a, b in zip(got[:5], same):
            assert np.array_equal(bits(np.asarray(a, np.float32)), bits(np.asarray(b, np.float32)))
        assert torch.equal(st.dhead, dhead) and dhead.any()
        assert torch.equal(st.norm_rewards.view(N, T), r)
    assert not one.stats.any() and not one.carry.any()


def test_for_envs_on_the_batched_envs(cuda):
    """The groups of the real env objects: device games (mixed at an offset, one game, through a
    MultiEnv), the synthetic stepper with and without games."""
    from actorcritic.envs.atari.wrappers import ATARI57, SyntheticAtariEnvs
    from actorcritic.envs.games import DeviceGameEnvs
    from actorcritic.multi_env import MultiEnv
    norm = rn.ReturnNormalizer.for_envs(DeviceGameEnvs('catch+breakout', 5, env_offset=1, device=cuda))
    assert norm.groups.tolist() == [1, 0, 1, 0, 1] and norm.num_groups == 2
    assert norm.group_names == ('catch', 'breakout')
    norm = rn.ReturnNormalizer.for_envs(MultiEnv(DeviceGameEnvs('breakout', 3, device=cuda)))
    assert norm.groups.tolist() == [1, 1, 1] and norm.num_groups == 2
    norm = rn.ReturnNormalizer.for_envs(SyntheticAtariEnvs(4, num_actions=18, games='atari57', env_offset=55,
                                                           device=cuda))
    assert norm.groups.tolist() == [55, 56, 0, 1] and norm.num_groups == 57 and norm.group_names == tuple(ATARI57)
    norm = rn.ReturnNormalizer.for_envs(SyntheticAtariEnvs(3, device=cuda))
    assert norm.groups.tolist() == [0, 0, 0] and norm.num_groups == 1 and norm.group_names is None


# -- learning -----------------------------------------------------------------------------------
def test_a2c_with_return_normalisation_learns_catch_in_the_mix(cuda):
    """The example's A2C on 'catch+breakout' (32 envs x 5 steps, seed 1) with
    normalize_returns=True: after RETNORM_LEARN_UPDATES updates the greedy policy, played on a
    fresh batch of Catch alone, beats the uniform policy's mean return over 256 episodes by more
    than 4 standard errors of the difference -- test_a2c_on_the_mixed_batch_learns_catch's bar."""
    from actorcritic import session as sess
    from actorcritic.envs.games import DeviceGameEnvs, evaluate
    from actorcritic.examples.atari.a2c_acktr import train_a2c_acktr
    sess.reset_default_graph()
    # the groups of a batch composed like the one the example builds (the example takes the object as it is)
    norm = rn.ReturnNormalizer.for_envs(DeviceGameEnvs('catch+breakout', 32, seed=1, device=cuda))
    assert norm.group_names == ('catch', 'breakout') and norm.groups.tolist() == [0, 1] * 16
    model, _ = train_a2c_acktr(False, 'catch+breakout', 32, 5, None, 'catch+breakout',
                               max_updates=RETNORM_LEARN_UPDATES, seed=1, game='catch+breakout',
                               normalize_returns=norm)
    stats = norm.stats.cpu().numpy()
    assert stats[:, 0].tolist() == [16 * 5 * RETNORM_LEARN_UPDATES] * 2 and int(norm.bad_envs.item()) == 0
    trained = evaluate(model, DeviceGameEnvs('catch', 32, num_actions=4, seed=1001, device=cuda), 8,
                       greedy=True).double().flatten()
    random = evaluate(None, DeviceGameEnvs('catch', 32, seed=1001, device=cuda), 8, uniform=True,
                      seed=7).double().flatten()
    assert trained.numel() == random.numel() == 256
    mt, mr = float(trained.mean()), float(random.mean())
    bound = 4.0 * math.sqrt(float(trained.var(unbiased=True)) / 256 + float(random.var(unbiased=True)) / 256)
    print('catch after {} A2C updates on catch+breakout with return normalisation: trained {:+.3f}, uniform {:+.3f}, '
          'bound {:.3f}, inv {}'.format(RETNORM_LEARN_UPDATES, mt, mr, bound, norm.inv.cpu().tolist()))
    assert torch.isfinite(model.params).all()
    assert mt - mr > bound
