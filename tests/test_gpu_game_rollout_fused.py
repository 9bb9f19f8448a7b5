"""The fused rollout step of the device games (acmi_rollout_step_games; DESIGN.md 7d,
"Fused step") against the three-call chain it replaces, bit for bit.

Twins as in test_gpu_rollout_forms.py: the same parameters and seeds, T = 3 (step 0 fused,
step 1 the fused middle step, step 2 the last step with the unfused tower).  Twin A is
DeviceGameEnvs(...), the default rollout: forward + sampler + acmi_game_step*.  Twin B is
DeviceGameEnvs(..., fused_step=True).  Three rollouts each: a warm-up, one with events
injected into the caller-owned state tensors, one more (a last-step terminal makes the
reset, or the stack restart after a lost life, cross the rollout boundary).  Everything a
rollout leaves behind is compared with torch.equal (NaN = NaN): the batch, truncations,
episode rewards, a1..a4, m1..m3, logits, values, the five game state arrays (vars and done
codes included), bad_envs and the engine's bad-row count.

Twin A is not the only judge: at N = 64 and 65 four envs replay through HostGame (the
rule book) behind a frame stack, and the actions against the float32 inverse-CDF draw of
the oracle on the recorded logits.  The forward's error against float64 is held by
test_gpu_rollout_forms.py on the same tower / fc4 / heads kernels.

Kernel forms by batch (csrc/forward.hpp): <= 64 the split form (7 workgroups per env, the
post-step state pending in the env's own buffer), 65..128 and 129..576 the tail + tower
kernel at its two split-K counts, above 576 the tail alone."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from actorcritic import _lib
from actorcritic.envs.games.host import HostGame, game_pattern

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
import oracle  # noqa: E402

pytestmark = pytest.mark.gpu

T = 3
ENV_SEED, SAMPLE_SEED, CAP = 5, 3, 60
MIXED = 'catch+breakout'
_ACT_KEYS = ('a1', 'a2', 'a3', 'a4', 'm1', 'm2', 'm3', 'logits', 'value')
_STATE_KEYS = ('_episode', '_step', '_total', '_done', '_vars')


@pytest.fixture
def forward_mode(lib):
    prev = lib.acmi_get_forward_mode()
    yield lambda m: _lib.call('acmi_set_forward_mode', _lib.FWD_BF16 if m == 'bf16' else _lib.FWD_F32)
    _lib.call('acmi_set_forward_mode', prev)


@functools.lru_cache(maxsize=None)
def _init_params(A, C3):
    return oracle.init_params(A, C3, seed=1)


def _form(monkeypatch, graph=False, halves=False):
    monkeypatch.setenv('ACMI_ROLLOUT_SPLIT', '1' if halves else '0')
    monkeypatch.setenv('ACMI_ROLLOUT_GRAPH', '1' if graph else '0')
    monkeypatch.setenv('ACMI_ROLLOUT_FUSED', '1')
    monkeypatch.setenv('ACMI_ROLLOUT_FUSE_STEPS', '1')


def _build(game, N, fused, C3=32, cuts=True, mask=True, num_actions=None):
    from actorcritic import session as sess
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.envs.games import DeviceGameEnvs
    from actorcritic.multi_env import MultiEnv
    sess.reset_default_graph()
    kw = dict(episodic_life=True, max_episode_steps=CAP) if cuts else {}
    if fused:
        kw['fused_step'] = True
    env = MultiEnv(DeviceGameEnvs(game, N, num_actions=num_actions, seed=ENV_SEED, **kw))
    assert env.batched.fused_step is bool(fused) and DeviceGameEnvs.fused_step is False
    A = env.action_space.n
    model = AtariModel(env.observation_space, env.action_space, C3, params=_init_params(A, C3).copy(),
                       random_seed=SAMPLE_SEED)
    agent = MultiEnvAgent(env, model, T, mask_actions=mask)
    return env, model, agent


def _snapshot(agent, env, model, data):
    obs, act, rew, term, nxt, info = data
    M = obs.shape[0] * obs.shape[1]
    out = dict(obs=obs, actions=act, rewards=rew, terminals=term, next_obs=nxt, episode_rewards=info.episode_rewards,
               bad_rows=model.engine._bad_rows)
    if agent.last_truncations is not None:
        out['truncations'] = agent.last_truncations
    for k in _ACT_KEYS:
        out[k] = getattr(agent._bufs.acts, k)[:M]
    for k in _STATE_KEYS:
        out[k] = getattr(env.batched, k)
    if env.batched.is_mixed:
        out['bad_envs'] = env.batched.bad_envs
    return {k: v.clone() for k, v in out.items()}


def _assert_same(a, b, where):
    assert a.keys() == b.keys(), where
    for k in a:
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, (where, k)
        if x.is_floating_point():
            assert torch.equal(torch.isnan(x), torch.isnan(y)), (where, k, 'NaN pattern')
            x, y = torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0)
        if not torch.equal(x, y):
            bad = (x != y).reshape(x.shape[0], -1).any(1).nonzero().flatten().tolist()
            raise AssertionError('{}: {} differs in leading rows {} (of {})'.format(where, k, bad[:8], x.shape[0]))


# -- events ------------------------------------------------------------------------------------
def _plan(names, cuts):
    """{env: [(kind, j)]}: what is injected before the second rollout, j the 1-based step of
    that rollout at which it shows.  The envs are 0, N-1 and, where present, 63, 64, N//2
    and N-2; a Breakout env can host one ball event in three steps, and the list holds as
    few as one Breakout env (N = 64, 65), so envs 1, 3 and 5 (Breakout in the mixed batch)
    join where present.  Catch envs land their ball at steps 1, 2, 3 in turn (fewer than
    three: the last steps, as test_gpu_rollout_forms does -- N = 1 is one Catch env and
    gets the step-3 landing, whose reset crosses the rollout boundary).  Breakout envs take
    in turn: a life lost with lives left at step 2 (with episodic life: done = 2, the stack
    restarts in place at step 3); a game over on the last life at step 3; a brick hit at
    step 1 and, under a cap, a truncation at step 3; a life lost at step 3 (the restart
    crosses the boundary); a game over at step 1; a brick hit at step 2."""
    N = len(names)
    listed = sorted({e for e in (0, 63, 64, N // 2, N - 2, N - 1) if 0 <= e < N})
    catch = [e for e in listed if names[e] == 'catch']
    breakout = [e for e in listed if names[e] == 'breakout']
    breakout += [e for e in (1, 3, 5) if e < N and names[e] == 'breakout' and e not in breakout]
    plan = {}
    steps = (1, 2, 3)[-len(catch):] if len(catch) < 3 else (1, 2, 3)
    for i, e in enumerate(catch):
        plan[e] = [('land', steps[i % len(steps)])]
    kinds = ([('life', 2)], [('over', 3)], [('brick', 1)] + ([('trunc', 3)] if cuts else []), [('life', 3)],
             [('over', 1)], [('brick', 2)])
    for i, e in enumerate(breakout):
        plan[e] = list(kinds[i % len(kinds)])
    return plan


def _inject(benv, plan):
    """Writes the plan into the caller-owned state tensors (vars: ball x, y, vx, vy, paddle
    x, lives, bricks).  A ball at x = 60 over a paddle at 0 cannot be reached in three steps."""
    idx = torch.tensor(sorted(plan), dtype=torch.long, device=benv.device)
    assert not benv._done[idx].any()
    for e, events in plan.items():
        for kind, j in events:
            if kind == 'land':
                benv._vars[e, 1] = 76 - 4 * j
            elif kind in ('life', 'over'):
                benv._vars[e, :6] = torch.tensor([60, 80 - 2 * j, 1, 2, 0, 3 if kind == 'life' else 1],
                                                 dtype=torch.int32, device=benv.device)
            elif kind == 'brick':  # moving up into row 5 (y 27..29), column 3: intact
                benv._vars[e, :4] = torch.tensor([20, 29 + 2 * j, 1, -2], dtype=torch.int32, device=benv.device)
            elif kind == 'trunc':
                benv._step[e] = CAP - j


def _assert_events(snap, plan, cuts):
    """On twin A's trace of the second rollout: every injected event did occur."""
    h = {k: v.cpu().numpy() for k, v in snap.items() if k in ('rewards', 'terminals', 'truncations',
                                                              'episode_rewards', '_done', '_vars')}
    seen = set()
    for e, events in plan.items():
        for kind, j in events:
            t = j - 1
            rew, term, ep = h['rewards'][e, t], bool(h['terminals'][e, t]), h['episode_rewards'][e, t]
            if kind == 'land':
                assert term and rew in (1.0, -1.0) and ep == rew, (e, kind)
            elif kind == 'life':
                assert term == cuts and np.isnan(ep) and rew == 0.0, (e, kind)
                assert h['_vars'][e, 5] == 2 and h['_done'][e] == (2 if cuts and j == T else 0), (e, kind)
            elif kind == 'over':
                assert term and not np.isnan(ep), (e, kind)
                assert h['_done'][e] == (1 if j == T else 0), (e, kind)
            elif kind == 'brick':
                assert rew == 1.0 and not term, (e, kind)
            elif kind == 'trunc':
                assert term and bool(h['truncations'][e, t]) and not np.isnan(ep), (e, kind)
            if cuts and kind != 'trunc' and 'truncations' in h:
                assert not h['truncations'][e, t], (e, kind)
            seen.add(kind)
    return seen


def _three_rollouts(monkeypatch, game, N, fused, C3=32, cuts=True, mask=True, before_second=None, **kw):
    from actorcritic import session as sess
    _form(monkeypatch, **kw)
    env, model, agent = _build(game, N, fused, C3=C3, cuts=cuts, mask=mask)
    plan = _plan(game_pattern(game, N), cuts)
    snaps, counters = [], []
    with sess.Session() as s:
        for r in range(3):
            if r == 1:
                _inject(env.batched, plan)
                if before_second is not None:
                    before_second(env.batched)
            counters.append(model.engine.sample_counter)
            snaps.append(_snapshot(agent, env, model, agent.interact(s)))
    torch.cuda.synchronize()
    rb = agent._bufs
    assert rb.fused is bool(fused) and rb.fuse_steps is bool(fused)
    return snaps, counters, plan, agent


def _twins(monkeypatch, game, N, C3=32, cuts=True, mask=True):
    a, counters, plan, _ = _three_rollouts(monkeypatch, game, N, False, C3, cuts, mask)
    b, counters_b, _, _ = _three_rollouts(monkeypatch, game, N, True, C3, cuts, mask)
    assert counters == counters_b == [0, T, 2 * T]
    seen = _assert_events(a[1], plan, cuts)
    assert not a[0]['terminals'].any()  # (the warm-up is uneventful: the events are the injected ones)
    for r in range(3):
        _assert_same(a[r], b[r], '{} N={} rollout {}'.format(game, N, r))
    return a, counters, plan, seen


ALL_KINDS = {'land', 'life', 'over', 'brick', 'trunc'}


# -- 1, 2: the mixed batch through every kernel form ------------------------------------------
@pytest.mark.parametrize('N', [1, 64, 65, 128, 129, 576, 577])
def test_mixed_batch_fused_is_bit_identical_c32_f32(lib, cuda, monkeypatch, forward_mode, N):
    """'catch+breakout' with episodic life, a step cap of 60 and legal-action masks, both
    sides of every kernel edge.  From N = 64 on every kind of event occurs and each of the
    three steps sees a terminal."""
    forward_mode('f32')
    a, _, plan, seen = _twins(monkeypatch, MIXED, N)
    term = a[1]['terminals'].cpu().numpy()
    if N >= 64:
        assert seen == ALL_KINDS and term.any(0).all()
        assert (a[1]['_done'].cpu().numpy() == 2).any() and (a[1]['_done'].cpu().numpy() == 1).any()
        assert a[2]['_episode'].any()  # the last-step game overs were reset across the boundary
    else:
        assert seen == {'land'} and term[0].tolist() == [False, False, True]
    assert ('bad_envs' in a[2]) == (N > 1)  # (one env is one game: no games array, no counter)
    assert int(a[2].get('bad_envs', torch.zeros(1)).item()) == 0 and int(a[2]['bad_rows'].sum()) == 0


@pytest.mark.parametrize('N', [64, 128, 576, 577])
@pytest.mark.parametrize('C3,fwd', [(64, 'f32'), (32, 'bf16'), (64, 'bf16')])
def test_mixed_batch_fused_is_bit_identical_other_forms(lib, cuda, monkeypatch, forward_mode, N, C3, fwd):
    """The same batch through the other compiled forms: one batch per kernel family."""
    forward_mode(fwd)
    _, _, _, seen = _twins(monkeypatch, MIXED, N, C3=C3)
    assert seen == ALL_KINDS


# -- 3: single games: games = NULL, rules {0, 0}, truncated = NULL ---------------------------
@pytest.mark.parametrize('N', [3, 65])
@pytest.mark.parametrize('game', ['catch', 'breakout'])
def test_single_game_without_options_fused_is_bit_identical(lib, cuda, monkeypatch, forward_mode, game, N):
    forward_mode('f32')
    a, _, plan, seen = _twins(monkeypatch, game, N, cuts=False, mask=False)
    assert 'truncations' not in a[0] and 'bad_envs' not in a[0]
    assert seen == ({'land'} if game == 'catch' else {'life', 'over', 'brick'})
    assert a[1]['terminals'].cpu().numpy().any(0).all() or game == 'breakout'
    if game == 'breakout':  # game overs at steps 1 and 3 (N = 65) or at step 3 (N = 3); a lost life is no terminal
        assert a[1]['terminals'][:, T - 1].any() and not (a[1]['_done'] == 2).any()


# -- 4: the rule book and the oracle's draw ----------------------------------------------------
class _Replay(object):
    """One HostGame under the cuts behind the lazy auto-reset, the 4-frame stack and the
    whole-game episode total (the stepper's wrapper semantics, restated)."""

    def __init__(self, game, e):
        self.g = HostGame(game, seed=ENV_SEED, env_id=e, episodic_life=True, max_episode_steps=CAP)
        self.stack = np.repeat(self.g.reset(), 4, axis=-1)
        self.done, self.total = 0, np.float32(0)

    def step(self, action):
        g = self.g
        if self.done:
            self.stack = np.repeat(g.reset(), 4, axis=-1)
            if self.done == 1:
                self.total = np.float32(0)
        frame, r, t, info = g.step(int(action))
        self.stack = np.roll(self.stack, -1, axis=-1)
        if t:
            self.stack.fill(0)
        self.stack[..., -1:] = frame
        self.total = np.float32(self.total + np.float32(r))
        self.done = 1 if info['game_over'] else (2 if t else 0)
        return np.float32(r), t, info['truncated'], (self.total if info['game_over'] else np.float32(np.nan))

    def state(self):
        g = self.g
        return g.episode, g.steps, (np.float32(0) if self.done == 1 else self.total), self.done, g.state


@pytest.mark.parametrize('N', [64, 65])
def test_fused_mixed_batch_against_the_rule_book_and_the_oracle_draw(lib, cuda, monkeypatch, forward_mode, N):
    """Twin B itself (fused) against HostGame for envs 0, 1, 63 or 64 and N-1 plus every env
    with an injected event, over the three rollouts, with the injected states loaded into
    the host games at the same point: frames, rewards, terminals, truncations, episode
    rewards and the state vectors exact.  Every action is the oracle's float32 inverse-CDF
    draw on the recorded logits, over the env's own actions (the masks: Catch 3, Breakout 4)."""
    forward_mode('f32')
    names = game_pattern(MIXED, N)
    injected = {}

    def grab(benv):  # the states as injected, for the host games
        injected['vars'], injected['step'] = benv._vars.cpu().numpy(), benv._step.cpu().numpy()

    snaps, counters, plan, _ = _three_rollouts(monkeypatch, MIXED, N, True, before_second=grab)
    host = [{k: v.cpu().numpy() for k, v in s.items() if k not in _ACT_KEYS or k == 'logits'} for s in snaps]
    own = np.array([3 if g == 'catch' else 4 for g in names])
    for r, h in enumerate(host):
        lg = h['logits'].reshape(N, T, 4)
        for t in range(T):
            u = oracle.sample_uniforms(SAMPLE_SEED, 0, counters[r] + t, N)
            for A in (3, 4):
                rows = np.nonzero(own == A)[0]
                np.testing.assert_array_equal(h['actions'][rows, t], oracle.sample_f32(lg[rows, t, :A], u[rows]),
                                              (r, t, A))
    subset = sorted(set(plan) | {0, 1, 63 if N == 64 else 64, N - 1})
    for e in subset:
        ref = _Replay(names[e], e)
        for r, h in enumerate(host):
            if r == 1:
                ref.g.set_state(injected['vars'][e])
                ref.g.steps = int(injected['step'][e])
            for t in range(T):
                np.testing.assert_array_equal(h['obs'][e, t], ref.stack, (e, r, t))
                rew, term, trunc, ep = ref.step(h['actions'][e, t])
                assert h['rewards'][e, t] == rew and bool(h['terminals'][e, t]) == term, (e, r, t)
                assert bool(h['truncations'][e, t]) == trunc, (e, r, t)
                got = h['episode_rewards'][e, t]
                assert (np.isnan(got) and np.isnan(ep)) or got == ep, (e, r, t)
            np.testing.assert_array_equal(h['next_obs'][e], ref.stack, (e, r))
            k, steps, total, done, vars_ = ref.state()
            assert (h['_episode'][e], h['_step'][e], h['_total'][e], h['_done'][e]) == (k, steps, total, done), (e, r)
            np.testing.assert_array_equal(h['_vars'][e], vars_, (e, r))


# -- 5: a bad env --------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [3, 65])
def test_bad_env_behaves_as_in_the_stand_alone_kernel(lib, cuda, monkeypatch, forward_mode, N):
    """One byte of games_tensor set to 7 in both twins after a first rollout: the state of
    that env stays, its stacks are zero (the towers run on zeros), reward 0, no terminal,
    no truncation, NaN episode rewards, bad_envs == 3 after the one rollout of three steps."""
    from actorcritic import session as sess
    forward_mode('f32')
    bad = N - 2
    runs = {}
    for fused in (False, True):
        _form(monkeypatch)
        env, model, agent = _build(MIXED, N, fused)
        with sess.Session() as s:
            first = _snapshot(agent, env, model, agent.interact(s))
            env.batched.games_tensor[bad] = 7
            runs[fused] = [first, _snapshot(agent, env, model, agent.interact(s))]
        torch.cuda.synchronize()
        assert agent._bufs.fused is fused
    for r in range(2):
        _assert_same(runs[False][r], runs[True][r], 'rollout {}'.format(r))
    before, after = runs[True]
    assert int(before['bad_envs'].item()) == 0 and int(after['bad_envs'].item()) == 3
    for k in _STATE_KEYS:
        assert torch.equal(before[k][bad], after[k][bad]), k
    assert not after['obs'][bad, 1:].any() and not after['next_obs'][bad].any()
    assert not after['rewards'][bad].any() and not after['terminals'][bad].any()
    assert not after['truncations'][bad].any() and torch.isnan(after['episode_rewards'][bad]).all()


# -- 6: reset_into clears what is pending ------------------------------------------------------
def test_reset_into_between_rollouts_clears_the_pending_states(lib, cuda, monkeypatch, forward_mode):
    """N = 32 (the split form).  After a rollout, steps 0 and 1 of the next are driven as
    MultiEnvAgent drives them and the rollout is abandoned there: step 1's post-step states
    are pending.  reset_into then re-initialises the envs; the next rollout equals a fresh
    env's first rollout (at the same sampler counter) -- a stale entry committed over the
    reset state would show in the state arrays and the frames."""
    from actorcritic import session as sess
    from actorcritic.agents import _half_step
    forward_mode('f32')
    N = 32
    _form(monkeypatch)
    env, model, agent = _build(MIXED, N, True)
    eng, benv = model.engine, env.batched
    with sess.Session() as s:
        agent.interact(s)
        rb = agent._bufs
        assert rb.fused and rb.fuse_steps
        eng.net()
        for t in (0, 1):
            _half_step(eng, benv, rb, 0, N, T, eng.A, t, SAMPLE_SEED, False, True)
            eng.sample_counter += 1
        torch.cuda.synchronize()
        assert bool((benv._pend[:, 16] == 1).all())  # step 1's states are pending (the flag)
        assert bool((benv._step == T + 1).all())     # and step 0's committed
        benv.reset_into(rb.next_obs.data_ptr())
        assert not benv._pend.any()
        counter = eng.sample_counter
        again = _snapshot(agent, env, model, agent.interact(s))
    env2, model2, agent2 = _build(MIXED, N, False)
    model2.engine.sample_counter = counter
    with sess.Session() as s:
        fresh = _snapshot(agent2, env2, model2, agent2.interact(s))
    torch.cuda.synchronize()
    _assert_same(fresh, again, 'after reset_into')
    assert bool((again['_step'] == T).all()) and not again['_episode'].any()


# -- 7: graph capture and the two halves -------------------------------------------------------
def test_graph_replay_of_the_fused_games_matches_eager(lib, cuda, monkeypatch, forward_mode):
    forward_mode('f32')
    eager, _, plan, _ = _three_rollouts(monkeypatch, MIXED, 32, True)
    graph, _, _, agent = _three_rollouts(monkeypatch, MIXED, 32, True, graph=True)
    assert agent._bufs.use_graph and agent._bufs.graph is not None
    assert _assert_events(eager[1], plan, True) == ALL_KINDS
    for r in range(3):
        _assert_same(eager[r], graph[r], 'rollout {}'.format(r))


def test_two_halves_of_the_fused_games_match_the_chain(lib, cuda, monkeypatch, forward_mode):
    """N = 256 under ACMI_ROLLOUT_SPLIT=1: the state, games and pending pointers of half 1
    are those of env 128.  Twin A runs its chain in the same two halves: fc4 splits K by
    the batch of a launch (16 chunks at 128 images, 8 at 256), so a4 of one 256-image chain
    is not the a4 of two 128-image ones, fused or not."""
    from actorcritic import session as sess
    forward_mode('f32')
    runs = {}
    for fused in (False, True):
        _form(monkeypatch, halves=True)
        env, model, agent = _build(MIXED, 256, fused)
        with sess.Session() as s:
            runs[fused] = _snapshot(agent, env, model, agent.interact(s))
        torch.cuda.synchronize()
        assert agent._bufs.halves is True and agent._bufs.fused is fused
    _assert_same(runs[False], runs[True], 'one rollout')


# -- 8: the head limit -----------------------------------------------------------------------------
def test_wide_head_rolls_out_unfused(lib, cuda, monkeypatch, forward_mode):
    from actorcritic import session as sess
    forward_mode('f32')
    runs = {}
    for fused in (False, True):
        _form(monkeypatch)
        env, model, agent = _build(MIXED, 4, fused, mask=False, num_actions=40)
        with sess.Session() as s:
            runs[fused] = [_snapshot(agent, env, model, agent.interact(s)) for _ in range(2)]
        torch.cuda.synchronize()
        assert agent._bufs.fused is False
    for r in range(2):
        _assert_same(runs[False][r], runs[True][r], 'rollout {}'.format(r))


# -- 9: end to end -----------------------------------------------------------------------------------
def test_twenty_a2c_updates_give_the_same_parameters(lib, cuda, monkeypatch, forward_mode):
    """train_a2c_acktr (the examples' --fused-games) at 32 x 5 on the mixed batch, from the
    same seeds: the parameter vectors after 20 updates are equal."""
    from actorcritic import session as sess
    from actorcritic.examples.atari.a2c_acktr import train_a2c_acktr
    forward_mode('f32')
    _form(monkeypatch)
    params = []
    for fused in (False, True):
        sess.reset_default_graph()
        model, _ = train_a2c_acktr(False, 'DeviceGame-' + MIXED, 32, 5, None, 'x', max_updates=20, seed=1,
                                   game=MIXED, episodic_life=True, max_episode_steps=CAP, fused_games=fused)
        torch.cuda.synchronize()
        params.append(model.params.clone())
    assert torch.isfinite(params[0]).all() and torch.equal(params[0], params[1])
