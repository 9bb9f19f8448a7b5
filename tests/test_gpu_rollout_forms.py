"""Every compiled form of the fused rollout step (acmi_rollout_step), at its batch edges.

csrc/forward.hpp (forward_impl) picks the step's kernel at launch time from the batch
size B, C3 and the forward precision:

  B <= 64 (kSplitMaxB)  rollout_tail_split_kernel<small_count(C3), C3, H16>: each image's
                        tower over 7 workgroups, the post-step env states pending in the
                        forward workspace until the next step's fc4 launch commits them
  65 .. 128             rollout_tail_tower_kernel<14 or 16, C3, H16>
  129 .. 576            rollout_tail_tower_kernel<8, C3, H16>
  above 576             no fused next tower: rollout_tail_kernel<NZ>, then the next
                        step's tower as a second launch

each for C3 in {32, 64} and the f32 / bf16 forward.  The header promises every one of
them bit-identical to acmi_forward_strided + the sampler + acmi_env_step; this file
holds them to it on both sides of every edge (1, 64 | 65, 128 | 129, 576 | 577), env
state arrays included, and holds the three-call chain itself to the float64 oracle
(oracle/oracle.py) so that it is not the only judge.

Tolerances are the project's own: fused against unfused torch.equal; the f32 forward
1e-5 of each tensor's range (test_rollout_matches_oracle_env_and_tower), the bf16
forward 1e-2 (test_bf16_forward_mode); sampling and the stepper exact.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from actorcritic import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
import oracle  # noqa: E402

FORMS_N = (1, 64, 65, 128, 129, 576, 577)
T = 3  # the shortest rollout with a fused step 0, a fused middle step and the unfused last one
ENV_SEED, SAMPLE_SEED = 5, 3

_ACT_KEYS = ('a1', 'a2', 'a3', 'a4', 'm1', 'm2', 'm3', 'logits', 'value')
_STATE_KEYS = ('_episode', '_step', '_length', '_total', '_done')


@pytest.fixture
def forward_mode(lib):
    """Sets acmi_set_forward_mode for one test and restores the previous mode."""
    prev = lib.acmi_get_forward_mode()
    yield lambda m: _lib.call('acmi_set_forward_mode', _lib.FWD_BF16 if m == 'bf16' else _lib.FWD_F32)
    _lib.call('acmi_set_forward_mode', prev)


@functools.lru_cache(maxsize=None)
def _init_params(A, C3, policy_gain):
    params = oracle.init_params(A, C3, seed=1)
    off, _ = oracle.param_offsets(A, C3)
    params[off[8]:off[9]] *= policy_gain
    return params


def _build(N, A=4, C3=32, games=None, mask_actions=False, policy_gain=1.0):
    from actorcritic import session as sess
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.envs.atari.wrappers import SyntheticAtariEnvs
    from actorcritic.multi_env import MultiEnv
    sess.reset_default_graph()
    kw = {} if games is None else dict(games=games)
    env = MultiEnv(SyntheticAtariEnvs(N, num_actions=A, seed=ENV_SEED, **kw))
    params = _init_params(A, C3, policy_gain).copy()
    model = AtariModel(env.observation_space, env.action_space, C3, params=params, random_seed=SAMPLE_SEED)
    agent = MultiEnvAgent(env, model, T, mask_actions=mask_actions)
    return env, model, agent, params


def _rollout_form(monkeypatch, fused):
    """The rollout a twin built next will run: the three-call chain (forward, sampler, env
    step) or the fused step with step fusion; one chain, no graph, either way."""
    monkeypatch.setenv('ACMI_ROLLOUT_SPLIT', '0')
    monkeypatch.setenv('ACMI_ROLLOUT_GRAPH', '0')
    monkeypatch.setenv('ACMI_ROLLOUT_FUSED', '1' if fused else '0')
    monkeypatch.setenv('ACMI_ROLLOUT_FUSE_STEPS', '1')


def _check_form(lib, agent, fused):
    rb = agent._bufs
    assert lib.acmi_get_gemm_mode() == _lib.GEMM_X3  # (step fusion needs the default mode)
    assert rb.fused == fused and rb.fuse_steps == fused
    assert not rb.halves and not rb.use_graph and rb.graph is None


def _snapshot(agent, env, data):
    """Everything a rollout leaves behind, cloned: the batch, the activation rows the
    update re-uses and the five env state arrays."""
    obs, act, rew, term, nxt, info = data
    M = obs.shape[0] * obs.shape[1]
    out = dict(obs=obs, actions=act, rewards=rew, terminals=term, next_obs=nxt,
               episode_rewards=info.episode_rewards)
    for k in _ACT_KEYS:
        out[k] = getattr(agent._bufs.acts, k)[:M]
    for k in _STATE_KEYS:
        out[k] = getattr(env.batched, k)
    return {k: v.clone() for k, v in out.items()}


def _assert_same(a, b, where):
    """torch.equal on every entry (NaN = NaN: episode rewards are NaN where no episode ended)."""
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, (where, k)
        if x.is_floating_point():
            assert torch.equal(torch.isnan(x), torch.isnan(y)), (where, k, 'NaN pattern')
            x, y = torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0)
        if not torch.equal(x, y):
            bad = (x != y).reshape(x.shape[0], -1).any(1).nonzero().flatten().tolist()
            raise AssertionError('{}: {} differs in leading rows {} (of {})'.format(where, k, bad[:8], x.shape[0]))


def _forced_terminals(N):
    """{env: j}: env's episode is made to end at the j-th step (1-based) of the rollout
    after the warm-up.  The envs are 0, N-1 and, where N has them, 63, 64 (either side of
    the 64-env edge), N//2 and N-2, dealt round-robin over j = 1, 2, 3.  Fewer than three
    envs cannot cover all three steps: they take the last ones (N = 1: only the
    last-step terminal, whose auto-reset crosses the rollout boundary; terminals at the
    fused steps 0 and 1 of its kernel, the split form, are covered at N = 64)."""
    envs = sorted({e for e in (0, 63, 64, N // 2, N - 2, N - 1) if 0 <= e < N})
    steps = (1, 2, 3)[-len(envs):] if len(envs) < 3 else (1, 2, 3)
    return {e: steps[i % len(steps)] for i, e in enumerate(envs)}


def _force_lengths(benv, forced):
    """The stepper's terminal is step >= length, and length is caller-owned state: env e
    ends its episode forced[e] steps from now."""
    idx = torch.tensor(sorted(forced), dtype=torch.long, device=benv.device)
    j = torch.tensor([forced[e] for e in sorted(forced)], dtype=torch.int32, device=benv.device)
    assert not benv._done[idx].any()  # (mid-episode: the next step does not reset and re-draw the length)
    benv._length[idx] = benv._step[idx] + j


def _three_rollouts(lib, monkeypatch, fused, N, C3, forced):
    """Warm-up, forced episode ends, one more -> ([snapshot] * 3, [sample counter at each
    rollout's step 0] * 3, params)."""
    from actorcritic import session as sess
    _rollout_form(monkeypatch, fused)
    env, model, agent, params = _build(N, C3=C3)
    snaps, counters = [], []
    with sess.Session() as s:
        for r in range(3):
            if r == 1:
                _force_lengths(env.batched, forced)
            counters.append(model.engine.sample_counter)
            snaps.append(_snapshot(agent, env, agent.interact(s)))
    torch.cuda.synchronize()
    _check_form(lib, agent, fused)
    return snaps, counters, params


# The largest forward error against float64 seen per (C3, forward), for the run's log.
_ORACLE_ERR = {}


def _check_chain_against_oracle(snaps, counters, params, N, A, C3, fwd, forced):
    """The three-call chain's own rollouts against float64 / exact restatements."""
    host = [{k: v.cpu().numpy() for k, v in s.items() if k not in ('m1', 'm2', 'm3')} for s in snaps]
    # every action of every env: the oracle's inverse-CDF draw on the GPU's logits with
    # the counter the rollout used (one per step, from the engine's sample counter)
    for r, h in enumerate(host):
        lg = h['logits'].reshape(N, T, A)
        for t in range(T):
            u = oracle.sample_uniforms(SAMPLE_SEED, 0, counters[r] + t, N)
            np.testing.assert_array_equal(h['actions'][:, t], oracle.sample_f32(lg[:, t], u), (r, t))
    # the stepper for the subset's envs: frames, rewards, terminals, episode totals and
    # the state arrays, replayed over all three rollouts with .L overwritten at the same point
    subset = sorted(set(forced) | {e for e in (0, 1, N - 2, N - 1) if 0 <= e < N})
    for e in subset:
        ref = oracle.SyntheticAtari(ENV_SEED, e)
        cur = ref.reset()
        for r, h in enumerate(host):
            if r == 1 and e in forced:
                ref.L = ref.t + forced[e]
            for t in range(T):
                np.testing.assert_array_equal(h['obs'][e, t], cur, (e, r, t))
                cur, rew, done, ep = ref.step(int(h['actions'][e, t]))
                assert h['rewards'][e, t] == rew and bool(h['terminals'][e, t]) == done, (e, r, t)
                got_ep = h['episode_rewards'][e, t]
                assert (np.isnan(got_ep) and np.isnan(ep)) or got_ep == np.float32(ep), (e, r, t)
            np.testing.assert_array_equal(h['next_obs'][e], cur, (e, r))
            state = (h['_episode'][e], h['_step'][e], h['_length'][e], h['_total'][e], bool(h['_done'][e]))
            assert state == (ref.k, ref.t, ref.L, np.float32(ref.total), ref.done), (e, r, state)
    # the tower and heads on at most 24 rows: all three steps of the subset's envs in
    # the rollout with the forced episode ends (zero-filled stacks at the terminals,
    # reset stacks after them) and step 0 of the last rollout for the envs that ended
    # on the last step (their reset across the rollout boundary)
    rows = [(1, e, t) for e in subset for t in range(T)] + [(2, e, 0) for e in subset if forced.get(e) == 3]
    assert len(rows) <= 24
    imgs = np.stack([host[r]['obs'][e, t] for r, e, t in rows])
    ref = oracle.forward(params, imgs, A, C3)
    bound = 1e-2 if fwd == 'bf16' else 1e-5
    for name in ('a1', 'a2', 'a3', 'a4', 'logits', 'value'):
        got = np.stack([host[r][name][e * T + t] for r, e, t in rows]).astype(np.float64)
        want = ref[name].reshape(got.shape)
        rel = np.abs(got - want).max() / np.abs(want).max()
        _ORACLE_ERR[(C3, fwd)] = max(_ORACLE_ERR.get((C3, fwd), 0.0), rel)
        print('oracle error C3=%d %s N=%d %-6s %.3e (bound %.0e; largest so far at this (C3, forward): %.3e)'
              % (C3, fwd, N, name, rel, bound, _ORACLE_ERR[(C3, fwd)]))
        assert rel < bound, (name, rel)


@pytest.mark.gpu
@pytest.mark.parametrize('fwd', ['f32', 'bf16'])
@pytest.mark.parametrize('C3', [32, 64])
@pytest.mark.parametrize('N', FORMS_N)
def test_fused_rollout_form_is_bit_identical_and_chain_matches_oracle(lib, cuda, monkeypatch, forward_mode, N, C3,
                                                                      fwd):
    """One (batch, C3, forward) cell of the form matrix, T = 3, A = 4, x3 gemm mode.
    Twin A rolls out through the three-call chain (ACMI_ROLLOUT_FUSED=0), twin B
    through acmi_rollout_step with step fusion.  After a warm-up rollout the episode
    lengths of envs 0, N-1, 63, 64, N//2, N-2 (_forced_terminals) are cut so that
    episodes end at step 0, step 1 and the last step of the second rollout; the
    last-step terminal's lazy reset falls on step 0 of the third -- at B <= 64 the
    commit of a done = 1 state across the rollout boundary.

    A against B after each rollout, torch.equal: the batch, episode rewards, every
    activation and ReLU' mask row, logits, values and the five env state arrays.

    A against the oracle: every action is the float32 inverse-CDF draw on the GPU's
    logits; the subset's envs replay exactly through oracle.SyntheticAtari (state
    arrays too); a1..a4, logits and value of <= 24 rows against oracle.forward, max
    |diff| / max |ref| per tensor under 1e-5 (f32) / 1e-2 (bf16 forward)."""
    A = 4
    forward_mode(fwd)
    forced = _forced_terminals(N)
    chain, counters, params = _three_rollouts(lib, monkeypatch, False, N, C3, forced)
    fused, counters_b, _ = _three_rollouts(lib, monkeypatch, True, N, C3, forced)
    assert counters == counters_b == [0, T, 2 * T]
    # the forced episode ends happened where they were put, and nowhere else
    term = chain[1]['terminals'].cpu().numpy()
    want = np.zeros((N, T), bool)
    for e, j in forced.items():
        want[e, j - 1] = True
    np.testing.assert_array_equal(term, want)
    assert list(want.any(0)) == ([True] * T if N >= 3 else [False] * (T - len(forced)) + [True] * len(forced))
    assert not chain[0]['terminals'].any() and not chain[2]['terminals'].any()
    assert (chain[2]['_episode'].cpu().numpy() == want.any(1)).all()  # every ended episode was reset
    for r in range(3):
        _assert_same(chain[r], fused[r], 'rollout {}'.format(r))
    _check_chain_against_oracle(chain, counters, params, N, A, C3, fwd, forced)


def test_form_matrix_sits_on_the_form_edges(lib):
    """Host-only: acmi_forward_ws_floats(B) = max over C3 of fc4's split count * (B + 1)
    * 512, plus B * 8 pending-state floats exactly at B <= kSplitMaxB.  Read back from
    it, the matrix's batches are where forward_impl changes form: pending states (the
    split step) at 1 and 64 and not from 65 on; the small-batch split count (16 at
    C3 = 64) up to 128, 8 at 129 and 576, and at 577 a count without a fused tail +
    tower.  A change to fc4_plan or kSplitMaxB that moves an edge fails here, instead
    of leaving the matrix beside the boundaries."""
    assert lib.acmi_get_gemm_mode() == _lib.GEMM_X3
    pending = {1: True, 64: True, 65: False, 128: False, 129: False, 576: False, 577: False}
    count = {1: 16, 64: 16, 65: 16, 128: 16, 129: 8, 576: 8, 577: None}
    assert tuple(pending) == tuple(count) == FORMS_N
    for B in FORMS_N:
        slab = (B + 1) * 512
        nz, rest = divmod(int(lib.acmi_forward_ws_floats(B)), slab)
        assert B * 8 < slab
        assert rest == (B * 8 if pending[B] else 0), (B, rest)
        if count[B] is None:
            assert nz >= 1 and nz not in (8, 14, 16), (B, nz)
        else:
            assert nz == count[B], (B, nz)


@pytest.mark.gpu
@pytest.mark.parametrize('N', [8, 64])
def test_abandoned_rollout_is_committed_by_the_next(lib, cuda, monkeypatch, forward_mode, N):
    """The acmi_rollout_io_t contract (include/acmi.h) at B <= 64: a rollout abandoned
    between fused steps leaves its last post-step states pending in acts->ws, and the
    next rollout's step 0 on the same workspace commits them.  After a warm-up
    interact, steps 0 and 1 of a rollout are driven through agents._half_step as
    MultiEnvAgent drives them, envs 0 and N-1 are made to end their episode at step 1
    (so done = 1 states are among the pending ones, the last env's too), and the
    rollout stops there.  Two more interact() calls then give, bit for bit, what the
    three-call chain gives through the same sequence -- batch, activations and env state
    arrays."""
    from actorcritic import session as sess
    from actorcritic.agents import _half_step
    A = 4
    forward_mode('f32')
    forced = {0: 2, N - 1: 2}
    later, left = {}, {}
    for fused in (False, True):
        _rollout_form(monkeypatch, fused)
        env, model, agent, _ = _build(N)
        eng, benv = model.engine, env.batched
        with sess.Session() as s:
            agent.interact(s)
            rb = agent._bufs
            _check_form(lib, agent, fused)
            step0 = benv._step.clone()
            _force_lengths(benv, forced)
            # the head of MultiEnvAgent._rollout_halves, then its first two steps
            seed = (model._random_seed or 0) & 0xFFFFFFFF
            if not rb.fused:
                rb.obs[:, 0].copy_(rb.next_obs)
            eng.net()
            fuse = bool(rb.fused and rb.fuse_steps and lib.acmi_get_gemm_mode() == _lib.GEMM_X3)
            assert fuse == fused
            for t in (0, 1):
                _half_step(eng, benv, rb, 0, N, T, A, t, seed, False, fuse)
                eng.sample_counter += 1
            torch.cuda.synchronize()
            left[fused] = dict(terminals=rb.terminals.cpu().numpy().astype(bool), step=(benv._step - step0).cpu(),
                               done=benv._done.cpu().clone())
            later[fused] = [_snapshot(agent, env, agent.interact(s)) for _ in range(2)]
        torch.cuda.synchronize()
    ended = np.zeros(N, bool)
    ended[list(forced)] = True
    for fused in (False, True):
        assert not left[fused]['terminals'][:, 0].any()
        np.testing.assert_array_equal(left[fused]['terminals'][:, 1], ended)
    # where the rollouts were left: the chain has stepped its state arrays twice; the
    # fused steps have committed step 0 only, step 1's states (done = 1 among them) pend
    assert (left[False]['step'] == 2).all() and left[False]['done'].numpy().astype(bool).tolist() == ended.tolist()
    assert (left[True]['step'] == 1).all() and not left[True]['done'].any()
    for r in range(2):
        _assert_same(later[False][r], later[True][r], 'rollout {} after the abandoned one'.format(r))
    # the pending done = 1 states were committed: both ended envs began a new episode
    assert later[True][0]['_episode'].cpu().numpy().tolist() == ended.astype(int).tolist()
    assert (later[True][1]['_step'].cpu().numpy() == np.where(ended, 2 * T, step0.cpu().numpy() + 2 + 2 * T)).all()


@pytest.mark.gpu
@pytest.mark.parametrize('N', [65, 129], ids=['one-block-count16', 'one-block-count8'])
def test_masked_rollout_through_the_one_block_forms(lib, cuda, monkeypatch, forward_mode, N):
    """Legal-action masks (a run-time pointer on the same kernels) through
    rollout_tail_tower_kernel at C3 = 64, both counts: A = 18, mixed Atari-57 games,
    MultiEnvAgent(mask_actions=True).  Fused against the three-call chain bit for bit
    over two rollouts, and every drawn action inside its env's legal set."""
    from actorcritic import session as sess
    A, C3 = 18, 64
    forward_mode('f32')
    runs = {}
    for fused in (False, True):
        _rollout_form(monkeypatch, fused)
        # (larger policy weights than the 0.01-gain init: the draws depend on the logits)
        env, model, agent, _ = _build(N, A, C3, games='atari57', mask_actions=True, policy_gain=60.0)
        with sess.Session() as s:
            runs[fused] = [_snapshot(agent, env, agent.interact(s)) for _ in range(2)]
        torch.cuda.synchronize()
        _check_form(lib, agent, fused)
        words = env.batched.legal_action_masks.cpu().numpy().astype(np.int64)
        assert model.engine.masks is not None and len(words) == N
        assert len(set(words.tolist())) > 4  # (mixed games: several different legal sets)
        for snap in runs[fused]:
            act = snap['actions'].cpu().numpy().astype(np.int64)
            assert (act >= 0).all() and (act < A).all()
            assert (((words[:, None] >> act) & 1) == 1).all()
    for r in range(2):
        _assert_same(runs[False][r], runs[True][r], 'rollout {}'.format(r))
