"""Device rollout for host-stepped Atari envs: acmi_atari_rollout_frames against the
numpy oracle, and MultiEnvAgent over HostAtariEnvs against the reference composition
_AutoResetWrapper(FrameStackWrapper(preprocess(raw chain))) replayed on the host.
Everything is byte work or a replay of the same draws: all comparisons are bit-exact.
"""
import ctypes
import hashlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
import oracle  # noqa: E402

pytestmark = pytest.mark.gpu

STACK = 4 * 84 * 84


# ---------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------
def _launch(lib, frames, nslots, H, W, N, step, reset, term, stack_in, in_stride, stack_out, out_stride, bad=None):
    """frames / step / reset / term / bad: device tensors; stack_in / stack_out: device
    addresses (stack_in may be None)."""
    import torch
    from actorcritic import _lib
    _lib.call('acmi_atari_rollout_frames', ctypes.c_void_p(frames.data_ptr()), H * W * 3, nslots, H, W, N,
              ctypes.c_void_p(step.data_ptr()), ctypes.c_void_p(reset.data_ptr()),
              None if term is None else ctypes.c_void_p(term.data_ptr()),
              None if stack_in is None else ctypes.c_void_p(stack_in), in_stride, ctypes.c_void_p(stack_out),
              out_stride, None if bad is None else ctypes.c_void_p(bad.data_ptr()), _lib.stream_handle())
    torch.cuda.synchronize()


def _expected(stack, G, R, term):
    """One env's row of the table, through the oracle's FrameStackWrapper."""
    if G is None and R is None:
        return stack
    if G is None:
        return oracle.atari_stack(None, R, reset=True)
    if R is not None:
        stack = oracle.atari_stack(None, R, reset=True)
    return oracle.atari_stack(stack, G, terminal=term)


# (has step frame, has reset frame, terminal flag): every row of the table, shared with
# tests/test_gpu_atari_shapes.py, which runs them at every shape of atari_frame_cases.SHAPES
from atari_frame_cases import CASES  # noqa: E402


# 100x92 has runs of at most 3 in both directions, like 210x160: both take the kernel with
# run lengths fixed at 3; 250x160 (y runs of 4) takes the table-driven one
# (tests/test_atari_frame_cases_host.py proves it through acmi_atari_plan)
@pytest.fixture(scope='module', params=[(210, 160), (100, 92), (250, 160)],
                ids=['210x160-fixed3x3', '100x92-fixed3x3', '250x160-generic'])
def kernel_case(request):
    """Five random frames spread over nslots = 2N slots, their oracle gray frames, and
    the per-env cases (which env gets which row is drawn)."""
    H, W = request.param
    N = len(CASES)
    rng = np.random.default_rng(H)
    distinct = rng.integers(0, 256, (5, H, W, 3), dtype=np.uint8)
    distinct[3] = 255  # saturated
    gray = [oracle.atari_preprocess(f) for f in distinct]
    which = rng.integers(0, 5, 2 * N)  # slot -> frame
    which[:5] = rng.permutation(5)
    cases = [CASES[i] for i in rng.permutation(N)]
    step = np.array([rng.integers(0, 2 * N) if c[0] else -1 - rng.integers(0, 3) for c in cases], np.int32)
    reset = np.array([rng.integers(0, 2 * N) if c[1] else -1 - rng.integers(0, 3) for c in cases], np.int32)
    term = np.array([c[2] for c in cases], np.uint8)
    stacks = rng.integers(0, 256, (N, 84, 84, 4), dtype=np.uint8)
    want = [_expected(stacks[n], gray[which[step[n]]] if step[n] >= 0 else None,
                      gray[which[reset[n]]] if reset[n] >= 0 else None, bool(term[n])) for n in range(N)]
    return dict(H=H, W=W, N=N, frames=distinct[which], step=step, reset=reset, term=term, stacks=stacks,
                want=np.stack(want), cases=cases)


@pytest.mark.parametrize('layout', ['strided-in', 'strided-out', 'in-place'])
def test_rollout_frames_kernel_matches_oracle(lib, cuda, kernel_case, layout):
    import torch
    c = kernel_case
    N, H, W = c['N'], c['H'], c['W']
    assert {(a, b) for a, b, _ in c['cases']} == {(True, False), (True, True), (False, True), (False, False)}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    frames, step, reset, term = dev(c['frames']), dev(c['step']), dev(c['reset']), dev(c['term'])
    rng = np.random.default_rng(7)
    GUARD = 4096
    # a [N, 5] block of stacks as the rollout's obs[:, t] (slot 2 of each env's five)
    wide = rng.integers(0, 256, (N, 5, STACK), dtype=np.uint8)
    wide[:, 2] = c['stacks'].reshape(N, STACK)
    if layout == 'strided-in':
        src = dev(wide)
        out0 = rng.integers(0, 256, N * STACK + GUARD, dtype=np.uint8)
        dst = dev(out0)
        _launch(lib, frames, 2 * N, H, W, N, step, reset, term, src.data_ptr() + 2 * STACK, 5 * STACK,
                dst.data_ptr(), STACK)
        got = dst.cpu().numpy()
        assert np.array_equal(got[N * STACK:], out0[N * STACK:])  # the guard behind stack_out
        assert np.array_equal(src.cpu().numpy(), wide)            # the input is only read
        got = got[:N * STACK].reshape(N, 84, 84, 4)
    elif layout == 'strided-out':
        src = dev(c['stacks'])
        out0 = np.concatenate([wide.reshape(-1), rng.integers(0, 256, GUARD, dtype=np.uint8)])
        dst = dev(out0)
        _launch(lib, frames, 2 * N, H, W, N, step, reset, term, src.data_ptr(), STACK,
                dst.data_ptr() + 3 * STACK, 5 * STACK)
        got = dst.cpu().numpy()
        assert np.array_equal(got[N * 5 * STACK:], out0[N * 5 * STACK:])
        got = got[:N * 5 * STACK].reshape(N, 5, STACK)
        keep = [0, 1, 2, 4]  # the other four stacks of each env: untouched
        assert np.array_equal(got[:, keep], wide[:, keep])
        got = got[:, 3].reshape(N, 84, 84, 4)
    else:
        out0 = np.concatenate([c['stacks'].reshape(-1), rng.integers(0, 256, GUARD, dtype=np.uint8)])
        dst = dev(out0)
        _launch(lib, frames, 2 * N, H, W, N, step, reset, term, dst.data_ptr(), STACK, dst.data_ptr(), STACK)
        got = dst.cpu().numpy()
        assert np.array_equal(got[N * STACK:], out0[N * STACK:])
        got = got[:N * STACK].reshape(N, 84, 84, 4)
        idle = [n for n, (a, b, _) in enumerate(c['cases']) if not a and not b]
        assert idle and all(np.array_equal(got[n], c['stacks'][n]) for n in idle)  # not stepped: unchanged
    for n in range(N):
        assert np.array_equal(got[n], c['want'][n]), (layout, n, c['cases'][n])


def test_rollout_frames_without_terminals_and_without_stack_in(lib, cuda, kernel_case):
    """terminals NULL is 'no terminal'; stack_in NULL serves a batch of first resets."""
    import torch
    c = kernel_case
    N, H, W = c['N'], c['H'], c['W']
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    frames = dev(c['frames'])
    gray = [oracle.atari_preprocess(f) for f in c['frames'][:2]]
    step, reset = dev(np.array([0, -1], np.int32)), dev(np.array([-1, 1], np.int32))
    src, dst = dev(c['stacks'][:2]), torch.zeros((2, 84, 84, 4), dtype=torch.uint8, device='cuda')
    _launch(lib, frames, 2 * N, H, W, 2, step, reset, None, src.data_ptr(), STACK, dst.data_ptr(), STACK)
    assert np.array_equal(dst[0].cpu().numpy(), oracle.atari_stack(c['stacks'][0], gray[0]))
    assert np.array_equal(dst[1].cpu().numpy(), oracle.atari_stack(None, gray[1], reset=True))
    dst.zero_()
    slots = dev(np.array([-1, -1], np.int32))
    _launch(lib, frames, 2 * N, H, W, 2, slots, dev(np.array([1, 0], np.int32)), None, None, 0, dst.data_ptr(), STACK)
    assert np.array_equal(dst[0].cpu().numpy(), oracle.atari_stack(None, gray[1], reset=True))
    assert np.array_equal(dst[1].cpu().numpy(), oracle.atari_stack(None, gray[0], reset=True))


def test_rollout_frames_slot_guard(lib, cuda, kernel_case):
    """A slot >= nslots reads nothing: that env's stack is zero, it is counted once, the
    other envs are as without it."""
    import torch
    c = kernel_case
    H, W = c['H'], c['W']
    nslots = 2
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    frames = dev(c['frames'][:nslots])  # exactly nslots frames: nothing to read behind them
    gray = [oracle.atari_preprocess(f) for f in c['frames'][:nslots]]
    step, reset = dev(np.array([1, nslots, 0], np.int32)), dev(np.array([-1, -1, 1], np.int32))
    term = dev(np.zeros(3, np.uint8))
    bad = torch.zeros(1, dtype=torch.int32, device='cuda')
    src = dev(c['stacks'][:3])
    dst = torch.full((3, 84, 84, 4), 0xA5, dtype=torch.uint8, device='cuda')
    _launch(lib, frames, nslots, H, W, 3, step, reset, term, src.data_ptr(), STACK, dst.data_ptr(), STACK, bad)
    got = dst.cpu().numpy()
    assert int(bad.item()) == 1
    assert not got[1].any()
    assert np.array_equal(got[0], oracle.atari_stack(c['stacks'][0], gray[1]))
    assert np.array_equal(got[2], oracle.atari_stack(oracle.atari_stack(None, gray[1], reset=True), gray[0]))
    # the counter accumulates: one more launch, one more env
    _launch(lib, frames, nslots, H, W, 3, step, reset, term, src.data_ptr(), STACK, dst.data_ptr(), STACK, bad)
    assert int(bad.item()) == 2


# ---------------------------------------------------------------------------
# the rollout
# ---------------------------------------------------------------------------
def _ale(seed, A, shape=(210, 160)):
    from actorcritic import spaces

    class ALE(oracle.FakeALE):
        action_space = spaces.Discrete(A)
        observation_space = spaces.Box(low=0, high=255, shape=tuple(shape) + (3,), dtype=np.uint8)

    return ALE(seed, height=shape[0], width=shape[1])


def _raw_chain(seed, A, shape=(210, 160)):
    from actorcritic.envs.atari import wrappers
    return wrappers.wrap_atari_env(_ale(seed, A, shape), preprocess=False)


_GRAY = {}


def _oracle_gray(frame):
    """oracle.atari_preprocess, once per distinct frame (the replays see the same frames)."""
    key = hashlib.sha1(frame).digest()
    if key not in _GRAY:
        _GRAY[key] = oracle.atari_preprocess(frame)[..., None]
    return _GRAY[key]


def _reference_envs(N, A, shape=(210, 160)):
    """The reference composition over an identical host chain, frames through the oracle."""
    from actorcritic import spaces
    from actorcritic.envs.atari import wrappers
    from actorcritic.multi_env import _AutoResetWrapper

    class OraclePreprocess(wrappers.ObservationWrapper):
        def __init__(self, env):
            super().__init__(env)
            self.observation_space = spaces.Box(low=0, high=255, shape=(84, 84, 1), dtype=np.uint8)

        def observation(self, frame):
            return _oracle_gray(np.ascontiguousarray(frame))

    return [_AutoResetWrapper(wrappers.FrameStackWrapper(OraclePreprocess(_raw_chain(100 + i, A, shape)), 4))
            for i in range(N)]


class _Replay(object):
    """Replays returned actions through the reference envs and compares every output of
    interact() bit for bit; counts what the run contained."""

    def __init__(self, N, A, shape=(210, 160)):
        self.envs = _reference_envs(N, A, shape)
        self.obs = [np.array(e.reset()) for e in self.envs]
        self.terminals = self.resets = self.both = 0
        self.prev = [False] * N

    def check(self, data):
        obs, act, rew, term, nxt, infos = data
        obs, act, rew, term, nxt = (x.cpu().numpy() for x in (obs, act, rew, term, nxt))
        ep = infos.episode_rewards.cpu().numpy()
        N, T = act.shape
        assert obs.shape == (N, T, 84, 84, 4) and nxt.shape == (N, 84, 84, 4)
        assert rew.dtype == np.float32 and term.dtype == np.bool_ and ep.dtype == np.float32
        for t in range(T):
            for n, env in enumerate(self.envs):
                assert np.array_equal(obs[n, t], self.obs[n]), ('observation', n, t)
                o, r, d, info = env.step(int(act[n, t]))
                self.obs[n] = np.array(o)
                assert rew[n, t] == np.float32(r) and bool(term[n, t]) == bool(d), ('reward/terminal', n, t)
                want_ep = np.float32(info['episode']['total_reward']) if 'episode' in info else np.float32(np.nan)
                assert np.array_equal(ep[n, t], want_ep, equal_nan=True), ('episode reward', n, t)
                self.terminals += bool(d)
                self.resets += self.prev[n]
                self.both += self.prev[n] and bool(d)
                self.prev[n] = bool(d)
        for n in range(N):
            assert np.array_equal(nxt[n], self.obs[n]), ('next observation', n)


def _host_agent(N, T, A, C3=32, copy_batches=False, shape=(210, 160)):
    from actorcritic import session as sess
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.envs.atari.wrappers import HostAtariEnvs
    from actorcritic.multi_env import MultiEnv
    sess.reset_default_graph()
    env = MultiEnv(HostAtariEnvs([_raw_chain(100 + i, A, shape) for i in range(N)], height=shape[0],
                                 width=shape[1]))
    assert env.batched is not None and env.num_envs == N and env.action_space.n == A
    assert tuple(env.observation_space.shape) == (84, 84, 4)
    params = oracle.init_params(A, C3, seed=1)
    model = AtariModel(env.observation_space, env.action_space, C3, params=params, random_seed=3)
    return env, model, MultiEnvAgent(env, model, T, copy_batches=copy_batches), params


def _replay_rollouts(shape):
    from actorcritic import session as sess
    N, T, A = 9, 5, 4
    env, model, agent, _ = _host_agent(N, T, A, shape=shape)
    replay = _Replay(N, A, shape)
    try:
        with sess.Session() as s:
            for _ in range(3):
                data = agent.interact(s)
                assert model.engine.lookup_rollout(data[0]) is not None
                replay.check(data)
    finally:
        env.close()
    print('host rollout {}x{}: {} terminals, {} resets, {} reset-and-terminal steps'.format(
        shape[0], shape[1], replay.terminals, replay.resets, replay.both))
    assert replay.terminals >= 1 and replay.resets >= 1 and replay.both >= 1


def test_host_rollout_replays_through_the_reference_chain(lib, cuda):
    """N = 9 FakeALE envs, T = 5, three interact() calls: observations, next
    observations, rewards, terminals and episode rewards (NaN positions included) equal
    the reference composition's on the returned actions.  The run must contain the
    interesting steps; the counts depend on the GPU's draws (with random_seed=3 and
    init_params seed 1 they were 29 terminals, 28 resets and 6 reset-and-terminal steps
    in 135 env-steps)."""
    _replay_rollouts((210, 160))


def test_host_rollout_replays_at_a_generic_shape(lib, cuda):
    """The same N, T and call count at 100x320, whose x runs of 5 take the table-driven
    rollout kernel (FakeALE's terminals and rewards do not depend on the frame shape; the
    actions drawn do)."""
    _replay_rollouts((100, 320))


def test_host_rollout_sampler_and_forward_consistency(lib, cuda):
    """The returned actions are acmi_sample_actions_at on the stored rollout logits with
    the recorded counters; the update finds the rollout's activations; an ACKTR update on
    them is bit-identical to one on a copy of the batch (a fresh forward)."""
    import torch
    from actorcritic import _lib
    from actorcritic import session as sess
    from actorcritic.examples.atari.a2c_acktr import create_optimizer
    from actorcritic.nn import linear_decay
    from actorcritic.objectives import A2CObjective
    N, T, A = 9, 5, 4

    def build():
        env, model, agent, params = _host_agent(N, T, A)
        obj = A2CObjective(model)
        gs = sess.get_or_create_global_step()
        op = obj.optimize_shared(create_optimizer(True, model, linear_decay(0.25, 0.025, gs, 1000)), 0.5,
                                 global_step=gs)
        return env, model, agent, op, params

    def feed(model, data):
        obs, act, rew, term, nxt, _ = data
        return {model.observations_placeholder: obs, model.bootstrap_observations_placeholder: nxt,
                model.actions_placeholder: act, model.rewards_placeholder: rew, model.terminals_placeholder: term}

    env, model, agent, op, params = build()
    eng = model.engine
    try:
        with sess.Session() as s:
            agent.interact(s)  # (a second rollout: counters and stacks past their initial values)
            c0 = eng.sample_counter
            data = agent.interact(s)
            assert eng.sample_counter - c0 == T
            obs, act = data[0], data[1]
            fwd = eng.lookup_rollout(obs)
            assert fwd is not None and fwd.acts is agent._bufs.acts and (fwd.batch, fwd.steps) == (N, T)
            logits = fwd.flat_logits  # row n*T + t
            again = torch.empty(N, dtype=torch.int32, device='cuda')
            bad = torch.zeros(1, dtype=torch.int32, device='cuda')
            for t in range(T):
                _lib.call('acmi_sample_actions_at', ctypes.c_void_p(logits.data_ptr() + 4 * t * A), T * A, N, A, 3, 0,
                          c0 + t, 0, None, 0, ctypes.c_void_p(again.data_ptr()), ctypes.c_void_p(bad.data_ptr()),
                          _lib.stream_handle())
                assert torch.equal(again, act[:, t]), t
            assert int(bad.item()) == 0
            kept = tuple(x.clone() if isinstance(x, torch.Tensor) else x for x in data)
            s.run(op, feed_dict=feed(model, data))
        torch.cuda.synchronize()
        cached = model.params.clone()
    finally:
        env.close()
    assert not torch.equal(cached, torch.from_numpy(params).cuda())

    env2, model2, agent2, op2, _ = build()
    try:
        with sess.Session() as s:
            assert model2.engine.lookup_rollout(kept[0]) is None
            s.run(op2, feed_dict=feed(model2, kept))
        torch.cuda.synchronize()
    finally:
        env2.close()
    assert torch.equal(model2.params, cached)


def test_host_rollout_equals_the_list_path(lib, cuda):
    """Same seeds, same initial parameters: MultiEnvAgent over a plain list of
    FrameStackWrapper(wrap_atari_env(preprocess=True)) envs takes _interact_lists and
    must draw the same actions and see the same rewards and terminals over two rollouts
    (the forward is bit-identical across batch shapes; both paths key the sampler
    (seed, 0, counter, row) at rank 0)."""
    from actorcritic import session as sess
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari import wrappers
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.multi_env import MultiEnv
    N, T, A = 9, 5, 4
    env, model, agent, params = _host_agent(N, T, A)
    try:
        with sess.Session() as s:
            dev = []
            for _ in range(2):
                data = agent.interact(s)
                dev.append([x.cpu().numpy() for x in data[1:4]])
    finally:
        env.close()

    sess.reset_default_graph()
    lists = MultiEnv([wrappers.FrameStackWrapper(wrappers.wrap_atari_env(_ale(100 + i, A), preprocess=True), 4)
                      for i in range(N)])
    assert lists.batched is None
    model2 = AtariModel(lists.observation_space, lists.action_space, 32, params=params, random_seed=3)
    agent2 = MultiEnvAgent(lists, model2, T)
    try:
        with sess.Session() as s:
            for k in range(2):
                _, act, rew, term, _, _ = agent2.interact(s)
                assert isinstance(act, list)  # the list path
                assert np.array_equal(np.asarray(act, np.int32), dev[k][0]), ('actions', k)
                assert np.array_equal(np.asarray(rew, np.float32), dev[k][1]), ('rewards', k)
                assert np.array_equal(np.asarray(term, bool), dev[k][2]), ('terminals', k)
    finally:
        lists.close()


def test_host_rollout_with_eighteen_actions(lib, cuda):
    """A = 18: this path does not inherit the fused step's 31-action limit, nor anything
    else about the action count (one rollout, replayed as above)."""
    from actorcritic import session as sess
    N, T, A = 9, 5, 18
    env, model, agent, _ = _host_agent(N, T, A)
    replay = _Replay(N, A)
    try:
        with sess.Session() as s:
            data = agent.interact(s)
            replay.check(data)
            assert int(data[1].max()) < A and int(data[1].min()) >= 0
    finally:
        env.close()


@pytest.mark.parametrize('subprocess', [False, True], ids=['in-process', 'subprocess'])
def test_example_host_environments_roll_out(lib, cuda, subprocess):
    """examples.atari.a2c_acktr.create_host_environments: env functions -> (SubprocessEnvs
    ->) HostAtariEnvs -> MultiEnv on the device path; two envs, one short rollout replayed."""
    import functools
    from actorcritic import session as sess
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.envs.atari.wrappers import HostAtariEnvs
    from actorcritic.examples.atari.a2c_acktr import create_host_environments
    N, T, A = 2, 3, 4
    sess.reset_default_graph()
    env = create_host_environments([functools.partial(_raw_chain, 100 + i, A) for i in range(N)],
                                   subprocess=subprocess)
    try:
        assert isinstance(env.batched, HostAtariEnvs) and env.num_envs == N
        model = AtariModel(env.observation_space, env.action_space, 32, params=oracle.init_params(A, 32, seed=1),
                           random_seed=3)
        with sess.Session() as s:
            _Replay(N, A).check(MultiEnvAgent(env, model, T).interact(s))
    finally:
        env.close()


def test_host_envs_gym_like_api_and_copy_batches(lib, cuda):
    """HostAtariEnvs.reset()/step() return device stacks like SyntheticAtariEnvs.step, and
    copy_batches=True hands out fresh tensors that the next interact() leaves alone."""
    import torch
    from actorcritic import session as sess
    from actorcritic.envs.atari.wrappers import EpisodeInfoBatch, HostAtariEnvs
    N, A = 3, 4
    envs = HostAtariEnvs([_raw_chain(100 + i, A) for i in range(N)])
    ref = _reference_envs(N, A)
    try:
        obs = envs.reset()
        assert obs.is_cuda and obs.dtype == torch.uint8 and tuple(obs.shape) == (N, 84, 84, 4)
        want = [np.array(e.reset()) for e in ref]
        rng = np.random.default_rng(3)
        for _ in range(4):
            assert all(np.array_equal(obs[n].cpu().numpy(), want[n]) for n in range(N))
            actions = rng.integers(0, A, N)
            obs, rew, term, infos = envs.step(torch.from_numpy(actions).cuda())
            out = [e.step(int(a)) for e, a in zip(ref, actions)]
            want = [np.array(o[0]) for o in out]
            assert rew.is_cuda and term.dtype == torch.bool and isinstance(infos, EpisodeInfoBatch)
            assert rew.cpu().tolist() == [float(o[1]) for o in out]
            assert term.cpu().tolist() == [bool(o[2]) for o in out]
            assert tuple(infos.episode_rewards.shape) == (N, 1)
    finally:
        envs.close()

    env, model, agent, _ = _host_agent(N, 4, A, copy_batches=True)
    try:
        with sess.Session() as s:
            first = agent.interact(s)
            kept = [x.clone() for x in first[:5]]
            second = agent.interact(s)
            assert all(torch.equal(a, b) for a, b in zip(first[:5], kept))
            assert first[0].data_ptr() != second[0].data_ptr()
            assert torch.equal(second[0][:, 0], first[4])  # carried over
    finally:
        env.close()
