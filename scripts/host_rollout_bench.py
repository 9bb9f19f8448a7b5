"""The device rollout for host-stepped envs, measured.

  kernel   acmi_atari_rollout_frames beside acmi_atari_stack (one frame per env, the same
           frames, the same bytes at a 0 % reset share) at 210x160: HIP events over
           back-to-back calls, alternating rounds, reset shares 0 / 10 / 100 % of the envs.
  rollout  MultiEnvAgent.interact env-steps/s and the following A2C update's ms, for
           in-process envs that replay pre-generated frames (the env costs next to nothing,
           so the two paths' own costs show): HostAtariEnvs (the device path) against the
           reference composition FrameStackWrapper(AtariPreprocessFrameWrapper(env)) in a
           plain MultiEnv list (_interact_lists), alternating rounds.

One JSON line per mode.  Algorithmic HBM bytes of one env-step of the kernel: one raw
frame (100,800) per frame read + the stack read and write (2 x 28,224)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'actor-critic_amd'))

from actorcritic import _lib, spaces  # noqa: E402
from actorcritic.envs.atari import wrappers  # noqa: E402

H, W = wrappers.RAW_HEIGHT, wrappers.RAW_WIDTH
FRAME, STACK = H * W * 3, 4 * 84 * 84


def _timed(fn, iters):
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(s)
    for _ in range(iters):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def kernel_mode(a):
    out = {'mode': 'kernel', 'iters': a.iters, 'rounds': a.rounds, 'us_per_call': {}}
    stream = _lib.stream_handle()
    for N in a.envs:
        frames = torch.randint(0, 256, (2 * N, H, W, 3), dtype=torch.uint8, device='cuda')
        stacks = torch.randint(0, 256, (N, 84, 84, 4), dtype=torch.uint8, device='cuda')
        term = (torch.rand(N, device='cuda') < 0.01).to(torch.uint8)
        step = torch.arange(N, dtype=torch.int32, device='cuda')
        variants = {}

        def stack_call():
            _lib.call('acmi_atari_stack', ctypes.c_void_p(frames.data_ptr()), FRAME, 0, None, N, H, W,
                      ctypes.c_void_p(term.data_ptr()), 0, ctypes.c_void_p(stacks.data_ptr()),
                      ctypes.c_void_p(stacks.data_ptr()), STACK, stream)

        variants['atari_stack'] = stack_call
        for share in (0, 10, 100):
            K = (N * share + 99) // 100
            reset = np.full(N, -1, np.int32)
            if K:
                reset[np.linspace(0, N - 1, K).round().astype(int)] = N + np.arange(K)
            reset_dev = torch.from_numpy(reset).cuda()

            def call(reset_dev=reset_dev, nslots=N + K):
                _lib.call('acmi_atari_rollout_frames', ctypes.c_void_p(frames.data_ptr()), FRAME, nslots, H, W, N,
                          ctypes.c_void_p(step.data_ptr()), ctypes.c_void_p(reset_dev.data_ptr()),
                          ctypes.c_void_p(term.data_ptr()), ctypes.c_void_p(stacks.data_ptr()), STACK,
                          ctypes.c_void_p(stacks.data_ptr()), STACK, None, stream)

            variants['rollout_frames_reset{}'.format(share)] = call
        res = {k: [] for k in variants}
        for fn in variants.values():  # warm-up: code objects loaded, frames touched
            _timed(fn, 10)
        for _ in range(a.rounds):
            for k, fn in variants.items():
                res[k].append(round(_timed(fn, a.iters), 3))
        out['us_per_call'][str(N)] = res
    print(json.dumps(out))


class ReplayEnv(object):
    """A host env that costs next to nothing: pre-generated raw frames in turn, hashed
    rewards, an episode end every `length` steps."""
    observation_space = spaces.Box(low=0, high=255, shape=(H, W, 3), dtype=np.uint8)
    action_space = spaces.Discrete(4)

    def __init__(self, frames, seed, length=50):
        self.frames, self.i, self.t, self.length, self.total = frames, seed, 0, length + seed % 7, 0.0

    def _frame(self):
        self.i += 1
        return self.frames[self.i % len(self.frames)]

    def reset(self):
        self.t, self.total = 0, 0.0
        return self._frame()

    def step(self, action):
        self.t += 1
        reward = float((self.i * 7 + int(action)) % 3 - 1)
        self.total += reward
        terminal = self.t >= self.length
        info = {'episode': {'total_reward': self.total}} if terminal else {}
        return self._frame(), reward, terminal, info


def rollout_mode(a):
    from actorcritic import session as sess
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.examples.atari.a2c_acktr import create_optimizer
    from actorcritic.multi_env import MultiEnv
    from actorcritic.objectives import A2CObjective
    N, T = a.envs[0], a.steps
    frames = np.random.default_rng(0).integers(0, 256, (64, H, W, 3), dtype=np.uint8)

    def host_path():
        return MultiEnv(wrappers.HostAtariEnvs([ReplayEnv(frames, n) for n in range(N)]))

    def list_path():
        return MultiEnv([wrappers.FrameStackWrapper(wrappers.AtariPreprocessFrameWrapper(ReplayEnv(frames, n)), 4)
                         for n in range(N)])

    sess.reset_default_graph()
    gs = sess.get_or_create_global_step()
    paths = {}
    for name, make in (('lists', list_path), ('host_device', host_path)):
        env = make()
        model = AtariModel(env.observation_space, env.action_space, 64, random_seed=1)
        agent = MultiEnvAgent(env, model, T)
        objective = A2CObjective(model)
        op = objective.optimize_shared(create_optimizer(False, model, 7e-4), 0.5, global_step=gs)
        paths[name] = (env, model, agent, op)
    res = {k: {'env_steps_per_s': [], 'update_ms': []} for k in paths}

    def iteration(s, env, model, agent, op):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        obs, act, rew, term, nxt, _ = agent.interact(s)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        s.run(op, feed_dict={model.observations_placeholder: obs, model.bootstrap_observations_placeholder: nxt,
                             model.actions_placeholder: act, model.rewards_placeholder: rew,
                             model.terminals_placeholder: term})
        torch.cuda.synchronize()
        return t1 - t0, time.perf_counter() - t1

    with sess.Session() as s:
        for p in paths.values():
            for _ in range(a.warmup):
                iteration(s, *p)
        for _ in range(a.rounds):
            for k, p in paths.items():
                ti, tu = zip(*[iteration(s, *p) for _ in range(a.iters)])
                res[k]['env_steps_per_s'].append(round(N * T * len(ti) / sum(ti), 1))
                res[k]['update_ms'].append(round(1e3 * sum(tu) / len(tu), 3))
    for env, _, _, _ in paths.values():
        env.close()
    print(json.dumps({'mode': 'rollout', 'envs': N, 'steps': T, 'iters': a.iters, 'rounds': a.rounds,
                      'h2d_bytes_per_step_no_reset': N * FRAME + (9 * N + 15) // 16 * 16,
                      'd2h_bytes_per_step': 4 * (N + 1), 'paths': res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernel', 'rollout'])
    ap.add_argument('--envs', type=int, nargs='+', default=None)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--iters', type=int, default=None)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    a = ap.parse_args()
    _lib.require_gpu()
    if a.mode == 'kernel':
        a.envs, a.iters = a.envs or [32, 512], a.iters or 200
        kernel_mode(a)
    else:
        a.envs, a.iters = a.envs or [32], a.iters or 5
        rollout_mode(a)


if __name__ == '__main__':
    main()
