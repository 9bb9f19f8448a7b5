#!/usr/bin/env python
"""Cost of the device games' stepper ("Measurements").  Needs a GPU.

  step   acmi_game_step (catch, breakout) against acmi_env_step at the same N, in place:
         the same 28 KB in + 28 KB out per env.  HIP events over --calls back-to-back
         launches, the cases in alternating rounds; us per launch and the GB/s of the
         stack traffic (2 * 28224 * N bytes a launch, computed from the shape).
         catch-cuts / breakout-cuts: acmi_game_step_cuts with every option on (episodic
         life, a step cap, the truncated array written).  mixed: acmi_game_step_mixed on a
         50/50 batch (catch+breakout, env by env), to be read against the mean of the two
         single-game timings of the same process.
  iter   the unfused 32 x 5 A2C iteration (rollout + update, a host clock around a device
         synchronise) on catch against the synthetic stepper forced onto the same
         unfused path (ACMI_ROLLOUT_FUSED=0), and the synthetic stepper's default
         (fused) path for scale; ms per iteration per round.  --env mixed is the
         catch+breakout batch; --fused puts the games on the rollout's fused step
         (DeviceGameEnvs(fused_step=True)) -- run it against the same command without it,
         in fresh processes in alternating order.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'actor-critic_amd'))
OBS = 84 * 84 * 4


def _torch():
    import torch
    assert torch.cuda.is_available(), 'no GPU: nothing is measured without one'
    torch.cuda.set_device(0)
    return torch


def cmd_step(args):
    torch = _torch()
    from actorcritic.envs.atari.wrappers import SyntheticAtariEnvs
    from actorcritic.envs.games import DeviceGameEnvs
    N = args.envs
    dev = torch.device('cuda:0')
    envs = {'synthetic': SyntheticAtariEnvs(N, num_actions=4, seed=1), 'catch': DeviceGameEnvs('catch', N, seed=1),
            'breakout': DeviceGameEnvs('breakout', N, seed=1)}
    if not args.no_cuts:
        for g in ('catch', 'breakout'):
            envs[g + '-cuts'] = DeviceGameEnvs(g, N, seed=1, episodic_life=True, max_episode_steps=1000)
    if not args.no_mixed:
        envs['mixed'] = DeviceGameEnvs('catch+breakout', N, seed=1)
    if args.cases:
        envs = {k: envs[k] for k in args.cases}
    trunc = torch.zeros(N, dtype=torch.uint8, device=dev)
    actions = torch.randint(0, 3, (N,), dtype=torch.int32, device=dev)
    rew = torch.zeros(N, device=dev)
    term = torch.zeros(N, dtype=torch.uint8, device=dev)
    ep = torch.zeros(N, device=dev)
    obs = {k: torch.zeros((N, OBS), dtype=torch.uint8, device=dev) for k in envs}
    for k, e in envs.items():
        e.reset_into(obs[k].data_ptr())

    def launch(k):
        p = obs[k].data_ptr()
        kw = {'trunc_ptr': trunc.data_ptr()} if k.endswith('-cuts') else {}
        envs[k].step_into(actions.data_ptr(), p, OBS, p, OBS, rew.data_ptr(), term.data_ptr(), ep.data_ptr(), 1, **kw)

    for k in envs:  # warm-up
        for _ in range(50):
            launch(k)
    torch.cuda.synchronize()
    times = {k: [] for k in envs}
    for _ in range(args.rounds):
        for k in envs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                launch(k)
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / args.calls)
    for k, us in times.items():
        print(json.dumps({'what': 'step', 'env': k, 'envs': N, 'calls': args.calls, 'bytes_per_launch': 2 * OBS * N,
                          'us_per_launch': [round(t, 2) for t in us],
                          'stack_GBps': [round(2 * OBS * N / t / 1e3, 1) for t in us]}), flush=True)


def cmd_iter(args):
    if args.env == 'synthetic-unfused':
        os.environ['ACMI_ROLLOUT_FUSED'] = '0'
    torch = _torch()
    from actorcritic import session as sess
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.envs.atari.wrappers import SyntheticAtariEnvs
    from actorcritic.envs.games import DeviceGameEnvs
    from actorcritic.examples.atari.a2c_acktr import create_optimizer
    from actorcritic.multi_env import MultiEnv
    from actorcritic.nn import linear_decay
    from actorcritic.objectives import A2CObjective
    sess.reset_default_graph()
    N, T = args.envs, args.steps
    if args.env in ('catch', 'mixed'):
        kw = {'fused_step': True} if args.fused else {}  # (an older DeviceGameEnvs has no such keyword)
        env = MultiEnv(DeviceGameEnvs('catch' if args.env == 'catch' else 'catch+breakout', N, seed=1, **kw))
    else:
        env = MultiEnv(SyntheticAtariEnvs(N, num_actions=3, seed=1))
    model = AtariModel(env.observation_space, env.action_space, 64, random_seed=1)
    agent = MultiEnvAgent(env, model, T)
    obj = A2CObjective(model, discount_factor=0.99, entropy_regularization_strength=0.01)
    gs = sess.get_or_create_global_step()
    op = obj.optimize_shared(create_optimizer(False, model, linear_decay(7e-4, 7e-5, gs, 1e6)), 0.5, global_step=gs)
    rounds = []
    with sess.Session() as s:
        def iteration():
            obs, act, rew, term, nxt, _ = agent.interact(s)
            s.run(op, feed_dict={model.observations_placeholder: obs, model.bootstrap_observations_placeholder: nxt,
                                 model.actions_placeholder: act, model.rewards_placeholder: rew,
                                 model.terminals_placeholder: term}, host=False)

        for _ in range(args.warmup):
            iteration()
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                iteration()
            torch.cuda.synchronize()
            rounds.append((time.perf_counter() - t0) * 1e3 / args.iters)
        model.engine.check_bad_rows()
    print(json.dumps({'what': 'a2c-iter', 'env': args.env, 'fused': bool(agent._bufs.fused), 'envs': N, 'steps': T,
                      'iters_per_round': args.iters, 'ms_per_iter': [round(r, 4) for r in rounds]}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='cmd', required=True)
    st = sub.add_parser('step')
    st.add_argument('--envs', type=int, default=1024)
    st.add_argument('--calls', type=int, default=500)
    st.add_argument('--rounds', type=int, default=3)
    st.add_argument('--cases', nargs='+', default=None,
                    help='only these cases (synthetic, catch, breakout, catch-cuts, breakout-cuts, mixed): a kernel '
                         'trace of one case per process tells the kernels of the two entry points apart')
    st.add_argument('--no-cuts', action='store_true',
                    help='leave the -cuts cases out (an older libacmi under ACMI_LIB has no acmi_game_step_cuts)')
    st.add_argument('--no-mixed', action='store_true',
                    help='leave the mixed case out (an older libacmi under ACMI_LIB has no acmi_game_step_mixed)')
    st.set_defaults(fn=cmd_step)
    it = sub.add_parser('iter')
    it.add_argument('--env', choices=('catch', 'mixed', 'synthetic-unfused', 'synthetic'), default='catch')
    it.add_argument('--fused', action='store_true', help='catch / mixed: the fused rollout step')
    it.add_argument('--envs', type=int, default=32)
    it.add_argument('--steps', type=int, default=5)
    it.add_argument('--iters', type=int, default=500)
    it.add_argument('--rounds', type=int, default=3)
    it.add_argument('--warmup', type=int, default=50)
    it.set_defaults(fn=cmd_iter)
    args = ap.parse_args()
    args.fn(args)


if __name__ == '__main__':
    main()
