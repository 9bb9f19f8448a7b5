#!/usr/bin/env python
"""Cost of the per-game reward scaling ("Return normalisation").  Needs a GPU.

  kernels  acmi_retnorm_scan + acmi_retnorm_apply (3 launches) beside acmi_adv_moments +
           acmi_adv_normalize (3 launches) on the same N x T batch: HIP events over
           back-to-back calls, the cases in alternating rounds, one JSON line per shape.
  update   the A2C update (RMSProp, conv3 64) of an N x T batch of the synthetic stepper, one
           objective without and one with a ReturnNormalizer of G groups, in alternating
           rounds in one process: ms per update (forward from the rollout's cache, targets,
           loss, backward, optimizer).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'actor-critic_amd'))


def _torch():
    import torch
    assert torch.cuda.is_available(), 'no GPU: nothing is measured without one'
    return torch


def _shape(text):
    n, t, g = (int(x) for x in text.split('x'))
    return n, t, g


def cmd_kernels(args):
    torch = _torch()
    import numpy as np
    from actorcritic import _lib
    lib = _lib.load()
    dev = torch.device('cuda:0')
    p, st = _lib.ptr, _lib.stream_handle()
    for N, T, G in args.shapes:
        rng = np.random.default_rng(1)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        r = up(np.where(rng.random((N, T)) < 0.2, 1.0, 0.0).astype(np.float32))
        d = up((rng.random((N, T)) < 0.05).astype(np.uint8))
        grp = up((np.arange(N) % G).astype(np.uint8))
        carry, out = torch.zeros(N, device=dev), torch.zeros(N, T, device=dev)
        z = lambda n: torch.zeros(n, dtype=torch.float64, device=dev)
        ws, mom, stats = z(int(lib.acmi_retnorm_ws_doubles(N))), z(3 * G), z(3 * G)
        inv, bad = torch.zeros(G, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        adv, aws, amom = up(rng.standard_normal(N * T).astype(np.float32)), z(
            int(lib.acmi_adv_moments_ws_doubles(N * T))), z(2)

        def retnorm():
            _lib.call('acmi_retnorm_scan', p(r), p(d), p(grp), N, T, G, 0.99, p(carry), p(ws), p(mom), p(bad), st)
            _lib.call('acmi_retnorm_apply', p(r), p(grp), N, T, G, p(mom), p(stats), 1e-8, 10.0, p(out), p(inv), st)

        def advnorm():
            _lib.call('acmi_adv_moments', p(adv), N * T, p(aws), p(amom), st)
            _lib.call('acmi_adv_normalize', p(adv), N * T, p(amom), float(N * T), 1e-8, st)

        cases = {'retnorm_scan+apply': retnorm, 'adv_moments+normalize': advnorm}
        for launch in cases.values():
            for _ in range(20):
                launch()
        torch.cuda.synchronize()
        times = {k: [] for k in cases}
        for _ in range(args.rounds):
            for key, launch in cases.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.calls):
                    launch()
                b.record()
                torch.cuda.synchronize()
                times[key].append(a.elapsed_time(b) * 1e3 / args.calls)
        assert int(bad.item()) == 0
        print(json.dumps({'what': 'kernels', 'envs': N, 'steps': T, 'groups': G, 'calls': args.calls,
                          'us_per_call': {k: [round(t, 2) for t in v] for k, v in times.items()}}), flush=True)


def cmd_update(args):
    torch = _torch()
    import time
    from actorcritic import session as sess
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.envs.atari.wrappers import SyntheticAtariEnvs
    from actorcritic.examples.atari.a2c_acktr import create_optimizer
    from actorcritic.multi_env import MultiEnv
    from actorcritic.objectives import A2CObjective
    from actorcritic.return_norm import ReturnNormalizer
    torch.cuda.set_device(0)
    for N, T, G in args.shapes:
        sess.reset_default_graph()
        env = MultiEnv(SyntheticAtariEnvs(N, num_actions=4, seed=1))
        model = AtariModel(env.observation_space, env.action_space, 64, random_seed=1)
        agent = MultiEnvAgent(env, model, T)
        gs = sess.get_or_create_global_step()
        norm = ReturnNormalizer([n % G for n in range(N)], num_groups=G)
        ops = {'off': A2CObjective(model).optimize_shared(create_optimizer(False, model, 7e-4), 0.5, global_step=gs),
               'on': A2CObjective(model, normalize_returns=norm).optimize_shared(
                   create_optimizer(False, model, 7e-4), 0.5, global_step=gs)}
        times = {k: [] for k in ops}
        with sess.Session() as s:
            def update(op):
                obs, act, rew, term, nxt, _ = agent.interact(s)
                feed = {model.observations_placeholder: obs, model.bootstrap_observations_placeholder: nxt,
                        model.actions_placeholder: act, model.rewards_placeholder: rew,
                        model.terminals_placeholder: term}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s.run(op, feed_dict=feed, host=False)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            for op in ops.values():
                for _ in range(args.warmup):
                    update(op)
            for _ in range(args.rounds):
                for key, op in ops.items():
                    v = [update(op) for _ in range(args.iters)]
                    times[key].append(sum(v) / len(v))
        print(json.dumps({'what': 'update', 'envs': N, 'steps': T, 'groups': G, 'iters_per_round': args.iters,
                          'update_ms': {k: [round(t, 4) for t in v] for k, v in times.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='cmd', required=True)
    for name, fn in (('kernels', cmd_kernels), ('update', cmd_update)):
        p = sub.add_parser(name)
        p.add_argument('--shapes', type=_shape, nargs='+', default=[(32, 5, 2), (512, 20, 1), (512, 20, 57)],
                       help='ENVSxSTEPSxGROUPS')
        p.add_argument('--rounds', type=int, default=3)
        p.set_defaults(fn=fn)
    sub.choices['kernels'].add_argument('--calls', type=int, default=500)
    sub.choices['update'].add_argument('--iters', type=int, default=20)
    sub.choices['update'].add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    args.fn(args)


if __name__ == '__main__':
    main()
