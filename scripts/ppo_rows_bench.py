#!/usr/bin/env python
"""Timing of PPO's row minibatches ("Row minibatches").  Needs a GPU.

  gather   acmi_gather_rows on a random permutation of M rows (observations + the five
           row vectors of the PPO update) and, as the lease's ceiling, a contiguous
           device copy of the same observations; HIP events over back-to-back calls,
           the cases in alternating rounds; TB/s = 2 * M * (28224 + 20) bytes / time.
  iter     one PPO configuration in this process: the iteration (rollout + update) and
           the update alone on a fed batch, per round of --iters iterations.
           --pkg DIR imports actorcritic (and its libacmi.so) from DIR instead of this
           tree: a checkout of another commit, built in place.
  ab       `iter` in fresh child processes, alternating: [--parent DIR envs,] this tree
           envs, this tree rows, --passes times; one JSON line each, then the summary.

The configuration is §7a's: 32 envs x 128 steps, conv3 64, 4 epochs x 4 minibatches, Adam
(epsilon 1e-5) + global-norm clip 0.5, synthetic Atari envs.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBS_BYTES = 84 * 84 * 4
HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.29  # MI355X: spec; measured float4 copy


def _import_package(pkg):
    pkg = os.path.abspath(pkg or os.path.join(ROOT, 'actor-critic_amd'))
    sys.path.insert(0, pkg)
    import torch
    assert torch.cuda.is_available(), 'no GPU: nothing is measured without one'
    return pkg, torch


def cmd_gather(args):
    _, torch = _import_package(None)
    import numpy as np
    from actorcritic import _lib
    lib = _lib.load()
    dev = torch.device('cuda:0')
    cases = {}
    for M in args.rows:
        gen = torch.Generator().manual_seed(M)
        obs = torch.randint(0, 256, (M, OBS_BYTES), generator=gen, dtype=torch.uint8).to(dev)
        out = torch.zeros_like(obs)
        vs = [torch.randn(M, generator=gen).to(dev) for _ in range(5)]
        vd = [torch.zeros_like(v) for v in vs]
        perm = torch.randperm(M, generator=gen)
        index = perm.to(torch.int32).to(dev)
        src = (ctypes.c_void_p * 5)(*[v.data_ptr() for v in vs])
        dst = (ctypes.c_void_p * 5)(*[v.data_ptr() for v in vd])

        def launch(obs=obs, out=out, index=index, src=src, dst=dst, M=M):
            _lib.call('acmi_gather_rows', _lib.ptr(obs), OBS_BYTES, M, _lib.ptr(index), M, _lib.ptr(out), OBS_BYTES,
                      5, src, dst, None, _lib.stream_handle())

        launch()
        torch.cuda.synchronize()
        assert torch.equal(out, obs[perm.to(dev)]) and torch.equal(vd[4], vs[4][perm.to(dev)])
        cases[('acmi_gather_rows', M)] = (launch, (obs, out, vs, vd, index))
        # the ceiling on the same lease: the same bytes as one contiguous device copy
        cases[('contiguous copy_', M)] = (lambda obs=obs, out=out: out.copy_(obs), None)
    for launch, _ in cases.values():  # warm-up
        for _ in range(20):
            launch()
    torch.cuda.synchronize()
    times = {key: [] for key in cases}
    for _ in range(args.rounds):
        for key, (launch, _) in cases.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                launch()
            b.record()
            torch.cuda.synchronize()
            times[key].append(a.elapsed_time(b) * 1e3 / args.calls)
    for (what, M), us in times.items():
        nbytes = 2 * M * (OBS_BYTES + (20 if what == 'acmi_gather_rows' else 0))
        tbs = [nbytes / (t * 1e-6) / 1e12 for t in us]
        print(json.dumps({'what': what, 'rows': M, 'bytes': nbytes, 'calls': args.calls,
                          'us_per_call': [round(t, 2) for t in us], 'TB_per_s': [round(x, 3) for x in tbs],
                          'share_of_hbm_spec': round(float(np.median(tbs)) / HBM_SPEC_TBS, 3),
                          'share_of_measured_copy_rate': round(float(np.median(tbs)) / HBM_COPY_TBS, 3)}))


def cmd_iter(args):
    pkg, torch = _import_package(args.pkg)
    from actorcritic import session as sess
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.envs.atari.wrappers import SyntheticAtariEnvs
    from actorcritic.examples.atari.ppo import create_optimizer
    from actorcritic.multi_env import MultiEnv
    from actorcritic.objectives import PPOObjective
    torch.cuda.set_device(0)
    sess.reset_default_graph()
    N, T = args.envs, args.steps
    env = MultiEnv(SyntheticAtariEnvs(N, num_actions=4, seed=1))
    model = AtariModel(env.observation_space, env.action_space, 64, random_seed=1)
    agent = MultiEnvAgent(env, model, T)
    obj = PPOObjective(model)
    gs = sess.get_or_create_global_step()
    kw = {} if args.mode == 'envs' else {'minibatch': args.mode}  # (a tree without the keyword: env slices)
    op = obj.optimize_shared(create_optimizer(2.5e-4), 0.5, num_epochs=args.epochs, num_minibatches=args.minibatches,
                             shuffle_seed=1, global_step=gs, **kw)

    def feed(data):
        obs, act, rew, term, nxt, _ = data
        return {model.observations_placeholder: obs, model.bootstrap_observations_placeholder: nxt,
                model.actions_placeholder: act, model.rewards_placeholder: rew, model.terminals_placeholder: term}

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    with sess.Session() as s:
        def iteration():
            s.run(op, feed_dict=feed(agent.interact(s)))

        for _ in range(args.warmup):
            iteration()
        it = [timed(iteration, args.iters) for _ in range(args.rounds)]
        fed = tuple(x.clone() if isinstance(x, torch.Tensor) else x for x in agent.interact(s))

        def update():
            s.run(op, feed_dict=feed(fed))

        for _ in range(3):
            update()
        up = [timed(update, args.iters) for _ in range(args.rounds)]
        finite = bool(torch.isfinite(model.params).all())
    print(json.dumps({'what': 'ppo', 'pkg': os.path.relpath(pkg, ROOT), 'mode': args.mode, 'envs': N, 'steps': T,
                      'epochs': args.epochs, 'minibatches': args.minibatches, 'iters_per_round': args.iters,
                      'iteration_ms': [round(x, 3) for x in it], 'update_on_fed_batch_ms': [round(x, 3) for x in up],
                      'env_steps_per_s': round(N * T / (min(it) * 1e-3)), 'params_finite': finite}))


def cmd_ab(args):
    runs = ([('parent-envs', args.parent, 'envs')] if args.parent else []) + \
        [('envs', None, 'envs'), ('rows', None, 'rows')]
    results = {name: {'iteration_ms': [], 'update_on_fed_batch_ms': []} for name, _, _ in runs}
    for _ in range(args.passes):
        for name, pkg, mode in runs:
            cmd = [sys.executable, os.path.abspath(__file__), 'iter', '--mode', mode, '--iters', str(args.iters),
                   '--rounds', str(args.rounds)] + (['--pkg', pkg] if pkg else [])
            out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=args.child_timeout).stdout.decode()
            line = [x for x in out.splitlines() if x.startswith('{')][-1]
            print(name, line, flush=True)
            rec = json.loads(line)
            for k in results[name]:
                results[name][k] += rec[k]
    summary = {name: {k: {'min': min(v), 'max': max(v), 'n': len(v)} for k, v in r.items()}
               for name, r in results.items()}
    print(json.dumps({'what': 'summary', 'runs': summary}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='cmd', required=True)
    g = sub.add_parser('gather')
    g.add_argument('--rows', type=int, nargs='+', default=[4096, 10240])
    g.add_argument('--calls', type=int, default=200)
    g.add_argument('--rounds', type=int, default=3)
    g.set_defaults(fn=cmd_gather)
    for name, fn in (('iter', cmd_iter), ('ab', cmd_ab)):
        p = sub.add_parser(name)
        p.add_argument('--iters', type=int, default=10)
        p.add_argument('--rounds', type=int, default=3)
        p.set_defaults(fn=fn)
    it = sub.choices['iter']
    it.add_argument('--mode', choices=('envs', 'rows'), default='envs')
    it.add_argument('--pkg', default=None)
    it.add_argument('--envs', type=int, default=32)
    it.add_argument('--steps', type=int, default=128)
    it.add_argument('--epochs', type=int, default=4)
    it.add_argument('--minibatches', type=int, default=4)
    it.add_argument('--warmup', type=int, default=5)
    ab = sub.choices['ab']
    ab.add_argument('--parent', default=None, help='package directory of a built checkout of the parent commit')
    ab.add_argument('--passes', type=int, default=2)
    ab.add_argument('--child-timeout', type=int, default=240)
    args = ap.parse_args()
    args.fn(args)


if __name__ == '__main__':
    main()
