#!/usr/bin/env python
"""Cost of the episode statistics.  Needs a GPU.

  kernels  acmi_epstats_update (2 launches) on an N x T batch of G groups: HIP events over
           back-to-back calls after a warm-up, one JSON line per shape with a figure per round.
  loop     the A2C example loop (examples/atari/a2c_acktr.train_a2c_acktr, RMSProp, conv3 64)
           writing a summary with log_every=10, with episode_stats off and on in alternating
           rounds in one process: updates per second over a window that starts after the
           warm-up updates and ends in a device synchronise.  GAME is a device game
           ('catch+breakout') or 'synthetic' (the synthetic stepper).
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'actor-critic_amd'))


def _torch():
    import torch
    assert torch.cuda.is_available(), 'no GPU: nothing is measured without one'
    return torch


def _shape(text):
    n, t, g = (int(x) for x in text.split('x'))
    return n, t, g


def _case(text):
    game, n, t, updates = text.split(':')
    return game, int(n), int(t), int(updates)


def cmd_kernels(args):
    torch = _torch()
    import numpy as np
    from actorcritic import _lib
    from actorcritic.episode_stats import cleared_acc
    lib = _lib.load()
    dev = torch.device('cuda:0')
    p, st = _lib.ptr, _lib.stream_handle()
    for N, T, G in args.shapes:
        rng = np.random.default_rng(1)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        ep = up(np.where(rng.random((N, T)) < 0.05, rng.integers(-5, 30, (N, T)), np.nan).astype(np.float32))
        grp = up((np.arange(N) % G).astype(np.uint8))
        carry = torch.zeros(N, dtype=torch.int32, device=dev)
        ws = torch.zeros(int(lib.acmi_epstats_ws_doubles(N)), dtype=torch.float64, device=dev)
        acc, bad = up(cleared_acc(G)), torch.zeros(1, dtype=torch.int32, device=dev)

        def launch():
            _lib.call('acmi_epstats_update', p(ep), p(grp), N, T, G, p(carry), p(ws), p(acc), p(bad), st)

        for _ in range(20):
            launch()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                launch()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) * 1e3 / args.calls)
        assert int(bad.item()) == 0
        print(json.dumps({'what': 'kernels', 'envs': N, 'steps': T, 'groups': G, 'calls': args.calls,
                          'us_per_call': [round(t, 2) for t in times]}), flush=True)


def cmd_loop(args):
    torch = _torch()
    from actorcritic import session as sess
    from actorcritic.examples.atari.a2c_acktr import train_a2c_acktr
    torch.cuda.set_device(0)
    for game, N, T, updates in args.cases:
        # (the example ends a job after 1e7 env-steps: the window must fit)
        assert (args.warmup + updates) * N * T <= 10000000, 'more than the example\'s 1e7 env-steps'
        last = args.warmup + updates
        rates = {'off': [], 'on': []}
        for _ in range(args.rounds):
            for key in ('off', 'on'):
                window = {}

                def on_update(done, model):
                    if done == args.warmup or done == last:
                        torch.cuda.synchronize()
                        window[done] = time.perf_counter()

                sess.reset_default_graph()
                with tempfile.TemporaryDirectory() as summary:
                    train_a2c_acktr(False, 'BreakoutNoFrameskip-v4', N, T, None, 'bench', summary_path=summary,
                                    max_updates=last, seed=1, log_every=10,
                                    game=None if game == 'synthetic' else game, on_update=on_update,
                                    episode_stats=key == 'on')
                rates[key].append(updates / (window[last] - window[args.warmup]))
        print(json.dumps({'what': 'loop', 'game': game, 'envs': N, 'steps': T, 'updates_per_round': updates,
                          'log_every': 10, 'updates_per_s': {k: [round(r, 1) for r in v] for k, v in rates.items()}}),
              flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='cmd', required=True)
    k = sub.add_parser('kernels')
    k.add_argument('--shapes', type=_shape, nargs='+', default=[(32, 5, 2), (512, 20, 1), (512, 20, 57)],
                   help='ENVSxSTEPSxGROUPS')
    k.add_argument('--calls', type=int, default=20000, help='back-to-back calls per round (a window of ~0.2 s)')
    k.set_defaults(fn=cmd_kernels)
    lp = sub.add_parser('loop')
    lp.add_argument('--cases', type=_case, nargs='+',
                    default=[('catch+breakout', 32, 5, 2000), ('synthetic', 512, 20, 800)],
                    help='GAME:ENVS:STEPS:UPDATES (updates in the timed window of a round)')
    lp.add_argument('--warmup', type=int, default=50)
    lp.set_defaults(fn=cmd_loop)
    for p in (k, lp):
        p.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    args.fn(args)


if __name__ == '__main__':
    main()
