#!/usr/bin/env python
"""Cost of a logging update with and without update diagnostics.  Needs a GPU.

  (default)  for every case ALGO:ENVSxSTEPS (default a2c:32x5 and acktr:512x20): --rounds fresh
             processes with diagnostics off and on, alternating; one JSON line per process and a
             summary line per case with the medians over the processes.
  once       one process: the example loop (examples/atari/a2c_acktr.train_a2c_acktr on Catch)
             writing a summary with --log-every, timed from its on_update callback with a host
             clock around a device synchronise: the wall time of every iteration (rollout +
             update, and on a logging update the fetch of the loss scalars and, with
             diagnostics, request() ... read()), after --warmup iterations.  Reported: the median
             over the logging iterations, the median over the others, and their difference --
             what logging costs on top of a plain iteration.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'actor-critic_amd'))


def _case(text):
    algo, shape = text.split(':')
    n, t = shape.split('x')
    if algo not in ('a2c', 'acktr'):
        raise argparse.ArgumentTypeError('ALGO is a2c or acktr, got {!r}'.format(algo))
    return algo, int(n), int(t)


def cmd_once(args):
    import torch
    assert torch.cuda.is_available(), 'no GPU: nothing is measured without one'
    from actorcritic import session as sess
    from actorcritic.examples.atari.a2c_acktr import train_a2c_acktr
    algo, N, T = args.case
    sess.reset_default_graph()
    gs = sess.get_or_create_global_step()
    marks = []  # (global step before the iteration, seconds)
    state = {'t': None, 'gs': 0}

    def on_update(updates, model):
        torch.cuda.synchronize()
        now = time.perf_counter()
        if state['t'] is not None and updates > args.warmup:
            marks.append((state['gs'], now - state['t']))
        state['t'], state['gs'] = now, gs.value

    with tempfile.TemporaryDirectory() as tmp:
        train_a2c_acktr(algo == 'acktr', 'DeviceGame-catch', N, T, None, 'bench', summary_path=tmp,
                        max_updates=args.warmup + args.updates, seed=1, log_every=args.log_every, game='catch',
                        on_update=on_update, diagnostics=bool(args.diagnostics))
    log = [1e3 * s for g, s in marks if g % args.log_every == 0]
    plain = [1e3 * s for g, s in marks if g % args.log_every != 0]
    med = lambda v: round(statistics.median(v), 4) if v else None
    rec = dict(algo=algo, envs=N, steps=T, diagnostics=int(args.diagnostics), log_every=args.log_every,
               logging_iterations=len(log), logging_ms=med(log), plain_ms=med(plain))
    if log and plain:
        rec['logging_extra_ms'] = round(rec['logging_ms'] - rec['plain_ms'], 4)
    print(json.dumps(rec), flush=True)


def cmd_all(args):
    for case in args.cases:
        text = '{}:{}x{}'.format(*case)
        runs = {0: [], 1: []}
        for _ in range(args.rounds):
            for diag in (0, 1):  # fresh processes, alternating
                out = subprocess.run([sys.executable, os.path.abspath(__file__), 'once', '--case', text,
                                      '--diagnostics', str(diag), '--updates', str(args.updates), '--warmup',
                                      str(args.warmup), '--log-every', str(args.log_every)],
                                     check=True, stdout=subprocess.PIPE, timeout=args.timeout).stdout.decode()
                line = [l for l in out.splitlines() if l.startswith('{')][-1]
                print(line, flush=True)
                runs[diag].append(json.loads(line))
        med = lambda diag, key: round(statistics.median(r[key] for r in runs[diag]), 4)
        off, on = med(0, 'logging_ms'), med(1, 'logging_ms')
        print(json.dumps(dict(case=text, rounds=args.rounds, logging_ms_off=off, logging_ms_on=on,
                              diagnostics_ms=round(on - off, 4), plain_ms_off=med(0, 'plain_ms'),
                              plain_ms_on=med(1, 'plain_ms'),
                              logging_ms_off_all=[r['logging_ms'] for r in runs[0]],
                              logging_ms_on_all=[r['logging_ms'] for r in runs[1]])), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('cmd', nargs='?', choices=('all', 'once'), default='all')
    ap.add_argument('--cases', type=_case, nargs='+', default=[_case('a2c:32x5'), _case('acktr:512x20')])
    ap.add_argument('--case', type=_case, default=_case('a2c:32x5'), help='once: ALGO:ENVSxSTEPS')
    ap.add_argument('--diagnostics', type=int, default=0, help='once: 0 or 1')
    ap.add_argument('--rounds', type=int, default=2, help='processes per setting and case')
    ap.add_argument('--updates', type=int, default=200, help='timed iterations per process')
    ap.add_argument('--warmup', type=int, default=60, help='iterations before the timed ones (ACKTR: past its cold start)')
    ap.add_argument('--log-every', type=int, default=10)
    ap.add_argument('--timeout', type=float, default=300.0, help='seconds per process')
    args = ap.parse_args()
    {'all': cmd_all, 'once': cmd_once}[args.cmd](args)


if __name__ == '__main__':
    main()
