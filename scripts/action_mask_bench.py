#!/usr/bin/env python
"""Cost of legal-action masks ("Measurements").  Needs a GPU.

  kernels  the sampler, the A2C loss and the PPO loss at M rows x A actions, masked
           (random non-empty legal sets) against unmasked on the same inputs: HIP
           events over back-to-back calls, the cases in alternating rounds.  With
           --forms unmasked and ACMI_LIB set to another build's libacmi.so the same
           unmasked calls are timed on that build (the parent commit's).
  iter     the mixed-game Atari-57 shard (BASELINE configs[4]: N envs x 20 steps, the
           18-action head, bf16 forward, ACKTR) in this process with mask_actions off
           or on: rollout ms and update ms per round of --iters iterations.
  ab       `iter` in fresh child processes, alternating off / on, --passes times; one
           JSON line each, then the summary with the raw ranges.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'actor-critic_amd'))


def _torch():
    import torch
    assert torch.cuda.is_available(), 'no GPU: nothing is measured without one'
    return torch


def cmd_kernels(args):
    torch = _torch()
    import numpy as np
    from actorcritic import _lib
    lib = _lib.load()
    dev = torch.device('cuda:0')
    M, A = args.rows, args.actions
    ldh = max(8, (A + 4) // 4 * 4)
    rng = np.random.default_rng(1)
    S = rng.random((M, A)) < 0.5
    S[np.arange(M), rng.integers(0, A, M)] = True
    words = (S.astype(np.uint64) << np.arange(A, dtype=np.uint64)).sum(1).astype(np.uint32)
    actions = np.array([rng.choice(np.flatnonzero(S[m])) for m in range(M)], np.int32)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    f = lambda: up(rng.standard_normal(M).astype(np.float32))
    logits, legal, act = up(rng.standard_normal((M, A)).astype(np.float32)), up(words.view(np.int32)), up(actions)
    values, targets, adv, olp, oval = f(), f(), f(), f() * 0.1 - 2.0, f()
    out_a = torch.zeros(M, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    dhead = torch.zeros(M, ldh, device=dev)
    ws = torch.zeros(int(max(lib.acmi_a2c_loss_ws_floats(M), lib.acmi_ppo_loss_ws_floats(M))), device=dev)
    loss, cf = torch.zeros(4, device=dev), torch.zeros(1, device=dev)
    p, st = _lib.ptr, _lib.stream_handle()
    a2c = [p(logits), A, p(values), p(act), p(targets), p(adv), M, A, 0.01, 0.5, 1.0, p(dhead), ldh, p(ws), p(loss)]
    ppo = [p(logits), A, p(values), p(act), p(olp), p(oval), p(targets), p(adv), M, A, 0.1, 0.2, 0.01, 0.5, 1.0,
           p(dhead), ldh, p(ws), p(loss), p(cf)]
    cases = {
        ('sample', 'unmasked'): lambda: _lib.call('acmi_sample_actions_dev', p(logits), A, M, A, 1, 0, None, 3, 0, None,
                                                  0, p(out_a), p(bad), st),
        ('sample', 'masked'): lambda: _lib.call('acmi_sample_actions_masked', p(logits), A, M, A, 1, 0, None, 3, 0,
                                                None, 0, p(legal), p(out_a), p(bad), st),
        ('a2c_loss', 'unmasked'): lambda: _lib.call('acmi_a2c_loss', *a2c, st),
        ('a2c_loss', 'masked'): lambda: _lib.call('acmi_a2c_loss_masked', *a2c, p(legal), p(bad), st),
        ('ppo_loss', 'unmasked'): lambda: _lib.call('acmi_ppo_loss', *ppo, st),
        ('ppo_loss', 'masked'): lambda: _lib.call('acmi_ppo_loss_masked', *ppo, p(legal), p(bad), st),
    }
    cases = {key: launch for key, launch in cases.items() if key[1] in args.forms}
    for launch in cases.values():  # warm-up
        for _ in range(20):
            launch()
    torch.cuda.synchronize()
    assert int(bad.item()) == 0
    times = {key: [] for key in cases}
    for _ in range(args.rounds):
        for key, launch in cases.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                launch()
            b.record()
            torch.cuda.synchronize()
            times[key].append(a.elapsed_time(b) * 1e3 / args.calls)
    for (what, form), us in times.items():
        print(json.dumps({'what': what, 'form': form, 'rows': M, 'actions': A, 'calls': args.calls,
                          'launches_per_call': 1 if what == 'sample' else 2, 'us_per_call': [round(t, 2) for t in us]}))


def cmd_iter(args):
    torch = _torch()
    from actorcritic import _lib
    from actorcritic import session as sess
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.envs.atari.wrappers import SyntheticAtariEnvs
    from actorcritic.examples.atari.a2c_acktr import create_optimizer
    from actorcritic.multi_env import MultiEnv
    from actorcritic.nn import linear_decay
    from actorcritic.objectives import A2CObjective
    torch.cuda.set_device(0)
    sess.reset_default_graph()
    N, T = args.envs, args.steps
    env = MultiEnv(SyntheticAtariEnvs(N, num_actions=18, seed=1, games='atari57'))
    model = AtariModel(env.observation_space, env.action_space, 32, random_seed=1, forward_mode=_lib.FWD_BF16)
    agent = MultiEnvAgent(env, model, T, mask_actions=bool(args.mask))
    obj = A2CObjective(model)
    gs = sess.get_or_create_global_step()
    gs.assign(40)  # past the cold start: statistics every update
    op = obj.optimize_shared(create_optimizer(True, model, linear_decay(0.25, 0.025, gs, 100000)), 0.5, global_step=gs)

    def feed(data):
        obs, act, rew, term, nxt, _ = data
        return {model.observations_placeholder: obs, model.bootstrap_observations_placeholder: nxt,
                model.actions_placeholder: act, model.rewards_placeholder: rew, model.terminals_placeholder: term}

    roll, upd = [], []
    with sess.Session() as s:
        def iteration(timed):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            data = agent.interact(s)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            s.run(op, feed_dict=feed(data), host=False)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if timed:
                roll[-1].append((t1 - t0) * 1e3)
                upd[-1].append((t2 - t1) * 1e3)

        for _ in range(args.warmup):
            iteration(False)
        for _ in range(args.rounds):
            roll.append([])
            upd.append([])
            for _ in range(args.iters):
                iteration(True)
        model.engine.check_bad_rows()
        finite = bool(torch.isfinite(model.params).all())
    mean = lambda v: round(sum(v) / len(v), 4)
    print(json.dumps({'what': 'acktr-atari57', 'mask_actions': bool(args.mask), 'envs': N, 'steps': T,
                      'iters_per_round': args.iters, 'rollout_ms': [mean(r) for r in roll],
                      'update_ms': [mean(u) for u in upd], 'params_finite': finite}))


def cmd_ab(args):
    results = {m: {'rollout_ms': [], 'update_ms': []} for m in (0, 1)}
    for _ in range(args.passes):
        for m in (0, 1):
            cmd = [sys.executable, os.path.abspath(__file__), 'iter', '--mask', str(m), '--iters', str(args.iters),
                   '--rounds', str(args.rounds), '--envs', str(args.envs), '--steps', str(args.steps)]
            out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=args.child_timeout).stdout.decode()
            line = [x for x in out.splitlines() if x.startswith('{')][-1]
            print(line, flush=True)
            rec = json.loads(line)
            for k in results[m]:
                results[m][k] += rec[k]
    summary = {('masked' if m else 'unmasked'): {k: {'min': min(v), 'max': max(v), 'n': len(v)} for k, v in r.items()}
               for m, r in results.items()}
    print(json.dumps({'what': 'summary', 'runs': summary}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='cmd', required=True)
    k = sub.add_parser('kernels')
    k.add_argument('--rows', type=int, default=10240)
    k.add_argument('--actions', type=int, default=18)
    k.add_argument('--calls', type=int, default=500)
    k.add_argument('--rounds', type=int, default=3)
    k.add_argument('--forms', nargs='+', choices=('unmasked', 'masked'), default=['unmasked', 'masked'],
                   help="'unmasked' alone also runs on a library without the masked entry points (ACMI_LIB=...)")
    k.set_defaults(fn=cmd_kernels)
    for name, fn in (('iter', cmd_iter), ('ab', cmd_ab)):
        p = sub.add_parser(name)
        p.add_argument('--iters', type=int, default=20)
        p.add_argument('--rounds', type=int, default=3)
        p.add_argument('--envs', type=int, default=1024)
        p.add_argument('--steps', type=int, default=20)
        p.set_defaults(fn=fn)
    it = sub.choices['iter']
    it.add_argument('--mask', type=int, choices=(0, 1), default=0)
    it.add_argument('--warmup', type=int, default=5)
    ab = sub.choices['ab']
    ab.add_argument('--passes', type=int, default=3)
    ab.add_argument('--child-timeout', type=int, default=240)
    args = ap.parse_args()
    args.fn(args)


if __name__ == '__main__':
    main()
