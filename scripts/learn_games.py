#!/usr/bin/env python
"""Learning curves on the device games.  Needs a GPU.

Trains A2C, ACKTR, PPO or the V-trace actor-critic (the examples' settings) on Catch or Breakout from a seed and,
every --every updates, plays a separate batch of envs with the greedy policy
(envs.games.evaluate): one JSON line per point with the env-steps so far and the mean
return, after a first line with the uniform policy's.  The lines also go to --out.

    python scripts/learn_games.py --algo a2c --game catch --updates 2000 --every 250 --seeds 1 2 3

--algo vtrace takes --epochs E --minibatches K (gradient steps per batch: E passes over K env slices; 1 x 1 is
A2C's update), --rho-bar, --c-bar and --lambda (examples/atari/vtrace.py).

--episodic-life and --max-episode-steps N train under those rules (DeviceGameEnvs); the
evaluation envs never take episodic life (evaluate counts terminals as finished games), so
returns stay whole-game returns and compare across the settings.

--game catch+breakout trains on the mixed batch (global env e plays the (e % 2)-th name, one
4-action head) and evaluates PER GAME, on single-game batches that the training never saw:
one line per game and point, with "eval_game".  --mask-actions: the 18-action head with every
env's own set as its legal-action mask (for the evaluation the model's mask words are
overwritten in place with the evaluation batch's and put back, so --eval-envs must be --envs).

--normalize-returns trains with the rewards scaled by the running std of the discounted return,
per game (actorcritic.return_norm); every line of a point then holds "inv", the scale per game.

--episode-stats keeps the training envs' episode statistics on the device (actorcritic.episode_stats) and
appends to every line of a point "train_episodes": count, return mean / std / min / max and length mean /
min / max of the TRAINING episodes that ended since the previous point (a mixed run: of the line's game).
With --run-state they travel with the run state.

--diagnostics records the update diagnostics (actorcritic.update_diag) of the update that ends at every point --
explained variance, the step's KL, gradient / step norms and, with ACKTR, the preconditioner's cosines and the
trust-region coefficient -- and appends them to the point's lines as "diagnostics".  The run itself is unchanged.

--checkpoint-dir DIR keeps checkpoints (every --checkpoint-every updates, default --every, and at the
end) under DIR/seed<seed>, and a later call with the same arguments goes on from the newest one up to
--updates.  With --run-state every checkpoint carries the run state and the continuation
is the run it would have been, bit for bit: "updates", "env_steps" and the evaluation schedule follow
the checkpoint's global step, so a curve cut at a lease boundary and resumed is the uncut curve
("wall_s" alone restarts).  Without --run-state the weights resume and the envs start afresh.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'actor-critic_amd'))


def run(args, seed, emit):
    import torch
    assert torch.cuda.is_available(), 'no GPU: nothing is learned without one'
    from actorcritic import session as sess
    from actorcritic.envs.games import GAMES, DeviceGameEnvs, evaluate
    from actorcritic.examples.atari.a2c_acktr import train_a2c_acktr
    from actorcritic.examples.atari.ppo import train_ppo
    torch.cuda.set_device(0)
    sess.reset_default_graph()
    N, T, E = args.envs, args.steps, args.episodes
    vt = dict(epochs=args.epochs, minibatches=args.minibatches, rho_bar=args.rho_bar, c_bar=args.c_bar,
              gae_lambda=args.gae_lambda) if args.algo == 'vtrace' else {}
    head = dict(algo=args.algo, **vt, game=args.game, seed=seed, envs=N, steps=T, eval_envs=args.eval_envs, eval_episodes=E,
                episodic_life=args.episodic_life, max_episode_steps=args.max_episode_steps,
                mask_actions=args.mask_actions, normalize_returns=args.normalize_returns,
                **(dict(episode_stats=True) if args.episode_stats else {}))
    eval_games = [g for g in GAMES if g in args.game.split('+')]
    mixed = len(eval_games) > 1
    # the head of the trained model: the mixed batch's (4) or the full set under masks (18)
    num_actions = 18 if args.mask_actions else (4 if mixed else None)
    episodes = lambda g: args.breakout_episodes if (mixed and g == 'breakout') else E
    rules = dict(episodic_life=args.episodic_life, max_episode_steps=args.max_episode_steps)
    fused = dict(fused_games=args.fused_games)
    ckpt_dir, start = None, 0
    if args.checkpoint_dir:
        from actorcritic import checkpoint
        ckpt_dir = os.path.join(args.checkpoint_dir, 'seed{}'.format(seed))
        os.makedirs(ckpt_dir, exist_ok=True)
        newest = checkpoint.latest(ckpt_dir)
        if newest is not None:  # the curve goes on at that checkpoint's global step (one per update)
            start = int(torch.load(newest, map_location='cpu', weights_only=True)['global_step'])
    if start >= args.updates:
        return
    keep = dict(run_state=args.run_state, checkpoint_every=args.checkpoint_every or args.every)

    def stats(returns):
        r = returns.double().flatten()
        return dict(mean_return=round(float(r.mean()), 4), var=round(float(r.var(unbiased=True)), 4), n=r.numel())

    eval_envs = lambda g: DeviceGameEnvs(g, args.eval_envs, num_actions=num_actions, seed=1000 + seed,
                                         max_episode_steps=args.max_episode_steps)
    tag = lambda g: dict(eval_game=g) if mixed else {}
    for g in eval_games if start == 0 else ():  # (a resumed curve has its first lines already)
        emit(dict(head, policy='uniform', updates=0, env_steps=0, **tag(g),
                  **stats(evaluate(None, eval_envs(g), episodes(g), uniform=True, seed=seed))))
    norm, ep_stats, diag = False, None, None
    point = lambda u: u % args.every == 0 or u == args.updates
    from actorcritic.envs.games.host import env_game_ids
    groups = dict(groups=env_game_ids(args.game, N), num_groups=len(GAMES), group_names=GAMES)  # one per game
    if args.normalize_returns:  # built here and handed to the example, so that its scale can be logged
        from actorcritic.return_norm import ReturnNormalizer
        norm = ReturnNormalizer(**groups)
    if args.episode_stats:  # built here and handed to the example (no summary path: it never reads them)
        from actorcritic.episode_stats import EpisodeStats
        ep_stats = EpisodeStats(**groups)
    if args.diagnostics:  # built here and armed here, for the update that ends at a point (no summary path)
        from actorcritic.update_diag import UpdateDiagnostics
        diag = UpdateDiagnostics(**groups)
        if point(start + 1):
            diag.request()
    t0 = time.perf_counter()

    def play(model, g):
        envs = eval_envs(g)
        words = model.engine.masks
        if words is None:
            return evaluate(model, envs, episodes(g), greedy=not args.sample, seed=seed)
        saved = words.clone()  # in place: a captured rollout keeps reading this tensor
        words.copy_(envs.legal_action_masks.view(torch.int32))
        try:
            return evaluate(model, envs, episodes(g), greedy=not args.sample, seed=seed)
        finally:
            words.copy_(saved)

    def on_update(updates, model):
        updates += start  # (of the whole run: the example counts this call's)
        update_diag = {}
        if diag is not None:
            if point(updates):
                update_diag = dict(diagnostics={k: (None if v != v else float('{:.6g}'.format(v)))
                                                for k, v in diag.read().items()})
            if point(updates + 1):
                diag.request()
        if point(updates):
            torch.cuda.synchronize()
            train_s = time.perf_counter() - t0
            inv = {} if not norm else dict(inv={n: round(float(v), 4) for n, v in
                                                    zip(norm.group_names, norm.inv.cpu().tolist())})
            interval = ep_stats.read() if ep_stats is not None else None
            for g in eval_games:
                train = {} if interval is None else dict(train_episodes={
                    k: (None if v != v else v if isinstance(v, int) else round(float(v), 4))
                    for k, v in interval[g if mixed else 'all'].items()})
                emit(dict(head, policy='sampled' if args.sample else 'greedy', updates=updates,
                          env_steps=updates * N * T, wall_s=round(train_s, 2), **tag(g), **inv,
                          **stats(play(model, g)), **train, **update_diag))

    kwargs = dict(max_updates=args.updates - start, seed=seed, game=args.game, on_update=on_update,
                  mask_actions=args.mask_actions, normalize_returns=norm, episode_stats=ep_stats,
                  diagnostics=diag or False, **rules, **fused, **keep)
    if args.algo == 'ppo':
        train_ppo(args.game, N, T, ckpt_dir, args.game, **kwargs)
    elif args.algo == 'vtrace':
        from actorcritic.examples.atari.vtrace import train_vtrace
        train_vtrace(args.game, N, T, ckpt_dir, args.game, num_epochs=args.epochs, num_minibatches=args.minibatches,
                     rho_bar=args.rho_bar, c_bar=args.c_bar, gae_lambda=args.gae_lambda, **kwargs)
    else:
        train_a2c_acktr(args.algo == 'acktr', args.game, N, T, ckpt_dir, args.game, **kwargs)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--algo', choices=('a2c', 'acktr', 'ppo', 'vtrace'), default='a2c')
    ap.add_argument('--game', choices=('catch', 'breakout', 'catch+breakout'), default='catch')
    ap.add_argument('--envs', type=int, default=32)
    ap.add_argument('--steps', type=int, default=None, help='rollout length (default: a2c 5, acktr 20, ppo 128)')
    ap.add_argument('--updates', type=int, default=2000)
    ap.add_argument('--epochs', type=int, default=1, help='vtrace: passes over a batch')
    ap.add_argument('--minibatches', type=int, default=1, help='vtrace: env slices (gradient steps) per pass')
    ap.add_argument('--rho-bar', type=float, default=1.0, help='vtrace: clip of the TD terms\' importance weights')
    ap.add_argument('--c-bar', type=float, default=1.0, help='vtrace: clip of the trace\'s importance weights')
    ap.add_argument('--lambda', dest='gae_lambda', type=float, default=1.0, help='vtrace: lambda in [0, 1]')
    ap.add_argument('--every', type=int, default=250)
    ap.add_argument('--seeds', type=int, nargs='+', default=[1])
    ap.add_argument('--eval-envs', type=int, default=32)
    ap.add_argument('--episodes', type=int, default=8, help='evaluation episodes per env')
    ap.add_argument('--breakout-episodes', type=int, default=2,
                    help='evaluation episodes per Breakout env of a mixed run (its episodes are long)')
    ap.add_argument('--mask-actions', action='store_true', help='18-action head, own sets as legal-action masks')
    ap.add_argument('--sample', action='store_true', help='evaluate draws from the policy instead of its mode')
    ap.add_argument('--episodic-life', action='store_true', help='train with a lost life as a terminal')
    ap.add_argument('--max-episode-steps', type=int, default=None, help='step cap (truncation), 1..2000')
    ap.add_argument('--normalize-returns', action='store_true',
                    help='scale rewards by the running std of the discounted return, per game')
    ap.add_argument('--fused-games', action='store_true',
                    help='train through the rollout\'s fused step (DeviceGameEnvs(fused_step=True))')
    ap.add_argument('--episode-stats', action='store_true',
                    help='append the training episodes\' statistics since the previous point to every line')
    ap.add_argument('--diagnostics', action='store_true',
                    help='append the update diagnostics of the update that ends at a point to its lines')
    ap.add_argument('--checkpoint-dir', default=None,
                    help='keep checkpoints under DIR/seed<seed> and go on from the newest one')
    ap.add_argument('--checkpoint-every', type=int, default=None, help='updates between checkpoints (default: --every)')
    ap.add_argument('--run-state', action='store_true',
                    help='checkpoints carry the run state: the resumed run is the uncut one, bit for bit')
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    args = ap.parse_args()
    if args.mask_actions and args.eval_envs != args.envs:
        ap.error('--mask-actions needs --eval-envs equal to --envs (one mask word per env)')
    if args.run_state and not args.checkpoint_dir:
        ap.error('--run-state needs --checkpoint-dir')
    if args.steps is None:
        args.steps = {'a2c': 5, 'acktr': 20, 'ppo': 128, 'vtrace': 5}[args.algo]  # the examples' rollout lengths
    out = open(args.out, 'a') if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out is not None:
            out.write(line + '\n')
            out.flush()

    for seed in args.seeds:
        run(args, seed, emit)


if __name__ == '__main__':
    main()
