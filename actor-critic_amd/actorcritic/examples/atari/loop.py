"""What the Atari examples share: the choice of envs, the training loop and the command line.

An algorithm (a2c_acktr.py, ppo.py) builds its collaborators -- ``make_multi_env`` here, then model, agent,
objective, optimizer and optimize op -- names the loss scalars it logs and hands all of it to ``train_loop``.
The helpers the loop calls (checkpoints, run state, episode scalars, env constructors) are a2c_acktr.py's.
"""

import os

import actorcritic.envs.atari.wrappers as wrappers
from actorcritic import checkpoint, parallel
from actorcritic.examples.atari.a2c_acktr import (check_run_state_args, create_environments,
                                                  create_game_environments, create_host_environments,
                                                  episode_reward_scalars, load_model, load_run_state,
                                                  save_checkpoint, save_model)
from actorcritic.multi_env import MultiEnv
from actorcritic.session import Session, no_op


def make_multi_env(env_id, num_envs, seed, env_fns, mask_actions, game, episodic_life, max_episode_steps,
                   fused_games, run_state, checkpoint_every):
    """The train functions' arguments, checked -> (MultiEnv, num_envs): a device game (``game``), host-stepped
    envs (``env_fns``: their number replaces ``num_envs``) or the synthetic stepper."""
    if game is None and (episodic_life or max_episode_steps is not None or fused_games):
        raise ValueError('episodic_life, max_episode_steps and fused_games need a device game (game=)')
    check_run_state_args(run_state, checkpoint_every, env_fns)
    if game is not None:
        return MultiEnv(create_game_environments(game, num_envs, seed=seed, full_action_set=mask_actions,
                                                 episodic_life=episodic_life, max_episode_steps=max_episode_steps,
                                                 fused_step=fused_games)), num_envs
    if env_fns is not None:
        multi_env = create_host_environments(env_fns)
        return multi_env, multi_env.num_envs
    return MultiEnv(create_environments(env_id, num_envs, seed=seed, full_action_set=mask_actions)), num_envs


def train_loop(multi_env, model, agent, objective, optimizer, optimize_op, global_step, max_step, scalars,
               checkpoint_path, model_name, summary_path, max_updates, log_every, on_update, run_state,
               checkpoint_every):
    """Interacts and runs ``optimize_op`` until ``max_step`` or ``max_updates`` (the train functions' docstrings
    say what the options do).  ``scalars``: (log key, node) pairs, fetched on the updates that log and written
    in this order, before the episode scalars and the diagnostics."""
    stats = agent.episode_stats
    read_stats = stats is not None and bool(summary_path)  # (every rank knows the path; rank 0 alone writes)
    diag = objective.diagnostics
    read_diag = diag is not None and bool(summary_path)  # (armed on every rank: read() is a collective)
    summary_writer = checkpoint.ScalarLog(summary_path) if (summary_path and parallel.rank() == 0) else None
    summary_op = no_op()

    with Session() as session:
        if checkpoint_path is not None:
            if load_model(checkpoint_path, model, optimizer, global_step, objective) and run_state:
                load_run_state(checkpoint_path, model_name, global_step.value, agent, objective)
        step = global_step.value
        updates = 0
        saved_step = None
        try:
            while step < max_step and (max_updates is None or updates < max_updates):
                observations, actions, rewards, terminals, next_observations, infos = agent.interact(session)
                episode_rewards = wrappers.EpisodeInfoWrapper.get_episode_rewards_from_info_batch(infos) \
                    if summary_writer is not None and stats is None else None
                log_now = step % log_every == 0

                fetches = [summary_op, global_step, optimize_op]
                if summary_writer is not None and log_now:
                    fetches += [node for _, node in scalars]
                feed_dict = {
                    model.observations_placeholder: observations,
                    model.bootstrap_observations_placeholder: next_observations,
                    model.actions_placeholder: actions,
                    model.rewards_placeholder: rewards,
                    model.terminals_placeholder: terminals,
                }
                if agent.last_truncations is not None:  # time limits keep their bootstrap (objectives.py)
                    feed_dict[model.truncations_placeholder] = agent.last_truncations
                if read_diag and log_now:
                    diag.request()
                out = session.run(fetches, feed_dict=feed_dict, host=len(fetches) > 3)
                step = global_step.value
                updates += 1
                diag_scalars = diag.read() if read_diag and log_now else {}
                # episode statistics: the interval's, over all ranks -- a collective, so EVERY rank reads
                interval = stats.read() if read_stats and log_now else None
                if len(out) > 3:
                    episode_scalars = stats.log_scalars(interval) if read_stats else \
                        episode_reward_scalars(multi_env.batched, episode_rewards)
                    summary_writer.add(step, **{key: float(v) for (key, _), v in zip(scalars, out[3:])},
                                       **episode_scalars, **diag_scalars)
                if on_update is not None:
                    on_update(updates, model)
                if checkpoint_path is not None and step % checkpoint_every == 0 and step > 0:
                    save_checkpoint(checkpoint_path, model_name, step, model, optimizer, objective,
                                    agent if run_state else None)
                    saved_step = step
            if run_state and checkpoint_path is not None and updates > 0 and saved_step != step:
                save_checkpoint(checkpoint_path, model_name, step, model, optimizer, objective, agent)
        except KeyboardInterrupt:
            print('Stop requested')
            if checkpoint_path is not None and parallel.rank() == 0 and not run_state:
                save_model(checkpoint_path, model_name, step, model, optimizer, objective)
        finally:
            multi_env.close()
            if summary_writer is not None:
                summary_writer.close()


def parse_flags(argv):
    """The examples' command line -> keyword arguments of a train function (``game`` among them)."""
    value = lambda flag, default: int(argv[argv.index(flag) + 1]) if flag in argv else default
    return dict(game=argv[argv.index('--game') + 1] if '--game' in argv else None,
                mask_actions='--mask-actions' in argv, episodic_life='--episodic-life' in argv,
                max_episode_steps=value('--max-episode-steps', None),
                normalize_returns='--normalize-returns' in argv, fused_games='--fused-games' in argv,
                run_state='--run-state' in argv, episode_stats='--episode-stats' in argv,
                diagnostics='--diagnostics' in argv, checkpoint_every=value('--checkpoint-every', 100))


def result_paths(game, suffix=''):
    """-> (env_id, checkpoint path, summary path) of a command-line run: ./results/checkpoints<suffix>/<env_id>
    and ./results/summaries<suffix>/<env_id>, made here."""
    env_id = 'BreakoutNoFrameskip-v4' if game is None else 'DeviceGame-' + game
    results_path = os.path.abspath('./results')
    paths = [results_path + kind + suffix + '/' + env_id for kind in ('/checkpoints', '/summaries')]
    for path in paths:
        os.makedirs(path, exist_ok=True)
    return (env_id, *paths)
