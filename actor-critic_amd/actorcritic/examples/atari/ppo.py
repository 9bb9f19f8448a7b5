"""PPO on Atari — beyond the reference, which stops at A2C / ACKTR.  The structure is
a2c_acktr.py's: environments -> MultiEnv -> AtariModel -> MultiEnvAgent -> PPOObjective
-> optimizer -> ``optimize_shared`` -> a session loop that interacts and runs the optimize
op; checkpoints and summaries are handled the same way.

Defaults are the common Atari PPO setting (Schulman et al. 2017, table 5, at 32 envs):
conv3 64, 32 envs x 128 steps, 4 epochs x 4 minibatches, clip 0.1, GAE(0.95) with
batch-normalised advantages, Adam (epsilon 1e-5) at 2.5e-4 decayed linearly to 0, global
gradient-norm clip 0.5.  Minibatches are env slices by default; ``minibatch='rows'`` shuffles
all env-steps of the batch per epoch (objectives.PPOOptimizeOp).
"""

import os
import sys

import actorcritic.envs.atari.wrappers as wrappers
from actorcritic import checkpoint, parallel
from actorcritic.agents import MultiEnvAgent
from actorcritic.envs.atari.model import AtariModel
from actorcritic.examples.atari.a2c_acktr import (check_run_state_args, create_environments,
                                                  create_game_environments, create_host_environments,
                                                  episode_reward_scalars, load_model, load_run_state,
                                                  make_diagnostics, make_normalizer, save_checkpoint, save_model)
from actorcritic.multi_env import MultiEnv
from actorcritic.nn import AdamOptimizer, ClipGlobalNormOptimizer, linear_decay
from actorcritic.objectives import PPOObjective
from actorcritic.session import Session, get_or_create_global_step, no_op


def train_ppo(env_id, num_envs, num_steps, checkpoint_path, model_name, summary_path=None, max_updates=None, seed=0,
              log_every=10, num_epochs=4, num_minibatches=4, clip_range=0.1, value_clip_range=None,
              minibatch='envs', env_fns=None, mask_actions=False, game=None, on_update=None, episodic_life=False,
              max_episode_steps=None, normalize_returns=False, fused_games=False, run_state=False,
              checkpoint_every=100, episode_stats=False, diagnostics=False):
    """Trains an Atari model (conv3 64) with PPO.

    ``num_envs`` is per GPU; with WORLD_SIZE > 1 (torchrun) every rank steps its own shard.
    ``minibatch``: 'envs' (contiguous env slices of the batch; ``num_minibatches`` must divide
    ``num_envs``) or 'rows' (the usual PPO minibatches: per epoch, a permutation of all
    ``num_envs * num_steps`` rows cut into ``num_minibatches`` parts, which must divide that
    product; costs a second copy of the batch's observations on the device).
    ``env_fns``: None (the synthetic batched stepper) or one function per env of this rank that
    makes a host env with raw RGB frames (a2c_acktr.create_host_environments); ``num_envs`` is
    then their number.
    ``mask_actions`` (``--mask-actions``): invalid-action masking, as in a2c_acktr.train_a2c_acktr.
    ``game`` (``--game catch|breakout``, or a mixed batch: ``catch+breakout``), ``episodic_life``
    (``--episodic-life``), ``max_episode_steps`` (``--max-episode-steps N``), ``checkpoint_path`` None and
    ``on_update``, ``normalize_returns`` (``--normalize-returns``), ``fused_games`` (``--fused-games``),
    ``run_state`` (``--run-state``), ``checkpoint_every`` (``--checkpoint-every K``) and ``episode_stats``
    (``--episode-stats``): as in a2c_acktr.train_a2c_acktr.
    ``diagnostics`` (``--diagnostics``): as there; the step and the KL are those of the whole op (all epochs),
    the gradient is the last minibatch's.
    """
    parallel.init_from_env()
    if game is None and (episodic_life or max_episode_steps is not None or fused_games):
        raise ValueError('episodic_life, max_episode_steps and fused_games need a device game (game=)')
    check_run_state_args(run_state, checkpoint_every, env_fns)
    if game is not None:
        multi_env = MultiEnv(create_game_environments(game, num_envs, seed=seed, full_action_set=mask_actions,
                                                      episodic_life=episodic_life,
                                                      max_episode_steps=max_episode_steps, fused_step=fused_games))
    elif env_fns is not None:
        multi_env = create_host_environments(env_fns)
        num_envs = multi_env.num_envs
    else:
        multi_env = MultiEnv(create_environments(env_id, num_envs, seed=seed, full_action_set=mask_actions))

    model = AtariModel(multi_env.observation_space, multi_env.action_space, 64, random_seed=seed)
    agent = MultiEnvAgent(multi_env, model, num_steps, mask_actions=mask_actions,
                          episode_stats=episode_stats or None)
    stats = agent.episode_stats
    read_stats = stats is not None and bool(summary_path)  # (every rank knows the path; rank 0 alone writes)
    normalizer = make_normalizer(normalize_returns, multi_env)
    objective = PPOObjective(model, discount_factor=0.99, entropy_regularization_strength=0.01,
                             clip_range=clip_range, value_clip_range=value_clip_range, gae_lambda=0.95,
                             normalize_advantages=True, normalize_returns=normalizer,
                             diagnostics=make_diagnostics(diagnostics, multi_env))
    diag = objective.diagnostics
    read_diag = diag is not None and bool(summary_path)  # (armed on every rank: read() is a collective)

    global_step = get_or_create_global_step()
    # 1e7 env-steps (4e7 frames) over the whole job; global steps = env-steps / batch
    max_step = 10000000 / (num_envs * num_steps * parallel.world_size())
    learning_rate = linear_decay(0.00025, 0.0, global_step, max_step, name='learning_rate')

    optimizer = create_optimizer(learning_rate)
    optimize_op = objective.optimize_shared(optimizer, baseline_loss_weight=0.5, num_epochs=num_epochs,
                                            num_minibatches=num_minibatches, shuffle_seed=seed,
                                            global_step=global_step, minibatch=minibatch)

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
                    fetches += [objective.policy_loss, objective.baseline_loss, objective.mean_entropy,
                                objective.approx_kl, objective.clip_fraction]
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
                    summary_writer.add(step, policy_loss=float(out[3]), baseline_loss=float(out[4]),
                                       policy_entropy=float(out[5]), approx_kl=float(out[6]),
                                       clip_fraction=float(out[7]), **episode_scalars, **diag_scalars)
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
    return model, optimizer


def create_optimizer(learning_rate):
    """Adam (epsilon 1e-5) + clip .5."""
    optimizer = AdamOptimizer(learning_rate=learning_rate, epsilon=1e-5)
    return ClipGlobalNormOptimizer(optimizer, clip_norm=0.5)


if __name__ == '__main__':
    argv = sys.argv[1:]
    game = argv[argv.index('--game') + 1] if '--game' in argv else None
    env_id = 'BreakoutNoFrameskip-v4' if game is None else 'DeviceGame-' + game
    num_envs = 32
    num_steps = 128
    results_path = os.path.abspath('./results')
    checkpoint_path = results_path + '/checkpoints-ppo/' + env_id
    summary_path = results_path + '/summaries-ppo/' + env_id
    os.makedirs(checkpoint_path, exist_ok=True)
    os.makedirs(summary_path, exist_ok=True)
    train_ppo(env_id, num_envs, num_steps, checkpoint_path, 'Atari-' + env_id, summary_path,
              mask_actions='--mask-actions' in argv, game=game, episodic_life='--episodic-life' in argv,
              max_episode_steps=(int(argv[argv.index('--max-episode-steps') + 1])
                                 if '--max-episode-steps' in argv else None),
              normalize_returns='--normalize-returns' in argv, fused_games='--fused-games' in argv,
              run_state='--run-state' in argv, episode_stats='--episode-stats' in argv,
              diagnostics='--diagnostics' in argv,
              checkpoint_every=(int(argv[argv.index('--checkpoint-every') + 1])
                                if '--checkpoint-every' in argv else 100))
