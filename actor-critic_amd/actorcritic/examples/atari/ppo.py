"""PPO on Atari — beyond the reference, which stops at A2C / ACKTR.  The structure is
a2c_acktr.py's: environments -> MultiEnv -> AtariModel -> MultiEnvAgent -> PPOObjective
-> optimizer -> ``optimize_shared`` -> the same session loop (loop.py) that interacts and runs
the optimize op; checkpoints and summaries are handled the same way.

Defaults are the common Atari PPO setting (Schulman et al. 2017, table 5, at 32 envs):
conv3 64, 32 envs x 128 steps, 4 epochs x 4 minibatches, clip 0.1, GAE(0.95) with
batch-normalised advantages, Adam (epsilon 1e-5) at 2.5e-4 decayed linearly to 0, global
gradient-norm clip 0.5.  Minibatches are env slices by default; ``minibatch='rows'`` shuffles
all env-steps of the batch per epoch (objectives.PPOOptimizeOp).
"""

import sys

from actorcritic import parallel
from actorcritic.agents import MultiEnvAgent
from actorcritic.envs.atari.model import AtariModel
from actorcritic.examples.atari.a2c_acktr import make_diagnostics, make_normalizer
from actorcritic.examples.atari.loop import make_multi_env, parse_flags, result_paths, train_loop
from actorcritic.nn import AdamOptimizer, ClipGlobalNormOptimizer, linear_decay
from actorcritic.objectives import PPOObjective
from actorcritic.session import get_or_create_global_step


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
    multi_env, num_envs = make_multi_env(env_id, num_envs, seed, env_fns, mask_actions, game, episodic_life,
                                         max_episode_steps, fused_games, run_state, checkpoint_every)

    model = AtariModel(multi_env.observation_space, multi_env.action_space, 64, random_seed=seed)
    agent = MultiEnvAgent(multi_env, model, num_steps, mask_actions=mask_actions,
                          episode_stats=episode_stats or None)
    objective = PPOObjective(model, discount_factor=0.99, entropy_regularization_strength=0.01,
                             clip_range=clip_range, value_clip_range=value_clip_range, gae_lambda=0.95,
                             normalize_advantages=True,
                             normalize_returns=make_normalizer(normalize_returns, multi_env),
                             diagnostics=make_diagnostics(diagnostics, multi_env))

    global_step = get_or_create_global_step()
    # 1e7 env-steps (4e7 frames) over the whole job; global steps = env-steps / batch
    max_step = 10000000 / (num_envs * num_steps * parallel.world_size())
    learning_rate = linear_decay(0.00025, 0.0, global_step, max_step, name='learning_rate')

    optimizer = create_optimizer(learning_rate)
    optimize_op = objective.optimize_shared(optimizer, baseline_loss_weight=0.5, num_epochs=num_epochs,
                                            num_minibatches=num_minibatches, shuffle_seed=seed,
                                            global_step=global_step, minibatch=minibatch)
    scalars = [('policy_loss', objective.policy_loss), ('baseline_loss', objective.baseline_loss),
               ('policy_entropy', objective.mean_entropy), ('approx_kl', objective.approx_kl),
               ('clip_fraction', objective.clip_fraction)]
    train_loop(multi_env, model, agent, objective, optimizer, optimize_op, global_step, max_step, scalars,
               checkpoint_path, model_name, summary_path, max_updates, log_every, on_update, run_state,
               checkpoint_every)
    return model, optimizer


def create_optimizer(learning_rate):
    """Adam (epsilon 1e-5) + clip .5."""
    optimizer = AdamOptimizer(learning_rate=learning_rate, epsilon=1e-5)
    return ClipGlobalNormOptimizer(optimizer, clip_norm=0.5)


if __name__ == '__main__':
    flags = parse_flags(sys.argv[1:])
    env_id, checkpoint_path, summary_path = result_paths(flags['game'], '-ppo')
    train_ppo(env_id, 32, 128, checkpoint_path, 'Atari-' + env_id, summary_path, **flags)
