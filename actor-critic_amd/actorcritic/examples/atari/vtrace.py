"""V-trace actor-critic on Atari -- beyond the reference: A2C's losses on off-policy-corrected targets
(actorcritic.objectives.VTraceObjective; Espeholt et al. 2018), which lets one batch take several gradient
steps.  The structure is a2c_acktr.py's: environments -> MultiEnv -> AtariModel -> MultiEnvAgent ->
VTraceObjective -> optimizer -> ``optimize_shared`` -> the same session loop (loop.py).

Defaults are the A2C example's (conv3 64, RMSProp 7e-4 decayed linearly to 7e-5, global gradient-norm clip 0.5,
discount 0.99, entropy 0.01, n-step targets: lambda = 1) with one pass over the batch, which IS A2C: the
importance weights are all 1.  ``--epochs E --minibatches K`` take E passes over the batch in K env slices each;
from the second gradient step on the data are off-policy and the weights, clipped at ``--rho-bar`` / ``--c-bar``,
correct the targets.  The behaviour policy is the rollout's: the agent's cached activations.
"""

import sys

from actorcritic import parallel
from actorcritic.agents import MultiEnvAgent
from actorcritic.envs.atari.model import AtariModel
from actorcritic.examples.atari.a2c_acktr import create_optimizer, make_diagnostics, make_normalizer
from actorcritic.examples.atari.loop import make_multi_env, parse_flags, result_paths, train_loop
from actorcritic.nn import linear_decay
from actorcritic.objectives import VTraceObjective
from actorcritic.session import get_or_create_global_step


def train_vtrace(env_id, num_envs, num_steps, checkpoint_path, model_name, summary_path=None, max_updates=None,
                 seed=0, log_every=10, num_epochs=1, num_minibatches=1, rho_bar=1.0, c_bar=1.0, gae_lambda=1.0,
                 env_fns=None, mask_actions=False, game=None, on_update=None, episodic_life=False,
                 max_episode_steps=None, normalize_returns=False, fused_games=False, run_state=False,
                 checkpoint_every=100, episode_stats=False, diagnostics=False):
    """Trains an Atari model (conv3 64) with the V-trace actor-critic.

    ``num_envs`` is per GPU; with WORLD_SIZE > 1 (torchrun) every rank steps its own shard.
    ``num_epochs`` (``--epochs``) x ``num_minibatches`` (``--minibatches``) gradient steps per batch, over env
    slices (``num_minibatches`` must divide ``num_envs``); ``rho_bar`` (``--rho-bar``) >= ``c_bar`` (``--c-bar``)
    > 0 clip the importance weights; ``gae_lambda`` (``--lambda``) in [0, 1].
    Every other argument: as in a2c_acktr.train_a2c_acktr (with several gradient steps ``diagnostics`` are
    those of the whole op, the gradient the last step's, as in ppo.train_ppo).
    """
    parallel.init_from_env()
    multi_env, num_envs = make_multi_env(env_id, num_envs, seed, env_fns, mask_actions, game, episodic_life,
                                         max_episode_steps, fused_games, run_state, checkpoint_every)

    model = AtariModel(multi_env.observation_space, multi_env.action_space, 64, random_seed=seed)
    agent = MultiEnvAgent(multi_env, model, num_steps, mask_actions=mask_actions,
                          episode_stats=episode_stats or None)
    objective = VTraceObjective(model, discount_factor=0.99, entropy_regularization_strength=0.01,
                                gae_lambda=gae_lambda, rho_bar=rho_bar, c_bar=c_bar,
                                normalize_returns=make_normalizer(normalize_returns, multi_env),
                                diagnostics=make_diagnostics(diagnostics, multi_env))

    global_step = get_or_create_global_step()
    # 1e7 env-steps (4e7 frames) over the whole job; global steps = env-steps / batch
    max_step = 10000000 / (num_envs * num_steps * parallel.world_size())
    learning_rate = linear_decay(0.0007, 0.00007, global_step, max_step, name='learning_rate')

    optimizer = create_optimizer(False, model, learning_rate)
    optimize_op = objective.optimize_shared(optimizer, baseline_loss_weight=0.5, num_epochs=num_epochs,
                                            num_minibatches=num_minibatches, shuffle_seed=seed,
                                            global_step=global_step)
    scalars = [('policy_loss', objective.policy_loss), ('baseline_loss', objective.baseline_loss),
               ('policy_entropy', objective.mean_entropy)]
    train_loop(multi_env, model, agent, objective, optimizer, optimize_op, global_step, max_step, scalars,
               checkpoint_path, model_name, summary_path, max_updates, log_every, on_update, run_state,
               checkpoint_every)
    return model, optimizer


def parse_vtrace_flags(argv):
    """``--epochs``, ``--minibatches``, ``--rho-bar``, ``--c-bar``, ``--lambda`` -> train_vtrace's keywords
    (those given), beside loop.parse_flags' for the rest of the command line."""
    names = {'--epochs': ('num_epochs', int), '--minibatches': ('num_minibatches', int),
             '--rho-bar': ('rho_bar', float), '--c-bar': ('c_bar', float), '--lambda': ('gae_lambda', float)}
    return {key: kind(argv[argv.index(flag) + 1]) for flag, (key, kind) in names.items() if flag in argv}


if __name__ == '__main__':
    flags = dict(parse_flags(sys.argv[1:]), **parse_vtrace_flags(sys.argv[1:]))
    env_id, checkpoint_path, summary_path = result_paths(flags['game'], '-vtrace')
    train_vtrace(env_id, 32, 5, checkpoint_path, 'Atari-' + env_id, summary_path, **flags)
