"""A2C / ACKTR on Atari — the reference entry point (actorcritic/examples/atari/a2c_acktr.py)
on the MI355X engine.  The structure is the reference's line for line: environments ->
MultiEnv -> AtariModel -> MultiEnvAgent -> A2CObjective -> optimizer ->
``optimize_shared`` -> a session loop that interacts and runs the optimize op (loop.py,
shared with ppo.py).  The differences are the imports (no tensorflow / kfac / gym) and the
synthetic batched Atari stepper in place of ALE subprocesses.
"""

import os
import sys

import numpy as np

import actorcritic.envs.atari.wrappers as wrappers
from actorcritic import checkpoint, parallel
from actorcritic.agents import MultiEnvAgent
from actorcritic.envs.atari.model import AtariModel
from actorcritic.kfac_utils import ColdStartPeriodicInvUpdateKfacOpt, LayerCollection
from actorcritic.multi_env import MultiEnv
from actorcritic.nn import ClipGlobalNormOptimizer, MomentumOptimizer, RMSPropOptimizer, linear_decay
from actorcritic.objectives import A2CObjective
from actorcritic.return_norm import ReturnNormalizer, own_or_for_envs
from actorcritic.session import get_or_create_global_step


def train_a2c_acktr(acktr, env_id, num_envs, num_steps, checkpoint_path, model_name, summary_path=None,
                    max_updates=None, seed=0, log_every=10, env_fns=None, mask_actions=False, game=None,
                    on_update=None, episodic_life=False, max_episode_steps=None, normalize_returns=False,
                    fused_games=False, run_state=False, checkpoint_every=100, episode_stats=False,
                    diagnostics=False):
    """Trains an Atari model with A2C (RMSProp, conv3 64) or ACKTR (K-FAC, conv3 32).

    ``num_envs`` is per GPU; with WORLD_SIZE > 1 (torchrun) every rank steps its own shard.
    ``env_fns``: None (the synthetic batched stepper) or one function per env of this rank
    that makes a host env with raw RGB frames (create_host_environments); ``num_envs`` is
    then their number.
    ``mask_actions`` (``--mask-actions``): invalid-action masking -- the synthetic game under the
    full 18-action head with its minimal action set as the legal set (host envs: their
    ``legal_action_masks``); actions, losses and K-FAC statistics then run over the legal set.
    ``game`` (``--game catch|breakout``): a device game (envs.games.DeviceGameEnvs) instead of the
    synthetic stepper -- something that can be learned; ``env_id`` then only names the results.
    ``--game catch+breakout`` is a mixed batch: global env e plays the (e % 2)-th name, one network and
    one head (4 actions; with ``mask_actions`` 18 and every env's own set as its mask), and the scalar
    log gains ``episode_reward/<game>`` beside ``episode_reward``.
    ``episodic_life`` (``--episodic-life``) and ``max_episode_steps`` (``--max-episode-steps N``), device
    games only: a lost life is a terminal for the learner, and a step cap of N (1..2000) whose terminals
    are truncations -- the targets keep their bootstrap there (``model.truncations_placeholder``).
    Evaluation envs are built without episodic life (envs.games.evaluate counts terminals as games).
    ``normalize_returns`` (``--normalize-returns``): rewards scaled by the running std of the discounted
    return, per game (actorcritic.return_norm; groups from ReturnNormalizer.for_envs); its statistics
    travel with the checkpoints.  A ReturnNormalizer of the caller's own is taken as it is (the caller
    keeps it: scripts/learn_games.py logs its scale).
    ``fused_games`` (``--fused-games``), device games only: the rollout's fused step
    (DeviceGameEnvs(fused_step=True)), bit-identical to the default three-call chain.
    ``checkpoint_path`` None: nothing is loaded or saved.  ``on_update(updates, model)`` is called
    after every update (learning curves: scripts/learn_games.py).
    ``checkpoint_every`` (``--checkpoint-every K``): a checkpoint whenever the global step is a multiple of K.
    ``run_state`` (``--run-state``), device envs only: every rank writes its run state
    (checkpoint.save_run_state: env state, next observations, sample counter, the normaliser's carry) whenever
    rank 0 writes a model checkpoint, and one more pair when the loop ends at ``max_updates`` or the last
    step; at start the latest model checkpoint is loaded WITH this rank's run state (a missing file is a
    ValueError, not a silent reset), and the run continues bit for bit.  A stop request then writes nothing:
    it may fall between a rollout and its update, and the last pair stays the point to resume from.
    ``episode_stats`` (``--episode-stats``): the agent keeps episode statistics on the device
    (actorcritic.episode_stats: returns AND lengths of every episode that ended since the last log line, per
    game, over all ranks; an EpisodeStats of the caller's own is taken as it is).  The loop then never copies
    ``infos`` to the host; with a ``summary_path`` (given to every rank), on the updates that log every rank
    calls ``read()`` (a collective) and rank 0 logs ``episode_reward`` (now the interval's mean),
    ``episode_reward_std`` / ``_min`` / ``_max``, ``episode_length``, ``episode_length_max`` and ``episodes``,
    per game too (``/<game>``) when the batch holds more than one.  With ``run_state`` the statistics travel
    with the run state.  Without a ``summary_path`` the loop never reads: the statistics gather until the
    caller does (scripts/learn_games.py reads them at its evaluation points).  Off (default):
    ``episode_reward`` is the last rollout's mean on rank 0, as ever.
    ``diagnostics`` (``--diagnostics``): update diagnostics (actorcritic.update_diag; an UpdateDiagnostics of the
    caller's own is taken as it is).  With a ``summary_path`` (given to every rank) the loop arms the object on
    the updates that log, every rank reads it (a collective) and rank 0's log line gains ``explained_variance``,
    ``policy_kl``, ``grad_norm``, ``step_norm``, ... (per layer, per game, and with ACKTR ``precon_*`` and
    ``kfac_coeff``).  The run itself stays bit for bit the run without the option; off (default): today's keys.
    """
    # (loop.py calls the helpers below, so it is imported here, not at the top)
    from actorcritic.examples.atari.loop import make_multi_env, train_loop
    parallel.init_from_env()
    multi_env, num_envs = make_multi_env(env_id, num_envs, seed, env_fns, mask_actions, game, episodic_life,
                                         max_episode_steps, fused_games, run_state, checkpoint_every)

    conv3_num_filters = 32 if acktr else 64
    model = AtariModel(multi_env.observation_space, multi_env.action_space, conv3_num_filters, random_seed=seed)
    agent = MultiEnvAgent(multi_env, model, num_steps, mask_actions=mask_actions,
                          episode_stats=episode_stats or None)
    objective = A2CObjective(model, discount_factor=0.99, entropy_regularization_strength=0.01,
                             normalize_returns=make_normalizer(normalize_returns, multi_env),
                             diagnostics=make_diagnostics(diagnostics, multi_env))

    global_step = get_or_create_global_step()
    # 1e7 env-steps (4e7 frames) over the whole job; global steps = env-steps / batch
    max_step = 10000000 / (num_envs * num_steps * parallel.world_size())
    if acktr:
        learning_rate = linear_decay(0.25, 0.025, global_step, max_step, name='learning_rate')
    else:
        learning_rate = linear_decay(0.0007, 0.00007, global_step, max_step, name='learning_rate')

    optimizer = create_optimizer(acktr, model, learning_rate)
    optimize_op = objective.optimize_shared(optimizer, baseline_loss_weight=0.5, global_step=global_step)
    scalars = [('policy_loss', objective.policy_loss), ('baseline_loss', objective.baseline_loss),
               ('policy_entropy', objective.mean_entropy)]
    train_loop(multi_env, model, agent, objective, optimizer, optimize_op, global_step, max_step, scalars,
               checkpoint_path, model_name, summary_path, max_updates, log_every, on_update, run_state,
               checkpoint_every)
    return model, optimizer


def make_diagnostics(diagnostics, multi_env):
    """``diagnostics`` of the train functions -> None (falsy), the caller's UpdateDiagnostics, or (True) one
    with the groups of the envs."""
    from actorcritic.update_diag import UpdateDiagnostics
    return own_or_for_envs(diagnostics, UpdateDiagnostics, multi_env)


def make_normalizer(normalize_returns, multi_env):
    """``normalize_returns`` of the train functions -> None (falsy), the caller's ReturnNormalizer, or
    (True) one with the groups of the envs."""
    return own_or_for_envs(normalize_returns, ReturnNormalizer, multi_env)


def create_environments(env_id, num_envs, seed=0, full_action_set=False):
    """The batched synthetic Atari stepper for this rank's env shard.  ``full_action_set``:
    the game (an Atari-57 name) under the full 18-action set, its minimal action set in
    ``legal_action_masks`` (MultiEnvAgent(mask_actions=True))."""
    if full_action_set:
        return wrappers.SyntheticAtariEnvs(num_envs, num_actions=18, seed=seed, games=[env_id] * num_envs,
                                           env_offset=parallel.rank() * num_envs)
    return wrappers.SyntheticAtariEnvs(num_envs, num_actions=wrappers.num_actions_for(env_id), seed=seed,
                                       env_offset=parallel.rank() * num_envs)


def create_game_environments(game, num_envs, seed=0, full_action_set=False, episodic_life=False,
                             max_episode_steps=None, env_offset=None, fused_step=False):
    """This rank's shard of a device game ('catch', 'breakout') or of a mixed batch (a pattern such as
    'catch+breakout': the game follows the global env id, so the shards agree with one large batch).
    ``full_action_set``: under the 18-action head, every env's own actions in ``legal_action_masks``.
    ``episodic_life`` and ``max_episode_steps``: DeviceGameEnvs' (training envs only: evaluate()
    refuses episodic life).  ``env_offset``: global id of the first env, default rank * num_envs.
    ``fused_step``: DeviceGameEnvs' (the rollout's fused step; off by default)."""
    from actorcritic.envs.games import DeviceGameEnvs
    if env_offset is None:
        env_offset = parallel.rank() * num_envs
    return DeviceGameEnvs(game, num_envs, num_actions=18 if full_action_set else None, seed=seed,
                          env_offset=env_offset, episodic_life=episodic_life, max_episode_steps=max_episode_steps,
                          fused_step=fused_step)


def episode_reward_scalars(batched, episode_rewards):
    """The scalar log's ``episode_reward`` of one rollout's [N][T] episode rewards (the reference's: their
    nanmean, NaN when no episode ended), and the per-game keys of a mixed batch."""
    mean_episode_reward = (np.nan if np.all(np.isnan(episode_rewards)) else float(np.nanmean(episode_rewards)))
    return dict(episode_reward=mean_episode_reward, **episode_rewards_by_game(batched, episode_rewards))


def episode_rewards_by_game(batched, episode_rewards):
    """The scalar log's per-game keys of a mixed device-game batch: {'episode_reward/<game>': mean over
    the episodes that game's envs finished in this batch (NaN: none did)}; {} for anything else."""
    if not getattr(batched, 'is_mixed', False):
        return {}
    out = {}
    for name in sorted(set(batched.games)):
        rows = episode_rewards[np.array([g == name for g in batched.games])]
        out['episode_reward/' + name] = np.nan if np.all(np.isnan(rows)) else float(np.nanmean(rows))
    return out


def create_host_environments(env_fns, subprocess=True):
    """Host-stepped envs on the device rollout path: each function makes a gym-like env
    that returns raw RGB frames (``wrappers.make_atari_env(env_id, preprocess=False)``, or
    ``wrappers.wrap_atari_env(ale_like, preprocess=False)``), in a process of its own
    (``subprocess``: the functions must be picklable) or in this one."""
    from actorcritic.multi_env import create_subprocess_envs
    envs = create_subprocess_envs(env_fns) if subprocess else [env_fn() for env_fn in env_fns]
    return MultiEnv(wrappers.HostAtariEnvs(envs))


def create_optimizer(acktr, model, learning_rate):
    """ACKTR: cold-start Momentum(3e-4, .9)+clip .5 for 30 updates, then K-FAC
    (invert every 10, EMA .99, damping .01, momentum .9, trust region 1e-4);
    A2C: RMSProp + clip .5 (a2c_acktr.py:218-253)."""
    if acktr:
        layer_collection = LayerCollection()
        model.register_layers(layer_collection)
        model.register_predictive_distributions(layer_collection)
        cold_optimizer = MomentumOptimizer(learning_rate=0.0003, momentum=0.9)
        cold_optimizer = ClipGlobalNormOptimizer(cold_optimizer, clip_norm=0.5)
        return ColdStartPeriodicInvUpdateKfacOpt(
            num_cold_updates=30, cold_optimizer=cold_optimizer, invert_every=10, learning_rate=learning_rate,
            cov_ema_decay=0.99, damping=0.01, layer_collection=layer_collection, momentum=0.9,
            norm_constraint=0.0001)
    optimizer = RMSPropOptimizer(learning_rate=learning_rate)
    return ClipGlobalNormOptimizer(optimizer, clip_norm=0.5)


def load_model(checkpoint_path, model, optimizer, global_step, objective=None):
    path = checkpoint.latest(checkpoint_path)
    if path is None:
        print('No model loaded')
        return False
    checkpoint.load(path, model, optimizer, global_step, objective=objective)
    print('Loaded model')
    return True


def save_model(checkpoint_path, model_name, step, model, optimizer, objective=None):
    checkpoint.save(os.path.join(checkpoint_path, model_name), step, model, optimizer, objective=objective)
    print('Saved model (step {})'.format(step))


def check_run_state_args(run_state, checkpoint_every, env_fns):
    if int(checkpoint_every) < 1:
        raise ValueError('checkpoint_every must be at least 1, got {}'.format(checkpoint_every))
    if run_state and env_fns is not None:
        raise ValueError('run_state needs device envs: host-stepped envs keep their state in the host envs')


def save_checkpoint(checkpoint_path, model_name, step, model, optimizer, objective=None, agent=None):
    """Rank 0 writes the model checkpoint; with ``agent`` (``run_state=True``) every rank first writes its run
    state, so the index never names a step whose rank-0 run state is missing."""
    if agent is not None:
        checkpoint.save_run_state(os.path.join(checkpoint_path, model_name), step, agent, objective)
    if parallel.rank() == 0:
        save_model(checkpoint_path, model_name, step, model, optimizer, objective)


def load_run_state(checkpoint_path, model_name, step, agent, objective=None):
    """This rank's run state of the model checkpoint just loaded (``step``: its global step)."""
    path = checkpoint.run_state_path(os.path.join(checkpoint_path, model_name), step, parallel.rank())
    if not os.path.exists(path):
        raise ValueError('run_state=True, but the checkpoint of step {} has no run state for rank {} ({}); '
                         'resume without run_state to restart the envs'.format(step, parallel.rank(), path))
    blob = checkpoint.load_run_state(path, agent, objective)
    if int(blob['global_step']) != int(step):
        raise ValueError('{} was saved at step {}, the model checkpoint at {}'.format(path, int(blob['global_step']),
                                                                                    step))
    print('Loaded run state')


if __name__ == '__main__':
    from actorcritic.examples.atari.loop import parse_flags, result_paths
    flags = parse_flags(sys.argv[1:])
    env_id, checkpoint_path, summary_path = result_paths(flags['game'])
    train_a2c_acktr(True, env_id, 32, 20, checkpoint_path, 'Atari-' + env_id, summary_path, **flags)
