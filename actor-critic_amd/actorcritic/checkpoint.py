"""Checkpoints and scalar summaries (reference: a2c_acktr.py:83-143, 256-303 —
tf.train.Saver files ``<path>/<model_name>-<step>`` + TensorBoard scalars).

TF checkpoints are unreadable without TensorFlow, so this engine writes its own:
``<prefix>-<step>.pt`` holding tensors and scalars only (loadable with
``torch.load(weights_only=True)``) and a ``checkpoint`` index file naming the latest,
like TF's.  Summaries are JSON lines (step, policy_loss, baseline_loss,
policy_entropy, episode_reward).

Beside a model checkpoint every rank may write its RUN STATE, ``<prefix>-<step>.run<rank>.pt``
(``save_run_state`` / ``load_run_state``): the envs' state, the next observations, the sample
counter, the return normaliser's carry and the agent's episode statistics -- with
it a run on the device envs resumes bit for bit.  The model checkpoint and the index file are what they were without it.
"""

import json
import os

import torch


def _first_order(optimizer):
    """The optimizer whose slot variables a checkpoint carries: the optimizer itself
    (A2C: clip-wrapped RMSProp) or, for ACKTR, its cold-start optimizer (clip-wrapped
    Momentum); the K-FAC state is saved separately under kfac/."""
    if optimizer is None:
        return None
    cold = getattr(optimizer, '_cold_optimizer', None)
    return cold if cold is not None else optimizer


def _optimizer_state(optimizer):
    out = {}
    if optimizer is None:
        return out
    st = getattr(optimizer, 'state', None)
    if isinstance(st, dict):
        for k, v in st.items():
            out['kfac/' + k] = v.detach().cpu()
    for attr in ('cov_updates', 'inverse_updates'):
        if hasattr(optimizer, attr):
            out['kfac_meta/' + attr] = torch.tensor(getattr(optimizer, attr))
    for name, v in _first_order(optimizer).slots().items():
        out['opt/' + name] = v.detach().cpu()
    return out


def _normalizer(objective):
    """The objective's ReturnNormalizer (normalize_returns=), or None."""
    return getattr(objective, 'return_normalizer', None)


def save(prefix, step, model, optimizer=None, objective=None):
    """``objective``: with a ReturnNormalizer its stats and settings are stored under retnorm/
    (not the envs' running returns: per-env state is not in this file but in the run state,
    ``save_run_state``)."""
    path = '{}-{}.pt'.format(prefix, int(step))
    blob = {'params': model.params.detach().cpu(), 'global_step': torch.tensor(int(step)),
            'num_actions': torch.tensor(model.num_actions), 'conv3_filters': torch.tensor(model.conv3_num_filters)}
    blob.update(_optimizer_state(optimizer))
    norm = _normalizer(objective)
    if norm is not None:
        st = norm.state_dict()
        blob['retnorm/stats'] = st['stats']
        blob['retnorm/epsilon'] = torch.tensor(st['epsilon'], dtype=torch.float64)
        blob['retnorm/clip'] = torch.tensor(st['clip'], dtype=torch.float64)
    tmp = path + '.tmp'
    torch.save(blob, tmp)
    os.replace(tmp, path)
    with open(os.path.join(os.path.dirname(prefix) or '.', 'checkpoint'), 'w') as f:
        json.dump({'model_checkpoint_path': os.path.basename(path)}, f)
    return path


def latest(directory):
    idx = os.path.join(directory, 'checkpoint')
    if not os.path.exists(idx):
        return None
    with open(idx) as f:
        name = json.load(f)['model_checkpoint_path']
    path = os.path.join(directory, name)
    return path if os.path.exists(path) else None


def load(path, model, optimizer=None, global_step=None, objective=None):
    """``objective``: its ReturnNormalizer takes the retnorm/ entries when the file has them
    (a checkpoint written without them leaves it as it is); its carry is zeroed, so a resume
    that continues the run loads the run state AFTER this (``load_run_state``)."""
    blob = torch.load(path, map_location='cpu', weights_only=True)
    if int(blob['num_actions']) != model.num_actions or int(blob['conv3_filters']) != model.conv3_num_filters:
        raise ValueError('checkpoint was written for a different model')
    model.params.copy_(blob['params'].to(model.params.device))
    model.engine.bump_version()
    if global_step is not None:
        global_step.assign(int(blob['global_step']))
    if optimizer is not None:
        eng = model.engine
        slots = {k[4:]: v for k, v in blob.items() if k.startswith('opt/')}
        if slots:
            # tf.train.Saver restores the slot variables too (a2c_acktr.py:101-102)
            _first_order(optimizer).restore_slots(eng, slots)
        if any(k.startswith('kfac/') for k in blob) and hasattr(optimizer, '_init_state'):
            st = optimizer._init_state(eng)
            for k, v in blob.items():
                if k.startswith('kfac/'):
                    st[k[5:]].copy_(v.to(eng.device))
            for attr in ('cov_updates', 'inverse_updates'):
                if 'kfac_meta/' + attr in blob:
                    setattr(optimizer, attr, int(blob['kfac_meta/' + attr]))
    norm = _normalizer(objective)
    if norm is not None and 'retnorm/stats' in blob:
        norm.load_state_dict({'stats': blob['retnorm/stats'], 'epsilon': float(blob['retnorm/epsilon']),
                              'clip': float(blob['retnorm/clip'])})
    return blob


# -- run state: what the rollout side carries from one update to the next --------
RUN_STATE_FORMAT = 1


def run_state_path(prefix, step, rank):
    """``<prefix>-<step>.run<rank>.pt``: rank ``rank``'s run state beside the model checkpoint
    ``<prefix>-<step>.pt``."""
    return '{}-{}.run{}.pt'.format(prefix, int(step), int(rank))


def save_run_state(prefix, step, agent, objective=None):
    """Called by EVERY rank, between an update and the next ``interact()``: writes this rank's
    ``agent.run_state()`` (next observations, sample counter, env state and, for an agent with
    episode statistics, their ``episode_stats`` state) and, with a ReturnNormalizer on
    ``objective``, its ``carry`` to ``run_state_path(prefix, step, rank)``.
    Tensors, ints and dicts of them only (``torch.load(weights_only=True)``); ``format``,
    ``rank``, ``world_size`` and ``global_step`` say what the file is.  Neither the model
    checkpoint nor the ``checkpoint`` index is touched."""
    from actorcritic import parallel
    rank, world = int(parallel.rank()), int(parallel.world_size())
    blob = {'format': RUN_STATE_FORMAT, 'rank': rank, 'world_size': world, 'global_step': int(step)}
    blob.update(agent.run_state())
    norm = _normalizer(objective)
    if norm is not None:
        blob['retnorm/carry'] = norm.carry_state()
    path = run_state_path(prefix, step, rank)
    tmp = path + '.tmp'
    torch.save(blob, tmp)
    os.replace(tmp, path)
    return path


def load_run_state(path, agent, objective=None):
    """Continues ``agent`` (and ``objective``'s ReturnNormalizer) from a ``save_run_state`` file.
    Call it AFTER ``load``: loading a model checkpoint zeroes the normalizer's carry.  ValueError
    when the file is another rank's or another world size's (the env shards would differ), of
    another format, or lacks the carry a normalizer needs or the ``episode_stats`` an agent with
    episode statistics needs (a file that has them loads into an agent without); and whatever
    ``agent.load_run_state`` refuses.  -> the blob (``global_step``: the step it was saved at)."""
    from actorcritic import parallel
    blob = torch.load(path, map_location='cpu', weights_only=True)
    if int(blob.get('format', -1)) != RUN_STATE_FORMAT:
        raise ValueError('{}: run state format {}, this build reads {}'.format(path, blob.get('format'),
                                                                               RUN_STATE_FORMAT))
    rank, world = int(parallel.rank()), int(parallel.world_size())
    if int(blob['world_size']) != world:
        raise ValueError('{}: run state of a world_size of {}, this job has {}'.format(path, int(blob['world_size']),
                                                                                     world))
    if int(blob['rank']) != rank:
        raise ValueError('{}: run state of rank {}, this is rank {}'.format(path, int(blob['rank']), rank))
    norm = _normalizer(objective)
    if norm is not None and 'retnorm/carry' not in blob:
        raise ValueError('{}: no retnorm/carry for the objective\'s ReturnNormalizer'.format(path))
    keys = ('next_obs', 'sample_counter', 'env')
    if getattr(agent, 'episode_stats', None) is not None:
        if 'episode_stats' not in blob:
            raise ValueError('{}: no episode_stats for the agent\'s EpisodeStats'.format(path))
        keys += ('episode_stats',)
    agent.load_run_state({k: blob[k] for k in keys})
    if norm is not None:
        norm.load_carry(blob['retnorm/carry'])
    return blob


class ScalarLog(object):
    """Append-only JSON-lines scalar summaries (the TensorBoard scalars of a2c_acktr.py:83-92)."""

    def __init__(self, directory):
        os.makedirs(directory, exist_ok=True)
        self._f = open(os.path.join(directory, 'scalars.jsonl'), 'a')

    def add(self, step, **scalars):
        rec = {'step': int(step)}
        rec.update({k: (None if v != v else float(v)) for k, v in scalars.items()})
        self._f.write(json.dumps(rec) + '\n')
        if int(step) % 10 == 0:
            self._f.flush()

    def close(self):
        self._f.close()
