"""Episode statistics on the device: per-game returns and lengths over a log interval.

Beyond the reference, whose loop copies one rollout's ``[N][T]`` episode rewards to the host
and logs their ``nanmean``: every episode that ends in ANY rollout of the interval is counted,
per GROUP of envs (per game), with its length in env-steps, beside the rollout and without a
host wait; under data parallelism over all ranks.  The host sees G x 8 doubles per log line.

The maths (include/acmi.h states it for the kernels, :func:`host_episode_stats` restates it in
numpy for the tests).  State across rollouts: ``length_carry[N]`` int32, the steps of each
env's running episode; ``acc[G][8]`` f64.  Per rollout over ``episode_rewards[N][T]`` f32 (an
episode's total reward at the step that ended it, a NaN elsewhere):

* per env, ascending t: ``len += 1``; where ``episode_rewards[n][t]`` is not a NaN -- by its
  bits, ``(bits & 0x7fffffff) > 0x7f800000`` is a NaN, so every payload means "none" and
  +-inf is a sample -- ``(ret, len)`` is one sample of the env's group and ``len = 0``;
* ``acc[g]`` = (episodes, sum ret, sum ret^2, sum len, max ret, max -ret, max len, max -len):
  the sums in double, the maxima from -inf (the minima negated, so that one MAX all-reduce
  serves both ends).  A rollout adds to it; ``read(reset=True)`` clears it.

An env whose group id is >= G joins no group; its length advances, ``bad_envs`` counts it.
"""

import numpy as np
import torch

from actorcritic import _lib
from actorcritic.return_norm import check_groups, groups_for_envs

COLS = 8  # episodes, sum ret, sum ret^2, sum len | max ret, max -ret, max len, max -len
NUM_SUMS = 4
STAT_KEYS = ('episodes', 'mean', 'std', 'min', 'max', 'mean_length', 'min_length', 'max_length')


# -- the numpy reference ------------------------------------------------------------------
def cleared_acc(num_groups):
    """[G][8] f64: 0 in the sums, -inf in the maxima."""
    acc = np.zeros((int(num_groups), COLS), np.float64)
    acc[:, NUM_SUMS:] = -np.inf
    return acc


def is_nan_bits(x):
    """``(bits & 0x7fffffff) > 0x7f800000`` of a float32 array."""
    bits = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return (bits & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)


def host_samples(episode_rewards, length_carry=None):
    """-> (per env the list of its (ret f32, len int) samples, length_carry int32 [N] after the batch)."""
    ep = np.ascontiguousarray(episode_rewards, np.float32)
    N, T = ep.shape
    none = is_nan_bits(ep)
    carry = np.zeros(N, np.int32) if length_carry is None else np.array(length_carry, dtype=np.int32).reshape(N)
    samples = []
    for n in range(N):
        row, length = [], int(carry[n])
        for t in range(T):
            length += 1
            if not none[n, t]:
                row.append((ep[n, t], length))
                length = 0
        carry[n] = length
        samples.append(row)
    return samples, carry


def host_episode_stats(episode_rewards, groups, num_groups, length_carry=None, acc=None):
    """The module docstring's maths in numpy, float64 -> (length_carry int32 [N], acc f64 [G][8]);
    the arguments are not written.  ``length_carry`` None: zeros; ``acc`` None: cleared."""
    G = int(num_groups)
    grp = np.asarray(groups).astype(np.int64)
    samples, carry = host_samples(episode_rewards, length_carry)
    acc = cleared_acc(G) if acc is None else np.array(acc, dtype=np.float64).reshape(G, COLS).copy()
    for n, row in enumerate(samples):
        g = int(grp[n])
        if g >= G:
            continue
        for ret, length in row:
            r, l = np.float64(ret), np.float64(length)
            with np.errstate(invalid='ignore', over='ignore'):  # (+inf and -inf in one group: a NaN sum)
                acc[g, :NUM_SUMS] += (1.0, r, r * r, l)
            acc[g, NUM_SUMS:] = np.maximum(acc[g, NUM_SUMS:], (r, -r, l, -l))
    return carry, acc


def stats_of(row):
    """One ``acc`` row (or a reduction of rows) -> the dict ``read`` returns for it."""
    c, s, q, sl, rmax, nrmin, lmax, nlmin = (float(x) for x in row)
    if c == 0:
        return dict({k: float('nan') for k in STAT_KEYS}, episodes=0)
    with np.errstate(invalid='ignore', over='ignore'):
        mean = np.float64(s) / c
        std = np.sqrt(np.maximum(np.float64(q) / c - mean * mean, 0.0))
    return {'episodes': int(c), 'mean': float(mean), 'std': float(std), 'min': -nrmin, 'max': rmax,
            'mean_length': sl / c, 'min_length': -nlmin, 'max_length': lmax}


def reduce_groups(acc):
    """The ``'all'`` row of an ``acc``: the sums summed, the maxima maximised over the groups."""
    acc = np.asarray(acc, np.float64)
    with np.errstate(invalid='ignore'):
        return np.concatenate([acc[:, :NUM_SUMS].sum(axis=0), acc[:, NUM_SUMS:].max(axis=0)])


class EpisodeStats(object):
    """The state of the statistics (module docstring) and their launches.

    Args:
        groups: one group id per env of this rank (ints 0..num_groups-1).
        num_groups: G, 1..64; default max(groups) + 1.  Every rank must use the same G.
        group_names: the keys of ``read()``'s dict, or None (then ``'0'``, ``'1'``, ...).

    ``acc`` ([G][8] f64), ``length_carry`` ([N] int32) and ``bad_envs`` (int32 [1]) live on the
    host until the first use on a device (``to``; ``update`` on a device tensor), then there.
    ``state_dict`` holds ``acc``, ``length_carry``, ``num_groups`` and the group ids: all of it is
    per-rank state of a run and travels with the run state (MultiEnvAgent.run_state).
    """

    def __init__(self, groups, num_groups=None, group_names=None):
        ids, G, self.group_names = check_groups(groups, num_groups, group_names)
        self.num_envs, self.num_groups = len(ids), G
        self.groups = torch.tensor(ids, dtype=torch.uint8)
        self.length_carry = torch.zeros(len(ids), dtype=torch.int32)
        self.acc = torch.from_numpy(cleared_acc(G))
        self.bad_envs = torch.zeros(1, dtype=torch.int32)
        self._cleared = self.acc.clone()
        self._ws = None

    @classmethod
    def for_envs(cls, batched_env):
        ids, G, names = groups_for_envs(batched_env)
        return cls(ids, num_groups=G, group_names=names)

    @property
    def device(self):
        return self.acc.device

    def to(self, device):
        device = torch.device(device)
        if self.acc.device != device:
            for name in ('groups', 'length_carry', 'acc', 'bad_envs', '_cleared'):
                setattr(self, name, getattr(self, name).to(device))
            self._ws = None
        return self

    def keys(self):
        """The group keys of ``read()``'s dict, in group order."""
        return self.group_names if self.group_names is not None else tuple(str(g) for g in range(self.num_groups))

    def update(self, episode_rewards, stream=None):
        """Adds one rollout's ``episode_rewards`` ([N][T] f32).  A device tensor: two launches on
        ``stream`` (a hipStream_t handle; None: the tensor's device's current stream), no host
        wait; the state moves to that device.  A numpy array or CPU tensor: the host function."""
        if torch.is_tensor(episode_rewards) and episode_rewards.is_cuda:
            N, T = episode_rewards.shape
            self._check_envs(N)
            if episode_rewards.dtype != torch.float32:
                raise ValueError('episode_rewards must be float32, got {}'.format(episode_rewards.dtype))
            self.to(episode_rewards.device)
            need = int(_lib.load().acmi_epstats_ws_doubles(N))
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.zeros(need, dtype=torch.float64, device=self.device)
            if stream is None:
                stream = _lib.stream_handle(self.device)
            _lib.call('acmi_epstats_update', _lib.ptr(episode_rewards), _lib.ptr(self.groups), N, T, self.num_groups,
                      _lib.ptr(self.length_carry), _lib.ptr(self._ws), _lib.ptr(self.acc), _lib.ptr(self.bad_envs),
                      stream)
            return
        ep = episode_rewards.detach().numpy() if torch.is_tensor(episode_rewards) else np.asarray(episode_rewards)
        if ep.ndim != 2:
            raise ValueError('episode_rewards must be [N][T], got shape {}'.format(ep.shape))
        self._check_envs(ep.shape[0])
        carry, acc = host_episode_stats(ep, self.groups.cpu().numpy(), self.num_groups,
                                        self.length_carry.cpu().numpy(), self.acc.cpu().numpy())
        self.length_carry.copy_(torch.from_numpy(carry))
        self.acc.copy_(torch.from_numpy(acc))

    def _check_envs(self, N):
        if N != self.num_envs:
            raise ValueError('episode rewards of {} envs for statistics of {}'.format(N, self.num_envs))

    def reset(self):
        """Clears ``acc`` (not ``length_carry``: the running episodes go on)."""
        self.acc.copy_(self._cleared)

    def read(self, reset=True):
        """-> {group key: stats, ..., 'all': stats} of the episodes since the last reset, each
        ``{'episodes', 'mean', 'std' (population), 'min', 'max', 'mean_length', 'min_length',
        'max_length'}``; everything but ``episodes`` is NaN where ``episodes == 0``.

        Under data parallelism a COLLECTIVE: every rank calls it at the same update (one SUM
        all-reduce of the sums, one MAX all-reduce of the maxima, on copies on the accumulators'
        device) and every rank gets the statistics over all ranks.  Then the one device-to-host
        copy, of G x 8 doubles.  ``reset``: the local accumulators are cleared afterwards;
        ``length_carry`` never is."""
        from actorcritic import parallel
        total = self.acc
        if parallel.world_size() > 1:
            sums = parallel.allreduce_sum_(self.acc[:, :NUM_SUMS].contiguous())
            maxima = parallel.allreduce_max_(self.acc[:, NUM_SUMS:].contiguous())
            total = torch.cat([sums, maxima], dim=1)
        host = np.array(total.detach().cpu().numpy())  # (a copy also of host accumulators: reset writes them)
        if reset:
            self.reset()
        out = {key: stats_of(row) for key, row in zip(self.keys(), host)}
        out['all'] = stats_of(reduce_groups(host))
        return out

    def state_dict(self):
        return {'acc': self.acc.detach().cpu().clone(), 'length_carry': self.length_carry.detach().cpu().clone(),
                'num_groups': self.num_groups, 'groups': self.groups.detach().cpu().clone()}

    def load_state_dict(self, state):
        """ValueError, naming the field, when the state is of another G, other group ids or
        another number of envs; nothing is written then."""
        if int(state['num_groups']) != self.num_groups:
            raise ValueError('episode statistics: num_groups {} for an object of {}'.format(int(state['num_groups']),
                                                                                          self.num_groups))
        groups = torch.as_tensor(state['groups']).to(torch.uint8).cpu()
        carry, acc = torch.as_tensor(state['length_carry']), torch.as_tensor(state['acc'])
        if tuple(carry.shape) != (self.num_envs,) or carry.dtype != torch.int32:
            raise ValueError('episode statistics: length_carry of shape {} {} for {} envs (int32 [{}])'.format(
                tuple(carry.shape), carry.dtype, self.num_envs, self.num_envs))
        if groups.shape != self.groups.shape or not torch.equal(groups, self.groups.cpu()):
            raise ValueError('episode statistics: groups of the state are not this object\'s group ids')
        if tuple(acc.shape) != (self.num_groups, COLS) or acc.dtype != torch.float64:
            raise ValueError('episode statistics: acc of shape {} {}, not float64 [{}][{}]'.format(
                tuple(acc.shape), acc.dtype, self.num_groups, COLS))
        self.acc.copy_(acc.to(self.device))
        self.length_carry.copy_(carry.to(self.device))

    def log_scalars(self, stats):
        """``read()``'s dict -> the scalar log's keys: from ``'all'`` ``episode_reward`` (the interval's
        mean), ``episode_reward_std``, ``_min``, ``_max``, ``episode_length``, ``episode_length_max`` and
        ``episodes``; when this rank's envs span more than one group and the groups have names, the same
        keys with a ``/<name>`` suffix for each of those groups."""
        def keys(s, suffix=''):
            return {'episode_reward' + suffix: s['mean'], 'episode_reward_std' + suffix: s['std'],
                    'episode_reward_min' + suffix: s['min'], 'episode_reward_max' + suffix: s['max'],
                    'episode_length' + suffix: s['mean_length'], 'episode_length_max' + suffix: s['max_length'],
                    'episodes' + suffix: s['episodes']}
        out = keys(stats['all'])
        present = sorted(set(self.groups.tolist()))
        if self.group_names is not None and len(present) > 1:
            for g in present:
                out.update(keys(stats[self.group_names[g]], '/' + self.group_names[g]))
        return out
