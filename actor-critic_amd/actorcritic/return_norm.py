"""Per-game reward scaling by the running standard deviation of the discounted return.

Beyond the reference, which feeds raw rewards to its targets: baselines'
``VecNormalize(ret=True)``, with one set of statistics per GROUP of envs (per game) so that
a batch of different games under one value head sees rewards of one scale.  The network,
the targets and the losses are untouched: the objective (``A2CObjective(...,
normalize_returns=)``) puts the scaled rewards in place of the fed ones.

The maths (include/acmi.h states it for the kernels, :func:`host_return_norm` restates it
in numpy for the tests).  State across updates: ``carry[N]`` f32, each env's running
discounted return; ``stats[G][3]`` f64, per group (count, mean, M2).  Per update over
``rewards[N][T]`` and ``terminals[N][T]`` (a truncation is a terminal here):

* scan: per env, ascending t, in float32: ``R = R*gamma; R = R + r``; that R is the sample
  u; a terminal sets R = 0 after the sample; ``carry = R`` at the end;
* moments: per group (c, s, q) = (samples, sum u, sum u^2) in double, fixed order;
  under data parallelism they are summed over ranks here;
* merge (Chan et al.), per group with c > 0: ``mb = s/c, M2b = max(q - s*s/c, 0), tot = n + c,
  d = mb - mean, mean += d*c/tot, M2 += M2b + d*d*n*c/tot, n = tot``;
* scale: ``inv[g] = f32(1/sqrt(M2/n + eps))`` from the MERGED stats (update first, then scale,
  as VecNormalize; n == 0: 1), ``out = clamp(r*inv[group], -clip, +clip)`` in float32.

An env whose group id is >= G joins no group and keeps its rewards; ``bad_envs`` counts it.
"""

import numpy as np
import torch

from actorcritic import _lib

MAX_GROUPS = 64


# -- the numpy reference ------------------------------------------------------------------
def host_samples(rewards, terminals, gamma, carry):
    """The float32 scan -> (samples u f32 [N][T], carry after the batch f32 [N])."""
    r = np.asarray(rewards, np.float32)
    d = np.asarray(terminals).astype(bool)
    N, T = r.shape
    g32 = np.float32(gamma)
    R = np.array(carry, dtype=np.float32).reshape(N).copy()
    u = np.empty((N, T), np.float32)
    for t in range(T):
        R = (R * g32).astype(np.float32)
        R = (R + r[:, t]).astype(np.float32)
        u[:, t] = R
        R = np.where(d[:, t], np.float32(0), R).astype(np.float32)
    return u, R


def host_scan(rewards, terminals, groups, num_groups, gamma, carry):
    """-> (carry after the batch f32 [N], moments f64 [G][3] = (c, s, q))."""
    grp = np.asarray(groups).astype(np.int64)
    G = int(num_groups)
    u, R = host_samples(rewards, terminals, gamma, carry)
    moments = np.zeros((G, 3), np.float64)
    u64 = u.astype(np.float64)
    for g in range(G):
        rows = u64[grp == g]
        moments[g] = (rows.size, rows.sum(), (rows * rows).sum())
    return R, moments


def host_merge(stats, moments):
    """Chan's update of stats [G][3] (count, mean, M2) by the batch moments (c, s, q) -> new stats."""
    out = np.array(stats, dtype=np.float64).copy()
    for g, (c, s, q) in enumerate(np.asarray(moments, np.float64)):
        if c > 0:
            n, mean, M2 = out[g]
            mb = s / c
            M2b = max(q - s * s / c, 0.0)
            tot = n + c
            dl = mb - mean
            out[g] = (tot, mean + dl * c / tot, M2 + M2b + dl * dl * n * c / tot)
    return out


def host_inv(stats, epsilon=1e-8):
    """inv[g] = f32(1/sqrt(M2/n + eps)), 1 for a group without samples."""
    st = np.asarray(stats, np.float64)
    inv = np.ones(st.shape[0], np.float32)
    for g, (n, _, M2) in enumerate(st):
        if n > 0:
            inv[g] = np.float32(1.0 / np.sqrt(M2 / n + epsilon))
    return inv


def host_scale(rewards, groups, stats, epsilon=1e-8, clip=10.0):
    """out = clamp(r * inv[group], -clip, +clip) in float32; a bad group id keeps r."""
    r = np.asarray(rewards, np.float32)
    grp = np.asarray(groups).astype(np.int64)
    inv = host_inv(stats, epsilon)
    good = grp < inv.shape[0]
    k = np.where(good, inv[np.where(good, grp, 0)], np.float32(1)).astype(np.float32)
    v = (r * k[:, None]).astype(np.float32)
    if clip > 0:
        c = np.float32(clip)
        v = np.where(v > c, c, np.where(v < -c, -c, v)).astype(np.float32)
    return np.where(good[:, None], v, r).astype(np.float32)


def host_return_norm(rewards, terminals, groups, num_groups, gamma, carry=None, stats=None, epsilon=1e-8, clip=10.0,
                     frozen=False):
    """The module docstring's maths in numpy: float32 scan, float64 moments and merge.
    -> (out f32 [N][T], carry f32 [N], stats f64 [G][3], moments f64 [G][3]); the arguments
    are not written.  ``frozen``: the given stats are applied; stats and carry come back
    as they went in (moments: zeros)."""
    r = np.asarray(rewards, np.float32)
    N = r.shape[0]
    G = int(num_groups)
    carry = np.zeros(N, np.float32) if carry is None else np.array(carry, dtype=np.float32).copy()
    stats = np.zeros((G, 3), np.float64) if stats is None else np.array(stats, dtype=np.float64).copy()
    if frozen:
        moments = np.zeros((G, 3), np.float64)
    else:
        carry, moments = host_scan(r, terminals, groups, G, gamma, carry)
        stats = host_merge(stats, moments)
    return host_scale(r, groups, stats, epsilon, clip), carry, stats, moments


# -- groups of a batched env --------------------------------------------------------------
def groups_for_envs(batched_env):
    """(group id per env, number of groups, group names) of a batched env (or of a ``MultiEnv``
    through ``.batched``): a DeviceGameEnvs' ``env_game_ids`` (envs.games.host.env_game_ids: its
    ``game_ids`` when mixed, else every env its ``game_id``; names of envs.games.GAMES), a
    SyntheticAtariEnvs' ``games`` tensor (Atari-57 indices), else one group."""
    env = getattr(batched_env, 'batched', None) or batched_env
    N = int(env.num_envs)
    if hasattr(env, 'env_game_ids'):  # DeviceGameEnvs
        from actorcritic.envs.games.host import GAMES
        return [int(i) for i in env.env_game_ids], len(GAMES), tuple(GAMES)
    games = getattr(env, 'games', None)
    if torch.is_tensor(games):  # SyntheticAtariEnvs: a u8 index per env
        from actorcritic.envs.atari.wrappers import ATARI57
        return [int(i) for i in games.cpu().tolist()], len(ATARI57), tuple(ATARI57)
    return [0] * N, 1, None


def check_groups(groups, num_groups, group_names):
    """The per-group classes' constructor arguments, checked -> (ids, G, names as a tuple of str or None)."""
    ids = [int(g) for g in groups]
    if not ids:
        raise ValueError('groups: one id per env, got none')
    G = max(ids) + 1 if num_groups is None else int(num_groups)
    if not 1 <= G <= MAX_GROUPS:
        raise ValueError('num_groups={} outside 1..{}'.format(G, MAX_GROUPS))
    if min(ids) < 0 or max(ids) >= G:
        raise ValueError('group ids must lie in 0..{}'.format(G - 1))
    if group_names is not None and len(group_names) != G:
        raise ValueError('group_names: {} names for {} groups'.format(len(group_names), G))
    return ids, G, None if group_names is None else tuple(str(n) for n in group_names)


def own_or_for_envs(option, cls, envs):
    """An option of the train functions or of the agent -> None (falsy), the caller's own ``cls`` object, or
    (anything else that is true) ``cls.for_envs(envs)``."""
    if isinstance(option, cls):
        return option
    return cls.for_envs(envs) if option else None


class ReturnNormalizer(object):
    """The state of the scaling (module docstring) and its launches.

    Args:
        groups: one group id per env of this rank (ints 0..num_groups-1).
        num_groups: G, 1..64; default max(groups) + 1.  Every rank must use the same G.
        group_names: names for logs, or None.
        epsilon, clip: the scale's (``clip <= 0``: no clamp).

    ``stats`` ([G][3] f64: count, mean, M2), ``carry`` ([N] f32), ``inv`` ([G] f32, the scale
    of the last call) and ``bad_envs`` (int32 [1]) live on the host until the first use on a
    device (``to``), then on the engine's.  ``frozen`` (default False): the current stats are
    applied, neither ``stats`` nor ``carry`` changes (evaluation, or a fixed scale).
    ``state_dict`` holds the stats and the settings, not ``carry``: that is per-env state of one
    rank and travels with the run state (``carry_state`` / ``load_carry``;
    checkpoint.save_run_state), so ``load_state_dict`` zeroes it.  The order of a resume is
    therefore the model checkpoint first (``load_state_dict``), the run state second
    (``load_carry``).  Loading also REPLACES ``epsilon`` and ``clip`` by the saved values (the
    statistics were applied with them); set them again after loading to change them.
    """

    def __init__(self, groups, num_groups=None, group_names=None, epsilon=1e-8, clip=10.0):
        ids, G, self.group_names = check_groups(groups, num_groups, group_names)
        if not float(epsilon) >= 0.0:
            raise ValueError('epsilon must not be negative, got {}'.format(epsilon))
        self.num_envs, self.num_groups = len(ids), G
        self.epsilon, self.clip = float(epsilon), float(clip)
        self.frozen = False
        self.groups = torch.tensor(ids, dtype=torch.uint8)
        self.carry = torch.zeros(len(ids), dtype=torch.float32)
        self.stats = torch.zeros((G, 3), dtype=torch.float64)
        self.inv = torch.ones(G, dtype=torch.float32)
        self.bad_envs = torch.zeros(1, dtype=torch.int32)
        self._moments = torch.zeros((G, 3), dtype=torch.float64)
        self._zero_moments = torch.zeros((G, 3), dtype=torch.float64)
        self._ws = None

    @classmethod
    def for_envs(cls, batched_env, epsilon=1e-8, clip=10.0):
        ids, G, names = groups_for_envs(batched_env)
        return cls(ids, num_groups=G, group_names=names, epsilon=epsilon, clip=clip)

    @property
    def device(self):
        return self.stats.device

    def to(self, device):
        device = torch.device(device)
        if self.stats.device != device:
            for name in ('groups', 'carry', 'stats', 'inv', 'bad_envs', '_moments', '_zero_moments'):
                setattr(self, name, getattr(self, name).to(device))
            self._ws = None
        return self

    def normalize(self, rewards, terminals, gamma, out, stream, world_size=1):
        """Scaled ``rewards`` ([N][T] f32 device tensor, not written unless it is ``out``) into
        ``out``; ``terminals`` [N][T] u8.  Not frozen: scan (2 launches), the moments summed over
        ranks when ``world_size > 1``, merge + scale (1 launch); frozen: the scale alone."""
        N, T = rewards.shape
        if N != self.num_envs:
            raise ValueError('rewards of {} envs for a normalizer of {}'.format(N, self.num_envs))
        self.to(rewards.device)
        G = self.num_groups
        moments = self._zero_moments  # (c == 0 in every group: the merge keeps the stats)
        if not self.frozen:
            need = int(_lib.load().acmi_retnorm_ws_doubles(N))
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.zeros(need, dtype=torch.float64, device=self.device)
            moments = self._moments
            _lib.call('acmi_retnorm_scan', _lib.ptr(rewards), _lib.ptr(terminals), _lib.ptr(self.groups), N, T, G,
                      float(gamma), _lib.ptr(self.carry), _lib.ptr(self._ws), _lib.ptr(moments),
                      _lib.ptr(self.bad_envs), stream)
            if world_size > 1:
                from actorcritic import parallel
                parallel.allreduce_sum_(moments)
        _lib.call('acmi_retnorm_apply', _lib.ptr(rewards), _lib.ptr(self.groups), N, T, G, _lib.ptr(moments),
                  _lib.ptr(self.stats), self.epsilon, self.clip, _lib.ptr(out), _lib.ptr(self.inv), stream)
        return out

    def state_dict(self):
        return {'stats': self.stats.detach().cpu().clone(), 'num_groups': self.num_groups, 'epsilon': self.epsilon,
                'clip': self.clip, 'group_names': None if self.group_names is None else list(self.group_names)}

    def carry_state(self):
        """The envs' running discounted returns, a [N] f32 CPU tensor (a copy): the part of the
        state that ``state_dict`` leaves out (class docstring)."""
        return self.carry.detach().cpu().clone()

    def load_carry(self, carry):
        """Puts back what ``carry_state`` returned; call it AFTER ``load_state_dict`` (or
        checkpoint.load), which zeroes the carry.  ValueError unless it is [num_envs] float32."""
        t = torch.as_tensor(carry)
        if tuple(t.shape) != (self.num_envs,) or t.dtype != torch.float32:
            raise ValueError('carry of shape {} {} for a normalizer of {} envs (float32 [{}])'.format(
                tuple(t.shape), t.dtype, self.num_envs, self.num_envs))
        self.carry.copy_(t.to(self.device))

    def load_state_dict(self, state):
        stats = torch.as_tensor(state['stats'], dtype=torch.float64)
        if int(state.get('num_groups', stats.shape[0])) != self.num_groups or \
                tuple(stats.shape) != (self.num_groups, 3):
            raise ValueError('return statistics of {} groups for a normalizer of {}'.format(stats.shape[0],
                                                                                         self.num_groups))
        self.stats.copy_(stats.to(self.device))
        self.epsilon = float(state.get('epsilon', self.epsilon))
        self.clip = float(state.get('clip', self.clip))
        self.carry.zero_()
        self.inv.copy_(torch.from_numpy(host_inv(stats.numpy(), self.epsilon)).to(self.device))
