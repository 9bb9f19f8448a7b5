"""CPU tests of the per-game reward scaling (actorcritic/return_norm.py): the
C-ABI of acmi_retnorm_scan / acmi_retnorm_apply (declared, bound, exported, argument errors),
the numpy reference host_return_norm against hand-computed numbers and its own algebra
(Chan's merge over time, moments summed over env shards), the group derivation for device-game
batches, and the checkpoint round trip of the statistics."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from actorcritic import _lib, checkpoint
from actorcritic import return_norm as rn
from actorcritic.envs.games import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('acmi_retnorm_ws_doubles', 'acmi_retnorm_scan', 'acmi_retnorm_apply')


def batch(N, T, G, seed, empty=()):
    """Rewards from {0, +-1, 3} with about one nonzero in five, terminals about one in seven,
    a non-zero carry, non-zero stats, groups cycling over the non-empty ones."""
    rng = np.random.RandomState(seed)
    r = np.where(rng.rand(N, T) < 0.2, rng.choice([-1.0, 1.0, 3.0], size=(N, T)), 0.0).astype(np.float32)
    d = (rng.rand(N, T) < 1 / 7).astype(np.uint8)
    live = [g for g in range(G) if g not in empty]
    grp = np.array([live[n % len(live)] for n in range(N)], np.uint8)
    carry = rng.randn(N).astype(np.float32)
    stats = np.stack([rng.randint(5, 50, G).astype(np.float64), rng.randn(G), rng.rand(G) * 20 + 1], axis=1)
    return r, d, grp, carry, stats


def stats_close(got, ref, rel=1e-12):
    """Elementwise |got - ref| <= rel |ref| on count, mean and M2 (the counts: equal)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.array_equal(got[:, 0], ref[:, 0]) and bool(np.all(np.abs(got - ref) <= rel * np.abs(ref)))


# -- the C-ABI ----------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported(lib):
    src = open(os.path.join(ROOT, 'include', 'acmi.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(acmi_[a-z0-9_]+)\s*\(', src))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.EXPORTED, name
        assert hasattr(lib, name), name
    flat = re.sub(r'\s+', ' ', src)
    assert ('int acmi_retnorm_scan(const float* rewards, const uint8_t* terminals, const uint8_t* groups, int N, '
            'int T, int G, float gamma, float* carry, double* ws, double* moments, int32_t* bad_envs, '
            'acmi_stream_t stream);') in flat
    assert ('int acmi_retnorm_apply(const float* rewards, const uint8_t* groups, int N, int T, int G, '
            'const double* moments, double* stats, double eps, float clip, float* out, float* inv_out, '
            'acmi_stream_t stream);') in flat
    assert len(_lib._SIGS['acmi_retnorm_scan'][1]) == 12 and len(_lib._SIGS['acmi_retnorm_apply'][1]) == 12
    assert lib.acmi_abi_version() == 4
    assert lib.acmi_retnorm_ws_doubles(1) >= 2 and lib.acmi_retnorm_ws_doubles(257) >= 2 * 257
    assert lib.acmi_retnorm_ws_doubles(0) == 0


def test_argument_errors_come_before_any_launch(lib):
    one = ctypes.c_void_p(16)  # a non-null pointer no call gets as far as using

    def scan(r=one, d=one, grp=one, N=1, T=1, G=1, gamma=0.99, carry=one, ws=one, mom=one, bad=one):
        return lib.acmi_retnorm_scan(r, d, grp, N, T, G, gamma, carry, ws, mom, bad, None)

    def apply(r=one, grp=one, N=1, T=1, G=1, mom=one, stats=one, eps=1e-8, clip=10.0, out=one, inv=one):
        return lib.acmi_retnorm_apply(r, grp, N, T, G, mom, stats, eps, clip, out, inv, None)

    for name in ('r', 'd', 'grp', 'carry', 'ws', 'mom'):
        assert scan(**{name: None}) == _lib.ERR_ARG, name
    for name in ('r', 'grp', 'mom', 'stats', 'out'):
        assert apply(**{name: None}) == _lib.ERR_ARG, name
    for kw in (dict(N=0), dict(N=-1), dict(T=0), dict(T=-3), dict(G=0), dict(G=65), dict(G=-1), dict(G=255)):
        assert scan(**kw) == _lib.ERR_ARG, kw
        assert apply(**kw) == _lib.ERR_ARG, kw
        assert scan(bad=None, **kw) == _lib.ERR_ARG and apply(inv=None, **kw) == _lib.ERR_ARG
    for gamma in (-0.01, 1.01, float('nan'), float('inf')):
        assert scan(gamma=gamma) == _lib.ERR_ARG, gamma
    assert b'acmi_retnorm_scan' in lib.acmi_last_error()
    assert apply(eps=-1.0) == _lib.ERR_ARG and apply(eps=float('nan')) == _lib.ERR_ARG
    assert b'acmi_retnorm_apply' in lib.acmi_last_error()


# -- host_return_norm -----------------------------------------------------------------------
def test_hand_computed_two_envs_three_steps():
    """gamma 1/2.  env 0 (group 0, carry 0): r = 1, 2, 4 with a terminal at t = 1 -> u = 1, 2.5, 4
    (the terminal cuts after its sample), carry 4.  env 1 (group 1, carry 2): r = 0, -1, 0 ->
    u = 1, -0.5, -0.25, carry -0.25.  From empty stats the merge is the batch's own mean and M2."""
    r = np.array([[1, 2, 4], [0, -1, 0]], np.float32)
    d = np.array([[0, 1, 0], [0, 0, 0]], np.uint8)
    out, carry, stats, moments = rn.host_return_norm(r, d, [0, 1], 2, 0.5, carry=[0.0, 2.0], clip=3.0)
    assert carry.dtype == np.float32 and carry.tolist() == [4.0, -0.25]
    assert moments.tolist() == [[3.0, 7.5, 23.25], [3.0, 0.25, 1.3125]]
    assert stats[0].tolist() == [3.0, 2.5, 4.5]
    assert stats[1, 0] == 3.0 and abs(stats[1, 1] - 1 / 12) < 1e-15 and abs(stats[1, 2] - (1.3125 - 0.0625 / 3)) < 1e-15
    inv0 = np.float32(1.0 / np.sqrt(1.5 + 1e-8))
    inv1 = np.float32(1.0 / np.sqrt(stats[1, 2] / 3 + 1e-8))
    assert out.dtype == np.float32
    assert out[0].tolist() == [np.float32(1) * inv0, np.float32(2) * inv0, 3.0]  # 4 * 0.8165 clamps at 3
    assert out[1].tolist() == [0.0, np.float32(-1) * inv1, 0.0]
    # clip <= 0: no clamp
    free = rn.host_return_norm(r, d, [0, 1], 2, 0.5, carry=[0.0, 2.0], clip=0.0)[0]
    assert free[0, 2] == np.float32(4) * inv0 > 3.0


def test_two_calls_over_time_are_one_call_over_the_concatenation():
    """Chan's merge: carry bit-identical, stats of the second call within 1e-12 relative of a
    one-shot reference over all samples."""
    N, T1, T2, G = 7, 5, 8, 3
    r, d, grp, carry, _ = batch(N, T1 + T2, G, seed=1)
    _, c1, s1, _ = rn.host_return_norm(r[:, :T1], d[:, :T1], grp, G, 0.99, carry=carry)
    _, c2, s2, _ = rn.host_return_norm(r[:, T1:], d[:, T1:], grp, G, 0.99, carry=c1, stats=s1)
    _, call, sall, _ = rn.host_return_norm(r, d, grp, G, 0.99, carry=carry)
    assert np.array_equal(c2.view(np.uint32), call.view(np.uint32))
    assert stats_close(s2, sall)
    # and against the two-pass mean and M2 of the samples themselves
    u = np.empty((N, T1 + T2))
    R = carry.copy()
    for t in range(T1 + T2):
        R = ((R * np.float32(0.99)).astype(np.float32) + r[:, t]).astype(np.float32)
        u[:, t] = R
        R = np.where(d[:, t] != 0, np.float32(0), R)
    direct = np.array([[u[grp == g].size, u[grp == g].mean(), ((u[grp == g] - u[grp == g].mean()) ** 2).sum()]
                       for g in range(G)])
    assert stats_close(s2, direct)


def test_moments_of_env_shards_sum_to_the_batchs():
    N, T, G = 10, 6, 2
    r, d, grp, carry, stats = batch(N, T, G, seed=2)
    out, call, sall, mall = rn.host_return_norm(r, d, grp, G, 0.9, carry=carry, stats=stats)
    h = N // 2
    ca, ma = rn.host_scan(r[:h], d[:h], grp[:h], G, 0.9, carry[:h])
    cb, mb = rn.host_scan(r[h:], d[h:], grp[h:], G, 0.9, carry[h:])
    total = ma + mb
    assert np.array_equal(total[:, 0], mall[:, 0])
    assert np.all(np.abs(total - mall) <= 1e-13 * (1 + mall[:, 2:3]))
    assert np.array_equal(np.concatenate([ca, cb]), call)
    merged = rn.host_merge(stats, total)
    assert stats_close(merged, sall)
    parts = [rn.host_scale(r[:h], grp[:h], merged), rn.host_scale(r[h:], grp[h:], merged)]
    got = np.concatenate(parts)
    assert np.all(np.abs(got - out) <= np.spacing(np.abs(out)))


def test_a_group_without_envs_keeps_its_stats():
    r, d, grp, carry, stats = batch(3, 5, 2, seed=3, empty=(1,))
    assert set(grp.tolist()) == {0}
    out, _, new, m = rn.host_return_norm(r, d, grp, 2, 0.99, carry=carry, stats=stats)
    assert m[1].tolist() == [0.0, 0.0, 0.0] and np.array_equal(new[1], stats[1])
    assert new[0, 0] == stats[0, 0] + 15
    # a group that never had a sample scales by one
    fresh = rn.host_return_norm(r, d, grp, 2, 0.99)[2]
    assert fresh[1].tolist() == [0.0, 0.0, 0.0] and rn.host_inv(fresh)[1] == 1.0
    one = rn.host_return_norm(r, d, np.ones(3, np.uint8), 2, 0.99, frozen=True)[0]
    assert np.array_equal(one, r)


def test_frozen_changes_nothing():
    r, d, grp, carry, stats = batch(6, 4, 2, seed=4)
    out, c, s, m = rn.host_return_norm(r, d, grp, 2, 0.99, carry=carry, stats=stats, frozen=True)
    assert np.array_equal(c, carry) and np.array_equal(s, stats) and not m.any()
    assert np.array_equal(out, rn.host_scale(r, grp, stats))


def test_a_bad_group_id_passes_through():
    r, d, grp, carry, stats = batch(4, 3, 2, seed=5)
    grp = np.array([0, 2, 1, 255], np.uint8)
    r[1, 0] = 300.0  # (past the clip: a pass-through is not clamped either)
    out, c, s, m = rn.host_return_norm(r, d, grp, 2, 0.99, carry=carry, stats=stats)
    assert np.array_equal(out[1], r[1]) and np.array_equal(out[3], r[3])
    assert m[:, 0].tolist() == [3.0, 3.0]
    keep = [0, 2]
    ref = rn.host_return_norm(r[keep], d[keep], grp[keep], 2, 0.99, carry=carry[keep], stats=stats)
    assert np.array_equal(m, ref[3]) and np.array_equal(out[keep], ref[0])
    assert not np.array_equal(c[[1, 3]], carry[[1, 3]])  # the carry advances all the same


# -- ReturnNormalizer on the host -------------------------------------------------------------
def _game_envs(game, N, offset):
    """What the group derivation reads of a DeviceGameEnvs: ``env_game_ids``, which its constructor
    takes from the same host.env_game_ids (envs/games/__init__.py)."""
    return types.SimpleNamespace(num_envs=N, env_game_ids=host.env_game_ids(game, N, offset))


def test_env_game_ids_is_what_device_game_envs_stores():
    import inspect
    from actorcritic.envs import games
    assert host.env_game_ids('catch+breakout', 5) == (0, 1, 0, 1, 0)
    assert host.env_game_ids('catch+breakout', 5, 1) == (1, 0, 1, 0, 1)
    assert host.env_game_ids('breakout', 3) == (1, 1, 1) and host.env_game_ids(0, 2, env_offset=7) == (0, 0)
    assert host.env_game_ids(['breakout', 0], 2) == (1, 0) and host.env_game_ids('catch', 0) == ()
    with pytest.raises(ValueError):
        host.env_game_ids('pong', 1)
    src = inspect.getsource(games.DeviceGameEnvs.__init__)
    assert 'self.env_game_ids = env_game_ids(game, self.num_envs, self.env_offset)' in src
    assert 'self.game_ids = self.env_game_ids' in src


def test_groups_of_a_mixed_batch_follow_the_global_env_id():
    ids, G, names = rn.groups_for_envs(_game_envs('catch+breakout', 5, 0))
    assert ids == [0, 1, 0, 1, 0] and G == 2 and names == ('catch', 'breakout')
    ids, G, names = rn.groups_for_envs(_game_envs('catch+breakout', 5, 1))
    assert ids == [1, 0, 1, 0, 1] and G == 2
    ids, G, names = rn.groups_for_envs(_game_envs('breakout', 3, 0))
    assert ids == [1, 1, 1] and G == 2 and names == ('catch', 'breakout')
    # through a MultiEnv's .batched; anything else is one group
    ids, G, names = rn.groups_for_envs(types.SimpleNamespace(batched=_game_envs('catch+breakout', 2, 1)))
    assert ids == [1, 0]
    assert rn.groups_for_envs(types.SimpleNamespace(num_envs=3, games=None)) == ([0, 0, 0], 1, None)
    assert rn.groups_for_envs(types.SimpleNamespace(num_envs=2)) == ([0, 0], 1, None)
    synthetic = types.SimpleNamespace(num_envs=3, games=torch.tensor([5, 56, 0], dtype=torch.uint8))
    ids, G, names = rn.groups_for_envs(synthetic)
    assert ids == [5, 56, 0] and G == 57 and len(names) == 57
    norm = rn.ReturnNormalizer.for_envs(_game_envs('catch+breakout', 4, 1))
    assert norm.groups.tolist() == [1, 0, 1, 0] and norm.groups.dtype == torch.uint8
    assert norm.num_groups == 2 and norm.group_names == ('catch', 'breakout') and norm.frozen is False
    assert norm.stats.shape == (2, 3) and norm.stats.dtype == torch.float64 and not norm.stats.any()
    assert norm.carry.shape == (4,) and norm.carry.dtype == torch.float32
    assert (norm.epsilon, norm.clip) == (1e-8, 10.0)


@pytest.mark.parametrize('kw', [dict(groups=[]), dict(groups=[0, 2], num_groups=2), dict(groups=[0], num_groups=65),
                                dict(groups=[-1]), dict(groups=[0], group_names=['a', 'b']),
                                dict(groups=[0], epsilon=-1.0), dict(groups=[64])])
def test_normalizer_argument_errors(kw):
    with pytest.raises(ValueError):
        rn.ReturnNormalizer(**kw)


def test_objectives_take_the_argument():
    import inspect
    from actorcritic.examples.atari import a2c_acktr, ppo
    from actorcritic.objectives import A2CObjective, PPOObjective
    for cls in (A2CObjective, PPOObjective):
        assert inspect.signature(cls.__init__).parameters['normalize_returns'].default is None
        assert hasattr(cls, 'normalized_rewards') and hasattr(cls, 'return_stats')
        with pytest.raises(TypeError):
            cls(None, normalize_returns=True)
    for fn in (a2c_acktr.train_a2c_acktr, ppo.train_ppo):
        assert inspect.signature(fn).parameters['normalize_returns'].default is False
    for fn in (checkpoint.save, checkpoint.load):
        assert inspect.signature(fn).parameters['objective'].default is None


# -- checkpoints --------------------------------------------------------------------------------
def _model(seed):
    g = torch.Generator().manual_seed(seed)
    eng = types.SimpleNamespace(version=0, device=torch.device('cpu'))
    eng.bump_version = lambda: setattr(eng, 'version', eng.version + 1)
    return types.SimpleNamespace(params=torch.randn(11, generator=g), num_actions=4, conv3_num_filters=64, engine=eng)


def test_checkpoint_round_trip_of_the_stats(tmp_path):
    norm = rn.ReturnNormalizer([0, 1, 0, 1], num_groups=2, group_names=('catch', 'breakout'), clip=5.0)
    norm.stats.copy_(torch.tensor([[120.0, 0.25, 7.5], [60.0, -1.0, 31.0]], dtype=torch.float64))
    norm.carry.fill_(3.0)
    objective = types.SimpleNamespace(return_normalizer=norm)
    path = checkpoint.save(str(tmp_path / 'm'), 9, _model(1), objective=objective)
    blob = torch.load(path, map_location='cpu', weights_only=True)
    assert torch.equal(blob['retnorm/stats'], norm.stats) and not any(k.startswith('retnorm/carry') for k in blob)

    fresh = rn.ReturnNormalizer([0, 1, 0, 1], num_groups=2)
    fresh.carry.fill_(-2.0)
    checkpoint.load(path, _model(2), objective=types.SimpleNamespace(return_normalizer=fresh))
    assert torch.equal(fresh.stats, norm.stats) and fresh.stats.dtype == torch.float64
    assert fresh.clip == 5.0 and fresh.epsilon == 1e-8
    assert not fresh.carry.any()  # env state is not checkpointed: the running returns start over
    assert np.array_equal(fresh.inv.numpy(), rn.host_inv(norm.stats.numpy()))
    # state_dict / load_state_dict directly
    sd = norm.state_dict()
    assert set(sd) == {'stats', 'num_groups', 'epsilon', 'clip', 'group_names'} and 'carry' not in sd
    with pytest.raises(ValueError):
        rn.ReturnNormalizer([0, 1, 2]).load_state_dict(sd)

    # a checkpoint without the entries loads as before and leaves the normalizer alone
    old = checkpoint.save(str(tmp_path / 'old'), 3, _model(3))
    assert not any(k.startswith('retnorm/') for k in torch.load(old, map_location='cpu', weights_only=True))
    before = fresh.stats.clone()
    checkpoint.load(old, _model(4), objective=types.SimpleNamespace(return_normalizer=fresh))
    assert torch.equal(fresh.stats, before)
    # and a checkpoint with them loads without an objective
    checkpoint.load(path, _model(5))
