"""CPU tests of the update diagnostics (actorcritic/update_diag.py): the C-ABI of the
three acmi_diag_* entry points (declared, bound, exported, argument errors before any launch), the
numpy restatements against plain float64 formulas, the derivations from accumulator rows, the host
path of UpdateDiagnostics with read()'s key set, and read() as a collective over two gloo ranks."""
import ctypes
import inspect
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from actorcritic import _lib
from actorcritic import update_diag as ud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('acmi_diag_ws_doubles', 'acmi_diag_value', 'acmi_diag_policy', 'acmi_diag_segments')
BASE = ['explained_variance', 'value_mean', 'target_mean', 'target_std', 'policy_kl', 'policy_kl_max',
        'policy_entropy_after']
NORMS = ['grad_norm', 'step_norm', 'param_norm'] + ['grad_norm/' + l for l in ud.LAYERS] + \
    ['step_norm/' + l for l in ud.LAYERS]
KFAC = ['precon_norm/' + l for l in ud.LAYERS] + ['precon_cos/' + l for l in ud.LAYERS] + ['kfac_coeff']


# -- the C-ABI --------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported(lib):
    src = open(os.path.join(ROOT, 'include', 'acmi.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(acmi_[a-z0-9_]+)\s*\(', src))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.EXPORTED, name
        assert hasattr(lib, name), name
    flat = re.sub(r'\s+', ' ', src)
    assert 'int64_t acmi_diag_ws_doubles(int64_t M, int64_t S);' in flat
    assert ('int acmi_diag_value(const float* values, const float* targets, const uint8_t* groups, int N, int T, '
            'int G, double* ws, double* acc, int32_t* bad_envs, acmi_stream_t stream);') in flat
    assert ('int acmi_diag_policy(const float* logits_old, int ld_old, const float* logits_new, int ld_new, '
            'const uint32_t* legal, const uint8_t* groups, int N, int T, int A, int G, double* ws, double* acc, '
            'int32_t* bad_envs, int32_t* bad_rows, acmi_stream_t stream);') in flat
    assert ('int acmi_diag_segments(const float* x, const float* y, const int64_t* offsets, int S, double* ws, '
            'double* out, acmi_stream_t stream);') in flat
    assert [len(_lib._SIGS[n][1]) for n in NEW[1:]] == [10, 15, 7]
    # additive: the ABI version and the struct sizes are the parent's
    assert lib.acmi_abi_version() == 4 and '#define ACMI_ABI_VERSION 4' in open(
        os.path.join(ROOT, 'include', 'acmi.h')).read()
    sizes = (ctypes.c_int64 * 16)()
    assert lib.acmi_abi_struct_sizes(sizes, 16) == 5
    # the workspace serves the value partials (5 per env, N <= M), the policy rows (3 per row), 64 x 4 per segment
    assert lib.acmi_diag_ws_doubles(264, 0) >= 5 * 264 and lib.acmi_diag_ws_doubles(0, 12) >= 12 * 256
    assert lib.acmi_diag_ws_doubles(10240, 12) >= max(5 * 10240, 12 * 256)
    assert lib.acmi_diag_ws_doubles(0, 0) == 0 and lib.acmi_diag_ws_doubles(-3, -1) == 0


def test_argument_errors_come_before_any_launch(lib):
    one = ctypes.c_void_p(16)  # a non-null pointer no call gets as far as using

    def value(v=one, y=one, grp=one, N=1, T=1, G=1, ws=one, acc=one, bad=one):
        return lib.acmi_diag_value(v, y, grp, N, T, G, ws, acc, bad, None)

    def policy(zo=one, ldo=4, zn=one, ldn=4, legal=None, grp=one, N=1, T=1, A=4, G=1, ws=one, acc=one, bad=one,
               rows=one):
        return lib.acmi_diag_policy(zo, ldo, zn, ldn, legal, grp, N, T, A, G, ws, acc, bad, rows, None)

    def segments(x=one, y=one, off=one, S=1, ws=one, out=one):
        return lib.acmi_diag_segments(x, y, off, S, ws, out, None)

    for name in ('v', 'y', 'ws', 'acc'):
        assert value(**{name: None}) == _lib.ERR_ARG, name
    assert b'acmi_diag_value' in lib.acmi_last_error()
    for name in ('zo', 'zn', 'ws', 'acc'):
        assert policy(**{name: None}) == _lib.ERR_ARG, name
        assert policy(legal=one, **{name: None}) == _lib.ERR_ARG, name
    for name in ('x', 'off', 'ws', 'out'):
        assert segments(**{name: None}) == _lib.ERR_ARG, name
        assert segments(y=None, **{name: None}) == _lib.ERR_ARG, name
    assert b'acmi_diag_segments' in lib.acmi_last_error()
    sizes = (dict(G=0), dict(G=65), dict(G=-1), dict(N=0), dict(N=-2), dict(T=0), dict(N=1 << 16, T=1 << 15))
    for kw in sizes:
        assert value(**kw) == _lib.ERR_ARG, kw
        assert value(grp=None, bad=None, **kw) == _lib.ERR_ARG, kw
        assert policy(**kw) == _lib.ERR_ARG, kw
    for kw in (dict(A=0), dict(A=-1), dict(A=65, ldo=65, ldn=65), dict(A=33, ldo=33, ldn=33, legal=one),
               dict(A=4, ldo=3), dict(A=4, ldn=3), dict(A=32, ldo=32, ldn=31, legal=one)):
        assert policy(**kw) == _lib.ERR_ARG, kw
        assert policy(bad=None, rows=None, grp=None, **kw) == _lib.ERR_ARG, kw
    assert b'acmi_diag_policy' in lib.acmi_last_error()
    for S in (0, -1, 65536):
        assert segments(S=S) == _lib.ERR_ARG, S


# -- the restatements against plain formulas ----------------------------------------------------
def test_host_value_diag_against_float64_formulas():
    rng = np.random.RandomState(0)
    N, T, G = 7, 5, 3
    v, y = rng.randn(N, T).astype(np.float32), (rng.randn(N, T) * 3 + 1).astype(np.float32)
    grp = [0, 2, 0, 2, 0, 2, 7]  # group 1 is empty, the last env joins no group
    acc, bad = ud.host_value_diag(v, y, grp, G)
    assert acc.dtype == np.float64 and acc.shape == (G, 6) and bad == 1
    assert acc[1].tolist() == [0, 0, 0, 0, 0, 0] and acc[:, 0].tolist() == [15, 0, 15]
    for g, envs in ((0, [0, 2, 4]), (2, [1, 3, 5])):
        v64, y64 = v[envs].astype(np.float64).ravel(), y[envs].astype(np.float64).ravel()
        want = [v64.size, v64.sum(), y64.sum(), (y64 ** 2).sum(), (y64 - v64).sum(), ((y64 - v64) ** 2).sum()]
        assert np.allclose(acc[g], want, rtol=1e-14, atol=0)
        ev = 1.0 - np.var(y64 - v64) / np.var(y64)
        assert abs(ud.explained_variance(acc[g]) - ev) <= 1e-12
        s = ud.value_scalars(acc[g])
        assert list(s) == BASE[:4]
        assert abs(s['value_mean'] - v64.mean()) <= 1e-14 and abs(s['target_mean'] - y64.mean()) <= 1e-14
        assert abs(s['target_std'] - y64.std()) <= 1e-12
    assert ud.host_value_diag(v, y, None, 1)[0][0, 0] == N * T  # no groups: every env in group 0


def test_explained_variance_is_1_0_and_nan():
    y = np.array([[1, 2, 3, 4], [5, 6, 7, 10]], np.float32)
    row = lambda v: ud.host_value_diag(np.asarray(v, np.float32), y, None, 1)[0][0]
    assert ud.explained_variance(row(y)) == 1.0                                  # v = y
    assert ud.explained_variance(row(np.full_like(y, y.mean()))) == 0.0          # v = mean(y) = 4.75: all exact
    assert ud.explained_variance(row(-y)) < 0.0
    const = np.full((2, 4), 0.1, np.float32)
    r = ud.host_value_diag(np.zeros((2, 4), np.float32), const, None, 1)[0][0]
    assert np.isnan(ud.explained_variance(r)) and ud.value_scalars(r)['target_std'] == 0.0  # constant y
    empty = np.zeros(6)
    assert np.isnan(ud.explained_variance(empty)) and all(np.isnan(x) for x in ud.value_scalars(empty).values())


def _softmax64(z):
    z = z.astype(np.float64)
    p = np.exp(z - z.max())
    return p / p.sum()


def test_host_policy_rows_against_float64_formulas():
    rng = np.random.RandomState(1)
    M, A = 12, 6
    zo, zn = (rng.randn(M, A) * 3).astype(np.float32), (rng.randn(M, A) * 3).astype(np.float32)
    good, kl, h = ud.host_policy_rows(zo, zn)
    assert good.all()
    for m in range(M):
        p, q = _softmax64(zo[m]), _softmax64(zn[m])
        assert abs(kl[m] - (p * np.log(p / q)).sum()) <= 1e-13
        assert abs(h[m] + (q * np.log(q)).sum()) <= 1e-13
    # masked: the sums run over S only, an illegal logit influences nothing; padded rows: ld > A
    legal = rng.randint(1, 1 << A, M).astype(np.uint32)
    wild = zo.copy()
    pad_o, pad_n = np.full((M, A + 3), 7e9, np.float32), np.full((M, A + 3), np.nan, np.float32)
    pad_o[:, :A], pad_n[:, :A] = zo, zn
    for m in range(M):
        for a in range(A):
            if not (int(legal[m]) >> a) & 1:
                wild[m, a] = 1e30 if a % 2 else -1e30
    got = ud.host_policy_rows(zo, zn, legal)
    for other in (ud.host_policy_rows(wild, zn, legal), ud.host_policy_rows(pad_o, pad_n, legal, num_actions=A)):
        assert all(np.array_equal(a, b) for a, b in zip(got, other))
    for m in range(M):
        S = ud.legal_columns(legal[m], A)
        p, q = _softmax64(zo[m, S]), _softmax64(zn[m, S])
        assert abs(got[1][m] - (p * np.log(p / q)).sum()) <= 1e-13
    # identical matrices: exactly zero; bad rows: empty S, a NaN in old (even at an illegal action), an inf in new
    same = ud.host_policy_rows(zo, zo.copy(), legal)
    assert same[0].all() and (same[1] == 0.0).all()
    legal[2] = 0
    zo[5, int(np.argmin([(int(legal[5]) >> a) & 1 for a in range(A)]))] = np.nan
    zn[9, 0] = np.inf
    good, kl, h = ud.host_policy_rows(zo, zn, legal)
    assert np.flatnonzero(~good).tolist() == [2, 5, 9] and (kl[~good] == 0).all() and (h[~good] == 0).all()
    acc, bad_envs, bad_rows = ud.host_policy_diag(zo, zn, legal, [0, 1, 5], 2, 4)
    assert (bad_envs, bad_rows) == (1, 3) and acc[:, 0].tolist() == [3, 3]  # rows 0-3 | 4-7; 8-11 join no group
    assert acc[0, 1] == kl[[0, 1, 3]].sum() and acc[1, 3] == kl[[4, 6, 7]].max()
    none = ud.host_policy_diag(zo[:4], zn[:4], np.zeros(4, np.uint32), None, 1, 4)[0]
    assert none[0].tolist() == [0, 0, 0, -np.inf]


def test_host_segment_sums_and_offsets():
    rng = np.random.RandomState(2)
    x, y = rng.randn(300).astype(np.float32), rng.randn(300).astype(np.float32)
    off = [0, 1, 64, 64, 300]
    out = ud.host_segment_sums(x, y, off)
    assert out.shape == (4, 4) and out[2].tolist() == [0, 0, 0, 0]
    for s in (0, 1, 3):
        a, b = x[off[s]:off[s + 1]].astype(np.float64), y[off[s]:off[s + 1]].astype(np.float64)
        assert np.allclose(out[s], [a @ a, b @ b, a @ b, (a - b) @ (a - b)], rtol=1e-13, atol=0)
    nul = ud.host_segment_sums(x, None, off)
    assert np.array_equal(nul[:, 0], out[:, 0]) and np.array_equal(nul[:, 3], out[:, 0]) and not nul[:, 1:3].any()
    for bad in ([0, 5, 4], [0], [-1, 3], [0, 301]):
        with pytest.raises(ValueError):
            ud.host_segment_sums(x, y, bad)
    assert ud.cosine([4.0, 9.0, -6.0, 0.0]) == -1.0 and np.isnan(ud.cosine([0.0, 9.0, 0.0, 0.0]))


# -- the class on the host path -------------------------------------------------------------------
def _batch(N, T, A, seed):
    rng = np.random.RandomState(seed)
    return dict(v=rng.randn(N, T).astype(np.float32), y=rng.randn(N, T).astype(np.float32),
                zo=rng.randn(N * T, A).astype(np.float32), zn=rng.randn(N * T, A).astype(np.float32),
                legal=rng.randint(1, 1 << A, N * T).astype(np.uint32))


def _feed(diag, b, norms=False, precon=False, rng=None):
    diag.request()
    assert diag.armed
    diag.record_value(b['v'], torch.from_numpy(b['y']))  # (numpy arrays and CPU tensors both take the host path)
    diag.record_policy(torch.from_numpy(b['zo']), b['zn'], b['legal'])
    if norms:
        rng = np.random.RandomState(9)
        off = np.arange(13) * 10
        g, p, w0, w1 = (rng.randn(120).astype(np.float32) for _ in range(4))
        diag.record_segments('grad', g, p if precon else None, off)
        diag.record_segments('step', w1, w0, off)
        if precon:
            diag.record_coeff(torch.tensor([0.25]))
        b = dict(b, g=g, p=p, w0=w0, w1=w1)
    diag.finish()
    assert not diag.armed
    return b


def test_read_key_set_and_values_on_the_host_path():
    N, T, A = 4, 3, 5
    b = _batch(N, T, A, 3)
    plain = ud.UpdateDiagnostics([0, 1, 0, 1])
    _feed(plain, b)
    out = plain.read()
    assert list(out) == BASE  # no names: no per-group keys; no segments fed: no norms
    named = ud.UpdateDiagnostics([0, 1, 0, 1], group_names=('catch', 'breakout'))
    b = _feed(named, b, norms=True, precon=True)
    out = named.read()
    per_game = [k + '/' + g for g in ('catch', 'breakout') for k in ('explained_variance', 'policy_kl')]
    assert list(out) == BASE + NORMS + KFAC + per_game
    first = ud.UpdateDiagnostics([0, 1, 0, 1], group_names=('catch', 'breakout'))
    _feed(first, b, norms=True)
    assert list(first.read()) == BASE + NORMS + per_game  # a first-order optimizer: no K-FAC keys
    one_game = ud.UpdateDiagnostics([1, 1, 1, 1], num_groups=2, group_names=('catch', 'breakout'))
    _feed(one_game, b)
    assert list(one_game.read()) == BASE
    # the values: against the restatements over the whole batch
    v64, y64 = b['v'].astype(np.float64), b['y'].astype(np.float64)
    assert abs(out['explained_variance'] - (1 - np.var(y64 - v64) / np.var(y64))) <= 1e-12
    good, kl, h = ud.host_policy_rows(b['zo'], b['zn'], b['legal'])
    assert abs(out['policy_kl'] - kl.mean()) <= 1e-14 and out['policy_kl_max'] == kl.max()
    assert abs(out['policy_entropy_after'] - h.mean()) <= 1e-14
    rows = np.repeat([0, 1, 0, 1], T) == 1
    assert abs(out['policy_kl/breakout'] - kl[rows].mean()) <= 1e-14
    g, p, w0, w1 = (b[k].astype(np.float64) for k in ('g', 'p', 'w0', 'w1'))
    assert abs(out['grad_norm'] - np.linalg.norm(g)) <= 1e-12 and abs(out['step_norm'] - np.linalg.norm(w1 - w0)) <= 1e-12
    assert abs(out['param_norm'] - np.linalg.norm(w1)) <= 1e-12 and out['kfac_coeff'] == 0.25
    sl = slice(60, 80)  # fc4: segments 6 and 7
    assert abs(out['grad_norm/fc4'] - np.linalg.norm(g[sl])) <= 1e-12
    assert abs(out['step_norm/fc4'] - np.linalg.norm((w1 - w0)[sl])) <= 1e-12
    assert abs(out['precon_norm/fc4'] - np.linalg.norm(p[sl])) <= 1e-12
    assert abs(out['precon_cos/fc4'] - g[sl] @ p[sl] / np.linalg.norm(g[sl]) / np.linalg.norm(p[sl])) <= 1e-12
    assert all(type(x) is float for x in out.values())


def test_read_without_an_armed_update_raises():
    diag = ud.UpdateDiagnostics([0, 0])
    with pytest.raises(RuntimeError, match='armed'):
        diag.read()
    diag.request()
    with pytest.raises(RuntimeError, match='armed'):  # armed, but its update has not run
        diag.read()
    _feed(diag, _batch(2, 2, 3, 4))
    assert diag.updates == 1 and list(diag.read()) == BASE
    with pytest.raises(RuntimeError, match='armed'):  # read once: nothing stale is logged twice
        diag.read()


@pytest.mark.parametrize('kw', [dict(groups=[]), dict(groups=[0, 2], num_groups=2), dict(groups=[0], num_groups=65),
                                dict(groups=[-1]), dict(groups=[0], group_names=['a', 'b']), dict(groups=[64]),
                                dict(groups=[0], forward_rows=0)])
def test_argument_errors_of_the_class(kw):
    with pytest.raises(ValueError):
        ud.UpdateDiagnostics(**kw)


def test_class_refuses_other_row_counts_and_objectives_check_the_type():
    diag = ud.UpdateDiagnostics([0, 0, 0])
    diag.request()
    with pytest.raises(ValueError, match='envs'):
        diag.record_value(np.zeros((4, 2), np.float32), np.zeros((4, 2), np.float32))
    from actorcritic.examples.atari import a2c_acktr, ppo
    from actorcritic.objectives import A2CObjective, PPOObjective
    for cls in (A2CObjective, PPOObjective):
        assert inspect.signature(cls.__init__).parameters['diagnostics'].default is None
        with pytest.raises(TypeError):
            cls(None, diagnostics='yes')
        assert cls(None, diagnostics=diag).diagnostics is diag and cls(None).diagnostics is None
    for fn in (a2c_acktr.train_a2c_acktr, ppo.train_ppo):
        assert inspect.signature(fn).parameters['diagnostics'].default is False


def test_groups_come_from_return_norm():
    import types
    from actorcritic.envs.games import host
    envs = types.SimpleNamespace(num_envs=4, env_game_ids=host.env_game_ids('catch+breakout', 4, 1))
    diag = ud.UpdateDiagnostics.for_envs(types.SimpleNamespace(batched=envs))
    assert diag.groups.tolist() == [1, 0, 1, 0] and diag.groups.dtype == torch.uint8
    assert diag.num_groups == 2 and diag.group_names == ('catch', 'breakout') and diag.forward_rows == 1024


# -- two ranks ----------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _two_rank_batch():
    b = _batch(4, 3, 5, 11)
    b['zn'][:6] = b['zo'][:6] + np.float32(0.01) * b['zn'][:6]  # rank 0's rows barely move: the max is rank 1's
    return b, [0, 1, 0, 1]


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, os.path.join(ROOT, 'actor-critic_amd'))
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from actorcritic import parallel, update_diag
    parallel.init_from_env(backend='gloo')
    assert parallel.world_size() == world and parallel.rank() == rank
    b, grp = _two_rank_batch()
    envs, rows = slice(2 * rank, 2 * rank + 2), slice(6 * rank, 6 * rank + 6)
    diag = update_diag.UpdateDiagnostics(grp[envs], num_groups=2, group_names=('catch', 'breakout'))
    diag.request()
    diag.record_value(b['v'][envs], b['y'][envs])
    diag.record_policy(b['zo'][rows], b['zn'][rows], b['legal'][rows])
    diag.finish()
    torch.save(diag.read(), os.path.join(out_dir, 'rank{}.pt'.format(rank)))
    parallel.barrier()
    parallel.destroy()


def test_read_over_two_gloo_ranks_gives_the_whole_batch(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    b, grp = _two_rank_batch()
    whole = ud.UpdateDiagnostics(grp, num_groups=2, group_names=('catch', 'breakout'))
    _feed(whole, b)
    want = whole.read()
    halves = []
    for rank in range(world):
        part = ud.UpdateDiagnostics(grp[2 * rank:2 * rank + 2], num_groups=2)
        _feed(part, {k: v[2 * rank:2 * rank + 2] if k in 'vy' else v[6 * rank:6 * rank + 6] for k, v in b.items()})
        halves.append(part.read())
    assert halves[0]['policy_kl_max'] < halves[1]['policy_kl_max'] == want['policy_kl_max']
    for rank in range(world):
        got = torch.load(str(tmp_path / 'rank{}.pt'.format(rank)))
        assert list(got) == list(want)
        assert got['policy_kl_max'] == want['policy_kl_max']  # the larger of the two ranks'
        for k in want:  # sums of two ranks' partial sums against one sum: within a few ulps
            assert abs(got[k] - want[k]) <= 1e-13 * max(1.0, abs(want[k])), (k, got[k], want[k])
