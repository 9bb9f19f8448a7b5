"""CPU tests of the V-trace feature's host side: the rule book (actorcritic/vtrace.py) against the GAE
restatement and against itself in float64, its edge rules, the entry point's declaration and binding, and the
argument contracts of VTraceObjective that need no GPU.

Bounds.  eps = 2^-23.  One step of the scan makes at most 8 float32 roundings (the two weights as they are
rounded to float32, gamma * V, + r, - V, * rho, (gamma lambda) * c, * acc, + delta, + V; the advantage's
three are not carried), each of a quantity of magnitude at most

    B = max|r| + max|V, v_boot| + max(max|V, v_boot|, max|target|)

and moves it by at most eps/2 of that; gamma * lambda is itself rounded once (eps/2, relative, of a term
bounded by B).  With rho, c <= 1 and gamma lambda <= 1 a step does not amplify what it carries, so after T
steps |f32 - f64| <= T * 4.5 eps * B < 5 T eps B, for targets and advantages alike.
"""
import os
import re
import sys

import numpy as np
import pytest

from actorcritic import _lib
from actorcritic import vtrace

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import oracle  # noqa: E402

EPS = float(np.finfo(np.float32).eps)


def batch(N, T, seed, p_term=0.25):
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((N, T)).astype(np.float32)
    d = rng.random((N, T)) < p_term
    d[0] = False
    if N > 1:
        d[1] = True
    v = rng.standard_normal((N, T)).astype(np.float32)
    vb = rng.standard_normal(N).astype(np.float32)
    return rng, r, d, v, vb


def magnitude(r, v, vb, tgt):
    mv = max(float(np.abs(v).max()), float(np.abs(vb).max()))
    return float(np.abs(r).max()) + mv + max(mv, float(np.abs(tgt).max()))


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


@pytest.mark.parametrize('lam', [0.0, 0.95, 1.0])
def test_unit_weights_give_the_gae_targets_bit_for_bit(lam):
    for N, T, seed in ((1, 1, 0), (7, 9, 1), (33, 20, 2)):
        _, r, d, v, vb = batch(N, T, seed)
        one = np.ones((N, T), np.float32)
        tgt, adv = vtrace.vtrace_f32(one, one, r, d, v, vb, 0.99, lam)
        ref, _ = oracle.gae_f32(r, d, v, vb, 0.99, lam)
        assert tgt.dtype == np.float32 and adv.dtype == np.float32
        assert np.array_equal(bits(tgt), bits(ref)), (N, T, lam)
        # truncated flags that are all clear, or set only where no terminal is, change nothing
        for tr in (np.zeros((N, T), bool), ~d):
            t2, a2 = vtrace.vtrace_f32(one, one, r, d, v, vb, 0.99, lam, truncated=tr)
            assert np.array_equal(bits(t2), bits(tgt)) and np.array_equal(bits(a2), bits(adv))


@pytest.mark.parametrize('lam', [0.0, 0.95, 1.0])
@pytest.mark.parametrize('truncated', [False, True])
def test_float32_scan_matches_float64(lam, truncated):
    N, T = 33, 20
    rng, r, d, v, vb = batch(N, T, 3)
    tr = (rng.random((N, T)) < 0.5) & d if truncated else None
    logp = -rng.uniform(0.05, 3.0, (N, T)).astype(np.float32)
    blogp = (logp - rng.uniform(-3.0, 3.0, (N, T))).astype(np.float32)
    t64, a64, rho64 = vtrace.vtrace_f64(logp, blogp, r, d, v, vb, 0.99, lam, 1.0, 1.0, truncated=tr)
    rho, c = vtrace.clipped_weights(logp, blogp, 1.0, 1.0, np.float32)
    assert rho.dtype == np.float32 and (rho == 1.0).any() and (rho < 1.0).any()
    assert np.abs(rho - rho64).max() <= EPS  # (one rounding of exp, one of the store, of values <= 1)
    t32, a32 = vtrace.vtrace_f32(rho, c, r, d, v, vb, 0.99, lam, truncated=tr)
    bound = 5 * T * EPS * magnitude(r, v, vb, t64)
    print('lambda', lam, 'max |f32 - f64|', float(np.abs(t32 - t64).max()), float(np.abs(a32 - a64).max()), 'bound',
          bound)
    assert np.abs(t32 - t64).max() <= bound
    assert np.abs(a32 - a64).max() <= bound


def test_on_policy_lambda_one_advantage_is_target_minus_value():
    """adv_t = (r + gamma vs_{t+1}) - V_t and target_t - V_t = (r + gamma V_{t+1} - V_t) + gamma (vs_{t+1} -
    V_{t+1}) are one number in exact arithmetic; in float32 they share acc_{t+1} and differ by the roundings
    of one step (at most 8, of quantities up to B)."""
    N, T = 33, 20
    _, r, d, v, vb = batch(N, T, 4)
    one = np.ones((N, T), np.float32)
    tgt, adv = vtrace.vtrace_f32(one, one, r, d, v, vb, 0.99, 1.0)
    diff = np.abs(adv.astype(np.float64) - (tgt.astype(np.float64) - v))
    bound = 4 * EPS * magnitude(r, v, vb, tgt)
    print('max |adv - (target - V)|', float(diff.max()), 'bound', bound)
    assert diff.max() <= bound
    # (the identity holds for any rho = c; with c below rho the trace is damped and the advantage is not)
    tgt2, adv2 = vtrace.vtrace_f32(one, 0.5 * one, r, d, v, vb, 0.99, 1.0)
    assert np.abs(adv2 - (tgt2 - v)).max() > 1e-2


def test_edge_rules_of_the_weights():
    inf = np.float32(np.inf)
    #                +inf: the bars   -inf: 0      NaN: 0       0: 1 (below the bars)   large finite: the bars
    logp = np.array([-1.0, -inf, -inf, -2.0, -0.5], np.float32)
    blogp = np.array([-inf, -1.0, -inf, -2.0, -80.0], np.float32)
    for dtype in (np.float32, np.float64):
        rho, c = vtrace.clipped_weights(logp, blogp, 2.0, 1.5, dtype)
        assert rho.dtype == dtype
        assert rho.tolist() == [2.0, 0.0, 0.0, 1.0, 2.0]
        assert c.tolist() == [1.5, 0.0, 0.0, 1.0, 1.5]
    # c = min(c_bar, rho): what lets the kernel carry rho alone
    rng = np.random.default_rng(5)
    lp = -rng.uniform(0, 3, 1000).astype(np.float32)
    bl = (lp - rng.uniform(-3, 3, 1000)).astype(np.float32)
    rho, c = vtrace.clipped_weights(lp, bl, 1.5, 0.8, np.float32)
    assert np.array_equal(c, np.minimum(np.float32(0.8), rho))
    for bad in ((1.0, 1.5), (0.0, 0.0), (1.0, 0.0), (-1.0, -2.0)):
        with pytest.raises(ValueError):
            vtrace.clipped_weights(lp, bl, *bad)


def test_a_zero_weight_row_contributes_nothing():
    """rho = c = 0 at (n, t): its target is V, its advantage 0, and nothing behind it reaches the steps before
    it -- they see vs_t = V_t, as if the trace had been cut there."""
    N, T, t0 = 2, 6, 3
    _, r, d, v, vb = batch(N, T, 6, p_term=0.0)
    d[:] = False
    w = np.ones((N, T), np.float32)
    w[0, t0] = 0.0
    tgt, adv = vtrace.vtrace_f32(w, w, r, d, v, vb, 0.99, 0.95)
    assert tgt[0, t0] == v[0, t0] and adv[0, t0] == 0.0
    r2, v2, vb2 = r.copy(), v.copy(), vb.copy()
    r2[0, t0:], v2[0, t0 + 1:], vb2[0] = 7.0, -3.0, 11.0  # (everything behind the row, and its own reward)
    tgt2, adv2 = vtrace.vtrace_f32(w, w, r2, d, v2, vb2, 0.99, 0.95)
    assert np.array_equal(bits(tgt2[0, :t0 + 1]), bits(tgt[0, :t0 + 1]))
    assert np.array_equal(bits(adv2[0, :t0 + 1]), bits(adv[0, :t0 + 1]))
    assert np.array_equal(bits(tgt2[1]), bits(tgt[1]))


def test_truncation_keeps_the_bootstrap_and_cuts_the_chain():
    r = np.array([[1.0, 2.0, 3.0]], np.float32)
    v = np.array([[0.5, 0.25, 0.125]], np.float32)
    vb = np.array([4.0], np.float32)
    d = np.array([[False, True, True]])
    tr = np.array([[False, True, True]])
    one = np.ones((1, 3), np.float32)
    g = 0.5  # (exact products)
    tgt, adv = vtrace.vtrace_f32(one, one, r, d, v, vb, g, 1.0, truncated=tr)
    # t = 2: truncated at T-1, boots from v_boot; t = 1: truncated mid-row, boots from V_2, not from vs_2
    assert tgt[0, 2] == 3.0 + g * 4.0 and adv[0, 2] == 3.0 + g * 4.0 - 0.125
    assert tgt[0, 1] == 2.0 + g * 0.125 and adv[0, 1] == 2.0 + g * 0.125 - 0.25
    assert tgt[0, 0] == 1.0 + g * tgt[0, 1]
    cut, _ = vtrace.vtrace_f32(one, one, r, d, v, vb, g, 1.0)
    assert cut[0, 2] == 3.0 and cut[0, 1] == 2.0


def test_entry_point_is_declared_bound_and_exported(lib):
    src = open(os.path.join(ROOT, 'include', 'acmi.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+acmi_vtrace\s*\(([^)]*)\)\s*;', src)
    assert m, 'acmi_vtrace is not declared in include/acmi.h'
    params = [p.strip() for p in m.group(1).split(',')]
    res, args = _lib._SIGS['acmi_vtrace']
    assert 'acmi_vtrace' in _lib.EXPORTED and hasattr(lib, 'acmi_vtrace')
    assert res is _lib.c_int and len(args) == len(params) == 23
    for p, a in zip(params, args):  # pointers and the stream are void*, float is float, int is int
        want = _lib.c_vp if ('*' in p or 'acmi_stream_t' in p) else _lib.c_float if p.startswith('float') else \
            _lib.c_int
        assert a is want, p
    assert lib.acmi_abi_version() == 4


def test_objective_contracts():
    from actorcritic.kfac_utils import KfacOptimizer
    from actorcritic.objectives import A2CObjective, VTraceObjective, VTraceOptimizeOp
    from actorcritic.nn import OptimizeOp, RMSPropOptimizer
    for bad in (dict(rho_bar=0.5, c_bar=1.0), dict(rho_bar=0.0, c_bar=0.0), dict(c_bar=0.0), dict(c_bar=-1.0),
                dict(rho_bar=-1.0, c_bar=-2.0), dict(gae_lambda=1.5), dict(gae_lambda=None)):
        with pytest.raises(ValueError):
            VTraceObjective(object(), **bad)
    obj = VTraceObjective(object(), 0.99, 0.01, gae_lambda=0.95, rho_bar=1.5, c_bar=1.0)
    assert isinstance(obj, A2CObjective)
    for name in ('policy_loss', 'baseline_loss', 'mean_entropy', 'target_values', 'advantage', 'importance_weights'):
        assert getattr(obj, name) is not None
    kfac = KfacOptimizer.__new__(KfacOptimizer)  # (no engine behind it: only its type matters)
    with pytest.raises(NotImplementedError, match='first-order'):
        obj.optimize_shared(kfac, num_epochs=2)
    with pytest.raises(NotImplementedError, match='first-order'):
        obj.optimize_shared(kfac, num_minibatches=2)
    for bad in (dict(num_epochs=0), dict(num_minibatches=0)):
        with pytest.raises(ValueError):
            obj.optimize_shared(RMSPropOptimizer(7e-4), **bad)
    # one pass is the inherited op, for any optimizer; more is the V-trace op
    assert type(obj.optimize_shared(RMSPropOptimizer(7e-4))) is OptimizeOp
    op = obj.optimize_shared(RMSPropOptimizer(7e-4), 0.25, num_epochs=2, num_minibatches=2, shuffle_seed=3)
    assert isinstance(op, VTraceOptimizeOp) and (op.num_epochs, op.num_minibatches, op.shuffle_seed) == (2, 2, 3)
    assert op.last_order is None and obj._vcoef == 0.25


def test_model_has_the_behaviour_placeholder_and_the_example_imports():
    from actorcritic.model import ActorCriticModel
    from actorcritic import spaces
    import actorcritic.examples.atari.vtrace as ex

    class M(ActorCriticModel):
        pass

    m = M(spaces.Box(0, 255, (84, 84, 4), np.uint8), spaces.Discrete(4))
    ph = m.behaviour_log_probs_placeholder
    assert ph.name == 'behaviour_log_probs' and np.dtype(ph.dtype) == np.float32 and ph.shape == (None, None)
    assert callable(ex.train_vtrace)
    assert ex.parse_vtrace_flags(['--game', 'catch', '--epochs', '2', '--minibatches', '4', '--rho-bar', '1.5',
                                  '--c-bar', '0.5', '--lambda', '0.9']) == dict(
        num_epochs=2, num_minibatches=4, rho_bar=1.5, c_bar=0.5, gae_lambda=0.9)
    assert ex.parse_vtrace_flags(['--game', 'catch']) == {}
