"""The float64 K-FAC oracle pinned on the CPU (oracle.ema_update,
oracle.damped_inverses, oracle.kfac_step): the GPU tests of the optimizer kernels
(test_gpu_kfac_opt.py) lean on these three functions, so their algebra is checked
here on small dense float64 cases -- hand-made 3 to 6 dimensional factors where the
function takes any size, the A = 4, C3 = 32 parameter layout where it walks it."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
import oracle  # noqa: E402

A, C3 = 4, 32


def _spd(rng, n, shift=0.1):
    x = rng.standard_normal((n + 3, n))
    return x.T @ x / x.shape[0] + shift * np.eye(n)


def _small_factors(seed=0):
    """Stand-ins for the five A and six G factors (fc_policy / fc_baseline share A_4)."""
    rng = np.random.default_rng(seed)
    Af = [_spd(rng, n, 0.0) for n in (3, 4, 5, 6, 4)]
    Gf = [_spd(rng, n, 0.0) for n in (3, 5, 4, 6, 2, 1)]
    return Af, Gf


def test_ema_constant_statistics_debias_to_themselves():
    """Zero-initialised EMA of a constant S: biased_t = (1 - decay^t) S, so the
    zero-debias returns S at every t."""
    S = np.random.default_rng(1).standard_normal(97)
    biased = np.zeros_like(S)
    for t in range(1, 6):
        biased, debiased = oracle.ema_update(biased, S, 0.99, t)
        np.testing.assert_allclose(biased, (1 - 0.99 ** t) * S, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(debiased, S, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize('conv_normalize', [False, True])
def test_damped_inverses_invert_the_pi_damped_factors(conv_normalize):
    Af, Gf = _small_factors()
    damping = 0.01
    inv = oracle.damped_inverses(Af, Gf, damping, conv_normalize=conv_normalize)
    assert len(inv) == 6
    for l in range(6):
        A_, G_ = Af[min(l, 4)], Gf[l]
        lam = damping / (oracle.CONV_LOCATIONS[l] if conv_normalize else 1)
        pi = np.sqrt((np.trace(A_) / A_.shape[0]) / (np.trace(G_) / G_.shape[0]))
        Ai, Gi = inv[l]
        ra = (A_ + pi * np.sqrt(lam) * np.eye(A_.shape[0])) @ Ai - np.eye(A_.shape[0])
        rg = (G_ + np.sqrt(lam) / pi * np.eye(G_.shape[0])) @ Gi - np.eye(G_.shape[0])
        assert np.abs(ra).max() <= 1e-9 and np.abs(rg).max() <= 1e-9, (l, np.abs(ra).max(), np.abs(rg).max())
        # the two damping terms, recovered from the inverses alone, multiply to lambda_l
        da = np.linalg.inv(Ai) - A_
        dg = np.linalg.inv(Gi) - G_
        assert np.abs(da - np.diag(np.diag(da))).max() <= 1e-9 and np.abs(dg - np.diag(np.diag(dg))).max() <= 1e-9
        assert np.ptp(np.diag(da)) <= 1e-9 and np.ptp(np.diag(dg)) <= 1e-9
        prod = np.diag(da).mean() * np.diag(dg).mean()
        assert prod == pytest.approx(lam, rel=1e-8), (l, prod, lam)
    if conv_normalize:
        plain = oracle.damped_inverses(Af, Gf, damping)
        for l in range(3):  # the conv layers are damped less ...
            assert np.abs(inv[l][0] - plain[l][0]).max() > 1e-3 * np.abs(plain[l][0]).max()
        for l in range(3, 6):  # ... the dense layers (one location) exactly the same
            assert np.array_equal(inv[l][0], plain[l][0]) and np.array_equal(inv[l][1], plain[l][1])


def test_damped_inverses_zero_g_factor_takes_pi_one():
    Af, Gf = _small_factors(3)
    Gf[4] = np.zeros_like(Gf[4])
    damping = 0.01
    inv = oracle.damped_inverses(Af, Gf, damping)
    Ai, Gi = inv[4]
    n = Af[4].shape[0]
    np.testing.assert_allclose(Gi, np.eye(Gf[4].shape[0]) / np.sqrt(damping), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(Ai, np.linalg.inv(Af[4] + np.sqrt(damping) * np.eye(n)), rtol=1e-10, atol=1e-12)
    assert np.isfinite(Ai).all() and np.isfinite(Gi).all()
    # the layer sharing A_4 with its own (non-zero) G keeps its pi
    ref = oracle.damped_inverses(*_small_factors(3), damping)
    assert np.array_equal(inv[5][0], ref[5][0]) and np.array_equal(inv[5][1], ref[5][1])


@pytest.fixture(scope='module')
def step_case():
    """Damped factors A_d, G_d (SPD) of the real A = 4, C3 = 32 layout, their
    inverses, gradients, a non-zero velocity, parameters and the base step."""
    rng = np.random.default_rng(7)
    din, dout = oracle.kfac_dims(A, C3)
    _, n = oracle.param_offsets(A, C3)
    damped, inverses = [], []
    for l in range(6):
        Ad, Gd = _spd(rng, din[l], 0.5), _spd(rng, dout[l], 0.5)
        damped.append((Ad, Gd))
        inverses.append((np.linalg.inv(Ad), np.linalg.inv(Gd)))
    grads = rng.standard_normal(n) * 1e-2
    vel = rng.standard_normal(n) * 1e-3
    params = rng.standard_normal(n)
    lr, c = 0.25, 1e-4
    _, _, precon, _ = oracle.kfac_step(params, vel, grads, inverses, lr, 0.9, c, A, C3)
    sq0 = float(grads @ precon) * lr * lr
    assert sq0 > 0
    return dict(damped=damped, inverses=inverses, grads=grads, vel=vel, params=params, lr=lr, c=c, precon=precon,
                sq0=sq0, n=n)


def _block_bounds():
    off, n = oracle.param_offsets(A, C3)
    din, dout = oracle.kfac_dims(A, C3)
    return [(off[2 * l], off[2 * l] + din[l] * dout[l], din[l], dout[l]) for l in range(6)]


def test_kfac_step_blocks_solve_the_damped_system(step_case):
    s = step_case
    covered = 0
    for l, (lo, hi, di, do) in enumerate(_block_bounds()):
        X = s['precon'][lo:hi].reshape(di, do)
        g = s['grads'][lo:hi].reshape(di, do)
        Ad, Gd = s['damped'][l]
        res = np.linalg.norm(Ad @ X @ Gd - g) / np.linalg.norm(g)
        assert res <= 1e-9, (l, res)
        covered += hi - lo
    assert covered == s['n']  # the six [W; b] blocks tile the parameter vector


def test_kfac_step_coefficient_regimes(step_case):
    s = step_case
    lr, c = s['lr'], s['c']
    run = lambda g, inv, nc: oracle.kfac_step(s['params'], s['vel'], g, inv, lr, 0.9, nc, A, C3)
    # sq 100x above c: clipped to sqrt(c / sq) = 0.1
    k = np.sqrt(100.0 * c / s['sq0'])
    _, _, precon, coeff = run(k * s['grads'], s['inverses'], c)
    sq = float((k * s['grads']) @ precon) * lr * lr
    assert sq == pytest.approx(100.0 * c, rel=1e-9)
    assert coeff == pytest.approx(np.sqrt(c / sq), rel=1e-12) and coeff == pytest.approx(0.1, rel=1e-9)
    # sq 100x below c: not clipped
    k = np.sqrt(0.01 * c / s['sq0'])
    assert run(k * s['grads'], s['inverses'], c)[3] == 1.0
    # no trust region
    assert run(s['grads'], s['inverses'], float('inf'))[3] == 1.0
    # sq <= 0: one factor of every layer negated (g . precon < 0), and zero gradients
    neg = [(-Ai, Gi) for Ai, Gi in s['inverses']]
    new_p, _, precon, coeff = run(s['grads'], neg, c)
    assert float(s['grads'] @ precon) < 0 and coeff == 1.0 and np.isfinite(new_p).all()
    assert run(np.zeros_like(s['grads']), s['inverses'], c)[3] == 1.0


def test_kfac_step_momentum_and_parameter_update(step_case):
    s = step_case
    lr, c, mom = s['lr'], s['c'], 0.9
    new_p, v, precon, coeff = oracle.kfac_step(s['params'], s['vel'], s['grads'], s['inverses'], lr, mom, c, A, C3)
    assert 0 < coeff < 1
    np.testing.assert_allclose(v, mom * s['vel'] + coeff * precon, rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(new_p, s['params'] - lr * v, rtol=1e-12, atol=1e-18)
    # the velocity enters as momentum * v, and only there
    new_p0, v0, precon0, coeff0 = oracle.kfac_step(s['params'], np.zeros(s['n']), s['grads'], s['inverses'], lr, mom,
                                                   c, A, C3)
    assert coeff0 == coeff and np.array_equal(precon0, precon)
    np.testing.assert_allclose(v - v0, mom * s['vel'], rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(new_p0 - new_p, lr * mom * s['vel'], rtol=1e-6, atol=1e-12)
    assert np.abs(v - v0).max() > 0
