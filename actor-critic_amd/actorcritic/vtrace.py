"""V-trace (Espeholt et al. 2018, IMPALA) in numpy: the rule book of acmi_vtrace.

V-trace is the actor-critic target for data that the policy being updated did not collect.  With the current
policy pi, the behaviour policy mu that acted and w_t = pi(a_t|s_t) / mu(a_t|s_t),

    rho_t = min(rho_bar, w_t),  c_t = min(c_bar, w_t)                    (rho_bar >= c_bar > 0)
    delta_t = rho_t (r_t + gamma V_{t+1} - V_t)
    vs_t - V_t = delta_t + gamma lambda c_t (vs_{t+1} - V_{t+1})         -> targets vs_t
    adv_t = rho_t (r_t + gamma vs_{t+1} - V_t)                           -> the policy gradient's advantage

On-policy (w = 1, bars >= 1) the targets are GAE(lambda)'s, and the n-step returns at lambda = 1.  Terminals and
time limits follow acmi_gae_trunc: ``live = !d_t`` carries the chain, ``boot = live or truncated_t`` keeps
gamma V_{t+1} in delta_t, and the advantage of a terminal step looks at 0 -- or, truncated, at V_{t+1}, the
value of the observation that the time limit cut off -- in place of vs_{t+1}.

Two statements, both normative for the kernel (csrc/rl.hip vtrace_kernel; tests/test_gpu_vtrace.py):

:func:`vtrace_f32`  phase 2 of the kernel -- the reverse scan -- in float32 with the kernel's operation order,
                    from given weights rho and c: bit for bit what the kernel writes.
:func:`vtrace_f64`  the whole definition in float64 from the two policies' log-probabilities.

:func:`clipped_weights` states phase 1's edge rules.
"""

import numpy as np


def clipped_weights(logp, behaviour_logp, rho_bar=1.0, c_bar=1.0, dtype=np.float64):
    """(rho, c) = (min(rho_bar, w), min(c_bar, w)), w = exp(logp - behaviour_logp), the difference formed in
    float32 as the kernel forms it and the rest in ``dtype``.  Edge rules: a difference of +inf gives the
    bars, -inf gives 0, a NaN (both log-probabilities -inf) gives rho = c = 0: the row contributes nothing."""
    _check_bars(rho_bar, c_bar)
    with np.errstate(invalid='ignore', over='ignore'):
        delta = (np.asarray(logp, np.float32) - np.asarray(behaviour_logp, np.float32)).astype(dtype)
        w = np.exp(delta)
    nan = np.isnan(w)
    rho = np.where(nan, 0, np.minimum(dtype(rho_bar), w)).astype(dtype)
    c = np.where(nan, 0, np.minimum(dtype(c_bar), w)).astype(dtype)
    return rho, c


def _check_bars(rho_bar, c_bar):
    if not float(c_bar) > 0.0 or not float(rho_bar) > 0.0:
        raise ValueError('rho_bar and c_bar must be positive, got {} and {}'.format(rho_bar, c_bar))
    if float(rho_bar) < float(c_bar):
        raise ValueError('rho_bar ({}) must not be below c_bar ({})'.format(rho_bar, c_bar))


def _scan(dtype, rho, c, rewards, terminals, truncated, values, v_boot, gamma, lam):
    """The reverse scan over t, every env at once; each statement is one rounded operation of ``dtype`` per
    element, in vtrace_kernel's order."""
    r = np.asarray(rewards, dtype)
    if r.ndim != 2:
        raise ValueError('rewards must be [env, step]')
    N, T = r.shape
    d = np.asarray(terminals, bool).reshape(N, T)
    tr = np.zeros((N, T), bool) if truncated is None else np.asarray(truncated, bool).reshape(N, T) & d
    v = np.asarray(values, dtype).reshape(N, T)
    rho = np.asarray(rho, dtype).reshape(N, T)
    c = np.asarray(c, dtype).reshape(N, T)
    vb = np.asarray(v_boot, dtype).reshape(N)
    if not 0.0 <= float(lam) <= 1.0:
        raise ValueError('lambda must be in [0, 1], got {}'.format(lam))
    g = dtype(gamma)
    gl = dtype(dtype(gamma) * dtype(lam))  # (as gae_launch forms it)
    zero = dtype(0)
    tgt = np.zeros((N, T), dtype)
    adv = np.zeros((N, T), dtype)
    next_v, next_vs, acc = vb.copy(), vb.copy(), np.zeros(N, dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        for t in range(T - 1, -1, -1):
            live = ~d[:, t]
            boot = live | tr[:, t]
            vi, ri, rh = v[:, t], r[:, t], rho[:, t]
            delta = rh * ((ri + np.where(boot, g * next_v, zero)) - vi)
            acc = delta + np.where(live, (gl * c[:, t]) * acc, zero)
            vs = acc + vi
            nextv = np.where(live, next_vs, np.where(tr[:, t], next_v, zero))
            adv[:, t] = rh * ((ri + g * nextv) - vi)
            tgt[:, t] = vs
            next_v, next_vs = vi, vs
    return tgt, adv


def vtrace_f32(rho, c, rewards, terminals, values, v_boot, gamma, lam, truncated=None):
    """float32 restatement of vtrace_kernel's scan: -> (targets, advantages), [N, T] float32, bit for bit the
    kernel's for the weights it used.  ``rho``, ``c``: the clipped weights [N, T] (the kernel's ``rho`` output
    and min(c_bar, rho)); ``truncated``: None or bool [N, T], read only where ``terminals`` is set.
    With rho = c = 1 the targets are oracle.gae_f32's bit for bit."""
    return _scan(np.float32, rho, c, rewards, terminals, truncated, values, v_boot, gamma, lam)


def vtrace_f64(logp, behaviour_logp, rewards, terminals, values, v_boot, gamma, lam, rho_bar=1.0, c_bar=1.0,
               truncated=None):
    """V-trace in float64 from the log-probabilities of the taken actions under the current and the behaviour
    policy: -> (targets, advantages, rho), [N, T] float64."""
    r = np.asarray(rewards, np.float64)
    rho, c = clipped_weights(np.asarray(logp).reshape(r.shape), np.asarray(behaviour_logp).reshape(r.shape),
                             rho_bar, c_bar, np.float64)
    tgt, adv = _scan(np.float64, rho, c, r, terminals, truncated, values, v_boot, gamma, lam)
    return tgt, adv, rho
