"""Cases, float64 references and error bounds of the rl.hip kernel tests
(test_gpu_rl_kernels.py on the GPU, test_rl_kernel_cases_host.py without one): the
first-order optimizers with global-norm clipping, the loss kernels' final reduction, the
advantage moments and normalisation, the categorical sampler and GAE.

Plain numpy on the CPU: no GPU, no libacmi.  Every case is a pure function of its
arguments (seeds are stated where something is drawn).

Bounds.  u = 2^-24 is the unit roundoff of float32: one rounding moves a value x by at
most u |x|.  An output that is a sum of terms, reached from the kernel's inputs by k
float32 roundings, is bounded by

    k u sum|terms|  +  the propagated error of an input that another kernel produced

(the clip factor, whose relative error e_sc comes from the norm reduction's shape).
k counts every rounding of the uncontracted form; the compiler may fuse a * b + c
(-ffp-contract=on), which only removes roundings.  The references take the scalar
arguments at the float32 values the C ABI receives (f32()).  No bound is fitted to a
kernel: test_rl_kernel_cases_host.py holds the plain float32 numpy restatement of each
formula (*_f32 below) to a quarter of every bound whose path is LONG_PATH roundings or
more, which leaves a kernel a factor of four for another legitimate operation order, and
to the bound itself on the shorter paths (K below).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
import oracle  # noqa: E402

U = 2.0 ** -24
F = np.float32

# k of each output whose path has a fixed length (the counts are derived where they are
# used).  A path shorter than LONG_PATH roundings cannot leave the restatement a factor
# of four: one rounding alone reaches u |x|, and the restatement makes most of the k
# counted ones.  The host test holds those bounds to the restatement itself (valid, not
# roomy) and every longer path to the quarter.
K = {('momentum', 'acc'): 3, ('momentum', 'p'): 5, ('rmsprop', 'ms'): 7, ('rmsprop', 'mom'): 14,
     ('rmsprop', 'p'): 15, ('adam', 'm'): 5, ('adam', 'v'): 7, ('adam', 'step'): 11, ('adam', 'p'): 12,
     ('gae', 'step'): 6}
LONG_PATH = 10


def f32(x):
    """The float32 value of a scalar argument, as a Python float."""
    return float(np.float32(x))


# ---------------------------------------------------------------------------
# 1. first-order optimizers
# ---------------------------------------------------------------------------
RED_THREADS = 512 * 256     # dot_partial_kernel's grid: its loop wraps above this
APPLY_THREADS = 2048 * 256  # the apply kernels' largest grid
PARAM_COUNT = oracle.param_offsets(18, 64)[1]  # acmi_param_count(18, 64)
OPT_SIZES = (1, 63, 257, RED_THREADS - 1, RED_THREADS + 1, APPLY_THREADS + 257, PARAM_COUNT)
CLIP_MODES = ('off', 'inactive', 'active', 'zero_grad')
# (state, gradient scale, norm_out given, RMSProp momentum, RMSProp eps): every pair
# (state, scale) once; the non-zero momentum meets a non-zero mom in profile 1
OPT_PROFILES = (('init', 1.0, True, 0.0, 1e-10), ('warm', 1e-4, False, 0.9, 1e-5),
                ('init', 1e-4, True, 0.9, 1e-5), ('warm', 1.0, False, 0.0, 1e-10))
ACTIVE_RATIO, INACTIVE_RATIO = 600.0, 0.1  # gn / clip_norm of the two clipping families

MOMENTUM_HP = dict(lr=f32(3e-4), mom=f32(0.9))
RMSPROP_HP = dict(lr=f32(7e-4), decay=f32(0.9))
ADAM_HP = dict(lr=f32(2.5e-4), beta1=f32(0.9), beta2=f32(0.999), eps=f32(1e-5))


def opt_case_ids():
    return [(clip, prof, pz) for clip in CLIP_MODES for prof in range(len(OPT_PROFILES)) for pz in (False, True)]


_base_cache = {}


def _opt_base(n):
    """The draws of size n (default_rng(7000 + n % 1009)): gradient, parameters and three
    state vectors, all float32; the last size asked for is kept.  The first element of
    the norm reduction's second trip is a 3-sigma gradient, so that a sum which loses
    that trip shows at RED_THREADS + 1 whatever the draw."""
    if n not in _base_cache:
        _base_cache.clear()
        rng = np.random.default_rng(7000 + n % 1009)
        _base_cache[n] = dict(g=rng.standard_normal(n, dtype=F), p=rng.standard_normal(n, dtype=F),
                              s1=rng.standard_normal(n, dtype=F), s2=rng.standard_normal(n, dtype=F),
                              su=rng.random(n, dtype=F))
        if n > RED_THREADS:
            _base_cache[n]['g'][RED_THREADS] = 3.0
    return _base_cache[n]


def opt_case(n, clip_mode, profile, p_zero):
    """One optimizer case: gradient g, parameters p, clip_norm, the states of the three
    optimizers (acc; ms, mom; m, v and Adam's step t) and the RMSProp settings.

    clip_norm: 0 (off); the power of two nearest gn / INACTIVE_RATIO (inactive: training's
    0.5 is a power of two as well, and clip * (1 / clip) is then exactly 1);
    gn / ACTIVE_RATIO (active); 0.5 at an all-zero gradient.
    warm states have the scale of the clipped gradient: acc, m ~ g sc, ms, v ~ (g sc)^2,
    mom ~ lr (RMSProp's step is lr g / sqrt(ms) ~ lr)."""
    state, gscale, norm_given, momentum, eps = OPT_PROFILES[profile]
    b = _opt_base(n)
    g = np.zeros(n, F) if clip_mode == 'zero_grad' else (F(gscale) * b['g']).astype(F)
    gn = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
    clip = {'off': 0.0, 'zero_grad': 0.5}.get(clip_mode)
    if clip_mode == 'inactive':
        clip = 2.0 ** round(np.log2(gn / INACTIVE_RATIO))
    elif clip_mode == 'active':
        clip = f32(gn / ACTIVE_RATIO)
    sc = clip_ref(g.astype(np.float64), clip)[0]
    c = dict(n=n, clip_mode=clip_mode, state=state, gscale=gscale, norm_given=norm_given, momentum=f32(momentum),
             eps=f32(eps), p_zero=p_zero, g=g, clip=clip, p=np.zeros(n, F) if p_zero else b['p'].copy())
    if state == 'init':
        c.update(acc=np.zeros(n, F), ms=np.ones(n, F), mom=np.zeros(n, F), m=np.zeros(n, F), v=np.zeros(n, F), t=1)
    else:
        ge = F(gscale * sc)
        c.update(acc=(ge * b['s1']).astype(F), ms=(ge * ge * (F(0.1) + b['su'])).astype(F),
                 mom=(F(RMSPROP_HP['lr']) * b['s2']).astype(F), m=(F(0.3) * ge * b['s1']).astype(F),
                 v=(ge * ge * (F(0.1) + b['su'])).astype(F), t=10)
    return c


def adam_lr_t(lr, beta1, beta2, t):
    """TF1 Adam's step size, computed by the host in double and passed as a float."""
    return f32(lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t))


def norm_roundings(n):
    """float32 roundings on the path of the sum of squares: the product; per thread
    ceil(n / RED_THREADS) sequential adds; 6 butterfly steps and 3 wave adds; in
    clip_scale_kernel 2 sequential adds (512 partials over 256 threads), 6 butterfly
    steps and 3 wave adds."""
    return 1 + -(-n // RED_THREADS) + 6 + 3 + 2 + 6 + 3


def norm_rel_bound(n):
    """All terms are squares, so K roundings move the sum by at most K u of itself; the
    square root halves that and rounds once."""
    return (norm_roundings(n) / 2.0 + 1.0) * U


def clip_ref(g64, clip):
    """(clip factor, global norm) in float64; clip is the float32 value of clip_norm."""
    gn = float(np.sqrt((g64 * g64).sum()))
    if clip <= 0:
        return 1.0, gn
    return clip * min(1.0 / gn if gn > 0 else np.inf, 1.0 / clip), gn


def clip_rel_bound(n, gn, clip):
    """e_sc: clip * (1 / max(gn, clip)) is a division and a product; the clipping branch
    also carries the norm's error."""
    if clip <= 0:
        return 0.0
    return 2 * U + (norm_rel_bound(n) if gn > clip else 0.0)


def inexact_clip(lo):
    """The first float32 c >= lo whose clip * (1 / clip) is not 1 in float32 (one ulp
    below): the inactive branch's factor as TF's clip_by_global_norm computes it."""
    c = F(lo)
    while F(c * (F(1) / c)) == F(1):
        c = np.nextafter(c, F(np.inf))
    return float(c)


def _absum(*terms):
    return sum(np.abs(t) for t in terms)


def momentum_ref(c, lr, mom):
    """{output: (float64 reference, bound)} of acmi_momentum_apply.
    acc' = mom acc + g sc: roundings g sc, mom acc, the add (3).
    p'   = p - lr acc': those and lr acc', the subtraction (5)."""
    g, acc, p = (c[k].astype(np.float64) for k in ('g', 'acc', 'p'))
    sc, gn = clip_ref(g, c['clip'])
    esc = clip_rel_bound(c['n'], gn, c['clip'])
    t1, t2 = mom * acc, g * sc
    a = t1 + t2
    return dict(acc=(a, K['momentum', 'acc'] * U * _absum(t1, t2) + esc * np.abs(t2)),
                p=(p - lr * a, K['momentum', 'p'] * U * _absum(p, lr * t1, lr * t2) + esc * np.abs(lr * t2)),
                norm=(gn, norm_rel_bound(c['n']) * gn))


def momentum_f32(c, lr, mom):
    g, sc, gn = _clip_f32(c)
    a = F(mom) * c['acc'] + g * sc
    return dict(acc=a, p=c['p'] - F(lr) * a, norm=gn)


def _clip_f32(c):
    g = c['g']
    gn = np.sqrt(np.sum(g * g, dtype=F))
    sc = F(1)
    if c['clip'] > 0:
        with np.errstate(divide='ignore'):
            sc = F(c['clip']) * min(F(1) / gn, F(1) / F(c['clip']))
    return g, F(sc), F(gn)


def rmsprop_terms(c, lr, decay):
    """float64 pieces of the RMSProp update: gi = g sc, the two terms of ms', d = ms' +
    eps, q = lr gi / sqrt(d), tm = momentum mom."""
    g, ms, mom = (c[k].astype(np.float64) for k in ('g', 'ms', 'mom'))
    sc, gn = clip_ref(g, c['clip'])
    gi = g * sc
    t1, t2 = decay * ms, (1.0 - decay) * gi * gi
    d = t1 + t2 + c['eps']
    return dict(gn=gn, sc=sc, gi=gi, t1=t1, t2=t2, d=d, q=lr * gi / np.sqrt(d), tm=c['momentum'] * mom)


def rmsprop_ref(c, lr, decay, drop_gradient_term=False, step_factor=1.0):
    """{output: (float64 reference, bound)} of acmi_rmsprop_apply.
    ms'  = decay ms + (1 - decay) gi gi: gi enters twice (2), 1 - decay, two products,
           decay ms, the add: k = 7; the clip factor enters squared: 2 e_sc.
    mom' = momentum mom + lr gi / sqrtf(ms' + eps): the 7 of ms', gi, lr gi, + eps,
           momentum mom, the add, plus 2 for sqrtf and the division: k = 14; e_sc once
           through gi and at most once more through the root of ms'.
    p'   = p - mom': one more (15).
    drop_gradient_term / step_factor state the two mutations the host test holds the
    bounds against (a reference that is wrong in that way); the bounds are always those
    of the true reference."""
    x = rmsprop_terms(c, lr, decay)
    esc = clip_rel_bound(c['n'], x['gn'], c['clip'])
    p = c['p'].astype(np.float64)
    t1, t2, q, tm = x['t1'], x['t2'], x['q'], x['tm']
    ms_new = t1 + (0.0 if drop_gradient_term else t2)
    if drop_gradient_term:
        q = lr * x['gi'] / np.sqrt(ms_new + c['eps'])
    mo = (tm + q) * step_factor
    return dict(ms=(ms_new, K['rmsprop', 'ms'] * U * _absum(t1, t2) + 2 * esc * np.abs(t2)),
                mom=(mo, K['rmsprop', 'mom'] * U * _absum(tm, x['q']) + 2 * esc * np.abs(x['q'])),
                p=(p - mo, K['rmsprop', 'p'] * U * _absum(p, tm, x['q']) + 2 * esc * np.abs(x['q'])),
                norm=(x['gn'], norm_rel_bound(c['n']) * x['gn']))


def rmsprop_f32(c, lr, decay):
    g, sc, gn = _clip_f32(c)
    gi = g * sc
    m2 = F(decay) * c['ms'] + (F(1) - F(decay)) * gi * gi
    mo = F(c['momentum']) * c['mom'] + F(lr) * gi / np.sqrt(m2 + F(c['eps']))
    return dict(ms=m2, mom=mo, p=c['p'] - mo, norm=gn)


def adam_ref(c, lr, beta1, beta2, eps, step_factor=1.0):
    """{output: (float64 reference, bound)} of acmi_adam_apply at step c['t'].
    m' = beta1 m + (1 - beta1) gi: gi, 1 - beta1, the product, beta1 m, the add: k = 5.
    v' = beta2 v + (1 - beta2) gi gi: as RMSProp's ms', k = 7 and 2 e_sc.
    step = lr_t m' / (sqrtf(v') + eps): m's error enters through lr_t / den; on top, the 7
           of v', sqrtf, + eps, lr_t m', the division: 11, and e_sc through the root of v'.
    p' = p - step: one more rounding, on p and the step."""
    g, m, v, p = (c[k].astype(np.float64) for k in ('g', 'm', 'v', 'p'))
    sc, gn = clip_ref(g, c['clip'])
    esc = clip_rel_bound(c['n'], gn, c['clip'])
    lr_t = adam_lr_t(lr, beta1, beta2, c['t'])
    gi = g * sc
    t1, t2 = beta1 * m, (1.0 - beta1) * gi
    v1, v2 = beta2 * v, (1.0 - beta2) * gi * gi
    m_new, v_new = t1 + t2, v1 + v2
    den = np.sqrt(v_new) + eps
    step = lr_t * m_new / den
    b_m = K['adam', 'm'] * U * _absum(t1, t2) + esc * np.abs(t2)
    b_step = lr_t / den * b_m + np.abs(step) * (K['adam', 'step'] * U + esc)
    return dict(m=(m_new, b_m), v=(v_new, K['adam', 'v'] * U * _absum(v1, v2) + 2 * esc * np.abs(v2)),
                p=(p - step * step_factor, b_step + K['adam', 'p'] * U * _absum(p, step)),
                norm=(gn, norm_rel_bound(c['n']) * gn))


def adam_f32(c, lr, beta1, beta2, eps):
    g, sc, gn = _clip_f32(c)
    gi = g * sc
    lr_t = F(adam_lr_t(lr, beta1, beta2, c['t']))
    mi = F(beta1) * c['m'] + (F(1) - F(beta1)) * gi
    vi = F(beta2) * c['v'] + (F(1) - F(beta2)) * gi * gi
    return dict(m=mi, v=vi, p=c['p'] - lr_t * mi / (np.sqrt(vi) + F(eps)), norm=gn)


def worst_ratio(got, ref_and_bound):
    """max |got - ref| / bound over the elements (0 where both are 0; inf where an error
    meets a zero bound or the value is not finite)."""
    ref, bound = ref_and_bound
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isfinite(got), r, np.inf)
    return float(np.max(r)) if r.size else 0.0


# ---------------------------------------------------------------------------
# 2. loss reduction
# ---------------------------------------------------------------------------
LOSS_BLOCK = 256
LOSS_A, LOSS_LDH = 4, 8
LOSS_SIZES = (1, 255, 257, 16384, 16385, 20480)
PPO_SIZES = (16385, 20480)
BETA, VCOEF = f32(0.01), f32(0.5)


def loss_blocks(M):
    return -(-M // LOSS_BLOCK)


def loss_case(M, seed=40):
    """Inputs of acmi_a2c_loss at A = LOSS_A (default_rng(seed + M % 97)); adv_sep is an
    advantage that is not targets - values."""
    rng = np.random.default_rng(seed + M % 97)
    d = dict(logits=rng.standard_normal((M, LOSS_A)).astype(F), values=rng.standard_normal(M).astype(F),
             actions=rng.integers(0, LOSS_A, M).astype(np.int32), targets=rng.standard_normal(M).astype(F),
             adv_sep=rng.standard_normal(M).astype(F))
    d['adv'] = (d['targets'] - d['values']).astype(F)
    return d


def tree_roundings(M):
    """float32 adds on the path of a loss sum: 6 butterfly steps, 3 wave adds,
    ceil(nb / 64) sequential adds in loss_final_kernel, 6 more butterfly steps."""
    return 6 + 3 + -(-loss_blocks(M) // 64) + 6


def logp_bound(z64, A):
    """Per row: a bound on the float32 error of log pi(a) = z[a] - (mx + logf(se)) for
    every a, from float64 values.  se sums A expf (<= 2 u each, their arguments z - mx
    exact or one rounding u |z - mx|, A - 1 adds): relative (A + 2 + max|z - mx|) u, which
    is its logarithm's absolute error; logf: 2 u |log se|; the add: u |lse|; the
    subtraction: u |log pi|."""
    mx = z64.max(-1, keepdims=True)
    se = np.exp(z64 - mx).sum(-1, keepdims=True)
    lse = mx + np.log(se)
    spread = np.abs(z64 - mx).max(-1, keepdims=True)
    return U * (A + 2 + spread + 2 * np.abs(np.log(se)) + np.abs(lse) + np.abs(z64 - lse))


def row_terms_a2c(d, adv):
    """float64 per-row terms of A2C's three sums (policy, entropy, value) and a bound on
    each term's own float32 error."""
    z = d['logits'].astype(np.float64)
    M, A = z.shape
    lp = oracle.log_softmax(z)
    p = np.exp(lp)
    b_lp = logp_bound(z, A)
    rows = np.arange(M)
    ad = np.asarray(adv, np.float64)
    lpa = lp[rows, d['actions']]
    H = -(p * lp).sum(-1)
    # expf(lp) lp: expf moves by (b_lp + 2u) p, lp by b_lp, the product and the add round
    b_H = (p * (np.abs(lp) * (b_lp + 2 * U) + b_lp) + (1 + A) * U * np.abs(p * lp)).sum(-1)
    diff = d['targets'].astype(np.float64) - d['values'].astype(np.float64)
    terms = [ad * lpa, H, 0.5 * diff * diff]
    bounds = [np.abs(ad) * b_lp[rows, d['actions']] + U * np.abs(ad * lpa), b_H, 3 * U * diff * diff]
    return terms, bounds


def sum_bound(term, term_bound, M):
    """Bound of a mean of M terms summed in float32 over the fixed tree: the tree's adds
    and the division by M on the sum of absolute values, plus the terms' own errors."""
    return ((tree_roundings(M) + 1) * U * np.abs(term).sum() + term_bound.sum()) / M


def a2c_scalar_bounds(d, adv, grad_scale=1.0):
    """Bounds of out[0..2] = scale (-(mean pl + beta mean H)), scale mean vl, scale mean H
    (the combination rounds 4 more times)."""
    M = d['logits'].shape[0]
    (t0, t1, t2), (b0, b1, b2) = row_terms_a2c(d, adv)
    s0, s1, s2 = (sum_bound(t, b, M) for t, b in ((t0, b0), (t1, b1), (t2, b2)))
    m0, m1, m2 = (np.abs(t).sum() / M for t in (t0, t1, t2))
    return (grad_scale * (s0 + BETA * s1 + 4 * U * (m0 + BETA * m1)), grad_scale * (s2 + 2 * U * m2),
            grad_scale * (s1 + 2 * U * m1))


def a2c_scalars_f32(d, adv, grad_scale=1.0):
    """Plain float32 restatement of out[0..2] (numpy's own summation order)."""
    z = d['logits']
    M = z.shape[0]
    mx = z.max(-1, keepdims=True)
    lse = mx + np.log(np.exp(z - mx).sum(-1, keepdims=True, dtype=F))
    lp = z - lse
    H = -(np.exp(lp) * lp).sum(-1, dtype=F)
    lpa = lp[np.arange(M), d['actions']]
    diff = d['targets'] - d['values']
    s = [np.sum(np.asarray(adv, F) * lpa, dtype=F), np.sum(H, dtype=F), np.sum(F(0.5) * diff * diff, dtype=F)]
    mh = s[1] / F(M)
    return (F(grad_scale) * -(s[0] / F(M) + F(BETA) * mh), F(grad_scale) * (s[2] / F(M)), F(grad_scale) * mh)


def ppo_row_terms(d, eps, vclip):
    """float64 per-row terms of PPO's five sums (surrogate, entropy, value, old_logp -
    logp, clipped) and bounds on the terms' own errors; no row may sit on a branch
    boundary (test_gpu_ppo.make_inputs keeps them 1e-3 away)."""
    z = d['logits'].astype(np.float64)
    M, A = z.shape
    rows = np.arange(M)
    (_, H, _), (_, b_H, _) = row_terms_a2c(d, d['adv'])
    b_lpa = logp_bound(z, A)[rows, d['actions']]
    lpa = oracle.log_softmax(z)[rows, d['actions']]
    olp, ad = d['old_logp'].astype(np.float64), d['adv'].astype(np.float64)
    v, tg = d['values'].astype(np.float64), d['targets'].astype(np.float64)
    r = np.exp(lpa - olp)
    s = np.minimum(r * ad, np.clip(r, 1.0 - eps, 1.0 + eps) * ad)
    e = (v - tg) ** 2
    if vclip > 0:
        vo = d['old_values'].astype(np.float64)
        e = np.maximum(e, (vo + np.clip(v - vo, -vclip, vclip) - tg) ** 2)
    kl = olp - lpa
    terms = [s, H, 0.5 * e, kl, (np.abs(r - 1.0) > eps).astype(np.float64)]
    # r: the subtraction rounds, expf 2 u, its argument's error b_lpa; the clamp and the
    # product round; the clipped square goes through 3 more adds than the plain one
    bounds = [np.abs(s) * (b_lpa + U * np.abs(kl) + 4 * U), b_H, 6 * U * e, b_lpa + U * np.abs(kl), np.zeros(M)]
    return terms, bounds


def ppo_scalar_bounds(d, eps, vclip):
    """Bounds of out[0..3] and clip_frac_out."""
    M = d['logits'].shape[0]
    terms, bounds = ppo_row_terms(d, eps, vclip)
    s = [sum_bound(t, b, M) for t, b in zip(terms, bounds)]
    m = [np.abs(t).sum() / M for t in terms]
    return (s[0] + BETA * s[1] + 4 * U * (m[0] + BETA * m[1]), s[2] + 2 * U * m[2], s[1] + 2 * U * m[1],
            s[3] + 2 * U * m[3], s[4] + 2 * U * m[4])


def ppo_scalars_f32(d, eps, vclip):
    """Plain float32 restatement of out[0..3] and clip_frac_out (numpy's summation)."""
    z = d['logits']
    M = z.shape[0]
    mx = z.max(-1, keepdims=True)
    lp = z - (mx + np.log(np.exp(z - mx).sum(-1, keepdims=True, dtype=F)))
    H = -(np.exp(lp) * lp).sum(-1, dtype=F)
    lpa = lp[np.arange(M), d['actions']]
    r = np.exp(lpa - d['old_logp'])
    s = np.minimum(r * d['adv'], np.clip(r, F(1) - F(eps), F(1) + F(eps)) * d['adv'])
    diff = d['targets'] - d['values']
    e = F(0.5) * diff * diff
    if vclip > 0:
        dc = d['targets'] - (d['old_values'] + np.clip(d['values'] - d['old_values'], -F(vclip), F(vclip)))
        e = np.maximum(e, F(0.5) * dc * dc)
    sums = [np.sum(t, dtype=F) for t in (s, H, e, d['old_logp'] - lpa, (np.abs(r - F(1)) > F(eps)).astype(F))]
    mh = sums[1] / F(M)
    return (-(sums[0] / F(M) + F(BETA) * mh), sums[2] / F(M), mh, sums[3] / F(M), sums[4] / F(M))


# ---------------------------------------------------------------------------
# 3. advantage moments and normalisation
# ---------------------------------------------------------------------------
MOM_THREADS = 256 * 256      # adv_moments_partial_kernel's grid
NORMALIZE_THREADS = 1024 * 256
ADV_SIZES = (1, 2, 255, MOM_THREADS - 1, MOM_THREADS + 1, NORMALIZE_THREADS + 257)
ADV_FAMILIES = ('normal', 'offset', 'constant')
ADV_EPS = 1e-8
CONSTANT_VALUES = (f32(0.3), f32(-1234.5678), f32(1e-3))


def adv_case(M, family, k=0):
    """normal: 0.3 + 2.5 N(0,1); offset: 1000 + 0.1 N(0,1) (mean / std = 1e4); constant:
    CONSTANT_VALUES[k] repeated.  default_rng(50 + M % 101)."""
    rng = np.random.default_rng(50 + M % 101)
    if family == 'normal':
        return rng.normal(0.3, 2.5, M).astype(F)
    if family == 'offset':
        return (1000.0 + 0.1 * rng.standard_normal(M)).astype(F)
    if family == 'constant':
        return np.full(M, CONSTANT_VALUES[k], F)
    raise ValueError(family)


def adv_onepass_f64(a, moments=None, count=None, eps=ADV_EPS):
    """adv_normalize_kernel's arithmetic in numpy double, before the rounding of the
    output to float32: mean = S / count, var = max(Q / count - mean^2, 0)."""
    a = np.asarray(a, np.float64)
    s, q = (a.sum(), (a * a).sum()) if moments is None else moments
    count = float(a.size) if count is None else count
    mean = s / count
    var = max(q / count - mean * mean, 0.0)
    return (a - mean) * (1.0 / (np.sqrt(var) + eps))


def moment_roundings(M, ranks=1):
    """Double roundings on the path of a moment: the square (Q only), per thread
    ceil(M / MOM_THREADS) sequential adds, 6 butterfly steps and 3 wave adds, in the
    final kernel 4 sequential adds (256 partials over 64 lanes) and 6 butterfly steps;
    ranks - 1 adds where the moments of several ranks are summed."""
    return 1 + -(-M // MOM_THREADS) + 6 + 3 + 4 + 6 + (ranks - 1)


def adv_bound(whole, part=None, ranks=1, eps=ADV_EPS):
    """(double part, whole bound) of the normalised advantages of `part` (default: the
    whole batch) under the moments of `whole`, against
    oracle.normalize_advantages(whole).

    The double part.  With K = moment_roundings and d = 2^-53, S is within K d sum|a| and
    Q within K d Q of the exact sums.  Q / count - mean^2 subtracts two numbers of size
    mean^2 + var that carry those errors and 4 roundings of their own: var is off by at
    most (K + 4) d (2 mean^2 + var), relative (K + 4) d (2 (mean/std)^2 + 1), and the
    standard deviation by half of that: the loss of a one-pass variance, which at
    mean / std = 1e4 is 2e8 times the roundings' own size.  (Summed in an arbitrary
    order K would be M: the (mean/std)^2 M 2^-52 of the textbook bound; the kernel's
    tree keeps K at 21 to 25.)  The mean is off by K d mean|a| / std in units of the
    output.  The subtraction, 1 / (sqrt + eps) and the product: 4 d.  A zero variance (a
    constant batch) makes every difference exactly 0: no error at all.
    Then the output rounds to float32 once: u |out|."""
    w = np.asarray(whole, np.float64)
    a = w if part is None else np.asarray(part, np.float64)
    n, mean, std = w.size, w.mean(), w.std()
    out = (a - mean) / (std + eps)
    if std == 0.0:
        return np.zeros(a.shape), np.zeros(a.shape)
    d = 2.0 ** -53
    k = moment_roundings(-(-n // ranks), ranks)
    rel_std = 0.5 * (k + 4) * d * (2.0 * (mean / std) ** 2 + 1.0)
    b_double = np.abs(out) * (rel_std + 4 * d) + k * d * np.abs(w).mean() / (std + eps)
    return b_double, b_double + U * np.abs(out)


# ---------------------------------------------------------------------------
# 4. sampler
# ---------------------------------------------------------------------------
SAMPLER_A = (1, 2, 6, 18, 32, 33, 64)
SAMPLER_SCALES = (2.0, 30.0)
SAMPLER_B = 4096
SAMPLER_EDGE_B = (1, 255, 256, 257)
U_MAX = f32(1.0 - 2.0 ** -24)  # the largest value u01 returns
FIXED_UNIFORMS = (0.0, U_MAX, 0.5, 2.0 ** -24)
CALIBRATION_ROW = (0.0, 0.7, -1.2, 1.5, -2.0, 0.3)
CALIBRATION_SEEDS = (5, 1, 11)  # seed, stream id, counter


def sampler_case(A, scale, B=SAMPLER_B):
    """logits [B, A] = scale N(0,1) and uniforms [B] (default_rng(3 + A)); the first rows
    draw with FIXED_UNIFORMS."""
    rng = np.random.default_rng(3 + A)
    z = (rng.standard_normal((B, A)) * scale).astype(F)
    u = rng.random(B).astype(F)
    k = min(B, len(FIXED_UNIFORMS))
    u[:k] = FIXED_UNIFORMS[:k]
    return z, u


def pad_columns(z, ld, fill=np.nan):
    """[B, A] -> [B, ld] with the padding columns filled (NaN: a read past A shows)."""
    out = np.full((z.shape[0], ld), fill, F)
    out[:, :z.shape[1]] = z
    return out


def inverse_cdf_f64(z, u):
    """(draw, near, p): the float64 inverse CDF of softmax(z) at u -- the first a with
    u < F(a), the last action where rounding leaves none -- and the rows whose u lies
    within delta = 4 A 2^-24 of a cumulative boundary F(0..A-2), where float32 may
    legitimately draw the neighbour.  (F(A-1) = 1 is no boundary: every u reaches it.)"""
    z = np.asarray(z, np.float64)
    B, A = z.shape
    p = np.exp(oracle.log_softmax(z))
    cdf = np.cumsum(p, 1)
    u = np.asarray(u, np.float64)[:, None]
    y = np.minimum((cdf <= u).sum(1), A - 1)
    near = np.zeros(B, bool) if A == 1 else (np.abs(cdf[:, :A - 1] - u).min(1) < 4 * A * U)
    return y, near, p


def sample_f32_rows(z, u):
    """oracle.sample_f32 vectorised over the rows: the same float32 operations in the
    same order."""
    z = np.asarray(z, F)
    B, A = z.shape
    e = np.exp(z - z.max(1, keepdims=True)).astype(F)
    se = np.zeros(B, F)
    for a in range(A):
        se = se + e[:, a]
    target = np.asarray(u, F) * se
    c = np.zeros(B, F)
    y = np.full(B, A - 1, np.int64)
    done = np.zeros(B, bool)
    for a in range(A):
        c = c + e[:, a]
        hit = ~done & (target < c)
        y[hit] = a
        done |= hit
    return y


def tie_case(A):
    """All-zero logits with A a power of two and u = k / A: every u sits exactly on a
    boundary of the CDF, in float32 as in exact arithmetic (the partial sums 1..A and
    u A = k are exact), so the draw is k: F(k-1) = k / A <= u < F(k)."""
    assert A & (A - 1) == 0
    return np.zeros((A, A), F), (np.arange(A) / A).astype(F), np.arange(A)


def mode_case(A, B=300, seed=9):
    """Rows for mode = 1 with exact ties: small-integer logits (default_rng(seed + A)),
    row 0 all equal, row 1 its maximum at both ends."""
    rng = np.random.default_rng(seed + A)
    z = rng.integers(-2, 3, (B, A)).astype(F)
    z[0] = 1.0
    if B > 1:
        z[1] = -1.0
        z[1, 0] = z[1, A - 1] = 2.0
    return z


# ---------------------------------------------------------------------------
# 5. GAE
# ---------------------------------------------------------------------------
# (N, T, gamma, lambda, family): every value of each, the block edges at T = 20
GAE_CASES = ((1, 1, 0.99, 0.95, 'unit'), (63, 20, 0.99, 0.95, 'unit'), (64, 20, 0.99, 0.0, 'unit'),
             (65, 20, 0.99, 1.0, 'unit'), (130, 20, 0.99, 0.95, 'big_v'), (130, 2, 1.0, 1.0, 'unit'),
             (65, 20, 0.0, 0.95, 'unit'), (64, 1, 1.0, 0.0, 'big_v'), (63, 2, 0.0, 1.0, 'unit'),
             (130, 20, 1.0, 0.95, 'unit'), (130, 20, 0.99, 1.0, 'big_v'))


def gae_case(N, T, family, seed=11):
    """rewards in {-1, 0, 1}, 8 % terminals (rows 0..3 where they exist: a terminal at
    t = 0, at T - 1, all, none), values N(0,1) -- 'big_v': 1000 + N(0,1), where
    target = A + V cancels.  default_rng(seed + N + T)."""
    rng = np.random.default_rng(seed + N + T)
    r = rng.choice([-1.0, 0.0, 1.0], size=(N, T)).astype(F)
    te = rng.random((N, T)) < 0.08
    te[0, 0] = True
    if N > 1:
        te[1, T - 1] = True
    if N > 3:
        te[2, :] = True
        te[3, :] = False
    off = 1000.0 if family == 'big_v' else 0.0
    v = (off + rng.normal(0, 1, size=(N, T))).astype(F)
    vb = (off + rng.normal(0, 1, size=N)).astype(F)
    return r, te, v, vb


def gae_ref(r, te, v, vb, gamma, lam):
    """(targets, advantages, target bound, advantage bound) in float64 at the float32
    values of gamma and lambda.

    A_t = (r + gamma V' - V) + gl A_{t+1}: five roundings a step (gamma V', the add, the
    subtraction, gl A', the add) and gl = gamma lambda itself rounded once by the
    launcher: 6 u on the step's |r| + |gamma V'| + |V| + |gl A_{t+1}|, plus gl times the
    bound of A_{t+1}.  target = A + V rounds once more."""
    g, lm = f32(gamma), f32(lam)
    tg, adv = oracle.gae_f64(r, te, v, vb, g, lm)
    r64, v64 = r.astype(np.float64), v.astype(np.float64)
    N, T = r.shape
    b_adv = np.zeros((N, T))
    nxt_v, nxt_a, nxt_b = vb.astype(np.float64), np.zeros(N), np.zeros(N)
    for t in range(T - 1, -1, -1):
        live = (~te[:, t]).astype(np.float64)
        terms = np.abs(r64[:, t]) + np.abs(g * nxt_v) * live + np.abs(v64[:, t]) + np.abs(g * lm * nxt_a) * live
        b_adv[:, t] = K['gae', 'step'] * U * terms + g * lm * live * nxt_b
        nxt_v, nxt_a, nxt_b = v64[:, t], adv[:, t], b_adv[:, t]
    return tg, adv, b_adv + U * (np.abs(adv) + np.abs(v64)), b_adv


def returns_bound(r, te, vb, gamma):
    """Bound of acmi_returns' targets against oracle.targets_f64: a target sums L <= T
    products r_i gp[i - t] and the bootstrap bp[T - t] vb, in order: each term is
    rounded as a product and passes at most L adds, gp[k] is a float32 power (2 u) and
    bp[k] a k-fold float32 product (k u): (L + T + 4) u on the sum of the absolute
    terms."""
    g = f32(gamma)
    r64 = np.abs(r.astype(np.float64))
    N, T = r.shape
    out = np.zeros((N, T))
    run, cnt = np.abs(vb.astype(np.float64)), np.ones(N)
    for t in range(T - 1, -1, -1):
        run = np.where(te[:, t], 0.0, run)
        cnt = np.where(te[:, t], 0.0, cnt)
        run = r64[:, t] + g * run
        cnt = cnt + 1
        out[:, t] = (cnt + T + 4) * U * run
    return out
