"""What tests/rl_kernel_cases.py claims, proved on the CPU (no GPU, no libacmi): every
named branch is taken by the case named for it, and the plain float32 numpy restatement
of each formula stays within a quarter of every bound against float64 (a bound whose
whole path is fewer than 10 roundings cannot leave that room and is held to the
restatement itself, see _limit) -- the bounds come from counted roundings and are
validated here, against the reference, never against a kernel.  The two mutations that the old optimizer test let through (the
gradient term of RMSProp's ms dropped, a step scaled by 1 +- 0.001) break the bounds
in every case family that can show them.
"""
import os
import sys

import numpy as np
import pytest

import rl_kernel_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
import oracle  # noqa: E402

QUARTER = 0.25
# rl_kernel_cases.K / LONG_PATH: an output reached by fewer than 10 roundings is held
# to the restatement itself (ratio <= 1: the derivation is valid), every longer path to
# the quarter.  Measured worst ratios of the short paths: momentum acc 0.61 (k = 3),
# momentum p 0.49 (5), Adam m 0.38 (5), RMSProp ms 0.32 (7), Adam v 0.28 (7), GAE 0.31 (6
# a step); of the long ones: RMSProp mom 0.23, p 0.22, Adam p 0.18, the norm 0.05.


def _limit(k):
    return QUARTER if k >= rc.LONG_PATH else 1.0


# the three largest sizes run half of their cases here (every clipping family and
# profile, p = 0 and random alternating): the float64 references of a 1.7 M element
# size take seconds
HOST_SIZES = rc.OPT_SIZES[:5]
BIG_SIZES = rc.OPT_SIZES[5:]


def _opt_cases(sizes):
    for n in sizes:
        for clip, prof, pz in rc.opt_case_ids():
            yield rc.opt_case(n, clip, prof, pz)


def _opt_refs(c):
    return (('momentum', rc.momentum_ref(c, **rc.MOMENTUM_HP), rc.momentum_f32(c, **rc.MOMENTUM_HP)),
            ('rmsprop', rc.rmsprop_ref(c, **rc.RMSPROP_HP), rc.rmsprop_f32(c, **rc.RMSPROP_HP)),
            ('adam', rc.adam_ref(c, **rc.ADAM_HP), rc.adam_f32(c, **rc.ADAM_HP)))


# ---------------------------------------------------------------------------
# optimizers
# ---------------------------------------------------------------------------
def test_optimizer_sizes_sit_on_both_sides_of_every_wrap():
    s = rc.OPT_SIZES
    assert s[0] == 1 and s[1] < 64 < 256 < s[2]
    assert s[3] < rc.RED_THREADS < s[4] < rc.APPLY_THREADS < s[5]
    assert s[6] == rc.PARAM_COUNT > rc.APPLY_THREADS
    assert rc.norm_roundings(s[3]) + 1 == rc.norm_roundings(s[4])  # the second trip adds one
    assert rc.norm_roundings(s[6]) == 21 + 13


@pytest.mark.parametrize('n', rc.OPT_SIZES)
def test_clipping_families_take_their_branches(n):
    for clip_mode in rc.CLIP_MODES:
        for prof in range(len(rc.OPT_PROFILES)):
            c = rc.opt_case(n, clip_mode, prof, False)
            sc, gn = rc.clip_ref(c['g'].astype(np.float64), c['clip'])
            if clip_mode == 'off':
                assert c['clip'] == 0 and sc == 1.0
            elif clip_mode == 'inactive':  # gn < clip, and 1 / clip exact
                assert 0.05 < gn / c['clip'] < 0.2 and sc == 1.0
                assert np.float32(c['clip']) * (np.float32(1) / np.float32(c['clip'])) == 1
            elif clip_mode == 'active':  # gn > clip
                assert gn / c['clip'] == pytest.approx(rc.ACTIVE_RATIO, rel=1e-6) and sc == pytest.approx(1 / 600, rel=1e-6)
            else:  # gn = 0 with clipping on
                assert gn == 0 and not c['g'].any() and c['clip'] == 0.5 and sc == 1.0
            assert c['clip'] == rc.f32(c['clip'])
            if c['state'] == 'init':
                assert not c['m'].any() and not c['v'].any() and c['t'] == 1
                assert (c['ms'] == 1).all() and not c['mom'].any() and not c['acc'].any()
            else:
                assert c['mom'].any() and c['acc'].any()
    profs = rc.OPT_PROFILES
    assert {(p[0], p[1]) for p in profs} == {(s, g) for s in ('init', 'warm') for g in (1.0, 1e-4)}
    assert {p[2] for p in profs} == {True, False} and {p[3] for p in profs} == {0.0, 0.9}
    assert {p[4] for p in profs} == {1e-10, 1e-5}
    assert any(p[0] == 'warm' and p[3] == 0.9 for p in profs)  # momentum meets a non-zero mom


@pytest.mark.parametrize('n', rc.OPT_SIZES[4:])
def test_norm_bound_catches_a_lost_second_trip(n):
    """The sum of squares without the elements past the reduction's first trip leaves
    the norm's bound at every size above RED_THREADS, one element past it included."""
    for clip_mode in rc.CLIP_MODES[:3]:
        for prof in range(len(rc.OPT_PROFILES)):
            c = rc.opt_case(n, clip_mode, prof, False)
            ref = rc.momentum_ref(c, **rc.MOMENTUM_HP)['norm']
            lost = np.sqrt((c['g'][:rc.RED_THREADS].astype(np.float64) ** 2).sum())
            assert rc.worst_ratio(lost, ref) > 10.0


def test_inexact_clip_factor_is_one_ulp_below_one():
    c = np.float32(rc.inexact_clip(37.0))
    assert 37.0 <= c < 37.1 and c * (np.float32(1) / c) == np.float32(1) - np.float32(2.0 ** -24)


def _check_quarter(cases, worst):
    for c in cases:
        for name, ref, f32 in _opt_refs(c):
            for out, rb in ref.items():
                ratio = rc.worst_ratio(f32[out], rb)
                key = (name, out)
                worst[key] = max(worst.get(key, 0.0), ratio)
                limit = _limit(rc.norm_roundings(c['n']) if out == 'norm' else rc.K[key])
                assert ratio <= limit, (name, out, c['n'], c['clip_mode'], c['state'], c['gscale'], c['p_zero'], ratio)


def test_optimizer_float32_restatement_within_a_quarter_of_the_bounds():
    worst = {}
    _check_quarter(_opt_cases(HOST_SIZES), worst)
    print('worst restatement / bound:', {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize('n', BIG_SIZES)
def test_optimizer_float32_restatement_within_a_quarter_at_the_large_sizes(n):
    worst = {}
    ids = rc.opt_case_ids()
    # every clipping family and profile once, p = 0 and random alternating
    picked = [ids[i] for i in range(0, len(ids), 2)][::1]
    picked = [(clip, prof, (i % 2) == 1) for i, (clip, prof, _) in enumerate(picked)]
    _check_quarter((rc.opt_case(n, *k) for k in picked), worst)
    print('worst restatement / bound:', {k: round(v, 3) for k, v in worst.items()})


def _detectable(c):
    """Can float32 hold RMSProp's gradient term next to decay ms at all?  From ms = 1 at
    gradients of 1e-4 the term (1e-9) is far below an ulp of 0.9."""
    x = rc.rmsprop_terms(c, **rc.RMSPROP_HP)
    return bool((x['t2'] > 4 * 7 * rc.U * (x['t1'] + x['t2'])).any())


def test_bounds_catch_a_dropped_gradient_term_and_a_scaled_step():
    """CPU arithmetic on the reference alone.  ms without (1 - decay) g^2 sc^2 leaves the
    ms bound in every family whose gradient term float32 can hold (every warm state --
    whose scale is the gradient's -- and ms = 1 at gradients of order 1); an RMSProp,
    momentum or Adam step times 1 +- 0.001 leaves the p bound, from p = 0, in every family
    with a non-zero step."""
    seen_ms = set()
    for c in _opt_cases((257, rc.OPT_SIZES[4])):
        fam = (c['clip_mode'], c['state'], c['gscale'])
        true = rc.rmsprop_ref(c, **rc.RMSPROP_HP)
        if c['clip_mode'] != 'zero_grad' and _detectable(c):
            mut = rc.rmsprop_ref(c, drop_gradient_term=True, **rc.RMSPROP_HP)
            assert rc.worst_ratio(mut['ms'][0], true['ms']) > 1.0, fam
            seen_ms.add(fam)
        for f in (0.999, 1.001):
            refs = [(true, rc.rmsprop_ref(c, step_factor=f, **rc.RMSPROP_HP))]
            ad = rc.adam_ref(c, **rc.ADAM_HP)
            refs.append((ad, rc.adam_ref(c, step_factor=f, **rc.ADAM_HP)))
            mo = rc.momentum_ref(c, **rc.MOMENTUM_HP)
            p64 = c['p'].astype(np.float64)
            refs.append((mo, dict(p=(p64 - f * (p64 - mo['p'][0]), None))))
            for k, (t, m) in enumerate(refs):
                step = c['p'].astype(np.float64) - t['p'][0]
                if not step.any():  # a zero gradient from a zero state moves nothing
                    assert c['clip_mode'] == 'zero_grad'
                    continue
                if not c['p_zero']:  # beside a random p only a large step shows: what p = 0 is for
                    continue
                assert rc.worst_ratio(m['p'][0], t['p']) > 1.0, (k, f, fam, c['p_zero'])
    warm = {(clip, 'warm', g) for clip in rc.CLIP_MODES[:3] for g in (1.0, 1e-4)}
    init1 = {(clip, 'init', 1.0) for clip in rc.CLIP_MODES[:3]}
    assert seen_ms >= warm | init1, (warm | init1) - seen_ms


def test_old_rmsprop_ms_check_could_not_see_the_gradient_term():
    """The inputs of test_first_order_optimizers_match_oracle: the true ms is within
    4.8e-6 of 0.9, inside the old rtol = 1e-5; the comparison that replaces it (ms -
    decay ms_old against (1 - decay) g^2 sc^2) is not met by 0."""
    rng = np.random.default_rng(6)
    n = 100003
    rng.standard_normal(n)
    g = rng.standard_normal(n).astype(np.float32).astype(np.float64)
    _, rms, _ = oracle.rmsprop_apply(np.zeros(n), np.ones(n), np.zeros(n), g, 7e-4, 0.5)
    assert np.abs(rms - 0.9).max() < 5e-6 < 1e-5 * 0.9
    term = rms - 0.9
    assert not np.allclose(np.zeros(n), term, rtol=1e-4, atol=2 * rc.U)


# ---------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------
def test_loss_sizes_reach_the_final_kernels_second_trip():
    nb = [rc.loss_blocks(M) for M in rc.LOSS_SIZES]
    assert nb == [1, 1, 2, 64, 65, 80]  # 65 and 80 > 64 partials: lanes 0 and 0..15 add twice
    assert [rc.tree_roundings(M) for M in rc.LOSS_SIZES] == [16, 16, 16, 16, 17, 17]
    assert all(rc.loss_blocks(M) > 64 for M in rc.PPO_SIZES)


@pytest.mark.parametrize('M', rc.LOSS_SIZES)
def test_a2c_scalars_float32_restatement_within_a_quarter(M):
    d = rc.loss_case(M)
    for adv, gs in ((d['adv'], 1.0), (d['adv_sep'], 0.25)):
        ref = oracle.a2c_loss_and_head_grads(d['logits'], d['values'], d['actions'], d['targets'], beta=rc.BETA,
                                             vcoef=rc.VCOEF, adv=adv)
        want = [gs * ref[k] for k in ('policy_loss', 'baseline_loss', 'mean_entropy')]
        got = rc.a2c_scalars_f32(d, adv, gs)
        for g, w, b in zip(got, want, rc.a2c_scalar_bounds(d, adv, gs)):
            assert abs(float(g) - w) <= QUARTER * b, (M, gs, float(g), w, b)


@pytest.mark.parametrize('vclip', [0.0, 0.2])
@pytest.mark.parametrize('M', rc.PPO_SIZES)
def test_ppo_scalars_float32_restatement_within_a_quarter(M, vclip):
    from test_gpu_ppo import EPS32, VCLIP32, make_inputs, ppo_ref
    vclip = VCLIP32 if vclip else 0.0
    d = make_inputs(M, rc.LOSS_A, EPS32, VCLIP32, seed=21)
    ref = ppo_ref(d['logits'], d['values'], d['actions'], d['old_logp'], d['old_values'], d['targets'], d['adv'],
                  EPS32, vclip, beta=rc.BETA, vcoef=rc.VCOEF)
    want = [ref[k] for k in ('policy_loss', 'baseline_loss', 'mean_entropy', 'approx_kl', 'clip_frac')]
    # the case module's own terms are the reference's
    terms, _ = rc.ppo_row_terms(d, EPS32, vclip)
    assert np.mean(terms[0]) == pytest.approx(-(ref['policy_loss'] + rc.BETA * ref['mean_entropy']), rel=1e-12)
    assert np.mean(terms[2]) == pytest.approx(ref['baseline_loss'], rel=1e-12)
    assert np.mean(terms[4]) == ref['clip_frac']
    for g, w, b in zip(rc.ppo_scalars_f32(d, EPS32, vclip), want, rc.ppo_scalar_bounds(d, EPS32, vclip)):
        assert abs(float(g) - w) <= QUARTER * b, (M, float(g), w, b)


# ---------------------------------------------------------------------------
# advantages
# ---------------------------------------------------------------------------
def test_adv_sizes_sit_on_both_sides_of_the_wraps():
    s = rc.ADV_SIZES
    assert s[:3] == (1, 2, 255) and s[3] < rc.MOM_THREADS < s[4] < rc.NORMALIZE_THREADS < s[5]


@pytest.mark.parametrize('M', rc.ADV_SIZES)
def test_constant_batch_has_variance_exactly_zero(M):
    """M x is exact in double for a float32 x and M < 2^29, and x^2 is exact (48 bits),
    so S / M = x, every difference is 0 and the output exactly 0.0 -- whatever Q gives,
    since var only scales."""
    for k, x in enumerate(rc.CONSTANT_VALUES):
        a = rc.adv_case(M, 'constant', k)
        assert (a == np.float32(x)).all() and x != 0
        s = float(M) * float(x)
        assert s / M == float(x)
        # the sum in any order is exact too: every partial sum is a multiple of x below 2^53 ulps
        assert a.astype(np.float64).sum() == s
        out = rc.adv_onepass_f64(a)
        assert not out.any() and not np.isnan(out).any()
        assert not rc.adv_bound(a)[1].any()


@pytest.mark.parametrize('M', rc.ADV_SIZES[2:])
@pytest.mark.parametrize('family', ['normal', 'offset'])
def test_onepass_double_within_a_quarter_of_the_double_bound(M, family):
    a = rc.adv_case(M, family)
    b_double, b = rc.adv_bound(a)
    ref = oracle.normalize_advantages(a, rc.ADV_EPS)
    err = np.abs(rc.adv_onepass_f64(a) - ref)
    assert (err <= QUARTER * b_double).all(), (err / b_double).max()
    # float32 of the one-pass result: the rounding of the output is the rest of the bound
    assert (np.abs(rc.adv_onepass_f64(a).astype(np.float32) - ref) <= b).all()
    w = a.astype(np.float64)
    if family == 'offset':
        assert 0.9e4 < w.mean() / w.std() < 1.1e4
        # the one-pass loss: 2e8 times a double rounding, a few float32 ulps -- and far
        # below the order-free (mean/std)^2 M 2^-52
        big = np.abs(ref) > 0.1
        assert (b_double[big] > 1e6 * 2.0 ** -53 * np.abs(ref[big])).all()
        assert (b_double[big] < 16 * rc.U * np.abs(ref[big])).all()
        assert (b_double[big] < 1e8 * min(M, 100) * 2.0 ** -52 * np.abs(ref[big])).all()


def test_half_batch_with_whole_moments():
    M = 255
    a = rc.adv_case(2 * M, 'normal')
    w = a.astype(np.float64)
    mom = (w[:M].sum() + w[M:].sum(), (w[:M] ** 2).sum() + (w[M:] ** 2).sum())
    ref = oracle.normalize_advantages(a, rc.ADV_EPS)[:M]
    b_double, b = rc.adv_bound(a, a[:M], ranks=2)
    assert (np.abs(rc.adv_onepass_f64(a[:M], mom, 2.0 * M) - ref) <= QUARTER * b_double).all()
    # count = M in its place is far outside
    assert (np.abs(rc.adv_onepass_f64(a[:M], mom, float(M)) - ref) > b).any()


# ---------------------------------------------------------------------------
# sampler
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('scale', rc.SAMPLER_SCALES)
@pytest.mark.parametrize('A', rc.SAMPLER_A)
def test_sampler_inputs_leave_at_most_one_percent_near_a_boundary(A, scale):
    z, u = rc.sampler_case(A, scale)
    assert tuple(u[:4]) == tuple(np.float32(x) for x in rc.FIXED_UNIFORMS) and u.max() <= np.float32(rc.U_MAX)
    y64, near, p = rc.inverse_cdf_f64(z, u)
    assert near.mean() <= 0.01, near.mean()
    y32 = rc.sample_f32_rows(z, u)
    assert (y32[~near] == y64[~near]).all()
    assert (p[np.arange(len(y32)), y32] > 0).all()
    if A > 1:
        assert y64[0] == int(np.argmax(p[0] > 0)) and y32[0] == y64[0]  # u = 0 draws the first action with mass
    k = 256
    np.testing.assert_array_equal(y32[:k], oracle.sample_f32(z[:k], u[:k]))  # the vectorised restatement


def test_sampler_edge_batches_are_the_head_of_the_large_case():
    for B in rc.SAMPLER_EDGE_B:
        z, u = rc.sampler_case(18, 2.0, B)
        assert z.shape == (B, 18) and u[0] == 0
    assert [(-(-B // 256)) for B in rc.SAMPLER_EDGE_B] == [1, 1, 1, 2]


@pytest.mark.parametrize('A', [2, 32, 64])
def test_tie_case_sits_exactly_on_the_boundaries(A):
    z, u, want = rc.tie_case(A)
    assert ((u.astype(np.float64) * A) == np.arange(A)).all()
    np.testing.assert_array_equal(rc.sample_f32_rows(z, u), want)
    np.testing.assert_array_equal(oracle.sample_f32(z, u), want)
    # `target <= c` in place of `target < c` would draw k - 1 on every row but the first
    # the rows within delta of a boundary (here: on it), which the float64 comparison skips
    assert rc.inverse_cdf_f64(z, u)[1][1:].all()


def test_calibration_row_and_seeds():
    p = np.exp(oracle.log_softmax(np.asarray(rc.CALIBRATION_ROW, np.float64)))
    B = rc.SAMPLER_B
    assert (p * B >= 50).all() and p.max() / p.min() > 10
    z = np.tile(np.asarray(rc.CALIBRATION_ROW, np.float32), (B, 1))
    y = rc.sample_f32_rows(z, oracle.sample_uniforms(*rc.CALIBRATION_SEEDS, B))
    counts = np.bincount(y, minlength=6)
    assert ((counts - p * B) ** 2 / (p * B)).sum() < 25.0


def test_mode_case_has_exact_ties():
    for A in (2, 33):
        z = rc.mode_case(A)
        ties = (z == z.max(1, keepdims=True)).sum(1) > 1
        assert ties[0] and ties[1] and ties.sum() > 20
        assert z.argmax(1)[0] == 0 and z.argmax(1)[1] == 0


# ---------------------------------------------------------------------------
# GAE
# ---------------------------------------------------------------------------
def test_gae_cases_cover_every_value():
    cs = rc.GAE_CASES
    assert {c[0] for c in cs} == {1, 63, 64, 65, 130} and {c[1] for c in cs} == {1, 2, 20}
    assert {c[2] for c in cs} == {0.0, 0.99, 1.0} and {c[3] for c in cs} == {0.0, 0.95, 1.0}
    assert {c[0] for c in cs if c[1] == 20} >= {63, 64, 65, 130}
    assert any(c[4] == 'big_v' and c[3] == 1.0 for c in cs)


@pytest.mark.parametrize('case', rc.GAE_CASES, ids=lambda c: '%d-%d-%g-%g-%s' % c)
def test_gae_float32_restatement_within_a_quarter(case):
    N, T, gamma, lam, family = case
    r, te, v, vb = rc.gae_case(N, T, family)
    tg, adv, b_tg, b_adv = rc.gae_ref(r, te, v, vb, gamma, lam)
    t32, a32 = oracle.gae_f32(r, te, v, vb, gamma, lam)
    assert rc.worst_ratio(a32, (adv, b_adv)) <= _limit(rc.K['gae', 'step'])
    assert rc.worst_ratio(t32, (tg, b_tg)) <= _limit(rc.K['gae', 'step'])
    if family == 'big_v':  # r + gamma V' - V cancels on the live rows: A is far smaller than its terms
        assert np.abs(v).min() > 900 and (np.abs(adv) < 0.5 * np.abs(v)).mean() > 0.5
    if lam == 1.0:  # the n-step targets, in exact arithmetic
        ret64 = oracle.targets_f64(r, te, vb, rc.f32(gamma))
        assert np.abs(tg - ret64).max() <= 1e-12 * max(1.0, np.abs(tg).max())
        b_ret = rc.returns_bound(r, te, vb, gamma)
        assert rc.worst_ratio(oracle.targets_f32(r, te, vb, gamma), (ret64, b_ret)) <= _limit(T + 5)
