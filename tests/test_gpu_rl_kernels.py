"""The oldest kernels of csrc/rl.hip at their edges, through the C ABI: the first-order
optimizers with global-norm clipping, the loss kernels' final reduction, the advantage
moments and normalisation, the categorical sampler and GAE.

Cases, float64 references and bounds: tests/rl_kernel_cases.py (every bound is counted
roundings x 2^-24 x sum|terms| plus the propagated error of the clip factor, validated
on the CPU by test_rl_kernel_cases_host.py, never fitted to a kernel).  An assertion
here is `worst |got - float64| / bound <= 1` over every element of every output.

Before each call every output and workspace buffer is filled with NaN and every integer
output with a sentinel, so an element the kernel leaves unwritten, or a workspace word it
reads before writing, shows; the padding columns of ld > A logits hold NaN, so a read one
column too far flags the row.

Worst |got - float64| / bound measured on an MI355X over all cases, per kernel and
output (each test prints its own, "RATIO ..."):
  momentum   acc 0.33, p 0.36, norm 0.08      RMSProp  ms 0.32, mom 0.23, p 0.21
  Adam       m 0.37, v 0.28, p 0.17           A2C      out[0..2] 0.02, 0.03, 0.04
  PPO        out[0..3] 0.003, 0.04, 0.02, 0.03, clip fraction 0.02
  normalise  1.00 (normal: the float32 rounding of the output is the whole bound and is
             reached), 0.18 (mean / std = 1e4)
  GAE        advantages 0.31, targets 0.25, against acmi_returns at lambda = 1 0.11
The sampler, the constant batch, the padding columns and GAE against its float32
restatement are exact comparisons.
"""
import numpy as np
import pytest
import torch

from actorcritic import _lib
import rl_kernel_cases as rc
from rl_kernel_cases import oracle
from test_gpu_ppo import EPS32, VCLIP32, make_inputs, ppo_ref

pytestmark = pytest.mark.gpu

SENTINEL = -12345
NAN = float('nan')


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def nans(n, cuda, dtype=torch.float32):
    return torch.full((int(n),) if np.isscalar(n) else tuple(n), NAN, dtype=dtype, device=cuda)


def host(t):
    return t.cpu().numpy()


def check(tag, got, ref_and_bound):
    """The worst ratio of one output, printed; it must not pass 1."""
    ratio = rc.worst_ratio(got, ref_and_bound)
    assert ratio <= 1.0, '%s: |got - float64| is %.3g x its bound' % (tag, ratio)
    return ratio


# ---------------------------------------------------------------------------
# 1. first-order optimizers
# ---------------------------------------------------------------------------
def _run_optimizer(lib, cuda, name, c):
    n = c['n']
    ws = nans(lib.acmi_opt_ws_floats(n), cuda)
    norm = nans(1, cuda) if c['norm_given'] else None
    P, G = dev(c['p']), dev(c['g'])
    s = _lib.stream_handle()
    if name == 'momentum':
        ACC = dev(c['acc'])
        hp = rc.MOMENTUM_HP
        _lib.call('acmi_momentum_apply', _lib.ptr(P), _lib.ptr(ACC), _lib.ptr(G), n, hp['lr'], hp['mom'], c['clip'],
                  _lib.ptr(ws), _lib.ptr(norm), s)
        got, ref = dict(acc=ACC, p=P), rc.momentum_ref(c, **hp)
    elif name == 'rmsprop':
        MS, MOM = dev(c['ms']), dev(c['mom'])
        hp = rc.RMSPROP_HP
        _lib.call('acmi_rmsprop_apply', _lib.ptr(P), _lib.ptr(MS), _lib.ptr(MOM), _lib.ptr(G), n, hp['lr'],
                  hp['decay'], c['momentum'], c['eps'], c['clip'], _lib.ptr(ws), _lib.ptr(norm), s)
        got, ref = dict(ms=MS, mom=MOM, p=P), rc.rmsprop_ref(c, **hp)
    else:
        M_, V_ = dev(c['m']), dev(c['v'])
        hp = rc.ADAM_HP
        lr_t = rc.adam_lr_t(hp['lr'], hp['beta1'], hp['beta2'], c['t'])
        _lib.call('acmi_adam_apply', _lib.ptr(P), _lib.ptr(M_), _lib.ptr(V_), _lib.ptr(G), n, lr_t, hp['beta1'],
                  hp['beta2'], hp['eps'], c['clip'], _lib.ptr(ws), _lib.ptr(norm), s)
        got, ref = dict(m=M_, v=V_, p=P), rc.adam_ref(c, **hp)
    if norm is not None:
        got = dict(norm=norm, **got)  # (the outputs are checked in this order: causes first)
    got = {k: host(v) for k, v in got.items()}
    assert np.array_equal(host(G), c['g'])  # the gradient is an input
    return got, ref


@pytest.mark.parametrize('n', rc.OPT_SIZES)
@pytest.mark.parametrize('name', ['momentum', 'rmsprop', 'adam'])
def test_first_order_optimizer_matches_float64_elementwise(lib, cuda, name, n):
    """Every clipping family (off, gn < clip, gn > clip, g = 0) x every profile (state,
    gradient scale, norm_out given or NULL, RMSProp momentum and eps) x (random p, p = 0)
    at one size: all outputs element by element within their counted bounds."""
    if n == rc.PARAM_COUNT:
        assert int(lib.acmi_param_count(18, 64)) == n
    worst = {}
    for clip_mode, prof, p_zero in rc.opt_case_ids():
        c = rc.opt_case(n, clip_mode, prof, p_zero)
        got, ref = _run_optimizer(lib, cuda, name, c)
        assert set(got) == set(ref) - (set() if c['norm_given'] else {'norm'})
        for out, g in got.items():
            tag = '%s %s n=%d %s profile %d p_zero=%s' % (name, out, n, clip_mode, prof, p_zero)
            worst[out] = max(worst.get(out, 0.0), check(tag, g, ref[out]))
        if clip_mode == 'zero_grad' and c['norm_given']:
            assert got['norm'][0] == 0.0
    print('RATIO', name, n, {k: round(v, 3) for k, v in worst.items()})


def test_inactive_clip_factor_is_clip_times_its_reciprocal(lib, cuda):
    """gn < clip_norm: the factor is clip_norm * (1 / clip_norm) in float32 as in TF's
    clip_by_global_norm, one ulp below 1 for this clip_norm -- not 1.  From acc = 0 the
    momentum accumulator is the float32 product g * sc whatever the compiler contracts,
    so it is compared bit for bit."""
    n = 257
    c = rc.opt_case(n, 'off', 0, False)
    clip = np.float32(rc.inexact_clip(37.0))
    sc = clip * (np.float32(1) / clip)
    assert sc != 1 and float(np.sqrt((c['g'].astype(np.float64) ** 2).sum())) < 0.8 * clip
    P, ACC, G = dev(c['p']), dev(np.zeros(n, np.float32)), dev(c['g'])
    ws, norm = nans(lib.acmi_opt_ws_floats(n), cuda), nans(1, cuda)
    _lib.call('acmi_momentum_apply', _lib.ptr(P), _lib.ptr(ACC), _lib.ptr(G), n, rc.MOMENTUM_HP['lr'],
              rc.MOMENTUM_HP['mom'], float(clip), _lib.ptr(ws), _lib.ptr(norm), _lib.stream_handle())
    want = c['g'] * sc
    assert (want != c['g']).sum() > n // 4  # the ulp shows in the product
    np.testing.assert_array_equal(host(ACC), want)


# ---------------------------------------------------------------------------
# 2. loss reduction
# ---------------------------------------------------------------------------
def _head_tolerances(M, grad_scale):
    """test_gpu_parity's rtol 1e-4 / 1e-5 with its atol 1e-9 / 1e-10 at M = 1000 carried
    to this M: the columns scale with grad_scale / M."""
    return dict(rtol=1e-4, atol=1e-6 * grad_scale / M), dict(rtol=1e-5, atol=1e-7 * grad_scale / M)


def _run_a2c(lib, cuda, d, adv, grad_scale):
    M, A, ldh = d['logits'].shape[0], rc.LOSS_A, rc.LOSS_LDH
    ld = A + 3
    L = dev(rc.pad_columns(d['logits'], ld))
    V, AC, TG, AD = dev(d['values']), dev(d['actions']), dev(d['targets']), dev(adv)
    dhead, out = nans((M, ldh), cuda), nans(4, cuda)
    ws = nans(lib.acmi_a2c_loss_ws_floats(M), cuda)
    _lib.call('acmi_a2c_loss', _lib.ptr(L), ld, _lib.ptr(V), _lib.ptr(AC), _lib.ptr(TG), _lib.ptr(AD), M, A, rc.BETA,
              rc.VCOEF, grad_scale, _lib.ptr(dhead), ldh, _lib.ptr(ws), _lib.ptr(out), _lib.stream_handle())
    return host(dhead), host(out)


@pytest.mark.parametrize('M', rc.LOSS_SIZES)
def test_a2c_loss_sums_and_head_gradients_past_64_blocks(lib, cuda, M):
    """out[0..2] within the bound of a float32 sum over the fixed tree (on the sum of the
    absolute terms), every dhead column against float64, the padding exactly 0; at
    M = 20480 also grad_scale = 0.25 with an advantage that is not targets - values."""
    d = rc.loss_case(M)
    runs = [(d['adv'], 1.0)] + ([(d['adv_sep'], 0.25)] if M == 20480 else [])
    for adv, gs in runs:
        dh, out = _run_a2c(lib, cuda, d, adv, gs)
        ref = oracle.a2c_loss_and_head_grads(d['logits'], d['values'], d['actions'], d['targets'], beta=rc.BETA,
                                             vcoef=rc.VCOEF, adv=adv)
        want = [gs * ref[k] for k in ('policy_loss', 'baseline_loss', 'mean_entropy')]
        ratios = [check('a2c out[%d] M=%d scale=%g' % (k, M, gs), out[k], (w, b))
                  for k, (w, b) in enumerate(zip(want, rc.a2c_scalar_bounds(d, adv, gs)))]
        assert np.isnan(out[3])  # A2C writes three scalars
        A = rc.LOSS_A
        tl, tv = _head_tolerances(M, gs)
        np.testing.assert_allclose(dh[:, :A], gs * ref['dlogits'], **tl)
        np.testing.assert_allclose(dh[:, A], gs * ref['dvalue'], **tv)
        assert np.array_equal(dh[:, A + 1:], np.zeros((M, rc.LOSS_LDH - A - 1), np.float32))
        print('RATIO a2c', M, gs, [round(r, 3) for r in ratios])


@pytest.mark.parametrize('vclip', [0.0, VCLIP32], ids=['vclip-off', 'vclip-0.2'])
@pytest.mark.parametrize('M', rc.PPO_SIZES)
def test_ppo_loss_sums_past_64_blocks(lib, cuda, M, vclip):
    """test_gpu_ppo's float64 reference and inputs (no row within 1e-3 of a branch
    boundary) at more than 64 block partials: out[0..3], clip_frac_out, dhead."""
    A, ldh, ld = rc.LOSS_A, rc.LOSS_LDH, rc.LOSS_A + 3
    d = make_inputs(M, A, EPS32, VCLIP32, seed=21)
    ref = ppo_ref(d['logits'], d['values'], d['actions'], d['old_logp'], d['old_values'], d['targets'], d['adv'],
                  EPS32, vclip, beta=rc.BETA, vcoef=rc.VCOEF)
    t = {k: dev(d[k]) for k in ('values', 'actions', 'old_logp', 'old_values', 'targets', 'adv')}
    L = dev(rc.pad_columns(d['logits'], ld))
    dhead, out, cf = nans((M, ldh), cuda), nans(4, cuda), nans(1, cuda)
    ws = nans(lib.acmi_ppo_loss_ws_floats(M), cuda)
    _lib.call('acmi_ppo_loss', _lib.ptr(L), ld, _lib.ptr(t['values']), _lib.ptr(t['actions']), _lib.ptr(t['old_logp']),
              _lib.ptr(t['old_values']), _lib.ptr(t['targets']), _lib.ptr(t['adv']), M, A, EPS32, vclip, rc.BETA,
              rc.VCOEF, 1.0, _lib.ptr(dhead), ldh, _lib.ptr(ws), _lib.ptr(out), _lib.ptr(cf), _lib.stream_handle())
    got = list(host(out)) + [float(cf)]
    want = [ref[k] for k in ('policy_loss', 'baseline_loss', 'mean_entropy', 'approx_kl', 'clip_frac')]
    assert 0.2 < ref['clip_frac'] < 0.8
    ratios = [check('ppo scalar %d M=%d' % (k, M), got[k], (w, b))
              for k, (w, b) in enumerate(zip(want, rc.ppo_scalar_bounds(d, EPS32, vclip)))]
    dh = host(dhead)
    tl, tv = _head_tolerances(M, 1.0)
    np.testing.assert_allclose(dh[:, :A], ref['dlogits'], **tl)
    np.testing.assert_allclose(dh[:, A], ref['dvalue'], **tv)
    assert np.array_equal(dh[:, A + 1:], np.zeros((M, ldh - A - 1), np.float32))
    print('RATIO ppo', M, vclip, [round(r, 3) for r in ratios])


@pytest.mark.parametrize('scale', [1.0, 30.0])
@pytest.mark.parametrize('A', [1, 64])
def test_categorical_at_the_action_limits(lib, cuda, A, scale):
    """acmi_categorical at A = 1 and A = 64 with ld = A + 3 (NaN padding): float64 at the
    tolerances of test_a2c_loss_and_categorical_match_oracle, and H >= 0, log pi <= 0
    exactly (scale 30: the saturated-logit form)."""
    B, ld = 1000, A + 3
    rng = np.random.default_rng(60 + A)
    z = (rng.standard_normal((B, A)) * scale).astype(np.float32)
    act = rng.integers(0, A, B).astype(np.int32)
    ent, lp = nans(B, cuda), nans(B, cuda)
    L, AC = dev(rc.pad_columns(z, ld)), dev(act)
    _lib.call('acmi_categorical', _lib.ptr(L), ld, B, A, _lib.ptr(AC), _lib.ptr(ent), _lib.ptr(lp),
              _lib.stream_handle())
    ent, lp = host(ent), host(lp)
    np.testing.assert_allclose(ent, oracle.entropy(z.astype(np.float64)), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(lp, oracle.log_softmax(z.astype(np.float64))[np.arange(B), act], rtol=1e-5, atol=1e-6)
    assert (ent >= 0).all() and (lp <= 0).all()
    if A == 1:
        assert not ent.any() and not lp.any()


# ---------------------------------------------------------------------------
# 3. advantage moments and normalisation
# ---------------------------------------------------------------------------
def _moments(lib, cuda, ad, M):
    ws = nans(lib.acmi_adv_moments_ws_doubles(M), cuda, torch.float64)
    mom = nans(2, cuda, torch.float64)
    _lib.call('acmi_adv_moments', _lib.ptr(ad), M, _lib.ptr(ws), _lib.ptr(mom), _lib.stream_handle())
    return mom


@pytest.mark.parametrize('family', ['normal', 'offset'])
@pytest.mark.parametrize('M', rc.ADV_SIZES)
def test_advantage_moments_and_normalisation(lib, cuda, M, family):
    a = rc.adv_case(M, family)
    ad = dev(a)
    mom = _moments(lib, cuda, ad, M)
    m, w = host(mom), a.astype(np.float64)
    assert m[0] == pytest.approx(w.sum(), rel=1e-12)
    assert m[1] == pytest.approx((w * w).sum(), rel=1e-12)
    _lib.call('acmi_adv_normalize', _lib.ptr(ad), M, _lib.ptr(mom), float(M), rc.ADV_EPS, _lib.stream_handle())
    ref = oracle.normalize_advantages(a, rc.ADV_EPS)
    r = check('adv_normalize %s M=%d' % (family, M), host(ad), (ref, rc.adv_bound(a)[1]))
    print('RATIO adv', family, M, round(r, 3))


@pytest.mark.parametrize('M', rc.ADV_SIZES)
def test_constant_batch_normalises_to_exactly_zero(lib, cuda, M):
    for k in range(len(rc.CONSTANT_VALUES)):
        ad = dev(rc.adv_case(M, 'constant', k))
        mom = _moments(lib, cuda, ad, M)
        _lib.call('acmi_adv_normalize', _lib.ptr(ad), M, _lib.ptr(mom), float(M), rc.ADV_EPS, _lib.stream_handle())
        assert np.array_equal(host(ad), np.zeros(M, np.float32)), rc.CONSTANT_VALUES[k]


@pytest.mark.parametrize('M', [255, rc.MOM_THREADS + 1])
def test_half_batch_normalised_with_the_moments_of_the_whole(lib, cuda, M):
    """count != M, the data-parallel case: two ranks' moments added, count = 2 M; each half
    equals the oracle on the whole batch."""
    a = rc.adv_case(2 * M, 'normal')
    halves = [dev(a[:M]), dev(a[M:])]
    mom = _moments(lib, cuda, halves[0], M) + _moments(lib, cuda, halves[1], M)
    ref = oracle.normalize_advantages(a, rc.ADV_EPS)
    for h, sl in zip(halves, (slice(0, M), slice(M, 2 * M))):
        _lib.call('acmi_adv_normalize', _lib.ptr(h), M, _lib.ptr(mom), float(2 * M), rc.ADV_EPS,
                  _lib.stream_handle())
        check('adv_normalize count=2M rows %s' % (sl,), host(h), (ref[sl], rc.adv_bound(a, a[sl], ranks=2)[1]))


# ---------------------------------------------------------------------------
# 4. sampler
# ---------------------------------------------------------------------------
def _sample(cuda, L, ld, B, A, seed=0, sid=0, ctr=0, uniforms=None, mode=0, entry='acmi_sample_actions', **kw):
    """(actions, bad_rows); actions start at the sentinel, bad_rows (a counter the kernel
    adds to) at 0."""
    out = torch.full((B,), SENTINEL, dtype=torch.int32, device=cuda)
    bad = torch.zeros(1, dtype=torch.int32, device=cuda)
    s = _lib.stream_handle()
    if entry == 'acmi_sample_actions':
        _lib.call(entry, _lib.ptr(L), ld, B, A, seed, sid, ctr, _lib.ptr(uniforms), mode, _lib.ptr(out),
                  _lib.ptr(bad), s)
    elif entry == 'acmi_sample_actions_at':
        _lib.call(entry, _lib.ptr(L), ld, B, A, seed, sid, ctr, kw['row_offset'], _lib.ptr(uniforms), mode,
                  _lib.ptr(out), _lib.ptr(bad), s)
    else:
        _lib.call(entry, _lib.ptr(L), ld, B, A, seed, sid, _lib.ptr(kw['counter_dev']), ctr, kw.get('row_offset', 0),
                  _lib.ptr(uniforms), mode, _lib.ptr(out), _lib.ptr(bad), s)
    return host(out), int(bad.item())


def _check_draws(cuda, A, pad, scale, B):
    z, u = rc.sampler_case(A, scale, B)
    ld = A + pad
    y, bad = _sample(cuda, dev(rc.pad_columns(z, ld)), ld, B, A, uniforms=dev(u))
    assert bad == 0
    np.testing.assert_array_equal(y, rc.sample_f32_rows(z, u))  # bit for bit the float32 restatement
    k = min(B, 512)
    np.testing.assert_array_equal(y[:k], oracle.sample_f32(z[:k], u[:k]))
    y64, near, p = rc.inverse_cdf_f64(z, u)
    assert near.mean() <= 0.01
    np.testing.assert_array_equal(y[~near], y64[~near])  # the float64 inverse CDF of softmax
    assert (p[np.arange(B), y] > 0).all()


@pytest.mark.parametrize('scale', rc.SAMPLER_SCALES)
@pytest.mark.parametrize('pad', [0, 3], ids=['ld=A', 'ld=A+3'])
@pytest.mark.parametrize('A', rc.SAMPLER_A)
def test_sampler_draws_the_float64_inverse_cdf(lib, cuda, A, pad, scale):
    _check_draws(cuda, A, pad, scale, rc.SAMPLER_B)


@pytest.mark.parametrize('B', rc.SAMPLER_EDGE_B)
def test_sampler_at_the_block_edges(lib, cuda, B):
    _check_draws(cuda, 18, 3, 2.0, B)


@pytest.mark.parametrize('A', [2, 32, 64])
def test_sampler_on_a_cdf_boundary_draws_the_action_above(lib, cuda, A):
    """u exactly on F(k - 1) = k / A draws k: the CDF interval of an action is closed
    below and open above."""
    z, u, want = rc.tie_case(A)
    y, bad = _sample(cuda, dev(rc.pad_columns(z, A + 3)), A + 3, A, A, uniforms=dev(u))
    assert bad == 0
    np.testing.assert_array_equal(y, want)


def test_sampler_counter_rng_is_calibrated_on_a_skewed_row(lib, cuda):
    """One non-uniform logit row repeated, the counter RNG at CALIBRATION_SEEDS (a seeded
    draw: the same every run): the oracle's draws exactly, and a chi-square against the
    float64 softmax under 25 (df = 5), every expected count at least 50."""
    B, A = rc.SAMPLER_B, 6
    z = np.tile(np.asarray(rc.CALIBRATION_ROW, np.float32), (B, 1))
    seed, sid, ctr = rc.CALIBRATION_SEEDS
    y, bad = _sample(cuda, dev(z), A, B, A, seed, sid, ctr)
    np.testing.assert_array_equal(y, rc.sample_f32_rows(z, oracle.sample_uniforms(seed, sid, ctr, B)))
    p = np.exp(oracle.log_softmax(np.asarray(rc.CALIBRATION_ROW, np.float64)))
    counts = np.bincount(y, minlength=A)
    assert (p * B >= 50).all() and ((counts - p * B) ** 2 / (p * B)).sum() < 25.0


def test_sampler_in_pieces_and_with_a_device_counter(lib, cuda):
    """A batch sampled in three pieces (row_offset 0, 1000, 3000) is the single launch bit
    for bit; *counter_dev = 7 with counter_add = 2 is counter = 9."""
    B, A, ld = rc.SAMPLER_B, 18, 21
    z, _ = rc.sampler_case(A, 2.0)
    L = dev(rc.pad_columns(z, ld))
    whole, _ = _sample(cuda, L, ld, B, A, 5, 1, 9)
    np.testing.assert_array_equal(whole, rc.sample_f32_rows(z, oracle.sample_uniforms(5, 1, 9, B)))
    pieces = []
    for lo, hi in ((0, 1000), (1000, 3000), (3000, B)):
        y, bad = _sample(cuda, L[lo:hi], ld, hi - lo, A, 5, 1, 9, entry='acmi_sample_actions_at', row_offset=lo)
        assert bad == 0
        pieces.append(y)
    np.testing.assert_array_equal(np.concatenate(pieces), whole)
    assert not np.array_equal(pieces[1], whole[:2000])  # the offset moves the draws
    ctr = torch.tensor([7], dtype=torch.int32, device=cuda)
    y, _ = _sample(cuda, L, ld, B, A, 5, 1, 2, entry='acmi_sample_actions_dev', counter_dev=ctr)
    np.testing.assert_array_equal(y, whole)
    assert int(ctr.item()) == 7  # read, not advanced


@pytest.mark.parametrize('A', [2, 33])
def test_sampler_mode_takes_the_first_maximum(lib, cuda, A):
    """mode = 1 on rows with exact ties; the padding of ld > A holds 3e38, which would win
    any maximum that read it."""
    z = rc.mode_case(A)
    B, ld = z.shape[0], A + 3
    y, bad = _sample(cuda, dev(rc.pad_columns(z, ld, fill=3e38)), ld, B, A, mode=1)
    assert bad == 0
    np.testing.assert_array_equal(y, z.argmax(1))


def test_sampler_counts_bad_rows_over_three_blocks(lib, cuda):
    B, A, ld = 600, 6, 9
    z, u = rc.sampler_case(A, 2.0, B)
    clean, bad = _sample(cuda, dev(rc.pad_columns(z, ld)), ld, B, A, uniforms=dev(u))
    assert bad == 0 and clean.min() >= 0
    rows = [3, 255, 256, 300, 599]
    zb = z.copy()
    for r, col, val in zip(rows, (0, 5, 2, 0, 5), (np.inf, -np.inf, np.nan, np.nan, np.inf)):
        zb[r, col] = val
    y, bad = _sample(cuda, dev(rc.pad_columns(zb, ld)), ld, B, A, uniforms=dev(u))
    assert bad == 5
    want = clean.copy()
    want[rows] = -1
    np.testing.assert_array_equal(y, want)


# ---------------------------------------------------------------------------
# 5. GAE
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', rc.GAE_CASES, ids=lambda c: '%d-%d-%g-%g-%s' % c)
def test_gae_bit_exact_and_within_its_float64_bound(lib, cuda, case):
    N, T, gamma, lam, family = case
    r, te, v, vb = rc.gae_case(N, T, family)
    R, TE, V, VB = dev(r), dev(te.astype(np.uint8)), dev(v), dev(vb)
    tg, adv = nans((N, T), cuda), nans((N, T), cuda)
    _lib.call('acmi_gae', _lib.ptr(R), _lib.ptr(TE), _lib.ptr(V), _lib.ptr(VB), N, T, gamma, lam, _lib.ptr(tg),
              _lib.ptr(adv), _lib.stream_handle())
    tg, adv = host(tg), host(adv)
    t32, a32 = oracle.gae_f32(r, te, v, vb, gamma, lam)
    np.testing.assert_array_equal(tg, t32)
    np.testing.assert_array_equal(adv, a32)
    t64, a64, b_tg, b_adv = rc.gae_ref(r, te, v, vb, gamma, lam)
    ratios = [check('gae advantages %s' % (case,), adv, (a64, b_adv)), check('gae targets %s' % (case,), tg, (t64, b_tg))]
    if lam == 1.0:  # acmi_returns' targets, equal in exact arithmetic
        gp, bp = oracle.gamma_tables(gamma, T)
        rt, ra = nans((N, T), cuda), nans((N, T), cuda)
        GP, BP = dev(gp), dev(bp)
        _lib.call('acmi_returns', _lib.ptr(R), _lib.ptr(TE), _lib.ptr(V), _lib.ptr(VB), N, T, _lib.ptr(GP),
                  _lib.ptr(BP), _lib.ptr(rt), _lib.ptr(ra), _lib.stream_handle())
        ratios.append(check('gae(lambda = 1) against acmi_returns %s' % (case,), tg,
                            (host(rt).astype(np.float64), b_tg + rc.returns_bound(r, te, vb, gamma))))
    print('RATIO gae', case, [round(x, 3) for x in ratios])
