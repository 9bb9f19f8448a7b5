"""The K-FAC optimizer kernels (csrc/kfac.hip: acmi_kfac_ema, acmi_kfac_inverse,
acmi_kfac_step) called through the C ABI and compared with float64 numpy on the
same f32 inputs, and ColdStartPeriodicInvUpdateKfacOpt followed update by update
against the float64 oracle from the GPU's own optimizer state.

Layouts (A, C3): (4, 32) the ACKTR config; (18, 32) the full action set; (6, 64) a
six-action game (the narrow first product with inv_ld = 8) on the wide tower, whose
fc4 A factor is 3137 x 3137 (np = 3168: 99 pivot steps of the block Gauss-Jordan).
The step also runs at the ends of the action range: (1, 32) a 1 x 1 policy block,
(33, 32) the narrow product at dout = 33 (inv_ld = 36), (64, 64) the widest one.

Scalars passed to the library as float are rounded to f32 in the references first
(1 - decay and damping / CONV_LOCATIONS[l] are formed in f32, as the kernels do).
"""
import ctypes
import time

import numpy as np
import pytest
import torch

from actorcritic import _lib
from test_gpu_parity import _blocks, _build, _feed, oracle

pytestmark = pytest.mark.gpu

LAYOUTS = [(4, 32), (18, 32), (6, 64), (1, 32), (33, 32), (64, 64)]
LAYOUT_IDS = ['a4-c32', 'a18-c32', 'a6-c64', 'a1-c32', 'a33-c32', 'a64-c64']
EPS = 2.0 ** -24  # one f32 rounding, relative
F32 = np.float32


def _layout(A, C3):
    from actorcritic._engine import Layout
    return Layout(A, C3)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---------------------------------------------------------------------------
# acmi_kfac_ema
# ---------------------------------------------------------------------------
GUARD = 64


def _ema_call(biased, factors, stats, n, decay, debias, scale):
    _lib.call('acmi_kfac_ema', _lib.ptr(biased), _lib.ptr(factors), _lib.ptr(stats), n, decay, debias, scale,
              _lib.stream_handle())
    torch.cuda.synchronize()


def _ema_check(b_prev, stats, b_got, f_got, decay, debias, scale, what):
    """One EMA step against float64 from the same f32 inputs: decay * b and
    (1 - decay) * (s * scale) each round once (s * scale is exact for the power-of-two
    scales used here) and their sum once -- `biased` within 2 roundings of the two
    terms' magnitudes; `factors` = biased * debias rounds once more."""
    d32, deb32, sc32 = F32(decay), F32(debias), F32(scale)
    omd = np.float64(F32(1.0) - d32)
    t1 = np.float64(d32) * b_prev.astype(np.float64)
    t2 = omd * (stats.astype(np.float64) * np.float64(sc32))
    mag = np.abs(t1) + np.abs(t2)
    ref_b = t1 + t2
    ref_f = ref_b * np.float64(deb32)
    err_b = np.abs(b_got.astype(np.float64) - ref_b)
    err_f = np.abs(f_got.astype(np.float64) - ref_f)
    assert np.all(err_b <= 3 * EPS * mag), (what, 'biased', float((err_b / np.maximum(mag, 1e-300)).max() / EPS))
    bound_f = 3 * EPS * mag * np.float64(deb32)
    assert np.all(err_f <= bound_f), (what, 'factors', float((err_f / np.maximum(bound_f, 1e-300)).max()))


@pytest.mark.parametrize('scale', [1.0, 0.5])
def test_ema_four_steps_match_float64(lib, cuda, scale):
    """Four successive acmi_kfac_ema calls on a carried `biased` (zero at first, as
    the optimizer's) with fresh statistics, decay 0.99, debias 1 / (1 - decay^t), at
    n = stat_total of (4, 32) -- 3.6 M elements, 7 passes of the 2048 x 256 grid-stride
    loop.  Every step is compared element-wise with the float64 recurrence applied to
    the carried f32 `biased` (bounds: _ema_check); the statistics are left unchanged
    and nothing past n is written."""
    n = _layout(4, 32).stat_total
    assert n > 2048 * 256
    rng = np.random.default_rng(31)
    nan_guard = lambda: torch.full((n + GUARD,), float('nan'), device=cuda)
    biased, factors = nan_guard(), nan_guard()
    biased[:n] = 0
    decay = 0.99
    for t in range(1, 5):
        stats_h = (rng.standard_normal(n) * rng.choice([1e-3, 1.0, 30.0], n)).astype(F32)
        stats = dev(stats_h)
        b_prev = biased[:n].cpu().numpy()
        debias = 1.0 / (1.0 - decay ** t)
        _ema_call(biased, factors, stats, n, decay, debias, scale)
        assert torch.equal(stats.cpu(), torch.from_numpy(stats_h)), 'the statistics are an input'
        b_got, f_got = biased.cpu().numpy(), factors.cpu().numpy()
        assert np.isnan(b_got[n:]).all() and np.isnan(f_got[n:]).all(), 'written past n'
        assert np.isfinite(f_got[n - 1]) and np.isfinite(b_got[n - 1])
        _ema_check(b_prev, stats_h, b_got[:n], f_got[:n], decay, debias, scale, t)
        if t > 1:  # the carried term is a real part of the sum
            assert np.abs(np.float64(decay) * b_prev).max() > 1e-3


@pytest.mark.parametrize('n', [1, 257])
def test_ema_small_sizes_stay_in_bounds(lib, cuda, n):
    rng = np.random.default_rng(32 + n)
    b_prev = rng.standard_normal(n).astype(F32)
    stats_h = rng.standard_normal(n).astype(F32)
    biased = torch.full((n + GUARD,), float('nan'), device=cuda)
    factors = torch.full((n + GUARD,), float('nan'), device=cuda)
    biased[:n] = dev(b_prev)
    stats = torch.full((n + GUARD,), float('nan'), device=cuda)
    stats[:n] = dev(stats_h)
    decay, t = 0.99, 3
    debias = 1.0 / (1.0 - decay ** t)
    _ema_call(biased, factors, stats, n, decay, debias, 1.0)
    b_got, f_got = biased.cpu().numpy(), factors.cpu().numpy()
    assert np.isnan(b_got[n:]).all() and np.isnan(f_got[n:]).all()
    _ema_check(b_prev, stats_h, b_got[:n], f_got[:n], decay, debias, 1.0, n)


# ---------------------------------------------------------------------------
# acmi_kfac_inverse
# ---------------------------------------------------------------------------
_FACTORS = {}


def _factors(A, C3):
    """The construction of test_kfac_inverse_matches_numpy: X^T X / rows with
    rows = n // 2 + 3 (rank-deficient before damping), rounded to f32."""
    if (A, C3) not in _FACTORS:
        L = _layout(A, C3)
        rng = np.random.default_rng(5)
        fac = np.zeros(L.stat_total, F32)
        for f in range(11):
            n = L.din[f] if f < 5 else L.dout[f - 5]
            x = rng.standard_normal((max(n // 2, 1) + 3, n))
            fac[L.stat_off[f]:L.stat_off[f] + n * n] = (x.T @ x / x.shape[0]).astype(F32).ravel()
        _FACTORS[(A, C3)] = fac
    return _FACTORS[(A, C3)]


def _factor(L, fac, f):
    n = L.din[f] if f < 5 else L.dout[f - 5]
    return fac[L.stat_off[f]:L.stat_off[f] + n * n].reshape(n, n).astype(np.float64)


def _run_inverse(lib, cuda, A, C3, fac, damping, conv_normalize, ws_fill=0.0):
    fac_d = dev(fac)
    inv = torch.full((int(lib.acmi_kfac_inverse_floats(A, C3)),), float('nan'), device=cuda)
    ws = torch.full((int(lib.acmi_kfac_inverse_ws_doubles(A, C3)),), ws_fill, dtype=torch.float64, device=cuda)
    _lib.call('acmi_kfac_inverse', A, C3, _lib.ptr(fac_d), ctypes.c_float(damping), conv_normalize, _lib.ptr(inv),
              _lib.ptr(ws), _lib.stream_handle())
    torch.cuda.synchronize()
    assert torch.equal(fac_d.cpu(), torch.from_numpy(fac)), 'the factors are an input'
    return inv.cpu()


def _inv_block(L, inv_h, m):
    """Block m of a host inverse buffer, after checking its zero padding columns."""
    n = L.dout[m // 2] if m % 2 else L.din[m // 2]
    o, ld = L.inv_off[m], L.inv_ld[m]
    b = inv_h[o:o + n * ld].reshape(n, ld)
    assert ld % 4 == 0 and n <= ld < n + 4 and not b[:, n:].any(), 'padding columns must be zero'
    return b[:, :n]


def _lambda32(damping, l, conv_normalize):
    lam = F32(damping) / F32(oracle.CONV_LOCATIONS[l]) if conv_normalize else F32(damping)
    return np.float64(lam)


def _check_inverse(L, fac, inv_h, damping, conv_normalize, layers=range(6), pi_one=()):
    inv_h = inv_h.numpy().astype(np.float64)
    for l in layers:
        Am, Gm = _factor(L, fac, min(l, 4)), _factor(L, fac, 5 + l)
        da, dg = Am.shape[0], Gm.shape[0]
        lam = _lambda32(damping, l, conv_normalize)
        pi = 1.0 if l in pi_one else np.sqrt((np.trace(Am) / da) / (np.trace(Gm) / dg))
        Am, Gm = 0.5 * (Am + Am.T), 0.5 * (Gm + Gm.T)
        for m, M, add in ((2 * l, Am, pi * np.sqrt(lam)), (2 * l + 1, Gm, np.sqrt(lam) / pi)):
            ref = np.linalg.inv(M + add * np.eye(M.shape[0]))
            got = _inv_block(L, inv_h, m)
            rel = np.abs(got - ref).max() / np.abs(ref).max()
            print('layer', l, 'AG'[m % 2], 'n', M.shape[0], 'rel %.2e' % rel)
            assert rel < 1e-5, (l, 'AG'[m % 2], rel)


@pytest.mark.parametrize('A,C3,conv_normalize',
                         [(4, 32, 0), (4, 32, 1), (18, 32, 0), (18, 32, 1), (6, 64, 0), (6, 64, 1)],
                         ids=['a4-c32-plain', 'a4-c32-convnorm', 'a18-c32-plain', 'a18-c32-convnorm',
                              'a6-c64-plain', 'a6-c64-convnorm'])
def test_inverse_matches_numpy(lib, cuda, A, C3, conv_normalize):
    """acmi_kfac_inverse against numpy.linalg.inv of the same f32 factors with the
    f32 lambda_l (damping 0.01; conv_normalize: lambda_l = damping / locations of
    layer l), rel 1e-5 of max-abs per block, zero padding columns.  (6, 64) is the
    inverse at its largest size -- the 3137-wide fc4 A factor, 99 pivot steps.
    Measured: 2.0e-8 .. 5.7e-8 on every block of every case, the 3137-wide one
    4.1e-8; the (6, 64) case takes 0.4 s, float64 reference included."""
    L = _layout(A, C3)
    fac = _factors(A, C3)
    t0 = time.time()
    inv_h = _run_inverse(lib, cuda, A, C3, fac, 0.01, conv_normalize)
    print('gpu inverse + copies %.2f s' % (time.time() - t0))
    assert torch.isfinite(inv_h).all()
    _check_inverse(L, fac, inv_h, 0.01, conv_normalize)


def test_inverse_conv_normalize_changes_only_the_conv_layers(lib, cuda):
    A, C3 = 4, 32
    L = _layout(A, C3)
    fac = _factors(A, C3)
    plain = _run_inverse(lib, cuda, A, C3, fac, 0.01, 0)
    norm = _run_inverse(lib, cuda, A, C3, fac, 0.01, 1)
    for m in range(12):
        a, b = L.inverse_block(plain, m), L.inverse_block(norm, m)
        if m < 6:  # conv1..conv3: lambda / 400, / 81, / 49
            rel = (a - b).abs().max().item() / a.abs().max().item()
            assert rel > 1e-2, (m, rel)
        else:      # fc4 and the heads: one location
            assert torch.equal(a, b), m


def test_inverse_zero_trace_takes_pi_one(lib, cuda):
    """fc_policy's G factor all zero (trace 0): damp_kernel falls back to pi = 1, so
    Ginv = I / sqrt(lambda) and Ainv = (A_4 + sqrt(lambda) I)^-1; the other five
    layers (fc_baseline shares A_4 but keeps its own G) are bit-identical to the run
    with the factor in place."""
    A, C3 = 4, 32
    L = _layout(A, C3)
    fac = _factors(A, C3)
    full = _run_inverse(lib, cuda, A, C3, fac, 0.01, 0)
    fz = fac.copy()
    nG = L.dout[4]
    fz[L.stat_off[9]:L.stat_off[9] + nG * nG] = 0
    got = _run_inverse(lib, cuda, A, C3, fz, 0.01, 0)
    assert torch.isfinite(got).all()
    for m in range(12):
        if m // 2 != 4:
            assert torch.equal(L.inverse_block(got, m), L.inverse_block(full, m)), m
    _check_inverse(L, fz, got, 0.01, 0, layers=[4], pi_one=(4,))
    ginv = _inv_block(L, got.numpy().astype(np.float64), 9)
    lam = _lambda32(0.01, 4, 0)
    np.testing.assert_allclose(ginv, np.eye(nG) / np.sqrt(lam), rtol=1e-5, atol=1e-5 / np.sqrt(lam))


def test_inverse_independent_of_workspace_contents(lib, cuda):
    A, C3 = 18, 32
    fac = _factors(A, C3)
    a = _run_inverse(lib, cuda, A, C3, fac, 0.01, 1, ws_fill=float('nan'))
    b = _run_inverse(lib, cuda, A, C3, fac, 0.01, 1, ws_fill=0.0)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# acmi_kfac_step
# ---------------------------------------------------------------------------
LR, MOM, NC = 0.25, 0.9, 1e-4
_STEP = {}


def _rel_l2(got, ref):
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def _rel_max(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def _step_case(A, C3):
    """Seeded inputs of one acmi_kfac_step and their references, built once per
    layout: SPD "inverse" blocks X^T X / rows + 0.1 I (exactly symmetric f32, in the
    padded layout with zero padding columns), gradients, a non-zero velocity,
    parameters; per K-FAC block the float64 Ainv g Ginv of the f32 inputs and the
    error of the same two products in f32 on the CPU (torch.float32 matmul).
    Gradients are used scaled by powers of two (s_clip: lr^2 g.precon >= 200 c,
    s_free: <= c / 200), which scales every product exactly."""
    if (A, C3) in _STEP:
        return _STEP[(A, C3)]
    L = _layout(A, C3)
    rng = np.random.default_rng(1000 + 10 * A + C3)
    inv = np.zeros(L.inv_total, F32)
    mats = []
    for m in range(12):
        n = L.dout[m // 2] if m % 2 else L.din[m // 2]
        x = rng.standard_normal((max(n // 2, 1) + 3, n))
        M = x.T @ x / x.shape[0] + 0.1 * np.eye(n)
        M = (0.5 * (M + M.T)).astype(F32)
        assert np.array_equal(M, M.T)
        o, ld = L.inv_off[m], L.inv_ld[m]
        inv[o:o + n * ld].reshape(n, ld)[:, :n] = M
        mats.append(M)
    n = L.nparams
    grads = (rng.standard_normal(n) * 1e-2).astype(F32)
    vel = (rng.standard_normal(n) * 1e-3).astype(F32)
    params = rng.standard_normal(n).astype(F32)
    precon = np.zeros(n)
    cpu_l2, cpu_max = {}, {}
    blocks = _blocks(A, C3)
    for l, (name, lo, hi) in enumerate(blocks):
        assert lo == L.offsets[2 * l] and hi - lo == L.din[l] * L.dout[l]
        g = grads[lo:hi].reshape(L.din[l], L.dout[l])
        ref = mats[2 * l].astype(np.float64) @ g.astype(np.float64) @ mats[2 * l + 1].astype(np.float64)
        f32 = (torch.from_numpy(mats[2 * l]) @ torch.from_numpy(g) @ torch.from_numpy(mats[2 * l + 1])).numpy()
        precon[lo:hi] = ref.ravel()
        cpu_l2[name] = _rel_l2(f32.astype(np.float64), ref)
        cpu_max[name] = _rel_max(f32.astype(np.float64), ref)
    c = np.float64(F32(NC))
    sq0 = float(grads.astype(np.float64) @ precon) * LR * LR
    assert sq0 > 0
    s_clip = 2.0 ** np.ceil(0.5 * np.log2(200.0 * c / sq0))
    s_free = 2.0 ** np.floor(0.5 * np.log2(c / (200.0 * sq0)))
    case = dict(L=L, inv=inv, grads=grads, vel=vel, params=params, precon=precon, sq0=sq0, c=c, blocks=blocks,
                cpu_l2=cpu_l2, cpu_max=cpu_max, s_clip=s_clip, s_free=s_free, dev={})
    _STEP[(A, C3)] = case
    return case


def _on_dev(case, key, make):
    if key not in case['dev']:
        case['dev'][key] = dev(make())
    return case['dev'][key]


def _run_step(lib, case, scale, inv_key='inv', nc=NC, ws_fill=0.0, want_coeff=True):
    """One acmi_kfac_step on fresh copies of params / velocity; `precon` (an output)
    and coeff_out start as NaN.  Returns host arrays (params, velocity, precon, coeff)."""
    L = case['L']
    make_inv = {'inv': lambda: case['inv'], 'neg_a': lambda: _negate_a(case),
                'identity': lambda: _identity(case)}[inv_key]
    inv = _on_dev(case, inv_key, make_inv)
    g = _on_dev(case, ('g', scale), lambda: (case['grads'] * F32(scale)).astype(F32))
    p = _on_dev(case, 'p', lambda: case['params']).clone()
    v = _on_dev(case, 'v', lambda: case['vel']).clone()
    precon = torch.full((L.nparams,), float('nan'), device='cuda')
    ws = torch.full((int(lib.acmi_kfac_step_ws_floats(L.A, L.C3)),), ws_fill, device='cuda')
    coeff = torch.full((1,), float('nan'), device='cuda') if want_coeff else None
    _lib.call('acmi_kfac_step', L.A, L.C3, _lib.ptr(p), _lib.ptr(v), _lib.ptr(g), _lib.ptr(inv), LR, MOM, nc,
              _lib.ptr(precon), _lib.ptr(ws), _lib.ptr(coeff), _lib.stream_handle())
    torch.cuda.synchronize()
    return (p.cpu().numpy(), v.cpu().numpy(), precon.cpu().numpy(),
            coeff.cpu().numpy()[0] if want_coeff else None)


def _negate_a(case):
    """The Ainv block of every layer negated: every preconditioned block changes sign
    (negating Ainv and Ginv both would cancel), so g . precon < 0."""
    L, inv = case['L'], case['inv'].copy()
    for l in range(6):
        o, sz = L.inv_off[2 * l], L.din[l] * L.inv_ld[2 * l]
        inv[o:o + sz] = -inv[o:o + sz]
    return inv


def _identity(case):
    L = case['L']
    inv = np.zeros(L.inv_total, F32)
    for m in range(12):
        n = L.dout[m // 2] if m % 2 else L.din[m // 2]
        o, ld = L.inv_off[m], L.inv_ld[m]
        inv[o:o + n * ld].reshape(n, ld)[:, :n] = np.eye(n, dtype=F32)
    return inv


def _check_apply(case, scale, p, v, precon, coeff):
    """kapply_kernel alone, from the GPU's own precon and coeff: v' = mom v + coeff d
    (two products and a sum: three f32 roundings of the terms' magnitudes) and
    p' = p - lr v' from the stored v' (a product and a sum)."""
    v0, p0 = case['vel'].astype(np.float64), case['params'].astype(np.float64)
    mv = np.float64(F32(MOM)) * v0
    cd = np.float64(coeff) * precon.astype(np.float64)
    assert np.all(np.abs(v.astype(np.float64) - (mv + cd)) <= 3 * EPS * (np.abs(mv) + np.abs(cd)))
    lv = np.float64(F32(LR)) * v.astype(np.float64)
    assert np.all(np.abs(p.astype(np.float64) - (p0 - lv)) <= 3 * EPS * (np.abs(p0) + np.abs(lv)))
    assert np.abs(mv).max() > 0 and np.abs(v - case['vel']).max() > 0 and np.abs(p - case['params']).max() > 0


@pytest.mark.parametrize('A,C3', LAYOUTS, ids=LAYOUT_IDS)
def test_step_precon_coeff_and_apply_match_float64(lib, cuda, A, C3):
    """precon = Ainv g Ginv per K-FAC block against float64 of the same f32 inputs, in
    the clipped trust-region regime with a non-zero velocity.  The bound is the
    measured error of the same two products in f32 on the CPU: the kernel (two
    grouped bf16x3 GEMMs; kfac_narrow_kernel for the heads) stays within 10x of it,
    floored at 5e-7 (the margin and floor of test_x3_gemms_are_f32_class), and under
    2e-5 (the gradient tolerance) -- in rel-L2 and in max-abs / max-abs per block, so
    one wrong entry of the 513-entry value block or the din x A policy block shows.
    Then coeff against float64 (rel 1e-5) and the momentum / parameter update
    element-wise from the GPU's own precon and coeff (_check_apply).

    Measured (rel-L2 gpu / f32-cpu | max-abs gpu / f32-cpu; printed on every run):
      block        (4, 32)                         (18, 32)                        (6, 64)
      conv1        3.0e-7/2.2e-7 | 5.3e-7/3.0e-7   2.8e-7/2.2e-7 | 2.8e-7/2.8e-7   3.0e-7/2.3e-7 | 4.7e-7/3.5e-7
      conv2        4.2e-7/2.7e-7 | 6.1e-7/4.1e-7   4.3e-7/2.8e-7 | 5.6e-7/4.1e-7   4.3e-7/2.8e-7 | 6.3e-7/3.4e-7
      conv3        4.4e-7/2.8e-7 | 6.8e-7/3.7e-7   4.3e-7/2.7e-7 | 5.7e-7/4.1e-7   4.5e-7/2.9e-7 | 5.6e-7/4.1e-7
      fc4          8.2e-7/3.5e-7 | 1.7e-6/5.9e-7   8.2e-7/3.5e-7 | 1.5e-6/7.5e-7   1.1e-6/3.6e-7 | 2.3e-6/6.1e-7
      fc_policy    4.2e-7/4.2e-7 | 7.0e-7/7.0e-7   1.2e-7/2.9e-7 | 1.7e-7/4.1e-7   9.8e-8/4.2e-7 | 1.5e-7/6.2e-7
      fc_baseline  8.1e-8/2.1e-7 | 7.4e-8/2.5e-7   8.8e-8/2.2e-7 | 1.1e-7/3.5e-7   8.7e-8/2.0e-7 | 1.4e-7/3.5e-7
      block        (1, 32)                         (33, 32)                        (64, 64)
      conv1        3.0e-7/2.2e-7 | 5.4e-7/2.5e-7   3.2e-7/2.4e-7 | 4.6e-7/3.1e-7   2.9e-7/2.3e-7 | 3.8e-7/2.8e-7
      conv2        4.4e-7/2.9e-7 | 6.7e-7/4.6e-7   4.4e-7/2.8e-7 | 5.1e-7/3.4e-7   4.4e-7/2.8e-7 | 8.5e-7/4.0e-7
      conv3        4.3e-7/2.7e-7 | 6.1e-7/4.2e-7   4.4e-7/2.8e-7 | 5.1e-7/2.9e-7   4.5e-7/2.8e-7 | 7.5e-7/4.7e-7
      fc4          8.2e-7/3.5e-7 | 1.6e-6/6.9e-7   8.2e-7/3.5e-7 | 1.7e-6/8.6e-7   1.1e-6/3.5e-7 | 2.0e-6/7.6e-7
      fc_policy    8.0e-8/2.2e-7 | 8.8e-8/3.9e-7   1.3e-7/2.7e-7 | 2.3e-7/3.6e-7   4.3e-7/2.8e-7 | 6.0e-7/5.3e-7
      fc_baseline  9.8e-8/2.3e-7 | 1.5e-7/3.8e-7   8.4e-8/2.1e-7 | 9.5e-8/3.0e-7   8.4e-8/1.8e-7 | 1.1e-7/2.1e-7
    (the f32-CPU figures depend on the host's BLAS; the worst ratio is fc4 at
    (6, 64), 3.8x in max-abs, K = 3137 in the first product)."""
    case = _step_case(A, C3)
    s = case['s_clip']
    p, v, precon, coeff = _run_step(lib, case, s)
    assert np.isfinite(precon).all() and np.isfinite(p).all() and np.isfinite(v).all()
    ref = case['precon'] * s
    fails = []
    for name, lo, hi in case['blocks']:
        got = precon[lo:hi].astype(np.float64)
        e_l2, e_max = _rel_l2(got, ref[lo:hi]), _rel_max(got, ref[lo:hi])
        c_l2, c_max = case['cpu_l2'][name], case['cpu_max'][name]
        print('A=%d C3=%d block %-11s rel-L2 gpu %.2e f32-cpu %.2e | max-abs gpu %.2e f32-cpu %.2e'
              % (A, C3, name, e_l2, c_l2, e_max, c_max))
        if not (e_l2 <= 10 * max(c_l2, 5e-7) and e_l2 <= 2e-5):
            fails.append((name, 'rel-L2', e_l2, c_l2))
        if not (e_max <= 10 * max(c_max, 5e-7) and e_max <= 2e-5):
            fails.append((name, 'max-abs', e_max, c_max))
    assert not fails, fails
    sq = case['sq0'] * s * s
    coeff_ref = min(1.0, np.sqrt(case['c'] / sq))
    assert sq >= 100 * case['c'] and coeff_ref < 0.1
    assert float(coeff) == pytest.approx(coeff_ref, rel=1e-5)
    _check_apply(case, s, p, v, precon, coeff)


@pytest.mark.parametrize('A,C3', LAYOUTS, ids=LAYOUT_IDS)
def test_step_coefficient_regimes(lib, cuda, A, C3):
    """min(1, sqrt(c / sq)) outside the clipped regime: sq 100x below c, no trust
    region (norm_constraint=None is passed as inf), and sq < 0 all give exactly
    1.0f; coeff_out is optional."""
    case = _step_case(A, C3)
    s = case['s_free']
    assert case['sq0'] * s * s <= case['c'] / 100
    p, v, precon, coeff = _run_step(lib, case, s)
    assert coeff == F32(1.0)
    _check_apply(case, s, p, v, precon, coeff)
    # no trust region, at gradients that would be clipped 14x or more
    p_inf, v_inf, precon_inf, coeff = _run_step(lib, case, case['s_clip'], nc=float('inf'))
    assert coeff == F32(1.0)
    _check_apply(case, case['s_clip'], p_inf, v_inf, precon_inf, coeff)
    # g . precon < 0
    p, v, precon, coeff = _run_step(lib, case, case['s_clip'], inv_key='neg_a')
    gdot = float((case['grads'] * F32(case['s_clip'])).astype(np.float64) @ precon.astype(np.float64))
    assert gdot < 0 and -gdot * LR * LR >= 100 * case['c']
    assert coeff == F32(1.0) and np.isfinite(p).all() and np.isfinite(v).all()
    _check_apply(case, case['s_clip'], p, v, precon, coeff)
    assert _rel_l2(precon.astype(np.float64), -case['precon'] * case['s_clip']) <= 2e-5
    # coeff_out = NULL: the same update
    p2, v2, precon2, none = _run_step(lib, case, case['s_clip'], nc=float('inf'), want_coeff=False)
    assert none is None
    assert np.array_equal(p2, p_inf) and np.array_equal(v2, v_inf) and np.array_equal(precon2, precon_inf)


@pytest.mark.parametrize('A,C3', LAYOUTS, ids=LAYOUT_IDS)
def test_step_identity_inverses_pass_the_gradient_through(lib, cuda, A, C3):
    """The state between the cold start and the first inversion: precon == grads,
    within 2^-22 relative per element (the split operands carry 24 bits)."""
    case = _step_case(A, C3)
    p, v, precon, coeff = _run_step(lib, case, 1.0, inv_key='identity')
    g = case['grads'].astype(np.float64)
    assert np.all(np.abs(precon.astype(np.float64) - g) <= 2.0 ** -22 * np.abs(g))
    _check_apply(case, 1.0, p, v, precon, coeff)


@pytest.mark.parametrize('A,C3', LAYOUTS, ids=LAYOUT_IDS)
def test_step_independent_of_workspace_and_deterministic(lib, cuda, A, C3):
    """The step workspace holds t1 = Ainv g with rows padded to ldg, which the second
    product reads along k: a workspace full of NaN and one full of zeros give the
    same bits, all finite; two identical calls are bit-identical."""
    case = _step_case(A, C3)
    s = case['s_clip']
    a = _run_step(lib, case, s, ws_fill=float('nan'))
    b = _run_step(lib, case, s, ws_fill=0.0)
    c = _run_step(lib, case, s, ws_fill=0.0)
    for x, y, z, what in zip(a, b, c, ('params', 'velocity', 'precon', 'coeff')):
        assert np.isfinite(x).all(), what
        assert np.array_equal(x, y), (what, 'NaN workspace vs zero workspace')
        assert np.array_equal(y, z), (what, 'two identical calls')


# ---------------------------------------------------------------------------
# the optimizer, update by update
# ---------------------------------------------------------------------------
def _read_state(L, model, opt):
    st = opt.state
    h = lambda t: t.detach().cpu().numpy().astype(np.float64).copy()
    return dict(params=h(model.params), biased=h(st['biased']), velocity=h(st['velocity']),
                inv=[h(L.inverse_block(st['inv'], m)) for m in range(12)], inv_raw=st['inv'].clone(),
                accum=h(opt._cold_optimizer.optimizer._accum), cov_updates=opt.cov_updates)


def _factor_list(L, flat):
    out = []
    for f in range(11):
        n = L.din[f] if f < 5 else L.dout[f - 5]
        out.append(flat[L.stat_off[f]:L.stat_off[f] + n * n].reshape(n, n))
    return out


@pytest.mark.parametrize('start,steps', [(28, (28, 30, 31)), (38, (38, 39, 40, 41))], ids=['cold-to-kfac', 'inversion'])
def test_optimizer_trajectory_matches_oracle_step_by_step(lib, cuda, start, steps):
    """ColdStartPeriodicInvUpdateKfacOpt over consecutive updates (2 envs x 3 steps,
    A = 4, C3 = 32).  From gs = 28: the last cold update (Momentum with clip 0.5, then
    the K-FAC apply with identity inverses on the same gradients; gs += 2), then 30
    and 31 (EMA t = 1, 2, identity inverses, non-zero velocity).  From gs = 38: 38,
    39, 40 (EMA t = 3 and the inversion), 41 (EMA t = 4, the inverse of 40 reused).

    Each update is compared with ONE float64 oracle update computed from the GPU's own
    state before it (parameters, biased factors, velocity, inverses, cold accumulator)
    and the GPU's own forward of that rollout (as test_acktr_update_matches_oracle,
    for the reason given there), so no drift accumulates and the bounds stay those of
    that test: factors 2e-5 (A) / 5e-5 (G) of max-abs, inverses rel 1e-4 against the
    float64 inverse of the GPU's f32 factors, preconditioned gradient, step and
    velocity rel-L2 1e-3 per K-FAC block, coefficient rel 1e-3."""
    from actorcritic import session as sess
    N, T, A, C3 = 2, 3, 4, 32
    M = N * T
    env, model, agent, obj, gs, opt, op, params = _build(N, T)
    gs.assign(start)
    eng = model.engine
    L = eng.layout
    opt._init_state(eng)
    opt._cold_optimizer._ensure_slots(eng)
    t_cov = 0
    with sess.Session() as s:
        for step_gs in steps:
            assert gs.value == step_gs
            pre = _read_state(L, model, opt)
            assert pre['cov_updates'] == t_cov
            data = agent.interact(s)
            feed = _feed(model, data)
            fwd_out = eng.lookup_rollout(data[0])
            logits32 = fwd_out.flat_logits.cpu().numpy().copy()
            acts = fwd_out.acts
            full = dict(a1=acts.a1[:M], a2=acts.a2[:M], a3=acts.a3[:M], a4=acts.a4[:M], logits=fwd_out.flat_logits,
                        value=fwd_out.flat_value)
            full = {k: v.cpu().double().numpy() for k, v in full.items()}
            obs, act = data[0].cpu().numpy(), data[1].cpu().numpy()
            tg = np.asarray(s.run(obj.target_values, feed_dict=feed), np.float64).reshape(-1)
            s.run(op, feed_dict=feed)
            torch.cuda.synchronize()
            post = _read_state(L, model, opt)
            fac_gpu = opt.state['factors'].cpu().numpy().astype(np.float64)
            precon_gpu = opt.state['precon'].cpu().numpy().astype(np.float64)
            coeff_gpu = float(opt.state['coeff'][0])

            # one oracle update from the pre-state
            cold, cov, inv, gs_after = oracle.schedule(step_gs)
            assert opt.last_flags == (cold, cov, inv) and gs.value == gs_after, (step_gs, opt.last_flags, gs.value)
            p0 = pre['params']
            full['x'] = obs.reshape(M, 84, 84, 4).astype(np.float64) / 255.0
            full['a3f'] = full['a3'].reshape(M, -1)
            lg = oracle.a2c_loss_and_head_grads(full['logits'], full['value'], act.reshape(-1), tg)
            grads, _, afac = oracle.backward(p0, full, lg['dlogits'], lg['dvalue'], A, C3, with_a_factors=True)
            if cov:
                t_cov += 1
                g_pi, g_v, _ = oracle.sampled_head_grads(logits32, 0x4b464143, 0, step_gs)
                stats = afac + oracle.g_factors(p0, full, g_pi, g_v, A, C3)
                b_pre, b_post, f_post = _factor_list(L, pre['biased']), _factor_list(L, post['biased']), \
                    _factor_list(L, fac_gpu)
                debiased = []
                for f in range(11):
                    b_ref, d_ref = oracle.ema_update(b_pre[f], stats[f], 0.99, t_cov)
                    debiased.append(d_ref)
                    tol = 2e-5 if f < 5 else 5e-5
                    rel_b = np.abs(b_post[f] - b_ref).max() / np.abs(b_ref).max()
                    rel_f = np.abs(f_post[f] - d_ref).max() / np.abs(d_ref).max()
                    assert rel_b < tol and rel_f < tol, (step_gs, 'factor', f, t_cov, rel_b, rel_f)
                if t_cov > 1:
                    assert np.abs(pre['biased']).max() > 0
            else:
                assert np.array_equal(post['biased'], pre['biased'])
            assert post['cov_updates'] == t_cov
            if inv:
                inv_ref = oracle.damped_inverses(debiased[:5], debiased[5:], 0.01)
                gpu_f = _factor_list(L, fac_gpu)
                inv_f32 = oracle.damped_inverses(gpu_f[:5], gpu_f[5:], 0.01)
                for l in range(6):
                    for m, ref in ((2 * l, inv_f32[l][0]), (2 * l + 1, inv_f32[l][1])):
                        rel = np.abs(post['inv'][m] - ref).max() / np.abs(ref).max()
                        assert rel < 1e-4, (step_gs, 'inverse', l, m % 2, rel)
            else:
                assert torch.equal(post['inv_raw'], pre['inv_raw']), 'no inversion scheduled'
                inv_ref = [(pre['inv'][2 * l], pre['inv'][2 * l + 1]) for l in range(6)]
                if step_gs < 40:  # still the identity the optimizer starts from
                    assert all(np.array_equal(b, np.eye(b.shape[0])) for b in pre['inv'])
            p1, acc_ref = p0, pre['accum']
            if cold:  # the cold optimizer first, on the same gradients; K-FAC then sees its parameters
                p1, acc_ref = oracle.momentum_apply(p0, pre['accum'], grads, 3e-4, 0.9, 0.5)
            lr = oracle.linear_decay(0.25, 0.025, step_gs, 1000)
            new_p, vel, precon, coeff = oracle.kfac_step(p1, pre['velocity'], grads, inv_ref, lr, 0.9, 1e-4, A, C3)
            if step_gs != steps[0]:
                assert np.abs(pre['velocity']).max() > 0
            for name, lo, hi in _blocks(A, C3):
                rl2 = lambda got, ref: np.linalg.norm(got[lo:hi] - ref[lo:hi]) / np.linalg.norm(ref[lo:hi])
                e_pre = rl2(precon_gpu, precon)
                e_step = np.linalg.norm(post['params'][lo:hi] - new_p[lo:hi]) / np.linalg.norm(new_p[lo:hi] - p0[lo:hi])
                e_vel = rl2(post['velocity'], vel)
                print('gs %d block %-11s precon %.2e step %.2e velocity %.2e' % (step_gs, name, e_pre, e_step, e_vel))
                assert e_pre < 1e-3 and e_step < 1e-3 and e_vel < 1e-3, (step_gs, name, e_pre, e_step, e_vel)
                if cold:
                    assert rl2(post['accum'], acc_ref) < 1e-3, (step_gs, name, 'cold accumulator')
            if not cold:
                assert np.array_equal(post['accum'], pre['accum'])
            print('gs %d coeff gpu %.6g oracle %.6g' % (step_gs, coeff_gpu, coeff))
            assert coeff_gpu == pytest.approx(coeff, rel=1e-3)
