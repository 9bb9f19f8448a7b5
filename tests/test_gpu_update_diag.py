"""Update diagnostics on the GPU, the kernels: acmi_diag_value, acmi_diag_policy and
acmi_diag_segments against the numpy restatements (actorcritic.update_diag.host_*) on the same
float32 inputs.

Tolerances, derived and not tuned.  Sums of value and segment terms: any-order double summation of
M exactly representable terms errs by at most (M - 1) 2^-53 sum|term|; the tests assert 2x that bound
(restatement and kernel may both err), computed here from the float64 terms.  KL and H: 1e-12
absolute per counted row (about 64 one-ulp exp/log differences at |logp| <~ 20, with a margin of
roughly 10).  Every call runs twice: the same bytes in, the same bytes out."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64
U = 2.0 ** -53
ROW_TOL = 1e-12


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int64)


def _guarded(n, fill):
    return torch.full((n + GUARD,), fill, dtype=torch.float64, device='cuda')


# -- value ----------------------------------------------------------------------------------------
def _device_value(lib, v, y, grp, G):
    """One acmi_diag_value with guards behind ws and acc, twice -> (acc [G][6], bad_envs) numpy."""
    from actorcritic import _lib
    N, T = v.shape
    need = int(lib.acmi_diag_ws_doubles(N * T, 0))
    outs = []
    for fill in (12345.0, -777.0):  # (the output is overwritten whatever it held)
        ws, acc = _guarded(need, float('nan')), _guarded(6 * G, fill)
        bad = torch.zeros(1, dtype=torch.int32, device='cuda')
        v_d, y_d, grp_d = _dev(v), _dev(y), None if grp is None else _dev(grp)
        _lib.call('acmi_diag_value', _lib.ptr(v_d), _lib.ptr(y_d), _lib.ptr(grp_d), N, T, G, _lib.ptr(ws), _lib.ptr(acc), _lib.ptr(bad), _lib.stream_handle())
        torch.cuda.synchronize()
        assert torch.isnan(ws[need:]).all() and bool((acc[6 * G:] == fill).all())
        assert np.array_equal(v_d.cpu().numpy().view(np.uint32), v.view(np.uint32))  # the inputs are only read
        outs.append((acc[:6 * G].clone(), int(bad.item())))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and outs[0][1] == outs[1][1]
    return outs[0][0].reshape(G, 6).cpu().numpy(), outs[0][1]


def _check_value(acc, v, y, grp, G):
    """Every column of every group within 2 (M - 1) 2^-53 sum|term| of the restatement."""
    from actorcritic import update_diag as ud
    want, _ = ud.host_value_diag(v, y, grp, G)
    N, T = v.shape
    g_of = np.zeros(N, np.int64) if grp is None else np.asarray(grp).astype(np.int64)
    v64, y64 = v.astype(np.float64), y.astype(np.float64)
    e = y64 - v64
    assert np.array_equal(acc[:, 0], want[:, 0])
    for g in range(G):
        sel = g_of == g
        M = int(sel.sum()) * T
        assert acc[g, 0] == M
        for col, terms in ((1, v64[sel]), (2, y64[sel]), (3, y64[sel] ** 2), (4, e[sel]), (5, e[sel] * e[sel])):
            bound = 2 * max(M - 1, 0) * U * np.abs(terms).sum()
            err = abs(acc[g, col] - want[g, col])
            print('value N={} T={} g={} col={} M={} err={:.3e} bound={:.3e}'.format(N, T, g, col, M, err, bound))
            assert err <= bound, (g, col, err, bound)
    return want


VALUE_SHAPES = [(1, 1, 1), (3, 5, 1), (33, 8, 3), (5, 64, 2)]


@pytest.mark.parametrize('N,T,G', VALUE_SHAPES, ids=['{}x{}x{}'.format(*s) for s in VALUE_SHAPES])
def test_value_kernel_against_the_restatement(lib, cuda, N, T, G):
    """(33, 8, 3): group 1 is empty and the 264 rows cross a 256-row block; (1, 1, 1): one term, exact."""
    from actorcritic import update_diag as ud
    rng = np.random.RandomState(10 * N + T)
    v, y = rng.randn(N, T).astype(np.float32), (rng.randn(N, T) * 2.5 + 0.5).astype(np.float32)
    grp = (np.arange(N) % G).astype(np.uint8)
    if G == 3:
        grp[grp == 1] = 2
    acc, bad = _device_value(lib, v, y, grp, G)
    want = _check_value(acc, v, y, grp, G)
    assert bad == 0
    if G == 3:
        assert acc[1].tolist() == [0.0] * 6
    ev, want_ev = ud.explained_variance(acc.sum(axis=0)), ud.explained_variance(want.sum(axis=0))
    assert np.isnan(ev) and np.isnan(want_ev) if N * T == 1 else abs(ev - want_ev) <= 1e-12  # (one row: Var(y) = 0)
    if G == 1:  # no groups: every env in group 0
        assert np.array_equal(_device_value(lib, v, y, None, 1)[0], acc)


def test_value_kernel_skips_an_env_with_a_bad_group_id(lib, cuda):
    rng = np.random.RandomState(5)
    N, T, G = 6, 4, 2
    v, y = rng.randn(N, T).astype(np.float32), rng.randn(N, T).astype(np.float32)
    grp = np.array([0, 1, 0, 2, 1, 0], np.uint8)
    acc, bad = _device_value(lib, v, y, grp, G)
    assert bad == 1 and acc[:, 0].tolist() == [12.0, 8.0]
    keep = [0, 1, 2, 4, 5]
    _check_value(acc, v[keep], y[keep], grp[keep], G)
    # that env adds nothing: its values may be anything
    v[3], y[3] = np.float32(1e30), np.float32(np.nan)
    assert np.array_equal(_device_value(lib, v, y, grp, G)[0], acc)


# -- policy ---------------------------------------------------------------------------------------
def _device_policy(lib, zo, zn, legal, grp, N, T, A, G):
    """One acmi_diag_policy on [M][ld] matrices with guards, twice -> (acc [G][4], bad_envs, bad_rows)."""
    from actorcritic import _lib
    need = int(lib.acmi_diag_ws_doubles(N * T, 0))
    outs = []
    for fill in (12345.0, -777.0):
        ws, acc = _guarded(need, float('nan')), _guarded(4 * G, fill)
        bad = torch.zeros(2, dtype=torch.int32, device='cuda')
        zo_d, zn_d = _dev(zo), _dev(zn)
        legal_d, grp_d = None if legal is None else _dev(legal), None if grp is None else _dev(grp)
        _lib.call('acmi_diag_policy', _lib.ptr(zo_d), zo.shape[1], _lib.ptr(zn_d), zn.shape[1],
                  _lib.ptr(legal_d), _lib.ptr(grp_d), N, T, A, G, _lib.ptr(ws), _lib.ptr(acc), _lib.ptr(bad[:1]), _lib.ptr(bad[1:]),
                  _lib.stream_handle())
        torch.cuda.synchronize()
        assert torch.isnan(ws[need:]).all() and bool((acc[4 * G:] == fill).all())
        outs.append((acc[:4 * G].clone(), bad.tolist()))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and outs[0][1] == outs[1][1]
    return (outs[0][0].reshape(G, 4).cpu().numpy(),) + tuple(outs[0][1])


def _check_policy(got, zo, zn, legal, grp, T, A, G):
    from actorcritic import update_diag as ud
    acc, bad_envs, bad_rows = got
    want, want_envs, want_rows = ud.host_policy_diag(zo, zn, legal, grp, G, T, A)
    assert (bad_envs, bad_rows) == (want_envs, want_rows)
    assert np.array_equal(acc[:, 0], want[:, 0])
    for g in range(G):
        n = want[g, 0]
        for col, name in ((1, 'KL'), (2, 'H'), (3, 'max KL')):
            if n == 0:
                assert acc[g, col] == want[g, col]  # 0, 0, -inf
                continue
            err = abs(acc[g, col] - want[g, col])
            tol = ROW_TOL * (1 if col == 3 else n)
            print('policy M={} A={} g={} {} n={:.0f} err={:.3e} per row {:.3e} tol/row={:.1e}'.format(
                zo.shape[0], A, g, name, n, err, err / (1 if col == 3 else n), ROW_TOL))
            assert err <= tol, (g, name, err, tol)
    return want


def _logits(M, A, ld, seed, scale=3.0):
    """Two [M][ld] float32 matrices: the second a small step from the first (an update's KL is
    small) on half of the rows and an unrelated draw on the others; the padding holds NaNs."""
    rng = np.random.RandomState(seed)
    zo = np.full((M, ld), np.nan, np.float32)
    zn = zo.copy()
    zo[:, :A] = rng.randn(M, A) * scale
    step = np.where(np.arange(M)[:, None] % 2 == 0, 0.01, 2.0) * rng.randn(M, A)
    zn[:, :A] = zo[:, :A] + step.astype(np.float32)
    return zo, zn


def _masks(M, A, seed):
    rng = np.random.RandomState(seed)
    hi = (1 << A) if A < 32 else (1 << 32)
    words = rng.randint(1, hi, M, dtype=np.int64).astype(np.uint32)
    words[0] = hi - 1          # all legal
    words[-1] = 1 << (A - 1)   # one action: KL = H = 0
    return words


POLICY_CASES = [(3, 3, False), (3, 3, True), (4, 4, False), (4, 4, True), (18, 18, True), (32, 32, True),
                (64, 64, False), (3, 8, False), (3, 8, True), (4, 7, False), (4, 7, True)]


@pytest.mark.parametrize('A,ld,masked', POLICY_CASES,
                         ids=['A{}ld{}{}'.format(a, l, 'm' if m else '') for a, l, m in POLICY_CASES])
def test_policy_kernel_over_actions_and_strides(lib, cuda, A, ld, masked):
    N, T, G = 5, 3, 2
    M = N * T
    zo, zn = _logits(M, A, ld, seed=A * 100 + ld)
    legal = _masks(M, A, seed=A) if masked else None
    grp = (np.arange(N) % G).astype(np.uint8)
    got = _device_policy(lib, zo, zn, legal, grp, N, T, A, G)
    want = _check_policy(got, zo, zn, legal, grp, T, A, G)
    assert want[:, 0].tolist() == [9.0, 6.0] and got[0][:, 1].min() > 0.0 and got[0][:, 3].min() > 0.0


@pytest.mark.parametrize('N,T', [(1, 1), (37, 1), (33, 8)], ids=['M1', 'M37', 'M264'])
def test_policy_kernel_over_rows(lib, cuda, N, T):
    A, G = 6, 3 if N > 1 else 1
    zo, zn = _logits(N * T, A, A, seed=N)
    legal = _masks(N * T, A, seed=N + 1)
    grp = (np.arange(N) % G).astype(np.uint8)
    if N == 33:
        grp[grp == 1] = 2  # an empty group: (0, 0, 0, -inf)
    got = _device_policy(lib, zo, zn, legal, grp, N, T, A, G)
    want = _check_policy(got, zo, zn, legal, grp, T, A, G)
    if N == 33:
        assert got[0][1].tolist() == [0.0, 0.0, 0.0, -np.inf] and want[:, 0].sum() == 264
    if N == 1:  # no groups: every env in group 0
        assert np.array_equal(_device_policy(lib, zo, zn, legal, None, N, T, A, 1)[0], got[0])


def test_policy_kernel_special_cases(lib, cuda):
    N, T, A, G = 6, 4, 5, 2
    M = N * T
    zo, zn = _logits(M, A, A, seed=77)
    grp = (np.arange(N) % G).astype(np.uint8)
    legal = _masks(M, A, seed=78)
    # identical old and new: the KL sums and maxima are exactly zero
    acc, _, _ = _device_policy(lib, zo, zo.copy(), legal, grp, N, T, A, G)
    assert (acc[:, 1] == 0.0).all() and (acc[:, 3] == 0.0).all() and (acc[:, 0] == 12).all() and (acc[:, 2] > 0).all()
    # all-legal masks: the bytes of the unmasked call (bits at or above A are ignored)
    plain = _device_policy(lib, zo, zn, None, grp, N, T, A, G)
    for word in ((1 << A) - 1, 0xFFFFFFFF):
        full = _device_policy(lib, zo, zn, np.full(M, word, np.uint32), grp, N, T, A, G)
        assert np.array_equal(full[0].view(np.uint64), plain[0].view(np.uint64)) and full[1:] == plain[1:]
    # illegal columns at +-1e30: the bytes of the same call with those columns at 0
    wild_o, wild_n, zero_o, zero_n = zo.copy(), zn.copy(), zo.copy(), zn.copy()
    for m in range(M):
        for a in range(A):
            if not (int(legal[m]) >> a) & 1:
                wild_o[m, a], wild_n[m, a] = (1e30, -1e30) if (m + a) % 2 else (-1e30, 1e30)
                zero_o[m, a] = zero_n[m, a] = 0.0
    wild = _device_policy(lib, wild_o, wild_n, legal, grp, N, T, A, G)
    zero = _device_policy(lib, zero_o, zero_n, legal, grp, N, T, A, G)
    assert np.array_equal(wild[0].view(np.uint64), zero[0].view(np.uint64)) and wild[1:] == zero[1:] == (0, 0)
    _check_policy(wild, wild_o, wild_n, legal, grp, T, A, G)
    # bad rows: an empty S, a NaN in old (at an illegal action: all A logits count), an inf in new
    legal[2] = 0
    legal[9] = 0b00110
    zo[9, 0] = np.nan
    zn[17, 3] = np.inf
    grp[5] = 9  # and an env outside the groups: rows 20..23 add nothing
    got = _device_policy(lib, zo, zn, legal, grp, N, T, A, G)
    want = _check_policy(got, zo, zn, legal, grp, T, A, G)
    assert got[1:] == (1, 3) and want[:, 0].tolist() == [9.0, 8.0]


# -- segments -------------------------------------------------------------------------------------
def _device_segments(lib, x, y, off):
    from actorcritic import _lib
    S = len(off) - 1
    need = int(lib.acmi_diag_ws_doubles(0, S))
    outs = []
    for fill in (12345.0, -777.0):
        ws, out = _guarded(need, float('nan')), _guarded(4 * S, fill)
        x_d, y_d, off_d = _dev(x), None if y is None else _dev(y), _dev(np.asarray(off, np.int64))
        _lib.call('acmi_diag_segments', _lib.ptr(x_d), _lib.ptr(y_d), _lib.ptr(off_d), S, _lib.ptr(ws),
                  _lib.ptr(out), _lib.stream_handle())
        torch.cuda.synchronize()
        assert torch.isnan(ws[need:]).all() and bool((out[4 * S:] == fill).all())
        outs.append(out[:4 * S].clone())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    return outs[0].reshape(S, 4).cpu().numpy()


def _check_segments(out, x, y, off):
    from actorcritic import update_diag as ud
    want = ud.host_segment_sums(x, y, off)
    x64 = x.astype(np.float64)
    y64 = np.zeros_like(x64) if y is None else y.astype(np.float64)
    for s in range(len(off) - 1):
        a, b = x64[off[s]:off[s + 1]], y64[off[s]:off[s + 1]]
        M = a.size
        for col, terms in enumerate((a * a, b * b, a * b, (a - b) * (a - b))):
            bound = 2 * max(M - 1, 0) * U * np.abs(terms).sum()
            err = abs(out[s, col] - want[s, col])
            print('segment s={} M={} col={} err={:.3e} bound={:.3e}'.format(s, M, col, err, bound))
            assert err <= bound, (s, col, err, bound)
    return want


OFFSETS = [0, 1, 64, 129, 386, 4483, 4483, 12000]


@pytest.mark.parametrize('with_y', [True, False], ids=['xy', 'x'])
def test_segment_kernel_against_the_restatement(lib, cuda, with_y):
    """A 1-element segment (exact), segments that straddle 64 and 256, an empty one (zeros) and one
    of several slices; the elements behind the last offset are never read (NaNs)."""
    rng = np.random.RandomState(3)
    x = np.full(12000 + 100, np.nan, np.float32)
    y = x.copy()
    x[:12000], y[:12000] = rng.randn(12000) * 2, rng.randn(12000)
    out = _device_segments(lib, x, y if with_y else None, OFFSETS)
    want = _check_segments(out, x, y if with_y else None, OFFSETS)
    assert out[5].tolist() == [0.0] * 4 and np.array_equal(out[0], want[0]) and np.isfinite(out).all()
    if not with_y:
        assert not out[:, 1:3].any() and np.array_equal(out[:, 3], out[:, 0])


def test_segment_kernel_on_the_parameter_layout(lib, cuda):
    import ctypes
    from actorcritic import _lib
    A, C3 = 4, 32
    n = int(lib.acmi_param_count(A, C3))
    off = (ctypes.c_int64 * 12)()
    _lib.call('acmi_param_offsets', A, C3, off)
    off = list(off) + [n]
    rng = np.random.RandomState(4)
    x, y = (rng.randn(n) * 0.05).astype(np.float32), (rng.randn(n) * 0.05).astype(np.float32)
    out = _device_segments(lib, x, y, off)
    _check_segments(out, x, y, off)
    d = x.astype(np.float64) - y.astype(np.float64)
    assert abs(np.sqrt(out[:, 3].sum()) - np.linalg.norm(d)) <= 1e-12 * np.linalg.norm(d)
