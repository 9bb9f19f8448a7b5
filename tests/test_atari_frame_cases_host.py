"""The claims of tests/atari_frame_cases.py, proved without a GPU: the library's own launch
plan (acmi_atari_plan) over every shape the launchers accept, the shape table, the set of
(kernel, form, mode) combinations the GPU tests run, and the oracle against the float64
area integral at the table's shapes."""
import ctypes

import numpy as np
import pytest

import atari_frame_cases as cases

PLAN_FIELDS = ('fixed3', 'max_run_y', 'max_run_x', 'band_rows', 'lds_bytes_frames', 'lds_bytes_rollout')


def _plan(lib, H, W):
    out = (ctypes.c_int32 * 6)()
    status = lib.acmi_atari_plan(H, W, out)
    return status, dict(zip(PLAN_FIELDS, out))


def test_plan_symbol_is_exported(lib):
    from actorcritic import _lib
    assert 'acmi_atari_plan' in _lib.EXPORTED and len(_lib._SIGS['acmi_atari_plan'][1]) == 3
    assert lib.acmi_abi_version() == 4  # no signature or struct changed
    assert lib.acmi_atari_plan(210, 160, None) == -1
    assert b'acmi_atari_plan' in lib.acmi_last_error()


def test_plan_over_every_accepted_shape(lib):
    """H = 84..504, W = 84..504 in steps of 4, and a margin around that (every W, sides from
    80 to 508) for the refusals: the plan succeeds exactly where the documented rule
    accepts, and on every accepted shape its runs, form, band rows and LDS bytes are what
    oracle.area_tables gives."""
    tables_bytes = (cases.BAND_ROWS + cases.OUT) * cases.AREA_RUN_BYTES
    accepted = generic = 0
    longest = 0
    for H in range(80, 509):
        for W in range(80, 509):
            status, p = _plan(lib, H, W)
            assert (status == 0) == cases.allowed(H, W), (H, W, status)
            if status != 0:
                assert status == -1, (H, W, status)
                continue
            accepted += 1
            ry, rx = cases.max_run(H), cases.max_run(W)
            assert (p['max_run_y'], p['max_run_x']) == (ry, rx), (H, W, p)
            assert p['fixed3'] == int(ry <= 3 and rx <= 3), (H, W, p)
            assert max(ry, rx) <= cases.K_MAX_TAB, (H, W, ry, rx)
            generic += not p['fixed3']
            longest = max(longest, ry, rx)
            for band in range(cases.BANDS):
                r0, r1 = cases.band_source_rows(H, band)
                assert 0 <= r0 <= r1 < H, (H, band, r0, r1)
                assert p['band_rows'] >= r1 - r0 + 1, (H, W, band, r0, r1, p)
            assert p['band_rows'] <= H, (H, W, p)
            gray = p['band_rows'] * W
            assert p['lds_bytes_frames'] == tables_bytes + gray, (H, W, p)
            assert p['lds_bytes_rollout'] == tables_bytes + cases.BAND_ROWS * cases.OUT + gray, (H, W, p)
            assert p['lds_bytes_rollout'] < cases.LDS_LIMIT, (H, W, p)
    assert (accepted, generic, longest) == (9778, 7286, 7)


def test_every_run_stays_inside_its_side_and_its_table():
    """Every run of every accepted side: at most kMaxTab entries, inside [0, side)."""
    for side in range(84, 505):
        for first, alphas in cases.tables(side):
            assert 1 <= len(alphas) <= cases.K_MAX_TAB, side
            assert 0 <= first and first + len(alphas) <= side, side


@pytest.mark.parametrize('shape', cases.SHAPES, ids=cases.SHAPE_IDS)
def test_shape_table_claims(lib, shape):
    H, W, fixed3, run_y, run_x, why = shape
    status, p = _plan(lib, H, W)
    assert status == 0 and cases.allowed(H, W), why
    assert (bool(p['fixed3']), p['max_run_y'], p['max_run_x']) == (fixed3, run_y, run_x), (why, p)
    assert (cases.max_run(H), cases.max_run(W)) == (run_y, run_x), why
    ty, tx = cases.tables(H), cases.tables(W)
    if (H, W) == (84, 88):
        assert all(len(a) == 1 and float(a[0]) == 1.0 and f == d for d, (f, a) in enumerate(ty))
    if (H, W) == (168, 160):
        assert H % 84 == 0 and W % 84 != 0
        assert all([float(x) for x in a] == [0.5, 0.5] for _, a in ty)
    if (H, W) == (256, 160):
        assert H * W == cases.MAX_AREA and not cases.allowed(H + 1, W) and not cases.allowed(H, W + 4)
    if (H, W) == (84, 484):
        assert H == cases.OUT and not cases.allowed(H, W + 4)
    if (H, W) == (487, 84):
        assert W == cases.OUT and not cases.allowed(H + 1, W)
        # the most source rows a band stages anywhere in the domain
        most = max(p2['band_rows'] for h in range(84, 505) for w in (84,) if cases.allowed(h, w)
                   for p2 in [_plan(lib, h, w)[1]])
        assert p['band_rows'] == most
    if (H, W) == (250, 160):
        assert run_y > 3 >= run_x
    if (H, W) == (100, 320):
        assert run_x > 3 >= run_y
    # runs longer in x than in y and the other way round both occur among the generic shapes
    gen = [(s[3], s[4]) for s in cases.SHAPES if not s[2]]
    assert any(a > b for a, b in gen) and any(a < b for a, b in gen)
    assert {max(a, b) for a, b in gen} >= {4, 5, 7}


def test_gpu_tests_run_both_forms_of_both_kernels_in_every_mode(lib):
    ran = set()
    for kernel, mode, H, W in cases.GPU_COMBOS:
        status, p = _plan(lib, H, W)
        assert status == 0
        ran.add((kernel, 'fixed3' if p['fixed3'] else 'generic', mode))
    want = {('frames', f, m) for f in ('fixed3', 'generic') for m in (0, 1, 2)} | \
           {('rollout', f, r) for f in ('fixed3', 'generic') for r in ('step', 'reset-and-step', 'reset', 'idle')}
    assert ran == want
    # and the run-7 shapes are there for the reset-and-step row, which reuses the LDS band
    for hw in ((487, 84), (84, 484)):
        assert ('rollout', 'reset-and-step') + hw in cases.GPU_COMBOS
    # each launch of the rollout tests holds every row
    for H, W in cases.HW:
        assert {(a, b) for a, b, _ in cases.rollout_case(H, W)['cases']} == set(cases.ROLLOUT_ROWS)


def test_frame_families():
    for H, W in cases.HW:
        fams = cases.family_frames(H, W)
        assert [n for n, _, _ in fams] == cases.FAMILY_NAMES
        by = {n: (a, b) for n, a, b in fams}
        assert all(a.shape == (H, W, 3) and a.dtype == np.uint8 and b.shape == a.shape for a, b in by.values())
        last, prev = by['max-pair']
        # neither frame dominates, in every dword of both frames
        l4, p4 = last.reshape(-1, 4), prev.reshape(-1, 4)
        assert ((l4 > p4).any(1) & (l4 < p4).any(1)).all()
        two = by['two-level'][0]
        assert set(np.unique(two)) == {0, 255}
        g = cases.oracle_gray(H, W)['two-level'][0]
        # edges inside cells: blended pixels (84x88 has the fewest: none in y, and in x an
        # edge every 5 columns under cells 1.05 wide, a fifth of the columns)
        assert ((g > 0) & (g < 255)).mean() > 0.15, (H, W)
    # the pure-channel values are those whose gray byte the rounding term decides
    for name, ch, v in cases.PURE:
        c = (4899, 9617, 1868)[ch]
        if name != 'R255' and name != 'B255':
            assert (v * c + 8192) >> 14 == ((v * c) >> 14) + 1, name
    assert [int(cases.oracle.atari_gray(np.array([255 if c == k else 0 for c in range(3)], np.uint8)))
            for k in range(3)] == [76, 150, 29]


@pytest.mark.parametrize('shape', cases.HW, ids=cases.SHAPE_IDS)
def test_oracle_stays_within_its_bound_of_the_integral(shape):
    """The bit-exact reference against the independent float64 area integral, every
    family, single frames and pairs."""
    H, W = shape
    half, f32, tab = cases.oracle_bound(H, W)
    bound = half + f32 + tab
    worst = 0.0
    for name, last, prev in cases.family_frames(H, W):
        single, pair = cases.oracle_gray(H, W)[name]
        for what, got, frame in (('single', single, last), ('pair', pair, np.maximum(last, prev))):
            ref = cases.integral_resize(cases.oracle.atari_gray(frame))
            err = np.abs(got.astype(np.float64) - ref).max()
            worst = max(worst, err)
            assert err <= bound, (shape, name, what, err, bound)
    print('{}x{}: worst |oracle - integral| - 0.5 = {:.3e}, bound - 0.5 = {:.3e}'.format(H, W, worst - 0.5, f32 + tab))


def test_integral_weights_are_an_area_mean():
    for side in (84, 88, 160, 168, 210, 256, 320, 484, 487):
        w = cases.integral_weights(side)
        assert w.shape == (84, side) and (w >= 0).all()
        assert np.abs(w.sum(1) - 1.0).max() < 1e-12
        assert np.abs(w.sum(0) - 84.0 / side).max() < 1e-12  # every source pixel counted once
