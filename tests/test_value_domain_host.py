"""The value-domain families (value_domain_cases.py) are what they claim to be, and the
cases of test_gpu_value_domain.py are not vacuous.  Runs without a GPU.

Generator claims: the game batches hold a stack straight after a reset and one straight
after a terminal, `saturating` reaches the weight-derived bound B1[c*] in float64,
`dead_conv1` gives a1 == 0, and every case's list of identically-zero float64 blocks
equals what test_gpu_bench_shard._Ref computes here on the CPU (ReLU gates from the
float64 reference's own activations).

Non-vacuity: for every case and every block (12 gradient blocks, 5 A factors, 6 G
factors, 6 forward tensors) the error of PLAIN FLOAT32 arithmetic of the reference
formulas against float64 is below a QUARTER of that block's tolerance
(test_gpu_layout_matrix.TOL).  The GPU test's escape is err < max(tol, 4 x the
plain-f32 error): with 4 x that error below tol the escape widens nothing, so it can
never be what lets a case pass.  No family had to be shrunk for this; what is chosen for
it is the seed of rand_params (test_gpu_value_domain.SEED): the first from 5 with
b1[c*] >= 0 (so that `saturating` reaches the bound) under which every reference is this
well conditioned.  Seed 7 meets the first condition and not the second: with `full`
images all 24 rows are one image, the value head is one cancelling sum of 512 terms and
the tensor's range is that one number -- plain f32 alone is at 4.3e-6 of it here (8.6e-6
on the GPU) against the forward tolerance 1e-5.
"""
import numpy as np
import pytest
import torch

import value_domain_cases as vd
from test_gpu_bench_shard import FWD_NAMES, _Ref, oracle
from test_gpu_layout_matrix import TOL
from test_gpu_value_domain import CASES, LARGE, RUNS, SEED, SMALL

CPU = torch.device('cpu')


def _cpu_errors(fams, A, C3, B):
    """What _stats_vs_float64 computes, without the kernels: the zero-reference list
    (in its order) and {(kind, block): plain-f32 error against float64}."""
    obs, params, dhead = vd.inputs(fams, A, C3, B, SEED)
    blocks = [torch.from_numpy(b) for b in oracle.unpack(params.numpy(), A, C3)]
    ref, ref32 = _Ref(blocks, A, C3, CPU), _Ref(blocks, A, C3, CPU, torch.float32)
    ins64, out64 = ref._forward(obs)
    ins32, out32 = ref32._forward(obs)
    g_pi, g_v, _ = oracle.sampled_head_grads(out64[4].float().numpy(), 0x4b464143, 0, 41)
    g_pi, g_v = torch.from_numpy(np.asarray(g_pi, np.float64)), torch.from_numpy(np.asarray(g_v, np.float64))
    dh = dhead.double()
    for r, ins in ((ref, ins64), (ref32, ins32)):
        r.add(obs, list(out64[:4]), dh[:, :A].to(r.dt), dh[:, A].to(r.dt), g_pi.to(r.dt), g_v.to(r.dt), ins=ins)
    (g64, a64, gf64), (g32, a32, gf32) = ref.result(), ref32.result()
    off, n = oracle.param_offsets(A, C3)
    zeros, errs = [], {}

    def rel(key, r32, r64):
        m = r64.abs().max().item()
        if m == 0.0:
            zeros.append(key)
            assert not r32.any().item(), key  # (plain f32 gets an exact zero too)
        else:
            errs[key] = (r32.double() - r64).abs().max().item() / m

    for blk, (o, e) in enumerate(zip(off, off[1:] + [n])):
        rel(('grad', blk), g32[o:e], g64[o:e])
    for f in range(5):
        rel(('A', f), a32[f], a64[f])
    for l in range(6):
        rel(('G', l), gf32[l], gf64[l])
    for k, o32, o64 in zip(FWD_NAMES, out32, out64):
        rel(('fwd', k), o32, o64)
    return zeros, errs, out64


def test_rand_params_layout():
    """rand_params fills oracle.param_offsets's layout: conv1 first, independent of (A, C3)."""
    p, q = vd.rand_params(4, 32, SEED), vd.rand_params(18, 64, SEED)
    assert p.numel() == oracle.param_offsets(4, 32)[1] == 865413
    assert torch.equal(p[:8192 + 32], q[:8192 + 32])


@pytest.mark.parametrize('game', ['catch', 'breakout'])
@pytest.mark.parametrize('B', [SMALL[2], LARGE[2]])
def test_game_batches_hold_reset_and_terminal_stacks(game, B):
    obs = vd.images(game, B, SEED + 10)
    assert obs.shape == (B, 84, 84, 4) and obs.dtype == torch.uint8
    assert vd.is_reset_stack(obs[0])
    assert vd.is_post_terminal_stack(obs[1])
    assert sum(not vd.is_reset_stack(o) and not vd.is_post_terminal_stack(o) for o in obs) >= B // 2  # mid-play
    assert torch.equal(obs, vd.images(game, B, SEED + 10))  # deterministic
    if game == 'catch':  # a ball of 16 and a paddle of 48 pixels per frame: > 99 % zero
        assert all(int((o[..., 3] != 0).sum()) == 64 for o in obs)
        assert (obs != 0).float().mean().item() < 0.01


def test_simple_image_families():
    B = SMALL[2]
    assert not vd.images('zeros', B, 0).any() and (vd.images('full', B, 0) == 255).all()
    one = vd.images('one_pixel', B, 3)
    assert all(int((o != 0).sum()) == 1 and int(o.max()) == 255 for o in one)
    for i, (y, x, c) in enumerate(vd.ONE_PIXEL_POSITIONS):
        assert one[i, y, x, c] == 255
    assert {c for _, _, c in vd.ONE_PIXEL_POSITIONS} == {0, 1, 2, 3}
    # (40, 82, 1): conv1's output column ow reads x = 4 ow .. 4 ow + 7 -- only ow = 19
    assert [ow for ow in range(20) if 4 * ow <= 82 <= 4 * ow + 7] == [19]
    b = vd.images('binary', B, 3)
    assert sorted(b.unique().tolist()) == [0, vd.BINARY_LEVEL] and 0.4 < (b != 0).float().mean().item() < 0.6


@pytest.mark.parametrize('wfam', ['base', 'conv1*2^6'])
@pytest.mark.parametrize('size', [SMALL, LARGE])
def test_saturating_reaches_the_conv1_bound(wfam, size):
    A, C3, B = size
    params = vd.weights(wfam, A, C3, SEED)
    B1, cstar, mass = vd.conv1_bound(params, A, C3)
    b1 = vd.blocks(params, A, C3)[1]
    assert b1[cstar] >= 0  # SEED is chosen for this: else a1 reaches mass + b1 < B1 only
    assert cstar == int(mass.argmax())
    obs = vd.images('saturating', B, SEED + 10, params, A, C3)
    blocks = [torch.from_numpy(b) for b in oracle.unpack(params.numpy(), A, C3)]
    a1 = _Ref(blocks, A, C3, CPU)._forward(obs)[1][0]
    assert abs(a1[0, 0, 0, cstar].item() - B1[cstar].item()) <= 1e-12 * B1[cstar].item()
    assert a1[0::2, 0, 0, cstar].min().item() == a1[:, :, :, cstar].max().item()  # the channel's maximum
    assert not obs[0::2, 8:].any() and not obs[0::2, :, 8:].any()
    assert vd.is_reset_stack(obs[1]) or vd.is_post_terminal_stack(obs[1])  # the other half is Catch


def test_weight_families():
    A, C3 = 4, 32
    base = vd.blocks(vd.weights('base', A, C3, SEED), A, C3)
    assert sorted(vd.WEIGHT_FAMILIES) == sorted(set(vd.WEIGHT_FAMILIES)) and len(vd.WEIGHT_FAMILIES) == 14
    for fam in vd.WEIGHT_FAMILIES:
        b = vd.blocks(vd.weights(fam, A, C3, SEED), A, C3)
        changed = [i for i in range(12) if not torch.equal(b[i], base[i])]
        if '*2^' in fam:
            l = vd.LAYERS.index(fam.split('*2^')[0])
            k = float(fam.split('*2^')[1])
            assert changed == [2 * l, 2 * l + 1]
            assert torch.equal(b[2 * l], base[2 * l] * 2.0 ** k) and torch.equal(b[2 * l + 1], base[2 * l + 1] * 2.0 ** k)
        elif fam == 'outlier':
            assert changed == [0, 2, 4]
            for i in changed:
                assert int((b[i] != base[i]).sum()) == 1
                assert b[i].max().item() == 2.0 ** vd.OUTLIER_LOG2 * base[i].abs().max().item()
        elif fam == 'heavy_tail':
            assert changed == [0, 2, 4, 6, 8, 10]
            r = (b[6] / base[6]).log()
            assert abs(r.std().item() - vd.HEAVY_TAIL_SIGMA) < 0.02 and abs(r.mean().item()) < 0.02
        elif fam == 'dead_half':
            assert changed == [0, 1] and (b[0][:, :16] <= 0).all() and (b[1][:16] <= 0).all()
            assert torch.equal(b[0][:, 16:], base[0][:, 16:]) and (b[0][:, 16:] > 0).any()
        elif fam == 'dead_conv1':
            assert changed == [0, 1] and (b[0] <= 0).all() and (b[1] <= 0).all()
            B1, _, _ = vd.conv1_bound(vd.weights(fam, A, C3, SEED), A, C3)
            assert not B1.any()  # the weight-derived a1 bound is exactly 0
        elif fam == 'zero_bias':
            assert changed == [1, 3, 5, 7, 9, 11] and not any(b[i].any() for i in changed)


def test_dhead_families():
    B, A = 24, 4
    base = vd.dheads('base', B, A, 5)
    assert torch.equal(base, torch.randn(B, A + 1, generator=torch.Generator().manual_seed(5)) / B)
    d = vd.dheads('outlier_row', B, A, 5)
    assert torch.equal(d[B // 3], base[B // 3] * 4096.0) and int((d != base).any(1).sum()) == 1
    d = vd.dheads('half_zero', B, A, 5)
    assert not d[0::2].any() and torch.equal(d[1::2], base[1::2])
    assert not vd.dheads('zero', B, A, 5).any()
    d = vd.dheads('value_only', B, A, 5)
    assert not d[:, :A].any() and torch.equal(d[:, A], base[:, A])
    d = vd.dheads('policy_only', B, A, 5)
    assert not d[:, A].any() and torch.equal(d[:, :A], base[:, :A])
    assert torch.equal(vd.dheads('*2^-40', B, A, 5), base * 2.0 ** -40)
    assert torch.equal(vd.dheads('*2^20', B, A, 5), base * 2.0 ** 20)


def test_case_list_covers_the_families():
    names = [c[0] for c in CASES]
    fams = [c[1] for c in CASES]
    for img in vd.IMAGE_FAMILIES[:-1]:
        assert (img, 'base', 'base') in fams
    for w in vd.WEIGHT_FAMILIES:
        assert ('catch', w, 'base') in fams and ('random', w, 'base') in fams
    for d in vd.DHEAD_FAMILIES:
        assert ('catch', 'base', d) in fams
    for corner in (('zeros', 'zero_bias', 'base'), ('zeros', 'dead_conv1', 'base'), ('full', 'dead_half', 'base'),
                   ('saturating', 'conv1*2^6', 'base'), ('zeros', 'base', 'zero')):
        assert corner in fams
    assert len(set(names)) == len(names) == len(set(fams))
    assert sum(1 for r in RUNS if r[2] == LARGE) == 6


_HOST_RUNS = [r for r in RUNS if r[0] == r[1][0] or r[2] == LARGE]  # each (case, size) once: modes do not matter here


@pytest.mark.parametrize('run', _HOST_RUNS, ids=[r[0] for r in _HOST_RUNS])
def test_zero_lists_and_plain_f32_is_within_tolerance(run):
    """The case's zero-reference list is the float64 reference's, dead_conv1 gives
    a1 == 0, and plain float32 arithmetic alone is below a quarter of every block's
    tolerance (the non-vacuity condition of the module docstring)."""
    rid, (name, fams, zeros), (A, C3, B), _ = run
    got_zeros, errs, out64 = _cpu_errors(fams, A, C3, B)
    assert got_zeros == zeros, (got_zeros, zeros)
    if fams[1] == 'dead_conv1':
        assert not out64[0].any()
    assert len(errs) + len(zeros) == 12 + 5 + 6 + 6
    worst = max(errs.items(), key=lambda kv: kv[1] / TOL[kv[0][0]])
    print('%s worst plain-f32 error / tolerance: %s %.2e / %.0e' % (rid, worst[0], worst[1], TOL[worst[0][0]]))
    bad = {k: v for k, v in errs.items() if not v < TOL[k[0]] / 4}
    assert not bad, bad
