"""The update kernels over their VALUE domain against float64.

Every other accuracy test of the hot path draws He-Gaussian weights, uniformly random
bytes and randn / B head gradients.  The arithmetic depends on values by design: the
f16x2 split operands take one power-of-two scale per tensor from a bound (max |W|, the
published max |dY|, the positive weight mass for activations, which assumes nothing
about the images and is loose), conv1 reads pixels as f16 subnormals with an exact
integer A factor, the bf16 forward mode rounds once to f16 against the same bounds.
The cases here (value_domain_cases.py) are what training on the device games feeds the
kernels -- Catch and Breakout frame stacks (> 99 % zero; one frame four times after a
reset; three zero channels after a terminal), black and white frames, single pixels,
weights that are no longer He-Gaussian (one layer scaled by 2^+-6, one outlier weight
per conv layer, log-normal magnitudes, dead channels, zero biases) and head gradients
with an outlier row, zero rows, zero columns and global scales 2^-40 .. 2^20.

Each case is one test_gpu_bench_shard._stats_vs_float64 call (forward, backward with
statistics, output statistics; outputs NaN-filled first): 12 gradient blocks, 5 A
factors, 6 G factors and 6 forward tensors against torch.float64 on the GPU.
Tolerances are test_gpu_layout_matrix.TOL (max-abs error over max-abs
value per block) with its escape err < max(tol, 4 x plain-f32 error), every use printed
("ESCAPE ...").  test_value_domain_host.py shows on the CPU that plain float32
arithmetic alone holds every block of every case below a quarter of its tolerance, so
the escape can never be what lets a case pass.  Each case lists the blocks whose float64
reference is identically zero; the harness must report exactly those, and they must be
exactly zero on the GPU.

Cases that needed the plain-f32 escape (kernel error / plain-f32 error): none.  The
worst errors measured over all 56 runs: forward 5.5e-6 (`zeros` at (18, 64, 65), the
value), gradients 1.5e-5 (`outlier-catch` at (18, 64, 65): the conv1 and conv2 bias
gradients, plain f32 2.8e-6; the next is `binary`'s conv1 weight gradient, 6.5e-6), A
factors 2.3e-6, G factors 4.3e-7.  bf16 forward, worst over the image families: 9.0e-4
of range.  The policy and value heads' sampled G factors at saturated logits: 1.9e-7.

What the cases found (measured on the parent of the commit that added them, SEED 7):
  * acmi_categorical / acmi_a2c_loss / acmi_ppo_loss rounded lse = mx + logf(se) to f32
    before subtracting it from a logit: at a common offset of +-1e4 the entropy was off
    by 2.4e-4 (A = 2) .. 1.5e-3 (A = 64) against the bound rtol 1e-5 + 1e-6
    (test_head_kernels_at_saturated_logits[2, 18, 64] failed).  Fixed in csrc/rl.hip:
    log pi = (z - mx) - logf(se) on rows with |mx| >= 8; below that lse's rounding is
    within the bound and the rows keep their form, and runs their bits.
  * the sampled head gradient p_y - 1.f cancels on a saturated row: the policy head's G
    factor was off by 2.3e-4 (conv2*2^6-catch) .. 5.5e-3 (fc4*2^6-random) of its range,
    and 1.0 .. 1.2 (all of it) in conv3*2^6-catch / -random and fc4*2^6-catch, bound 5e-5
    (those cases and conv1*2^6-random, saturating-conv1*2^6 failed).  Fixed in
    csrc/backward.hpp: -(the other actions' sum) / se where the others hold less than 2^-7
    of the sum (elsewhere the subtraction is within 2^-17 of the column and stays, so
    unsaturated runs reproduce bit for bit); oracle.sampled_head_grads takes that form
    on every row.
  * conv1 reads pixels as f16 subnormals, which the MFMA adder does not normalise: a
    byte n carries about 14 + log2(n) bits in a sum.  conv1's weight gradient over 24
    images of bytes {0, n}: 1.2e-4 of range at n = 1, 5.7e-5 at 2, 2.6e-5 at 4 (bound
    2e-5), 6.5e-6 at 16, 1.3e-6 at 255; plain f32 2e-6 .. 3e-6 throughout; the f32 gemm
    mode 4e-7 throughout.  A documented limit (f16x2.hpp u8x8_to_f16),
    not fixed: `binary` runs at {0, 16} (value_domain_cases.BINARY_LEVEL).  Its exact
    checks do not depend on the level: the integer A factor is within 2e-9 of the Gram.
"""
import ctypes

import numpy as np
import pytest
import torch

import value_domain_cases as vd
from actorcritic import _lib
from test_gpu_bench_shard import FWD_NAMES, _Ref, _stats_vs_float64, oracle
from test_gpu_kernels import alloc_acts, rand_params
from test_gpu_layout_matrix import BAND, F32, PATCHES, TOL, X3, _modes

pytestmark = pytest.mark.gpu

SEED = 8  # of rand_params; test_value_domain_host.py shows what it was chosen for


def Z(grad=(), G=(), fwd=()):
    """A zero-reference list in the harness's order: gradient blocks, G factors,
    forward tensors (an A factor is never zero: its homogeneous corner is 1)."""
    return [('grad', b) for b in grad] + [('G', l) for l in G] + [('fwd', k) for k in fwd]


# gradient blocks: 0 W1, 1 b1, 2 W2, 3 b2, 4 W3, 5 b3, 6 W4, 7 b4, 8 Wpi, 9 bpi, 10 Wv, 11 bv
# G factors: 0..3 conv1, conv2, conv3, fc4 (the sampled chain's d1..d4), 4 policy, 5 value
NONE = Z()
# black frames: every conv1 patch is zero, so dW1 = P^T d1 = 0 (a1 = relu(b1) is not)
BLACK = Z(grad=[0])
# no conv1 channel fires: a1 = 0, its mask stops d1 (dW1, db1, conv1's G factor), and
# conv2's patches are zero (dW2)
DEAD1 = Z(grad=[0, 1, 2], G=[0], fwd=['a1'])
# black frames and no bias: every activation, logit and value is 0; every mask stops
# its gradient (d1..d4 = 0 in both chains); only the head biases see dhead
# logits so far apart (every row's gap > 2000 > 745) that softmax is a one-hot in
# float64 too: the sampled policy gradient p - onehot(y) is exactly 0
ONE_HOT = Z(G=[4])
_WEIGHT_ZEROS = {('dead_conv1', 'catch'): DEAD1, ('dead_conv1', 'random'): DEAD1, ('heavy_tail', 'catch'): ONE_HOT,
                 ('heavy_tail', 'random'): ONE_HOT, ('outlier', 'random'): ONE_HOT}
ALL_DARK = Z(grad=[0, 1, 2, 3, 4, 5, 6, 7, 8, 10], G=[0, 1, 2, 3], fwd=FWD_NAMES)

_IMG = [(img, (img, 'base', 'base'), BLACK if img == 'zeros' else NONE)
        for img in ('zeros', 'full', 'catch', 'breakout', 'one_pixel', 'binary', 'saturating')]
_WGT = [('%s-%s' % (w, img), (img, w, 'base'), _WEIGHT_ZEROS.get((w, img), NONE))
        for w in vd.WEIGHT_FAMILIES for img in ('catch', 'random') if (w, img) != ('base', 'catch')]
_DHEAD_ZEROS = {'zero': Z(grad=range(12)), 'value_only': Z(grad=[8, 9]), 'policy_only': Z(grad=[10, 11])}
_DH = [('dhead-%s' % d, ('catch', 'base', d), _DHEAD_ZEROS.get(d, NONE)) for d in vd.DHEAD_FAMILIES if d != 'base']
_CORNERS = [
    ('zeros-zero_bias', ('zeros', 'zero_bias', 'base'), ALL_DARK),
    ('zeros-dead_conv1', ('zeros', 'dead_conv1', 'base'), DEAD1),
    ('full-dead_half', ('full', 'dead_half', 'base'), NONE),
    ('saturating-conv1*2^6', ('saturating', 'conv1*2^6', 'base'), NONE),
    ('zeros-dhead-zero', ('zeros', 'base', 'zero'), Z(grad=range(12))),
]
CASES = _IMG + _WGT + _DH + _CORNERS  # (name, (images, weights, dhead), zero references)
_BY_NAME = {c[0]: c for c in CASES}
assert len(_BY_NAME) == len(CASES)

SMALL, LARGE = (4, 32, 24), (18, 64, 65)  # (A, C3, B): inside one tile | past the 64-image tile, split tower
DEFAULT = _modes(X3, BAND, True)
LARGE_CASES = ('catch', 'zeros', 'outlier-catch', 'heavy_tail-catch', 'dhead-outlier_row', 'saturating')
MODE_CASES = ('catch', 'outlier-catch')
OTHER_MODES = [('noprep', _modes(X3, BAND, False)), ('f32-patches', _modes(F32, PATCHES, True))]

# (id, case, (A, C3, B), modes)
RUNS = ([(c[0], c, SMALL, DEFAULT) for c in CASES] +
        [('a18-c64-b65-' + n, _BY_NAME[n], LARGE, DEFAULT) for n in LARGE_CASES] +
        [('%s-%s' % (m, n), _BY_NAME[n], SMALL, kw) for n in MODE_CASES for m, kw in OTHER_MODES])


def test_rand_params_restated(lib, cuda):
    """value_domain_cases.rand_params (no library) draws test_gpu_kernels.rand_params."""
    for A, C3 in ((4, 32), (18, 64)):
        assert torch.equal(vd.rand_params(A, C3, SEED), rand_params(A, C3, 'cpu', seed=SEED))


@pytest.mark.parametrize('run', RUNS, ids=[r[0] for r in RUNS])
def test_update_matches_float64(lib, cuda, run):
    """Forward, backward with statistics and output statistics of one case, every
    block against float64 (module docstring), and the checks that are exact."""
    rid, (name, fams, zeros), (A, C3, B), kw = run
    obs, params, dhead = vd.inputs(fams, A, C3, B, SEED)
    zero_refs, out = [], {}
    errs = _stats_vs_float64(lib, cuda, B, params.to(cuda), A=A, C3=C3, fill=float('nan'), zero_refs=zero_refs,
                             obs=obs, dhead=dhead, out=out, **kw)
    want = ([('grad', b) for b in range(12)] + [('A', f) for f in range(5)] + [('G', l) for l in range(6)] +
            [('fwd', k) for k in FWD_NAMES])
    assert sorted(errs) == sorted(want)
    assert zero_refs == zeros, (zero_refs, zeros)
    fails = []
    for k, (v, v32) in errs.items():
        tol = TOL[k[0]]
        if k in zero_refs:
            if v != 0.0:
                fails.append((k, 'must be exactly zero'))
        elif not v < tol:
            print('ESCAPE %s %s kernel %.2e plain f32 %.2e' % (rid, k, v, v32))
            if not v < max(tol, 4 * v32):
                fails.append((k, v, v32))
    for kind in ('fwd', 'grad', 'A', 'G'):
        print('WORST %s %s %.2e' % (rid, kind, max(v for k, (v, _) in errs.items() if k[0] == kind)))
    # every factor is exactly symmetric
    for kind in ('afac', 'gfac'):
        for i, F in enumerate(out[kind]):
            if not torch.equal(F, F.t()):
                fails.append((kind, i, 'not symmetric'))
    # conv1's A factor is integer arithmetic on the bytes
    img = fams[0]
    A0 = out['afac'][0]
    if img == 'full':  # every patch entry and the homogeneous coordinate are 1
        if not (A0 == 1.0).all():
            fails.append(('A0', 'full', (A0 - 1.0).abs().max().item()))
    if img == 'zeros':
        want0 = torch.zeros_like(A0)
        want0[256, 256] = 1.0
        if not torch.equal(A0, want0):
            fails.append(('A0', 'zeros', (A0 - want0).abs().max().item()))
    if img in ('binary', 'one_pixel'):  # against the exact integer Gram, within 1e-6 of range
        p = obs.double().unfold(1, 8, 4).unfold(2, 8, 4).permute(0, 1, 2, 4, 5, 3).reshape(-1, 256)
        pb = torch.cat([p, torch.full((p.shape[0], 1), 255.0, dtype=torch.float64)], 1)
        gram = (pb.t() @ pb) / (65025.0 * p.shape[0])  # integer sums: exact in float64
        e = ((A0.cpu().double() - gram).abs().max() / gram.abs().max()).item()
        print('A0 vs the integer Gram %s %.2e' % (rid, e))
        if not e < 1e-6:
            fails.append(('A0', img, e))
    if img == 'saturating':  # a1 reaches its weight-derived bound
        B1, cstar, _ = vd.conv1_bound(params, A, C3)
        a1 = out['acts']['a1'][0, 0, 0, cstar].item()
        ref = out['fwd64']['a1'][0, 0, 0, cstar].item()
        amax = out['fwd64']['a1'].abs().max().item()
        print('saturating %s a1 %.9g float64 %.9g B1 %.9g' % (rid, a1, ref, B1[cstar].item()))
        if not abs(ref - B1[cstar].item()) <= 1e-12 * B1[cstar].item():
            fails.append(('saturating', 'the float64 a1 is not the bound', ref, B1[cstar].item()))
        if not abs(a1 - B1[cstar].item()) < TOL['fwd'] * amax:
            fails.append(('saturating', a1, B1[cstar].item()))
    assert not fails, fails


@pytest.mark.parametrize('img', ['zeros', 'full', 'catch', 'breakout', 'one_pixel', 'binary', 'saturating'])
def test_bf16_forward_over_image_families(lib, cuda, img):
    """The bf16 forward mode (one f16 rounding against the same loose bounds) on every
    image family with the base weights, forward only: each of a1..a4, logits and value
    within 1e-2 of its float64 range (test_bf16_forward_mode's bound); a tensor that is
    identically zero in float64 is exactly zero.  (The wide-range weight families are
    not run: acmi.h says the mode loses them.)"""
    A, C3, B = SMALL
    obs, params, _ = vd.inputs((img, 'base', 'base'), A, C3, B, SEED)
    obs, params = obs.to(cuda), params.to(cuda)
    prep = torch.empty(int(lib.acmi_conv_prep_bytes(C3)), dtype=torch.uint8, device=cuda)
    net = _lib.Net(A, C3, params.data_ptr(), prep.data_ptr())
    _lib.call('acmi_conv_prepare', ctypes.byref(net), _lib.ptr(prep), _lib.stream_handle())
    from actorcritic._engine import Layout
    ref = _Ref(Layout(A, C3).split(params), A, C3, cuda)._forward(obs)[1]
    prev = lib.acmi_get_forward_mode()
    try:
        _lib.call('acmi_set_forward_mode', _lib.FWD_BF16)
        t, acts = alloc_acts(B, A, C3, cuda)
        for v in t.values():
            v.fill_(float('nan'))
        _lib.call('acmi_forward', ctypes.byref(net), _lib.ptr(obs), 84 * 84 * 4, B, ctypes.byref(acts), 1,
                  _lib.stream_handle())
        torch.cuda.synchronize()
    finally:
        _lib.call('acmi_set_forward_mode', prev)
    for name, r in zip(FWD_NAMES, ref):
        got = t[name].double().reshape(r.shape)
        assert torch.isfinite(got).all(), name
        m = r.abs().max().item()
        if m == 0.0:
            assert not got.any().item(), name
            continue
        err = (got - r).abs().max().item() / m
        print(name, 'bf16 forward rel err %.2e' % err)
        assert err < 1e-2, (name, err)


# ---------------------------------------------------------------------------
# the head kernels at saturated logits
# ---------------------------------------------------------------------------
M_HEAD = 300  # one past a 256-row block
LOGIT_FAMILIES = ('equal', 'ahead30', 'ahead87', 'ahead200', 'offset+1e4', 'offset-1e4')
U_FAMILIES = ('zero', 'below1', 'boundary', 'random')


def _head_inputs(A):
    """Row r: logit family r % 6 over u family (r // 6) % 4; odd groups of 24 rows add
    0.5 N(0,1) to the logits (the equal family stays exactly equal).  u 'boundary' is
    k / A, which on the equal family is exactly the cumulative sum after k actions."""
    rng = np.random.default_rng(100 + A)
    z = np.zeros((M_HEAD, A), np.float32)
    u = np.zeros(M_HEAD, np.float32)
    for r in range(M_HEAD):
        fam, uf = LOGIT_FAMILIES[r % 6], U_FAMILIES[(r // 6) % 4]
        if (r // 24) % 2 and fam != 'equal':
            z[r] = 0.5 * rng.standard_normal(A)
        if fam.startswith('ahead'):
            z[r, (r // 6) % A] += float(fam[5:])
        elif fam.startswith('offset'):
            z[r] += float(fam[6:])
        elif fam == 'equal':
            z[r] = (-3.0, 0.0, 7.5)[(r // 6) % 3]
        u[r] = {'zero': 0.0, 'below1': np.nextafter(np.float32(1), np.float32(0)),
                'boundary': np.float32(((r // 24) % A) / A), 'random': rng.random()}[uf]
    return z, u, rng


def _padded(z, ld, pad, cuda):
    t = torch.full((z.shape[0], ld), pad, dtype=torch.float32)
    t[:, :z.shape[1]] = torch.from_numpy(z)
    return t.to(cuda)


@pytest.mark.parametrize('A', [1, 2, 18, 64])
def test_head_kernels_at_saturated_logits(lib, cuda, A):
    """acmi_sample_actions (given uniforms), acmi_categorical, acmi_a2c_loss,
    acmi_ppo_loss and the sampled head gradients of acmi_kfac_output_stats (through
    oracle.sampled_head_grads: its draw is the sampler's) on M = 300 rows of logits with
    ld = A + 3: all equal, one ahead by 30 / 87 (exp(-87) is an f32 subnormal) / 200
    (exp(-200) is 0), a common offset of +-1e4; u = 0, the largest float below 1 and
    exactly on a cumulative boundary.  NaN in the padding columns changes no byte of
    any output.  The sampler equals oracle.sample_f32; entropy, log-probability, losses
    and dhead stay within test_a2c_loss_and_categorical_match_oracle's bounds of float64;
    an entropy that is 0 in float64 is finite and >= 0."""
    M, ld = M_HEAD, A + 3
    z, u, rng = _head_inputs(A)
    z64 = z.astype(np.float64)
    values = rng.standard_normal(M).astype(np.float32)
    targets = rng.standard_normal(M).astype(np.float32)
    actions = rng.integers(0, A, M).astype(np.int32)
    adv = (targets - values).astype(np.float32)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(cuda)
    U, V, AC, TG, AD = dev(u), dev(values), dev(actions), dev(targets), dev(adv)
    st = _lib.stream_handle()
    ldh = (A + 1 + 3) // 4 * 4
    res = {}
    for pad in (float('nan'), 0.0):
        L = _padded(z, ld, pad, cuda)
        o = {}
        o['y'] = torch.full((M,), -7, dtype=torch.int32, device=cuda)
        bad = torch.zeros(1, dtype=torch.int32, device=cuda)
        _lib.call('acmi_sample_actions', _lib.ptr(L), ld, M, A, 0, 0, 0, _lib.ptr(U), 0, _lib.ptr(o['y']), _lib.ptr(bad),
                  st)
        o['ent'] = torch.full((M,), float('nan'), device=cuda)
        o['lp'] = torch.full((M,), float('nan'), device=cuda)
        _lib.call('acmi_categorical', _lib.ptr(L), ld, M, A, _lib.ptr(AC), _lib.ptr(o['ent']), _lib.ptr(o['lp']), st)
        o['dh'] = torch.zeros(M, ldh, device=cuda)
        o['loss'] = torch.zeros(4, device=cuda)
        ws = torch.zeros(int(lib.acmi_a2c_loss_ws_floats(M)), device=cuda)
        _lib.call('acmi_a2c_loss', _lib.ptr(L), ld, _lib.ptr(V), _lib.ptr(AC), _lib.ptr(TG), _lib.ptr(AD), M, A, 0.01,
                  0.5, 1.0, _lib.ptr(o['dh']), ldh, _lib.ptr(ws), _lib.ptr(o['loss']), st)
        o['pdh'] = torch.zeros(M, ldh, device=cuda)
        o['ploss'] = torch.zeros(4, device=cuda)
        o['pclip'] = torch.zeros(1, device=cuda)
        ws2 = torch.zeros(int(lib.acmi_ppo_loss_ws_floats(M)), device=cuda)
        _lib.call('acmi_ppo_loss', _lib.ptr(L), ld, _lib.ptr(V), _lib.ptr(AC), _lib.ptr(o['lp']), None, _lib.ptr(TG),
                  _lib.ptr(AD), M, A, 0.2, 0.0, 0.01, 0.5, 1.0, _lib.ptr(o['pdh']), ldh, _lib.ptr(ws2),
                  _lib.ptr(o['ploss']), _lib.ptr(o['pclip']), st)
        torch.cuda.synchronize()
        assert int(bad.item()) == 0
        res[pad == 0.0] = {k: v.cpu() for k, v in o.items()}
    got, zero_pad = res[False], res[True]
    for k in got:  # the padding influences nothing: byte-identical outputs
        assert got[k].numpy().tobytes() == zero_pad[k].numpy().tobytes(), k

    np.testing.assert_array_equal(got['y'].numpy(), oracle.sample_f32(z, u))
    H64, lp64 = oracle.entropy(z64), oracle.log_softmax(z64)[np.arange(M), actions]
    ent = got['ent'].numpy()
    assert np.isfinite(ent).all()
    assert (ent[H64 < 1e-30] >= 0).all(), ent[H64 < 1e-30].min()  # (all of A = 1; the 200-ahead rows)
    np.testing.assert_allclose(ent, H64, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got['lp'].numpy(), lp64, rtol=1e-5, atol=1e-6)
    ref = oracle.a2c_loss_and_head_grads(z64, values, actions, targets)
    # PPO with old_logp of the same logits: r == 1, the surrogate is adv itself, the approximate KL 0
    ppo_policy_loss = -(np.mean(adv.astype(np.float64)) + 0.01 * ref['mean_entropy'])
    assert got['ploss'][3].item() == 0.0
    for key, dh_key, pl in (('loss', 'dh', ref['policy_loss']), ('ploss', 'pdh', ppo_policy_loss)):
        loss, dh = got[key].numpy(), got[dh_key].numpy()
        assert loss[0] == pytest.approx(pl, rel=1e-5, abs=1e-7), key
        assert loss[1] == pytest.approx(ref['baseline_loss'], rel=1e-5), key
        assert loss[2] == pytest.approx(ref['mean_entropy'], rel=1e-5), key
        np.testing.assert_allclose(dh[:, :A], ref['dlogits'], rtol=1e-4, atol=1e-9, err_msg=key)
        np.testing.assert_allclose(dh[:, A], ref['dvalue'], rtol=1e-5, atol=1e-10, err_msg=key)
        assert not dh[:, A + 1:].any()
    assert got['pclip'].item() == 0.0

    # the sampled head gradients (the G factors of the two heads) on the same logits:
    # zero activations, so the chain below the heads is idle
    C3 = 32
    params = rand_params(A, C3, cuda, seed=SEED)
    net = _lib.Net(A, C3, params.data_ptr())
    so = (ctypes.c_int64 * 11)()
    tot = ctypes.c_int64()
    _lib.call('acmi_kfac_layout', A, C3, None, None, so, ctypes.byref(tot))
    seed_s, counter = 0x4b464143, 17
    heads = {}
    for pad in (float('nan'), 0.0):
        L = _padded(z, ld, pad, cuda)
        t, acts = alloc_acts(M, A, C3, cuda)
        acts.logits, acts.ld_logits = L.data_ptr(), ld
        d = [torch.zeros(M, 20, 20, 32, device=cuda), torch.zeros(M, 9, 9, 64, device=cuda),
             torch.zeros(M, 7, 7, C3, device=cuda), torch.zeros(M, 512, device=cuda)]
        dh = torch.zeros(M, ldh, device=cuda)
        bwd = _lib.Bwd(*[x.data_ptr() for x in d], dh.data_ptr(), ldh)
        ws = torch.full((int(lib.acmi_backward_ws_floats(M, A, C3)),), float('nan'), device=cuda)
        gstat = torch.full((tot.value,), float('nan'), device=cuda)
        _lib.call('acmi_kfac_output_stats', ctypes.byref(net), M, ctypes.byref(acts), ctypes.byref(bwd), seed_s, 0,
                  counter, _lib.ptr(gstat), _lib.ptr(ws), ws.numel(), st)
        torch.cuda.synchronize()
        heads[pad == 0.0] = (gstat[so[9]:so[9] + A * A].cpu().reshape(A, A), gstat[so[10]:so[10] + 1].cpu())
    for a, b in zip(heads[False], heads[True]):
        assert a.numpy().tobytes() == b.numpy().tobytes()
    g_pi, g_v, _ = oracle.sampled_head_grads(z, seed_s, 0, counter)
    for got_f, g in zip(heads[False], (g_pi, g_v[:, None])):
        ref_f = g.T @ g / M
        assert torch.equal(got_f, got_f.t())
        if np.abs(ref_f).max() == 0.0:  # one action: p - onehot(y) = 0
            assert A == 1 and not got_f.any().item()
            continue
        e = np.abs(got_f.double().numpy() - ref_f).max() / np.abs(ref_f).max()
        print('sampled head G factor A=%d rel err %.2e' % (A, e))
        assert e < TOL['G'], e
