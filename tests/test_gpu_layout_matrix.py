"""The update kernels over the whole (A, C3) domain of include/acmi.h against float64.

acmi.h promises 1 <= num_actions <= 64 and conv3_filters in {32, 64} to every entry
point that takes a net.  Each case here runs acmi_forward, acmi_backward with
statistics and acmi_kfac_output_stats once (test_gpu_bench_shard._stats_vs_float64:
torch.float64 on the GPU over the same formulas, the chains on the GPU forward's
ReLU gates) with the workspace, gradients, statistics and d1..d4 filled with NaN
first, and checks all 12 parameter-gradient blocks, 5 A factors, 6 G factors and the
6 forward tensors (a1..a4, logits, value).

What the layouts reach that (4, 32) and (18, 64) do not: the head Gram's wide branch
(A + 1 > 32, np = roundup4(A + 1): 36 at A = 33, 68 at A = 64, neither 64 nor 512),
the tiled finalize with sub = 64 != np = 68 (A = 64), the heads' weight gradient with
33..65 dY columns, heads_dx_kernel / heads_kernel past 32 actions, the boundary
A + 1 = 32 | 33 on both sides (A = 31, 32), and a 1 x 1 policy block whose sampled
gradient p - onehot is exactly 0 (A = 1).  C3 = 64: conv3's band plan with 64 outputs,
the 3137-wide fc4 A factor, the 64 x 64 conv3 G factor.  The batch edges: one image,
one past the band reduction's 16-image stage, both sides of the 64-image tile and of
the split-tower boundary, and more than two tiles.

Tolerances (max-abs error over max-abs value per block): forward
1e-5, gradients and A factors 2e-5, G factors 5e-5, each with the bench-shard test's
escape err < max(tol, 4 x the plain-float32 error of the same formulas).  Every use of
the escape is printed ("ESCAPE ...").  A block whose float64 reference is identically
zero must be exactly zero on the GPU; only the policy head's G factor at A = 1 may be
such a block.

acmi_backward takes head gradients with a row stride that is a multiple of 4
(ldh % 4 == 0, zero padded: float4 loads): A + 1 itself where that is one (A = 31,
63), the next multiple elsewhere, a wider one (40 at A = 33) in one case, and
ldh = A + 1 = 34 is refused with ACMI_ERR_ARG before anything is enqueued
(test_backward_refuses_unpadded_head_gradients).

Cases that needed the plain-f32 escape (kernel error / plain-f32 error): none.  The
worst errors measured over all 28 cases: forward 2.3e-6, gradients 4.8e-6, A factors
1.3e-6, G factors 3.3e-7.
"""
import ctypes

import pytest
import torch

from actorcritic import _lib
from test_gpu_bench_shard import FWD_NAMES, _stats_vs_float64
from test_gpu_kernels import alloc_acts, rand_params

pytestmark = pytest.mark.gpu

TOL = {'fwd': 1e-5, 'grad': 2e-5, 'A': 2e-5, 'G': 5e-5}
X3, F32 = _lib.GEMM_X3, _lib.GEMM_F32
BAND, PATCHES = _lib.CONV_STATS_BAND, _lib.CONV_STATS_PATCHES


def _case(A, C3, B=24, **kw):
    return (A, C3, B, kw)


def _modes(gemm, conv_stats, use_prep, masks=True):
    return dict(gemm_mode=gemm, forward_mode=_lib.FWD_F32, conv_stats_mode=conv_stats, use_prep=use_prep, masks=masks)


_LAYOUT_CASES = [_case(A, C3) for A, C3 in [(1, 32), (5, 64), (18, 64), (31, 32), (32, 64), (33, 32), (63, 64),
                                            (64, 32), (64, 64)]] + [_case(33, 32, ldh=40)]
_MODE_CASES = ([_case(18, 64, **_modes(g, c, p)) for g in (X3, F32) for c in (BAND, PATCHES) for p in (True, False)]
               + [_case(18, 64, **_modes(X3, BAND, True, masks=False)),
                  _case(33, 32, **_modes(F32, PATCHES, False)),
                  _case(33, 32, **_modes(X3, BAND, True)),
                  _case(33, 32, **_modes(X3, BAND, True, masks=False))])
_BATCH_CASES = [_case(18, 64, B) for B in (1, 2, 17, 63, 65, 129)]


def _id(case):
    A, C3, B, kw = case
    s = 'a%d-c%d-b%d' % (A, C3, B)
    if 'ldh' in kw:
        s += '-ldh%d' % kw['ldh']
    if 'gemm_mode' in kw:
        s += '-%s-%s-%s' % ('x3' if kw['gemm_mode'] == X3 else 'f32',
                            'band' if kw['conv_stats_mode'] == BAND else 'patches',
                            'prep' if kw['use_prep'] else 'noprep')
        if not kw['masks']:
            s += '-nomasks'
    return s


_CASES = _LAYOUT_CASES + _MODE_CASES + _BATCH_CASES


@pytest.mark.parametrize('case', _CASES, ids=[_id(c) for c in _CASES])
def test_update_matches_float64(lib, cuda, case):
    """Forward, backward with statistics and output statistics of one (A, C3, B,
    modes) case, every block against float64 (module docstring)."""
    A, C3, B, kw = case
    params = rand_params(A, C3, cuda, seed=100 + A + C3)
    zero_refs = []
    errs = _stats_vs_float64(lib, cuda, B, params, seed=7000 + 64 * B + A, A=A, C3=C3, fill=float('nan'),
                             zero_refs=zero_refs, **kw)
    want = ([('grad', b) for b in range(12)] + [('A', f) for f in range(5)] + [('G', l) for l in range(6)] +
            [('fwd', k) for k in FWD_NAMES])
    assert sorted(errs) == sorted(want)
    # the sampled policy gradient p - onehot(y) is exactly 0 with one action: that G
    # factor (one element) must be exactly 0, and no other reference block is zero
    assert zero_refs == ([('G', 4)] if A == 1 else []), zero_refs
    fails = []
    for k, (v, v32) in errs.items():
        tol = TOL[k[0]]
        if k in zero_refs:
            if v != 0.0:
                fails.append((k, 'must be exactly zero'))
        elif not v < tol:
            print('ESCAPE %s %s kernel %.2e plain f32 %.2e' % (_id(case), k, v, v32))
            if not v < max(tol, 4 * v32):
                fails.append((k, v, v32))
    assert not fails, fails


def test_backward_refuses_unpadded_head_gradients(lib, cuda):
    """acmi_backward at (33, 32) with ldh = A + 1 = 34, not a multiple of 4: the
    kernels read dhead rows as float4, so the call returns ACMI_ERR_ARG with nothing
    enqueued -- sentinel-filled gradients, statistics and d4 are unchanged after a
    synchronise."""
    A, C3, B = 33, 32, 3
    params = rand_params(A, C3, cuda, seed=1)
    obs = torch.zeros(B, 84, 84, 4, dtype=torch.uint8, device=cuda)
    t, acts = alloc_acts(B, A, C3, cuda)
    net = _lib.Net(A, C3, params.data_ptr())
    st = _lib.stream_handle()
    _lib.call('acmi_forward', ctypes.byref(net), _lib.ptr(obs), 84 * 84 * 4, B, ctypes.byref(acts), 1, st)
    ldh = A + 1
    dhead = torch.zeros(B, ldh, device=cuda)
    tot = ctypes.c_int64()
    _lib.call('acmi_kfac_layout', A, C3, None, None, None, ctypes.byref(tot))
    full = lambda *s: torch.full(s, 7.0, device=cuda)
    d = [full(B, 20, 20, 32), full(B, 9, 9, 64), full(B, 7, 7, C3), full(B, 512)]
    ws = full(int(lib.acmi_backward_ws_floats(B, A, C3)))
    grads, astat = full(params.numel()), full(tot.value)
    bwd = _lib.Bwd(*[x.data_ptr() for x in d], dhead.data_ptr(), ldh)
    rc = lib.acmi_backward(ctypes.byref(net), _lib.ptr(obs), 84 * 84 * 4, B, ctypes.byref(acts), ctypes.byref(bwd),
                           _lib.ptr(grads), _lib.ptr(astat), _lib.ptr(ws), ws.numel(), st)
    torch.cuda.synchronize()
    assert rc == _lib.ERR_ARG, rc
    assert b'multiple of 4' in lib.acmi_last_error()
    for x in d + [ws, grads, astat]:
        assert (x == 7.0).all()
