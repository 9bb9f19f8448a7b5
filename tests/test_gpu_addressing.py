"""acmi_forward, acmi_forward_strided, acmi_backward, acmi_backward_stacked and
acmi_kfac_output_stats over their stride and alignment domain (include/acmi.h,
"Addressing"; the cases and the buffer layout: tests/addressing_cases.py).

Every buffer of a case -- observations, a1..a4, logits, value, m1..m3, the forward
workspace, head gradients, d1..d4 of both chains, gradients, statistics, backward
workspaces -- is one allocation with 256 guard elements before and after it and a
gap between strided rows, filled beforehand with NaN (floats), 0x7fffffff (masks) or
255 (observations: a patch load that runs past a row's 28224 bytes changes the
result).  After the calls every guard and gap element must hold its fill, bit for bit.

Two kinds of assertion (DESIGN.md "Addressing tests"):
 * against float64 (test_gpu_bench_shard._Ref, the chains on the GPU forward's ReLU
   gates): forward 1e-5, gradients and A factors 2e-5, G factors 5e-5 of each block's
   range, each with the layout matrix's escape err < max(tol, 4 x plain-f32 error),
   every use printed ("ESCAPE ..."); the 16-bit forward 1e-2 of each tensor's range;
 * bit identity with the dense call of the same case (same B, net, modes, images,
   head gradients, seed / counter) wherever both launch the same kernels -- every
   layout of a case whose forward takes the same path as the dense call's -- and, for
   the alignments that send a prepared bf16x3 net to the per-layer kernels, with the
   img_stride = 28224 + 8 call of the same case (so +4 against +8, base + 4 against
   base + 8).  conv1's A factor (exact integer sums of the observations) is
   bit-identical to the dense call's whichever forward ran.

No case passes an address the contract refuses to a kernel: the refused calls of
test_refused_calls_launch_nothing return before anything is enqueued, which is what
they assert.

Measured on an MI355X, the worst over all cases (forward / gradients / A / G): fused
tower 2.0e-6 / 3.7e-6 / 1.9e-6 / 3.1e-7, per-layer kernels 1.8e-6 / 3.7e-6 / 1.5e-6 /
3.8e-7, 16-bit forward 7.0e-4 of range.  Cases that needed the plain-f32 escape: the
one logit column at (A, C3, B) = (1, 32, 3), ld_logits 1 and 4 (the same forward:
1.20e-5, plain f32 3.39e-6).
"""
import ctypes

import numpy as np
import pytest
import torch

import addressing_cases as ac
from actorcritic import _lib
from test_gpu_bench_shard import FWD_NAMES, _Ref, _rel, oracle
from test_gpu_kernels import rand_params

pytestmark = pytest.mark.gpu

TOL = {'fwd': 1e-5, 'grad': 2e-5, 'A': 2e-5, 'G': 5e-5}
NAN_BITS, INT_FILL, OBS_FILL = 0x7fc00000, 0x7fffffff, 255
SEED_S, COUNTER = 0x4b464143, 41
MASKS = ('m1', 'm2', 'm3')


class Buf(object):
    """n rows of per_row elements, stride apart, off elements into one sentinel-filled
    allocation (addressing_cases: GUARD, row_start, buffer_elems).  kind: 'f32' (NaN),
    'i32' (0x7fffffff) or 'u8' (255)."""

    def __init__(self, dev, kind, n, per_row, stride=None, off=0):
        stride = per_row if stride is None else stride
        self.kind, self.n, self.per_row, self.stride, self.off = kind, n, per_row, stride, off
        self.fill = {'f32': NAN_BITS, 'i32': INT_FILL, 'u8': OBS_FILL}[kind]
        self.raw = torch.full((ac.buffer_elems(n, per_row, stride, off),), self.fill,
                              dtype=torch.uint8 if kind == 'u8' else torch.int32, device=dev)
        assert self.raw.data_ptr() % 16 == 0
        self.start = ac.row_start(0, stride, off)
        self.ptr = self.raw.data_ptr() + self.start * self.raw.element_size()

    def get(self):
        """The rows as a dense tensor (float32 for 'f32')."""
        v = self.raw.as_strided((self.n, self.per_row), (self.stride, 1), self.start).contiguous()
        return v.view(torch.float32) if self.kind == 'f32' else v

    def put(self, x):
        x = x.reshape(self.n, self.per_row)
        self.raw.as_strided((self.n, self.per_row), (self.stride, 1), self.start).copy_(
            x.view(torch.int32) if self.kind == 'f32' else x)

    def guards_intact(self):
        end = self.start + (self.n - 1) * self.stride + self.per_row
        parts = [self.raw[:self.start], self.raw[end:]]
        if self.n > 1 and self.stride > self.per_row:
            parts.append(self.raw.as_strided((self.n - 1, self.stride - self.per_row), (self.stride, 1),
                                             self.start + self.per_row))
        return not any(bool((p != self.fill).any()) for p in parts)

    def untouched(self):
        return not bool((self.raw != self.fill).any())


_PARAMS, _INPUTS, _RUNS = {}, {}, {}


def _params(A, C3, dev):
    if (A, C3) not in _PARAMS:
        _PARAMS[(A, C3)] = rand_params(A, C3, dev, seed=100 + A + C3)
    return _PARAMS[(A, C3)]


def _inputs(A, C3, B, dev):
    """The images and head gradients of every case with this (A, C3, B)."""
    if (A, C3, B) not in _INPUTS:
        gen = torch.Generator(device=dev).manual_seed(9000 + 64 * B + A)
        obs = torch.randint(0, 256, (B, 84, 84, 4), generator=gen, device=dev, dtype=torch.uint8)
        dhead = torch.randn(B, A + 1, generator=gen, device=dev) / B
        _INPUTS[(A, C3, B)] = (obs, dhead)
    return _INPUTS[(A, C3, B)]


def _mode(m):
    return 0 if m is None else m + 1


def run(lib, dev, c):
    """The calls of one case on guarded buffers: {name: dense tensor} of everything
    they wrote, after the guard check.  One run per distinct case (memoised)."""
    if c in _RUNS:
        return _RUNS[c]
    assert not ac.case_violations(c), (c, ac.case_violations(c))
    A, C3, B = c.A, c.C3, c.B
    params = _params(A, C3, dev)
    obs, dhead_in = _inputs(A, C3, B, dev)
    ldl = A if c.ldl is None else c.ldl
    bufs = {'obs': Buf(dev, 'u8', B, ac.OBS_BYTES, c.stride, c.off)}
    bufs['obs'].put(obs)
    for k, (per, stride) in ac.act_rows(A, C3, ldl, c.act).items():
        bufs[k] = Buf(dev, 'i32' if k in MASKS else 'f32', B, per, stride)
    acts = _lib.Acts(*[bufs[k].ptr for k in FWD_NAMES], ldl)
    if c.value == 'null':
        acts.value = None
    acts.m1, acts.m2, acts.m3 = bufs['m1'].ptr, bufs['m2'].ptr, bufs['m3'].ptr
    if c.fws:
        n = int(lib.acmi_forward_ws_floats(B))
        bufs['fws'] = Buf(dev, 'f32', 1, n)
        acts.ws, acts.ws_floats = bufs['fws'].ptr, n
    prep = None
    if c.prep:
        prep = torch.empty(int(lib.acmi_conv_prep_bytes(C3)), dtype=torch.uint8, device=dev)
    net = _lib.Net(A, C3, params.data_ptr(), prep.data_ptr() if c.prep else None, _mode(c.gemm),
                   _mode(_lib.FWD_BF16 if c.bf16 else None), _mode(c.conv_stats))
    st = _lib.stream_handle()
    if c.prep:
        _lib.call('acmi_conv_prepare', ctypes.byref(net), _lib.ptr(prep), st)
    obs_p = ctypes.c_void_p(bufs['obs'].ptr)
    if c.act == 1:
        _lib.call('acmi_forward', ctypes.byref(net), obs_p, c.stride, B, ctypes.byref(acts), c.want_value, st)
    else:
        _lib.call('acmi_forward_strided', ctypes.byref(net), obs_p, c.stride, B, ctypes.byref(acts), c.want_value,
                  c.act, st)
    if c.bwd:
        assert c.act == 1
        ldh = (A + 1 + 3) // 4 * 4
        din, so, tot = (ctypes.c_int64 * 6)(), (ctypes.c_int64 * 11)(), ctypes.c_int64()
        _lib.call('acmi_kfac_layout', A, C3, din, None, so, ctypes.byref(tot))
        need = int(lib.acmi_backward_ws_floats(B, A, C3))
        dims = dict(d1=ac.A1_FLOATS, d2=81 * 64, d3=49 * C3, d4=512)
        for sfx in ('', '_s'):
            for k, per in dims.items():
                bufs[k + sfx] = Buf(dev, 'f32', 1, B * per)
            bufs['dhead' + sfx] = Buf(dev, 'f32', B, ldh)
            bufs['dhead' + sfx].put(torch.zeros(B, ldh, device=dev))
            bufs['ws' + sfx] = Buf(dev, 'f32', 1, need)
        dh = torch.zeros(B, ldh, device=dev)
        dh[:, :A + 1] = dhead_in
        bufs['dhead'].put(dh)
        for k, n in (('grads', params.numel()), ('astat', tot.value), ('gstat', tot.value)):
            bufs[k] = Buf(dev, 'f32', 1, n)
        bwd, bwd_s = [_lib.Bwd(*[bufs[k + sfx].ptr for k in ('d1', 'd2', 'd3', 'd4', 'dhead')], ldh)
                      for sfx in ('', '_s')]
        P = lambda k: ctypes.c_void_p(bufs[k].ptr)
        if c.bwd == 'stacked':
            _lib.call('acmi_backward_stacked', ctypes.byref(net), obs_p, c.stride, B, ctypes.byref(acts),
                      ctypes.byref(bwd), P('grads'), P('astat'), P('ws'), need, ctypes.byref(bwd_s), SEED_S, 0, COUNTER,
                      P('ws_s'), need, st)
            _lib.call('acmi_kfac_output_stats_finish', ctypes.byref(net), B, ctypes.byref(acts), ctypes.byref(bwd_s),
                      P('gstat'), P('ws_s'), need, st)
        else:
            _lib.call('acmi_backward', ctypes.byref(net), obs_p, c.stride, B, ctypes.byref(acts), ctypes.byref(bwd),
                      P('grads'), P('astat') if c.bwd == 'stats' else None, P('ws'), need, st)
            _lib.call('acmi_kfac_output_stats', ctypes.byref(net), B, ctypes.byref(acts), ctypes.byref(bwd_s), SEED_S,
                      0, COUNTER, P('gstat'), P('ws_s'), need, st)
    torch.cuda.synchronize()
    bad = [k for k, b in bufs.items() if not b.guards_intact()]
    assert not bad, ('guard or gap elements overwritten', ac.case_id(c), bad)
    if c.value == 'guard' or (c.value == 'null' and not c.want_value):
        assert bufs['value'].untouched(), 'value written with want_value = 0'
    if c.bwd == 'nostats':
        assert bufs['astat'].untouched()
    out = {k: bufs[k].get() for k in FWD_NAMES + MASKS if not (k == 'value' and not c.want_value)}
    if c.bwd:
        out.update({k: bufs[k].get().reshape(-1) for k in ('grads', 'd1', 'd2', 'd3', 'd4')})
        nf = list(din)[:5] + [32, 64, C3, 512, A, 1]
        fac = lambda k, f: bufs[k].get().reshape(-1)[so[f]:so[f] + nf[f] ** 2].reshape(nf[f], nf[f])
        if c.bwd != 'nostats':
            out['afac'] = [fac('astat', f) for f in range(5)]
        out['gfac'] = [fac('gstat', 5 + l) for l in range(6)]
    _RUNS[c] = out
    return out


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def reference_case(c):
    """The case whose bytes c must reproduce: the dense call where both forwards take
    the same path, else the img_stride = 28224 + 8 call (module docstring)."""
    d = ac.dense(c)
    return d if ac.uses_tower(c) == ac.uses_tower(d) else d._replace(stride=ac.OBS_BYTES + 8)


def check_bits(lib, dev, c, out):
    ref_c = reference_case(c)
    d = run(lib, dev, ac.dense(c))
    if 'afac' in out:  # exact integer sums of the observations, whichever forward ran
        assert _same_bits(out['afac'][0], d['afac'][0]), 'conv1 A factor differs from the dense call'
    if ref_c == c:
        return
    ref = run(lib, dev, ref_c)
    diff = []
    for k, v in out.items():
        if c.fws and k in ('a4', 'logits', 'value'):
            continue  # split-K fc4 + heads: other kernels than the call without a workspace
        pairs = zip(v, ref[k]) if isinstance(v, list) else [(v, ref[k])]
        diff += [(k, i) for i, (x, y) in enumerate(pairs) if not _same_bits(x, y)]
    assert not diff, ('not bit-identical to', ac.case_id(ref_c), diff)


_WORST, _FWD64 = {}, {}


def check_float64(dev, c, out):
    """Every block the case wrote against float64, by the layout matrix's rule."""
    from actorcritic._engine import Layout
    A, C3, B = c.A, c.C3, c.B
    L = Layout(A, C3)
    params = _params(A, C3, dev)
    obs, dhead = _inputs(A, C3, B, dev)
    ref = _Ref(L.split(params), A, C3, dev)
    ref32 = _Ref(L.split(params), A, C3, dev, torch.float32)
    if (A, C3, B) not in _FWD64:  # computed once per (A, C3, B), left unchanged
        _FWD64[(A, C3, B)] = ref._forward(obs) + ref32._forward(obs)
    ins, o64, ins32, o32 = _FWD64[(A, C3, B)]
    errs, zero = {}, []

    def rel(key, got, r64, r32):
        if r64.abs().max().item() == 0.0:
            zero.append(key)
            return (0.0 if not got.any().item() else float('inf'), 0.0)
        return (_rel(got.reshape(r64.shape), r64), _rel(r32, r64))

    for k, r64, r32 in zip(FWD_NAMES, o64, o32):
        if k in out:
            errs[('fwd', k)] = rel(('fwd', k), out[k], r64, r32)
    if c.bwd:
        g_pi, g_v, _ = oracle.sampled_head_grads(out['logits'].cpu().numpy(), SEED_S, 0, COUNTER)
        g_pi = torch.from_numpy(np.asarray(g_pi, np.float64)).to(dev)
        g_v = torch.from_numpy(np.asarray(g_v, np.float64)).to(dev)
        dh = dhead.double()
        shapes = ((B, 20, 20, 32), (B, 9, 9, 64), (B, 7, 7, C3), (B, 512))
        gpu_acts = [out[k].reshape(s) for k, s in zip(FWD_NAMES, shapes)]
        for r, i in ((ref, ins), (ref32, ins32)):
            r.add(obs, gpu_acts, dh[:, :A].to(r.dt), dh[:, A].to(r.dt), g_pi.to(r.dt), g_v.to(r.dt), ins=i)
        g64, a64, gf64 = ref.result()
        g32, a32, gf32 = ref32.result()
        ends = L.offsets[1:] + [L.nparams]
        for blk, (o, e) in enumerate(zip(L.offsets, ends)):
            errs[('grad', blk)] = rel(('grad', blk), out['grads'][o:e], g64[o:e], g32[o:e])
        for f in range(5 if 'afac' in out else 0):
            errs[('A', f)] = rel(('A', f), out['afac'][f], a64[f], a32[f])
        for l in range(6):
            errs[('G', l)] = rel(('G', l), out['gfac'][l], gf64[l], gf32[l])
    # the sampled policy gradient p - onehot(y) is exactly 0 with one action
    assert zero == ([('G', 4)] if A == 1 and c.bwd else []), zero
    fails = []
    cls = ('bf16' if c.bf16 else 'tower' if ac.uses_tower(c) else 'per-layer') + ('/' + c.bwd if c.bwd else '')
    for k, (v, v32) in errs.items():
        tol = 1e-2 if c.bf16 else TOL[k[0]]
        w = _WORST.setdefault((cls, k[0]), [0.0, ''])
        if v > w[0]:
            w[:] = [v, ac.case_id(c)]
            print('WORST so far %s %s: %.2e' % (cls, k[0], v))
        if k in zero:
            if v != 0.0:
                fails.append((k, 'must be exactly zero'))
        elif not v < tol:
            print('ESCAPE %s %s kernel %.2e plain f32 %.2e' % (ac.case_id(c), k, v, v32))
            if c.bf16 or not v < max(tol, 4 * v32):
                fails.append((k, v, v32))
    assert not fails, fails
    return errs


def _ids(cases):
    return [ac.case_id(c) for c in cases]


def _check(lib, cuda, c):
    out = run(lib, cuda, c)
    check_float64(cuda, c, out)
    check_bits(lib, cuda, c, out)
    return out


_FWD = (ac.FWD_STRIDE + ac.FWD_STRIDE_PERLAYER + ac.FWD_BASE + ac.FWD_ACT + ac.FWD_LDL + ac.FWD_NOVALUE + ac.FWD_BF16)
_BWD = ac.BWD_X3 + ac.BWD_F32 + ac.BWD_NOSTATS + ac.BWD_CONV_STATS


@pytest.mark.parametrize('c', _FWD, ids=_ids(_FWD))
def test_forward_addressing(lib, cuda, c):
    """Image strides, base offsets, activation row strides (with and without the
    forward workspace), ld_logits (with the output statistics that read it),
    want_value = 0 and the 16-bit forward: guards, float64, bit identity."""
    _check(lib, cuda, c)


@pytest.mark.parametrize('c', _BWD, ids=_ids(_BWD))
def test_backward_addressing(lib, cuda, c):
    """acmi_backward + acmi_kfac_output_stats on padded strides and offset bases: the
    fused conv1 A factor + weight gradient (bf16x3), the i8 A factor + u8-patch weight
    gradient (f32), statistics off (4-byte alignment legal: the accepting side of the
    8-byte rule), both conv statistics modes."""
    _check(lib, cuda, c)


@pytest.mark.parametrize('c', ac.BWD_STACKED, ids=_ids(ac.BWD_STACKED))
def test_stacked_backward_addressing(lib, cuda, c):
    """acmi_backward_stacked + acmi_kfac_output_stats_finish at img_stride = 28224 + 16:
    bit-identical to acmi_backward + acmi_kfac_output_stats at the same stride and to
    the dense pair."""
    out = _check(lib, cuda, c)
    for other in (c._replace(bwd='stats'), ac.dense(c)._replace(bwd='stats')):
        ref = run(lib, cuda, other)
        for k, v in out.items():
            pairs = zip(v, ref[k]) if isinstance(v, list) else [(v, ref[k])]
            assert all(_same_bits(x, y) for x, y in pairs), (ac.case_id(other), k)


def test_two_images_one_step_inside_the_2_31_limit(lib, cuda):
    """B = 2 with the second image 2^31 - 28224 - 16 bytes after the first -- the
    largest 16-byte multiple acmi.h's (B - 1) * img_stride + 28224 < 2^31 admits: the
    forward, the backward with statistics and the output statistics return ACMI_OK,
    leave the 2 GiB gap untouched and reproduce the dense call's bytes."""
    (c,) = ac.FWD_SPAN
    assert c.stride + ac.OBS_BYTES < 2 ** 31 <= c.stride + 16 + ac.OBS_BYTES
    _check(lib, cuda, c)
    del _RUNS[c]


def test_empty_batch_writes_nothing(lib, cuda):
    """B = 0: both forward entry points return ACMI_OK and write nothing."""
    A, C3 = 18, 64
    params = _params(A, C3, cuda)
    obs = Buf(cuda, 'u8', 1, ac.OBS_BYTES)
    bufs = {k: Buf(cuda, 'i32' if k in MASKS else 'f32', 1, per)
            for k, (per, _) in ac.act_rows(A, C3, A, 1).items()}
    acts = _lib.Acts(*[bufs[k].ptr for k in FWD_NAMES], A)
    acts.m1, acts.m2, acts.m3 = bufs['m1'].ptr, bufs['m2'].ptr, bufs['m3'].ptr
    net = _lib.Net(A, C3, params.data_ptr())
    st = _lib.stream_handle()
    o = ctypes.c_void_p(obs.ptr)
    assert lib.acmi_forward(ctypes.byref(net), o, ac.OBS_BYTES, 0, ctypes.byref(acts), 1, st) == 0
    assert lib.acmi_forward_strided(ctypes.byref(net), o, ac.OBS_BYTES + 4, 0, ctypes.byref(acts), 1, 3, st) == 0
    torch.cuda.synchronize()
    assert all(b.untouched() for b in bufs.values())


_REFUSED = [r for r in ac.REFUSED if r[0] in ac.BWD_ENTRIES and r[3] in ('stride_align', 'obs_align', 'stride_min')]


@pytest.mark.parametrize('entry,a_stats,kw,clause', _REFUSED, ids=[ac.refused_id(r) for r in _REFUSED])
def test_refused_calls_launch_nothing(lib, cuda, entry, a_stats, kw, clause):
    """A backward the contract refuses for its stride or alignment -- first of all
    acmi_backward(img_stride = 28228, a_stats != NULL), which used to be refused by
    conv1's A factor after the input-gradient chain had been enqueued -- returns
    ACMI_ERR_ARG with nothing enqueued: after a synchronise every byte of the
    sentinel-filled d1..d4, gradients, statistics and workspaces is unchanged."""
    A, C3, B = 18, 64, 3
    stride = kw.get('img_stride', ac.OBS_BYTES)
    off = kw.get('obs', 16) - 16
    params = _params(A, C3, cuda)
    img, dhead_in = _inputs(A, C3, B, cuda)
    # the forward on a dense copy (legal); the refused call on the case's own stride / base
    fwd = run(lib, cuda, ac.case(B=B))
    dense = {k: fwd[k].contiguous() for k in FWD_NAMES + MASKS}
    acts = _lib.Acts(*[dense[k].data_ptr() for k in FWD_NAMES], A)
    acts.m1, acts.m2, acts.m3 = [dense[k].data_ptr() for k in MASKS]
    obs = Buf(cuda, 'u8', B, ac.OBS_BYTES, max(stride, ac.OBS_BYTES), off)
    obs.put(img)
    ldh = 20
    dh = torch.zeros(B, ldh, device=cuda)
    dh[:, :A + 1] = dhead_in
    tot = ctypes.c_int64()
    _lib.call('acmi_kfac_layout', A, C3, None, None, None, ctypes.byref(tot))
    need = int(lib.acmi_backward_ws_floats(B, A, C3))
    dims = (B * ac.A1_FLOATS, B * 81 * 64, B * 49 * C3, B * 512)
    out = {}
    for sfx in ('', '_s'):
        out.update({'d%d%s' % (i + 1, sfx): Buf(cuda, 'f32', 1, n) for i, n in enumerate(dims)})
        out['ws' + sfx] = Buf(cuda, 'f32', 1, need)
    out.update(grads=Buf(cuda, 'f32', 1, params.numel()), astat=Buf(cuda, 'f32', 1, tot.value))
    bwd, bwd_s = [_lib.Bwd(*[out['d%d%s' % (i, sfx)].ptr for i in (1, 2, 3, 4)], dh.data_ptr(), ldh)
                  for sfx in ('', '_s')]
    net = _lib.Net(A, C3, params.data_ptr())
    P = lambda k: ctypes.c_void_p(out[k].ptr)
    st = _lib.stream_handle()
    astat = P('astat') if a_stats else None
    if entry == 'acmi_backward':
        rc = lib.acmi_backward(ctypes.byref(net), ctypes.c_void_p(obs.ptr), stride, B, ctypes.byref(acts),
                               ctypes.byref(bwd), P('grads'), astat, P('ws'), need, st)
    else:
        rc = lib.acmi_backward_stacked(ctypes.byref(net), ctypes.c_void_p(obs.ptr), stride, B, ctypes.byref(acts),
                                       ctypes.byref(bwd), P('grads'), astat, P('ws'), need, ctypes.byref(bwd_s),
                                       SEED_S, 0, COUNTER, P('ws_s'), need, st)
    msg = lib.acmi_last_error()
    torch.cuda.synchronize()
    assert rc == _lib.ERR_ARG, rc
    touched = [k for k, b in out.items() if not b.untouched()]
    assert not touched, ('written by a refused call', touched)
    assert entry.encode() + b':' in msg, msg
