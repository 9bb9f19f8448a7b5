"""The addressing contract of the obs-taking entry points, host side (include/acmi.h
"Addressing"; DESIGN.md "Addressing tests"): every stride / alignment / leading-
dimension refusal of acmi_forward, acmi_forward_strided, acmi_backward and
acmi_backward_stacked on pointers no call gets as far as using (nothing is enqueued,
so no GPU is needed), and a self-check of the case table that
tests/test_gpu_addressing.py runs.  The accepting side of every boundary would launch:
it is in the GPU file."""
import ctypes
import os
import re

import pytest

import addressing_cases as ac
from actorcritic import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p
ONE = P(16)  # a non-null, 16-byte aligned pointer no call gets as far as using


def _call(lib, entry, a_stats=True, obs=16, img_stride=ac.OBS_BYTES, B=2, A=18, act_stride=1, ld_logits=None,
          want_value=1, value_null=False, bf16=False, prep=True, gemm=None):
    """One call of `entry` that is legal but for the keywords given."""
    acts = _lib.Acts(ONE, ONE, ONE, ONE, ONE, None if value_null else ONE, A if ld_logits is None else ld_logits,
                     None, 0, None, None, None)
    mode = lambda m: 0 if m is None else m + 1
    net = _lib.Net(A, 64, ONE, ONE if prep else None, mode(gemm), mode(_lib.FWD_BF16 if bf16 else None), 0)
    n, a = ctypes.byref(net), ctypes.byref(acts)
    if entry == 'acmi_forward':
        assert act_stride == 1
        return lib.acmi_forward(n, P(obs), img_stride, B, a, want_value, None)
    if entry == 'acmi_forward_strided':
        return lib.acmi_forward_strided(n, P(obs), img_stride, B, a, want_value, act_stride, None)
    bwd = _lib.Bwd(ONE, ONE, ONE, ONE, ONE, 20)
    big = 1 << 60
    if entry == 'acmi_backward':
        return lib.acmi_backward(n, P(obs), img_stride, B, a, ctypes.byref(bwd), ONE, ONE if a_stats else None, ONE,
                                 big, None)
    assert entry == 'acmi_backward_stacked' and a_stats
    bwd_s = _lib.Bwd(P(32), P(32), P(32), P(32), ONE, 20)
    return lib.acmi_backward_stacked(n, P(obs), img_stride, B, a, ctypes.byref(bwd), ONE, ONE, ONE, big,
                                     ctypes.byref(bwd_s), 1, 0, 1, P(48), big, None)


def test_constants_match_the_binding():
    assert (ac.X3, ac.F32, ac.BF16) == (_lib.GEMM_X3, _lib.GEMM_F32, _lib.FWD_BF16)
    assert (ac.BAND, ac.PATCHES) == (_lib.CONV_STATS_BAND, _lib.CONV_STATS_PATCHES)


@pytest.mark.parametrize('entry,a_stats,kw,clause', ac.REFUSED, ids=[ac.refused_id(r) for r in ac.REFUSED])
def test_refusals(lib, entry, a_stats, kw, clause):
    """Every refusal of the contract, for each entry point it applies to: ACMI_ERR_ARG
    and the entry point's own name in acmi_last_error()."""
    rc = _call(lib, entry, a_stats, **kw)
    assert rc == _lib.ERR_ARG, rc
    msg = lib.acmi_last_error()
    assert msg.startswith(entry.encode() + b':'), msg


def test_the_2_31_limit_is_the_headers_formula():
    """(B - 1) * img_stride + 28224 < 2^31 (acmi.h): the largest B of a stride and the
    largest stride of a B pass, one more does not, by the formula itself."""
    src = open(os.path.join(ROOT, 'include', 'acmi.h')).read()
    assert '(B - 1) * img_stride + 28224 < 2^31' in re.sub(r'\s*\n\s*\*\s*', ' ', src)
    for s in (ac.OBS_BYTES, ac.OBS_BYTES + 4, ac.OBS_BYTES + 16, 5 * ac.OBS_BYTES, 20 * ac.OBS_BYTES):
        b = ac.max_batch(s)
        assert (b - 1) * s + ac.OBS_BYTES < 2 ** 31 <= b * s + ac.OBS_BYTES
        for e in ac.ENTRIES:
            al = ac.obs_align(e)
            if s % al == 0:
                assert ac.violations(e, 16, s, b) == [] and ac.violations(e, 16, s, b + 1) == ['spans32']
    for B in (2, 3, 66):
        for al in (4, 8, 16):
            s = ac.max_stride(B, al)
            assert s % al == 0 and (B - 1) * s + ac.OBS_BYTES < 2 ** 31 <= (B - 1) * (s + al) + ac.OBS_BYTES


def test_spans32_refusing_side(lib):
    """The smallest (B, img_stride) past the limit is refused by every entry point; the
    largest that passes would launch (test_gpu_addressing runs B = 2 at its largest
    stride)."""
    for e in ac.ENTRIES:
        for s in (ac.OBS_BYTES, ac.OBS_BYTES + 16, 5 * ac.OBS_BYTES):
            assert _call(lib, e, B=ac.max_batch(s) + 1, img_stride=s) == _lib.ERR_ARG, (e, s)
            assert b'2^31' in lib.acmi_last_error() and e.encode() + b':' in lib.acmi_last_error()
        for B in (2, 66):
            s = ac.max_stride(B, 16) + 16
            assert _call(lib, e, B=B, img_stride=s) == _lib.ERR_ARG, (e, B)
            assert b'2^31' in lib.acmi_last_error()


def test_header_and_integration_state_the_alignment():
    src = re.sub(r'\s*\n\s*\*\s*', ' ', open(os.path.join(ROOT, 'include', 'acmi.h')).read())
    for text in ('obs and img_stride multiples of 4', 'multiples of 16', 'multiples of 8',
                 'act_img_stride >= 1', 'ld_logits >= num_actions'):
        assert text in src, text
    assert 'aligned' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_case_table_is_legal_and_fits_its_buffers():
    """Every GPU case satisfies the contract at the address its buffer gives it, its
    rows lie inside the allocation without overlapping, and it stays small."""
    assert len(set(ac.GPU_CASES)) == len(ac.GPU_CASES)
    assert len(set(ac.case_id(c) for c in ac.GPU_CASES)) == len(ac.GPU_CASES)
    for c in ac.GPU_CASES:
        for base in (0, 256, 4096):  # any allocation aligned to 256 bytes or more
            assert ac.case_violations(c, base) == [], (ac.case_id(c), ac.case_violations(c, base))
        assert c.B <= 65 or (c.B == 96 and c.gemm == ac.F32), ac.case_id(c)
        assert c.bwd is None or c.act == 1  # the update takes dense activations
        ldl = c.A if c.ldl is None else c.ldl
        rows = dict(ac.act_rows(c.A, c.C3, ldl, c.act), obs=(ac.OBS_BYTES, c.stride))
        for k, (per, stride) in rows.items():
            off = c.off if k == 'obs' else 0
            total = ac.buffer_elems(c.B, per, stride, off)
            assert stride >= per
            first, last = ac.row_start(0, stride, off), ac.row_start(c.B - 1, stride, off)
            assert first >= ac.GUARD and last + per + ac.GUARD == total, (ac.case_id(c), k)
        assert rows['logits'][0] == c.A and rows['logits'][1] == c.act * ldl >= c.A
        # what the contract says of the kernels reached: the fused tower needs 16-byte images
        assert ac.uses_tower(c) == (c.prep and c.gemm != ac.F32 and (ac.GUARD + c.off) % 16 == 0 and
                                    c.stride % 16 == 0)
        assert not c.bf16 or ac.uses_tower(c)
    # the span case sits one alignment step inside the limit
    (s,) = ac.FWD_SPAN
    assert ac.case_violations(s._replace(stride=s.stride + 16)) == ['spans32', 'spans32']


def test_refused_table_breaks_one_clause_each():
    legal = dict(obs_addr=16, img_stride=ac.OBS_BYTES, B=2)
    for e in ac.ENTRIES:
        for st in (True, False):
            assert ac.violations(e, a_stats=st, **legal) == []
    for entry, a_stats, kw, clause in ac.REFUSED:
        f = dict(legal, a_stats=a_stats)
        f.update({'obs_addr' if k == 'obs' else k: v for k, v in kw.items()})
        assert ac.violations(entry, **f) == [clause], (entry, a_stats, kw, ac.violations(entry, **f))
    # every alignment / stride clause for each of the four entry points
    for e in ac.ENTRIES:
        got = set(r[3] for r in ac.REFUSED if r[0] == e)
        assert {'stride_min', 'stride_align', 'obs_align', 'spans32'} <= got, (e, got)
        if e in ac.FWD_ENTRIES:
            assert {'ld_logits', 'value_null', 'bf16_tower'} <= got, (e, got)
    assert 'act_stride' in set(r[3] for r in ac.REFUSED if r[0] == 'acmi_forward_strided')


def test_guard_check_sees_every_stray_write():
    """The GPU file's guarded buffer (on the CPU here): one element changed in the
    leading guard, in a gap between rows, past the last row or in the offset bytes
    fails guards_intact; writes to the rows themselves do not."""
    import torch
    from test_gpu_addressing import Buf
    for kind, n, per, stride, off in (('f32', 3, 18, 40, 0), ('i32', 2, 5, 5, 0), ('u8', 3, 28224, 28232, 8),
                                      ('f32', 1, 7, 7, 0)):
        b = Buf(torch.device('cpu'), kind, n, per, stride, off)
        assert b.raw.numel() == ac.buffer_elems(n, per, stride, off) and b.guards_intact() and b.untouched()
        b.put(torch.zeros(n, per, dtype=torch.float32 if kind == 'f32' else b.raw.dtype))
        assert b.guards_intact() and not b.untouched()
        assert not b.get().any()
        end = ac.row_start(n - 1, stride, off) + per
        stray = [0, ac.row_start(0, stride, off) - 1, end, b.raw.numel() - 1]
        if stride > per and n > 1:
            stray += [ac.row_start(0, stride, off) + per, ac.row_start(1, stride, off) - 1]
        for i in stray:
            keep = b.raw[i].clone()
            b.raw[i] = 0
            assert not b.guards_intact(), (kind, i)
            b.raw[i] = keep
            assert b.guards_intact()
