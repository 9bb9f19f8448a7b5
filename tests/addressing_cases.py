"""The addressing domain of the obs-taking entry points as plain data (no torch, no
library): the contract of include/acmi.h, the layout of the guarded buffers and the
case tables that tests/test_addressing_host.py checks on a CPU-only machine and
tests/test_gpu_addressing.py runs.

Contract (acmi.h, "Addressing"; DESIGN.md "Addressing tests"):

    entry point                               obs, img_stride multiple of
    acmi_forward, acmi_forward_strided        4   (16: the fused tower; 16-bit forward needs it)
    acmi_backward, a_stats == NULL            4
    acmi_backward, a_stats != NULL            8
    acmi_backward_stacked                     8

    img_stride >= 28224; act_img_stride >= 1; ld_logits >= A; value non-NULL when
    want_value; (B - 1) * img_stride + 28224 < 2^31 and, for the forward,
    (B - 1) * act_img_stride * 12800 + 12800 < 2^31 (32-bit element offsets).
"""
import collections

OBS_BYTES = 84 * 84 * 4  # 28224
A1_FLOATS = 20 * 20 * 32
FWD_ENTRIES = ('acmi_forward', 'acmi_forward_strided')
BWD_ENTRIES = ('acmi_backward', 'acmi_backward_stacked')
ENTRIES = FWD_ENTRIES + BWD_ENTRIES
X3, F32 = 1, 0  # _lib.GEMM_X3 / GEMM_F32 (asserted equal in the host test)
BF16 = 1  # _lib.FWD_BF16
BAND, PATCHES = 1, 0


def obs_align(entry, a_stats=True):
    """Bytes obs and img_stride must be a multiple of."""
    if entry in FWD_ENTRIES:
        return 4
    return 8 if (entry == 'acmi_backward_stacked' or a_stats) else 4


def spans32(rows, stride, per_row):
    return rows <= 0 or (rows - 1) * stride + per_row < 2 ** 31


def max_batch(img_stride):
    """Largest B with (B - 1) * img_stride + 28224 < 2^31."""
    return (2 ** 31 - 1 - OBS_BYTES) // img_stride + 1


def max_stride(B, align):
    """Largest img_stride (a multiple of align) that B >= 2 images may have."""
    return (2 ** 31 - 1 - OBS_BYTES) // (B - 1) // align * align


def tower(obs_addr, img_stride, prep=True, gemm=X3):
    """The forward runs the fused tower (else the per-layer kernels)."""
    return gemm == X3 and prep and obs_addr % 16 == 0 and img_stride % 16 == 0


def violations(entry, obs_addr, img_stride, B, A=18, act_stride=1, ld_logits=None, want_value=1, value_null=False,
               a_stats=True, prep=True, gemm=X3, bf16=False):
    """The clauses of the contract a call breaks (empty: the call is legal)."""
    ld_logits = A if ld_logits is None else ld_logits
    al = obs_align(entry, a_stats)
    v = []
    fwd = entry in FWD_ENTRIES
    if B < 0 or (B == 0 and not fwd):
        v.append('B')
    if img_stride < OBS_BYTES:
        v.append('stride_min')
    if img_stride % al:
        v.append('stride_align')
    if obs_addr % al:
        v.append('obs_align')
    if fwd:
        if act_stride < 1:
            v.append('act_stride')
        if ld_logits < A:
            v.append('ld_logits')
        if want_value and value_null:
            v.append('value_null')
        if bf16 and not tower(obs_addr, img_stride, prep, gemm):
            v.append('bf16_tower')
    if not (spans32(B, img_stride, OBS_BYTES) and spans32(B, (act_stride if fwd else 1) * A1_FLOATS, A1_FLOATS)):
        v.append('spans32')
    return v


# ---------------------------------------------------------------------------
# guarded buffers: [guard | off | row 0 | gap | row 1 | ... | row n-1 | guard]
# ---------------------------------------------------------------------------
GUARD = 256  # elements before and after (a multiple of 16 bytes for every element size)


def row_start(b, stride, off=0):
    """Element index of row b in the allocation."""
    return GUARD + off + b * stride


def buffer_elems(n, per_row, stride, off=0):
    """Elements of the allocation holding n rows of per_row elements, stride apart."""
    assert n >= 1 and stride >= per_row >= 1 and off >= 0
    return GUARD + off + (n - 1) * stride + per_row + GUARD


def act_rows(A, C3, ld_logits, act_stride):
    """{tensor: (elements per row, elements between rows)} of the forward's outputs:
    row b of every output lands at b * act_stride rows of its own tensor (logits rows
    are ld_logits wide, its padding columns belong to the gap)."""
    st = act_stride
    per = dict(a1=A1_FLOATS, a2=9 * 9 * 64, a3=49 * C3, a4=512, value=1, m1=400, m2=162, m3=49 * C3 // 32)
    rows = {k: (n, st * n) for k, n in per.items()}
    rows['logits'] = (A, st * ld_logits)
    return rows


# ---------------------------------------------------------------------------
# the GPU cases
# ---------------------------------------------------------------------------
_FIELDS = dict(B=2, A=18, C3=64, stride=OBS_BYTES, off=0, act=1, ldl=None, want_value=1, value='buf', prep=True,
               gemm=None, bf16=False, conv_stats=None, fws=False, bwd=None)
Case = collections.namedtuple('Case', list(_FIELDS))
# bwd: None (forward only), 'stats' (acmi_backward with a_stats + acmi_kfac_output_stats), 'nostats' (a_stats NULL),
# 'stacked' (acmi_backward_stacked + acmi_kfac_output_stats_finish).  value: 'buf', 'null' or 'guard' (a sentinel-
# filled buffer passed with want_value = 0).  fws: with the forward workspace (acts->ws).


def case(**kw):
    f = dict(_FIELDS)
    f.update(kw)
    return Case(**f)


def dense(c):
    """The dense call of the same case: same B, net, modes, images, head gradients, seed."""
    return c._replace(stride=OBS_BYTES, off=0, act=1, ldl=None, want_value=1, value='buf', fws=False)


def case_id(c):
    parts = ['b%d' % c.B]
    if (c.A, c.C3) != (18, 64):
        parts.append('a%d-c%d' % (c.A, c.C3))
    if c.stride != OBS_BYTES:
        d = c.stride - OBS_BYTES
        parts.append('stride+%d' % d if d < OBS_BYTES else ('stride%dx' % (c.stride // OBS_BYTES) if
                                                           c.stride % OBS_BYTES == 0 else 'stride%d' % c.stride))
    if c.off:
        parts.append('base+%d' % c.off)
    if c.act != 1:
        parts.append('act%d' % c.act)
    if c.ldl is not None:
        parts.append('ldl%d' % c.ldl)
    if not c.want_value:
        parts.append('novalue-' + c.value)
    if not c.prep:
        parts.append('noprep')
    if c.gemm is not None:
        parts.append('x3' if c.gemm == X3 else 'f32')
    if c.bf16:
        parts.append('bf16')
    if c.conv_stats is not None:
        parts.append('band' if c.conv_stats == BAND else 'patches')
    if c.fws:
        parts.append('ws')
    if c.bwd:
        parts.append(c.bwd)
    return '-'.join(parts)


def entries_of(c):
    """(entry point, a_stats) of every obs-taking call the case makes."""
    e = [('acmi_forward' if c.act == 1 else 'acmi_forward_strided', False)]
    if c.bwd:
        e.append(('acmi_backward_stacked' if c.bwd == 'stacked' else 'acmi_backward', c.bwd != 'nostats'))
    return e


def case_violations(c, base_addr=0):
    """Every clause any call of the case breaks (base_addr: the allocation's address,
    a multiple of 16 and more)."""
    v = []
    for entry, st in entries_of(c):
        v += violations(entry, base_addr + GUARD + c.off, c.stride, c.B, A=c.A, act_stride=c.act, ld_logits=c.ldl,
                        want_value=c.want_value, value_null=c.value == 'null', a_stats=st, prep=c.prep,
                        gemm=X3 if c.gemm is None else c.gemm, bf16=c.bf16)
    return v


def uses_tower(c):
    return tower(GUARD + c.off, c.stride, c.prep, X3 if c.gemm is None else c.gemm)


_PAD = (OBS_BYTES + 16, OBS_BYTES + 4, OBS_BYTES + 8, 5 * OBS_BYTES)
_BS = (1, 2, 17, 65)

# forward: img_stride x B, conv_prep set (the fused tower where 16-byte aligned)
FWD_STRIDE = [case(B=B, stride=s) for s in (OBS_BYTES,) + _PAD for B in _BS]
# the first four strides without prepared weights and in f32 gemm mode: always the per-layer kernels
FWD_STRIDE_PERLAYER = [case(B=B, stride=s, **kw) for kw in (dict(prep=False), dict(gemm=F32))
                       for s in (OBS_BYTES,) + _PAD[:3] for B in _BS]
FWD_BASE = [case(B=B, off=o) for o in (16, 4, 8) for B in (2, 65)]
FWD_ACT = [case(B=B, act=a, fws=w) for a in (2, 5) for B in (1, 3, 65) for w in (False, True)]
FWD_LDL = ([case(B=3, ldl=l, bwd='stats') for l in (18, 19, 20, 64)] +
           [case(B=3, A=1, C3=32, ldl=l, bwd='stats') for l in (1, 4)])
FWD_NOVALUE = [case(B=B, want_value=0, value=v) for B in (3, 65) for v in ('null', 'guard')]
FWD_BF16 = [case(B=B, bf16=True, **kw) for B in (2, 65) for kw in (dict(stride=OBS_BYTES + 16), dict(off=16))]
# one step inside the 2^31 limit: two images, the second 2^31 - 28224 - 16 bytes after the first
FWD_SPAN = [case(B=2, stride=max_stride(2, 16), bwd='stats')]

# backward with statistics, bf16x3 mode: the fused conv1 A factor + weight gradient (buffer loads, 32-bit offsets).
# af_plan_tri gives ceil(400 B / 64) chunks of 64 rows up to B = 40 -- 7 chunks at B = 1, every boundary but the
# first inside the image; 13 at B = 2, the 7th chunk running from image 0 into image 1 -- and 128-row chunks (two
# stages each, the gather position advancing inside a chunk) from B = 41: 129 chunks there, 204 at B = 65.
_BWD_ADDR = [dict(stride=OBS_BYTES), dict(stride=OBS_BYTES + 8), dict(stride=OBS_BYTES + 16),
             dict(stride=5 * OBS_BYTES), dict(off=8)]
BWD_X3 = [case(B=B, gemm=X3, bwd='stats', **kw) for kw in _BWD_ADDR for B in _BS] + \
         [case(B=41, gemm=X3, bwd='stats', stride=OBS_BYTES + 16)]
# f32 mode: conv1_afactor_i8_kernel + the ConvRows<uint8_t> weight gradient
BWD_F32 = [case(B=B, gemm=F32, bwd='stats', **kw) for kw in _BWD_ADDR for B in (2, 65)] + \
          [case(B=96, gemm=F32, bwd='stats', stride=OBS_BYTES + 8)]
# statistics off (the A2C path): 4-byte alignment is legal
BWD_NOSTATS = [case(B=B, bwd='nostats', **kw) for B in (2, 65)
               for kw in (dict(stride=OBS_BYTES), dict(stride=OBS_BYTES + 4), dict(off=4))]
BWD_CONV_STATS = [case(B=17, conv_stats=m, bwd='stats', stride=OBS_BYTES + 16) for m in (BAND, PATCHES)]
BWD_STACKED = [case(B=B, bwd='stacked', stride=OBS_BYTES + 16) for B in (24, 65)]

GPU_CASES = (FWD_STRIDE + FWD_STRIDE_PERLAYER + FWD_BASE + FWD_ACT + FWD_LDL + FWD_NOVALUE + FWD_BF16 + FWD_SPAN +
             BWD_X3 + BWD_F32 + BWD_NOSTATS + BWD_CONV_STATS + BWD_STACKED)

# calls the contract refuses, one broken clause each: (entry, a_stats, keyword overrides of a legal call, clause).
# obs is the pointer's value; a legal call has obs = 16, img_stride = 28224, B = 2, A = 18.
REFUSED = []
for _e in ENTRIES:
    for _st in ((True, False) if _e == 'acmi_backward' else (True,)):
        _al = obs_align(_e, _st)
        REFUSED += [(_e, _st, dict(img_stride=OBS_BYTES - 8), 'stride_min'),
                    (_e, _st, dict(img_stride=0), 'stride_min'),
                    (_e, _st, dict(img_stride=OBS_BYTES + _al // 2), 'stride_align'),
                    (_e, _st, dict(img_stride=OBS_BYTES + 2), 'stride_align'),
                    (_e, _st, dict(obs=16 + _al // 2), 'obs_align'),
                    (_e, _st, dict(obs=16 + 1), 'obs_align'),
                    (_e, _st, dict(B=max_batch(OBS_BYTES) + 1), 'spans32'),
                    (_e, _st, dict(B=max_batch(OBS_BYTES + 16) + 1, img_stride=OBS_BYTES + 16), 'spans32'),
                    (_e, _st, dict(B=2, img_stride=max_stride(2, 16) + 16), 'spans32'),
                    (_e, _st, dict(B=-1), 'B')]
    if _e in FWD_ENTRIES:
        REFUSED += [(_e, False, dict(ld_logits=17), 'ld_logits'),
                    (_e, False, dict(want_value=1, value_null=True), 'value_null'),
                    (_e, False, dict(bf16=True, img_stride=OBS_BYTES + 4), 'bf16_tower'),
                    (_e, False, dict(bf16=True, obs=16 + 8), 'bf16_tower'),
                    (_e, False, dict(bf16=True, prep=False), 'bf16_tower')]
    else:
        REFUSED.append((_e, True, dict(B=0), 'B'))
REFUSED += [('acmi_forward_strided', False, dict(act_stride=0), 'act_stride'),
            ('acmi_forward_strided', False, dict(act_stride=-1), 'act_stride'),
            ('acmi_forward_strided', False, dict(B=2 ** 31 // (3 * A1_FLOATS) + 1, act_stride=3), 'spans32')]


def refused_id(r):
    entry, a_stats, kw, clause = r
    return '%s-%s-%s' % (entry[5:] + ('' if a_stats or entry != 'acmi_backward' else '-nostats'), clause,
                         '-'.join('%s=%s' % kv for kv in sorted(kw.items())))


# the defect this table was written after: accepted by the argument check, refused after the dX chain had run
LATE_REFUSAL = ('acmi_backward', True, dict(img_stride=OBS_BYTES + 4), 'stride_align')
assert LATE_REFUSAL in REFUSED
