"""The Atari frame kernels over their shape domain (tests/atari_frame_cases.py): both
compiled forms of atari_frames_kernel (acmi_atari_preprocess, acmi_atari_stack) and of
atari_rollout_kernel (acmi_atari_rollout_frames), bit-exact against
oracle.atari_preprocess / oracle.atari_stack.  Every output lives inside a buffer of
random bytes with a guard behind it and is compared as a whole, gaps and guard included;
inputs are compared after the launch.  At most 8 envs a launch.
tests/test_atari_frame_cases_host.py proves which form each shape selects."""
import ctypes

import numpy as np
import pytest

import atari_frame_cases as cases
from atari_frame_cases import OUT, STACK, oracle

pytestmark = pytest.mark.gpu

GRAY = OUT * OUT
GUARD = 4096
SHAPES = pytest.mark.parametrize('shape', cases.SHAPES, ids=cases.SHAPE_IDS)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order='C')).cuda()  # (a copy: the cases are read-only)


def _ptr(t, offset=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + offset)


def _form(shape):
    return '{}x{} {}'.format(shape[0], shape[1], 'fixed3 <3,3>' if shape[2] else 'generic <0,0>')


def _check_buffer(got, expected, n, stride, size, what, labels=None):
    """`got` against `expected`, both whole buffers: env by env first (so that a failure
    names every env that differs), then everything else (gaps between envs and the guard
    behind them)."""
    wrong = []
    for e in range(n):
        a, b = got[e * stride:e * stride + size], expected[e * stride:e * stride + size]
        if not np.array_equal(a, b):
            wrong.append('env {}{}: {} bytes differ'.format(e, ' ' + str(labels[e]) if labels else '', int((a != b).sum())))
    assert not wrong, '{}: {}'.format(what, '; '.join(wrong))
    assert np.array_equal(got, expected), '{}: bytes outside the outputs were written'.format(what)


def _raw_batch(entries, H, W):
    """[n][2][H][W][3]: slot 0 the last frame, slot 1 the frame before it -- or 255
    everywhere where the env has one frame only (it must not be read)."""
    raw = np.full((len(entries), 2, H, W, 3), 255, np.uint8)
    for i, (last, prev) in enumerate(entries):
        raw[i, 0] = last
        if prev is not None:
            raw[i, 1] = prev
    return raw


# ---------------------------------------------------------------------------
# acmi_atari_preprocess (mode 0)
# ---------------------------------------------------------------------------
def _preprocess(lib, raw, two, nframes, H, W, out_stride, want, what, names):
    import torch
    from actorcritic import _lib
    n = raw.shape[0]
    rng = np.random.default_rng(n + out_stride)
    out0 = rng.integers(1, 256, n * out_stride + GUARD, dtype=np.uint8)
    d_raw, d_out = _dev(raw), _dev(out0)
    d_nf = None if nframes is None else _dev(nframes)
    _lib.call('acmi_atari_preprocess', _ptr(d_raw), raw[0].nbytes, raw[0, 0].nbytes if two else 0, _ptr(d_nf), n,
              H, W, _ptr(d_out), out_stride, _lib.stream_handle())
    torch.cuda.synchronize()
    expected = out0.copy()
    for e in range(n):
        expected[e * out_stride:e * out_stride + GRAY] = want[e].reshape(-1)
    _check_buffer(d_out.cpu().numpy(), expected, n, out_stride, GRAY, what, names)
    assert np.array_equal(d_raw.cpu().numpy(), raw), what + ': the frames were written'


@SHAPES
def test_preprocess_every_family(lib, cuda, shape):
    H, W = shape[:2]
    fams, ref = cases.family_frames(H, W), cases.oracle_gray(H, W)
    for lo in range(0, len(fams), 8):
        chunk = fams[lo:lo + 8]
        names = [c[0] for c in chunk]
        what = 'acmi_atari_preprocess {}'.format(_form(shape))
        pairs = _raw_batch([(a, b) for _, a, b in chunk], H, W)
        # pairs, nframes NULL
        _preprocess(lib, pairs, True, None, H, W, GRAY, [ref[n][1] for n in names], what + ' pairs', names)
        # single frames (frame_stride 0), nframes NULL
        _preprocess(lib, pairs, False, None, H, W, GRAY, [ref[n][0] for n in names], what + ' singles', names)
        # nframes 1 / 2 mixed, slot 1 of a one-frame env all 255; a wider out_stride
        nf = np.array([1 + (i + lo // 8) % 2 for i in range(len(chunk))], np.uint8)
        mixed = _raw_batch([(a, b if k == 2 else None) for (_, a, b), k in zip(chunk, nf)], H, W)
        _preprocess(lib, mixed, True, nf, H, W, GRAY + 52, [ref[n][k - 1] for n, k in zip(names, nf)],
                    what + ' nframes {}'.format(list(nf)), names)
    assert set(nf) == {1, 2}


# ---------------------------------------------------------------------------
# acmi_atari_stack (modes 2 and 1)
# ---------------------------------------------------------------------------
def _stack_script(H, W, n=6, steps=3):
    """Per launch (a reset, then `steps` steps): the raw batch, nframes, terminals and the
    oracle's gray frame per env.  Env i of launch s shows family (i + 4 s) mod 11."""
    fams, ref = cases.family_frames(H, W), cases.oracle_gray(H, W)
    rng = np.random.default_rng(H + W)
    script = []
    for s in range(steps + 1):
        pick = [fams[(i + 4 * s) % len(fams)] for i in range(n)]
        nf = rng.permutation(np.arange(n) % 2 + 1).astype(np.uint8)
        term = rng.permutation((np.arange(n) % 3 == 0)).astype(np.uint8)
        raw = _raw_batch([(a, b if k == 2 else None) for (_, a, b), k in zip(pick, nf)], H, W)
        script.append((raw, nf, term, [ref[name][k - 1] for (name, _, _), k in zip(pick, nf)],
                       ['{} x{}'.format(name, k) for (name, _, _), k in zip(pick, nf)]))
    return script


@SHAPES
@pytest.mark.parametrize('in_place', [False, True], ids=['out-of-place', 'in-place'])
def test_stack_reset_then_steps(lib, cuda, shape, in_place):
    import torch
    from actorcritic import _lib
    H, W = shape[:2]
    n = 6
    stride = STACK if in_place else STACK + 64
    rng = np.random.default_rng(3)
    bufs = [rng.integers(1, 256, n * stride + GUARD, dtype=np.uint8) for _ in range(2)]
    dev = [_dev(b) for b in bufs]
    stacks, cur = None, 0
    for s, (raw, nf, term, gray, names) in enumerate(_stack_script(H, W, n)):
        what = 'acmi_atari_stack {} {} launch {} ({})'.format(
            _form(shape), 'in place' if in_place else 'out of place', s, 'mode 2 reset' if s == 0 else
            'mode 1 step, terminals {}'.format(list(term)))
        nxt = cur if in_place else 1 - cur
        d_raw, d_nf, d_term = _dev(raw), _dev(nf), _dev(term)
        _lib.call('acmi_atari_stack', _ptr(d_raw), raw[0].nbytes, raw[0, 0].nbytes, _ptr(d_nf), n, H, W,
                  _ptr(d_term), int(s == 0), _ptr(dev[cur]), _ptr(dev[nxt]), stride, _lib.stream_handle())
        torch.cuda.synchronize()
        if s == 0:
            stacks = [oracle.atari_stack(None, gray[e], reset=True) for e in range(n)]
        else:
            stacks = [oracle.atari_stack(stacks[e], gray[e], terminal=bool(term[e])) for e in range(n)]
        before = bufs[cur].copy()
        for e in range(n):
            bufs[nxt][e * stride:e * stride + STACK] = stacks[e].reshape(-1)
        _check_buffer(dev[nxt].cpu().numpy(), bufs[nxt], n, stride, STACK, what, names)
        if not in_place:
            assert np.array_equal(dev[cur].cpu().numpy(), before), what + ': stack_in was written'
        assert np.array_equal(d_raw.cpu().numpy(), raw), what + ': the frames were written'
        cur = nxt


def test_frame_pipeline_at_a_generic_shape(lib, cuda):
    from actorcritic.envs.atari import wrappers
    H, W = 100, 320
    n = 6
    pipe = wrappers.AtariFramePipeline(n, height=H, width=W)
    stacks = None
    for s, (raw, nf, term, gray, _) in enumerate(_stack_script(H, W, n)):
        pipe.load([(raw[e, 0], raw[e, 1] if nf[e] == 2 else None) for e in range(n)])
        got = (pipe.reset() if s == 0 else pipe.step(term.astype(bool))).cpu().numpy()
        if s == 0:
            stacks = [oracle.atari_stack(None, gray[e], reset=True) for e in range(n)]
        else:
            stacks = [oracle.atari_stack(stacks[e], gray[e], terminal=bool(term[e])) for e in range(n)]
        for e in range(n):
            assert np.array_equal(got[e], stacks[e]), ('AtariFramePipeline 100x320 generic <0,0>', s, e)


# ---------------------------------------------------------------------------
# acmi_atari_rollout_frames
# ---------------------------------------------------------------------------
def _rollout(lib, frames, nslots, H, W, n, step, reset, term, stack_in, in_stride, stack_out, out_stride, bad=None):
    import torch
    from actorcritic import _lib
    _lib.call('acmi_atari_rollout_frames', _ptr(frames), H * W * 3, nslots, H, W, n, _ptr(step), _ptr(reset),
              _ptr(term), stack_in, in_stride, stack_out, out_stride, _ptr(bad), _lib.stream_handle())
    torch.cuda.synchronize()


def _row_message(shape, c, e):
    row = cases.ROLLOUT_ROWS[c['cases'][e][:2]]
    msg = 'row {!r} terminal {}'.format(row, c['cases'][e][2])
    if row == 'reset-and-step' and shape[:2] in ((487, 84), (84, 484)):
        msg += ' (the LDS band is staged again after the reset frame went to rpix, runs of 7)'
    return msg


@SHAPES
@pytest.mark.parametrize('layout', ['strided-in', 'strided-out', 'in-place'])
def test_rollout_frames_every_row(lib, cuda, shape, layout):
    H, W = shape[:2]
    c = cases.rollout_case(H, W)
    n = c['N']
    what = 'acmi_atari_rollout_frames {} {}'.format(_form(shape), layout)
    frames, step, reset, term = _dev(c['frames']), _dev(c['step']), _dev(c['reset']), _dev(c['term'])
    rng = np.random.default_rng(7)
    in_stride = {'strided-in': 5 * STACK, 'strided-out': STACK, 'in-place': STACK}[layout]
    out_stride = {'strided-in': STACK, 'strided-out': 5 * STACK, 'in-place': STACK}[layout]
    in_off, out_off = (2 * STACK if layout == 'strided-in' else 0), (3 * STACK if layout == 'strided-out' else 0)
    # [n, 5] blocks of stacks as the rollout's obs[:, t]: the strided side uses one slot of five
    src0 = rng.integers(1, 256, n * in_stride + GUARD, dtype=np.uint8)
    for e in range(n):
        src0[in_off + e * in_stride:in_off + e * in_stride + STACK] = c['stacks'][e].reshape(-1)
    dst0 = src0 if layout == 'in-place' else rng.integers(1, 256, n * out_stride + GUARD, dtype=np.uint8)
    src = _dev(src0)
    dst = src if layout == 'in-place' else _dev(dst0)
    _rollout(lib, frames, 2 * n, H, W, n, step, reset, term, _ptr(src, in_off), in_stride, _ptr(dst, out_off),
             out_stride)
    expected = dst0.copy()
    for e in range(n):
        expected[out_off + e * out_stride:out_off + e * out_stride + STACK] = c['want'][e].reshape(-1)
    got = dst.cpu().numpy()
    wrong = []
    for e in range(n):
        lo = out_off + e * out_stride
        a, b = got[lo:lo + STACK], expected[lo:lo + STACK]
        if not np.array_equal(a, b):
            wrong.append('env {} {}: {} bytes differ'.format(e, _row_message(shape, c, e), int((a != b).sum())))
    assert not wrong, '{}: {}'.format(what, '; '.join(wrong))
    assert np.array_equal(got, expected), what + ': bytes outside the stacks were written'
    if layout != 'in-place':
        assert np.array_equal(src.cpu().numpy(), src0), what + ': stack_in was written'
    assert np.array_equal(frames.cpu().numpy(), c['frames']), what + ': the frames were written'


@SHAPES
def test_rollout_frames_null_terminals_null_stack_in_and_slot_guard(lib, cuda, shape):
    import torch
    H, W = shape[:2]
    c = cases.rollout_case(H, W)
    what = 'acmi_atari_rollout_frames ' + _form(shape)
    gray = c['grays']
    i32 = lambda *v: _dev(np.array(v, np.int32))
    # terminals NULL is 'no terminal': a step, a reset, a reset-and-step
    frames = _dev(c['frames'][:3])
    src = _dev(c['stacks'][:3])
    dst = torch.full((3 * STACK + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    _rollout(lib, frames, 3, H, W, 3, i32(0, -1, 2), i32(-1, 1, 0), None, _ptr(src), STACK, _ptr(dst), STACK)
    got = dst.cpu().numpy()
    want = [oracle.atari_stack(c['stacks'][0], gray[0]), oracle.atari_stack(None, gray[1], reset=True),
            oracle.atari_stack(oracle.atari_stack(None, gray[0], reset=True), gray[2])]
    for e in range(3):
        assert np.array_equal(got[e * STACK:(e + 1) * STACK], want[e].reshape(-1)), (what, 'terminals NULL', e)
    assert (got[3 * STACK:] == 0xA5).all(), what
    # stack_in NULL serves a batch of first resets (and a terminal step, which reads no stack)
    dst.fill_(0xA5)
    _rollout(lib, frames, 3, H, W, 3, i32(-1, -2, 2), i32(1, 0, -1), _dev(np.array([0, 0, 1], np.uint8)), None, 0,
             _ptr(dst), STACK)
    got = dst.cpu().numpy()
    want = [oracle.atari_stack(None, gray[1], reset=True), oracle.atari_stack(None, gray[0], reset=True),
            oracle.atari_stack(c['stacks'][2], gray[2], terminal=True)]
    for e in range(3):
        assert np.array_equal(got[e * STACK:(e + 1) * STACK], want[e].reshape(-1)), (what, 'stack_in NULL', e)
    assert (got[3 * STACK:] == 0xA5).all(), what
    # a slot >= nslots reads nothing: exactly nslots frames are allocated, that env's stack is
    # zero and it is counted once; the other envs are as without it
    nslots = 2
    frames = _dev(c['frames'][:nslots])
    bad = torch.zeros(1, dtype=torch.int32, device='cuda')
    dst.fill_(0xA5)
    args = (frames, nslots, H, W, 3, i32(1, nslots, 0), i32(-1, -1, 1), _dev(np.zeros(3, np.uint8)), _ptr(src), STACK,
            _ptr(dst), STACK, bad)
    _rollout(lib, *args)
    got = dst.cpu().numpy()
    assert int(bad.item()) == 1, what
    assert not got[STACK:2 * STACK].any(), what
    assert np.array_equal(got[:STACK], oracle.atari_stack(c['stacks'][0], gray[1]).reshape(-1)), what
    assert np.array_equal(got[2 * STACK:3 * STACK], oracle.atari_stack(
        oracle.atari_stack(None, gray[1], reset=True), gray[0]).reshape(-1)), what
    assert (got[3 * STACK:] == 0xA5).all(), what
    _rollout(lib, *args)  # the counter accumulates
    assert int(bad.item()) == 2, what


def test_frames_kernel_and_rollout_kernel_agree_at_250x160(lib, cuda):
    """The same frames and stacks through atari_frames_kernel<0,0> in mode 1 and through
    atari_rollout_kernel<0,0>'s plain step row: identical stacks (and the oracle's)."""
    import torch
    from actorcritic import _lib
    H, W = 250, 160
    fams = cases.family_frames(H, W)
    pick = [f for f in fams if f[0] in ('random', 'two-level', 'max-pair', 'Gmid')]
    n = len(pick)
    raw = np.stack([a for _, a, _ in pick])
    rng = np.random.default_rng(11)
    stacks = rng.integers(0, 256, (n, OUT, OUT, 4), dtype=np.uint8)
    term = np.array([0, 1, 0, 0], np.uint8)
    d_raw, d_in, d_term = _dev(raw), _dev(stacks), _dev(term)
    a = torch.full((n * STACK,), 0xA5, dtype=torch.uint8, device='cuda')
    b = torch.full((n * STACK,), 0x5A, dtype=torch.uint8, device='cuda')
    _lib.call('acmi_atari_stack', _ptr(d_raw), raw[0].nbytes, 0, None, n, H, W, _ptr(d_term), 0, _ptr(d_in), _ptr(a),
              STACK, _lib.stream_handle())
    _rollout(lib, d_raw, n, H, W, n, _dev(np.arange(n, dtype=np.int32)), _dev(np.full(n, -1, np.int32)), d_term,
             _ptr(d_in), STACK, _ptr(b), STACK)
    assert torch.equal(a, b), '250x160 generic <0,0>: frames kernel mode 1 and rollout step row differ'
    ref = cases.oracle_gray(H, W)
    for e, (name, _, _) in enumerate(pick):
        want = oracle.atari_stack(stacks[e], ref[name][0], terminal=bool(term[e]))
        assert np.array_equal(a[e * STACK:(e + 1) * STACK].cpu().numpy(), want.reshape(-1)), (name, e)
