"""Host-stepped envs on the device rollout path, the parts that need no GPU: the
acmi_atari_rollout_frames entry point's argument checks, the slot planner of
HostAtariEnvs, and MultiEnv's recognition of the adaptor (tests/test_gpu_host_envs.py
has the kernel and the rollout)."""
import ctypes

import numpy as np
import pytest

H, W = 210, 160
FRAME = H * W * 3
STACK = 4 * 84 * 84


def test_rollout_frames_symbol_is_exported(lib):
    from actorcritic import _lib
    assert 'acmi_atari_rollout_frames' in _lib.EXPORTED
    assert lib.acmi_atari_rollout_frames.argtypes is not None and len(lib.acmi_atari_rollout_frames.argtypes) == 15
    assert lib.acmi_abi_version() == 4


_BUFFERS = (ctypes.create_string_buffer(2 * FRAME + 16), (ctypes.c_int32 * 2)(0, -1),
            ctypes.create_string_buffer(2 * STACK + 16))


def _call(lib, **kw):
    """One env, one frame, a step without reset: every argument valid unless overridden.
    Host buffers: an argument error returns before anything is enqueued."""
    frames, slots, stack = _BUFFERS
    a = dict(frames=ctypes.addressof(frames), frame_stride=FRAME, nslots=1, H=H, W=W, N=1,
             step_slot=ctypes.addressof(slots), reset_slot=ctypes.addressof(slots) + 4, terminals=None,
             stack_in=ctypes.addressof(stack), in_stride=STACK, stack_out=ctypes.addressof(stack) + STACK,
             out_stride=STACK, bad_envs=None)
    a.update(kw)
    status = lib.acmi_atari_rollout_frames(a['frames'], a['frame_stride'], a['nslots'], a['H'], a['W'], a['N'],
                                           a['step_slot'], a['reset_slot'], a['terminals'], a['stack_in'],
                                           a['in_stride'], a['stack_out'], a['out_stride'], a['bad_envs'], None)
    return status, a


@pytest.mark.parametrize('bad', [
    dict(H=168, W=168, frame_stride=168 * 168 * 3),  # both integer ratios: cv2's fast path, not restated
    dict(H=80, frame_stride=80 * W * 3),             # below 84
    dict(W=162, frame_stride=H * 162 * 3),           # W not a multiple of 4
    dict(H=510, W=84, frame_stride=510 * 84 * 3),    # above 6 * 84
    dict(H=300, W=160, frame_stride=300 * 160 * 3),  # H * W > 40960
    dict(frame_stride=FRAME + 2),                    # misaligned strides
    dict(in_stride=STACK + 2),
    dict(out_stride=STACK + 2),
    dict(frame_stride=FRAME - 4),                    # frames would overlap
    dict(out_stride=STACK - 4),                      # stacks would overlap
    dict(in_stride=STACK - 4),
    dict(nslots=-1),
    dict(N=-1),
    dict(N=65536),                                   # above the grid's y extent
    dict(frames=None),
    dict(stack_out=None),
    dict(step_slot=None),
    dict(reset_slot=None),
], ids=lambda d: ','.join('{}={}'.format(k, v) for k, v in d.items()))
def test_rollout_frames_rejects_bad_arguments(lib, bad):
    status, _ = _call(lib, **bad)
    assert status == -1, bad
    assert b'acmi_atari_rollout_frames' in lib.acmi_last_error()


def test_rollout_frames_rejects_misaligned_pointers_and_in_place_with_two_strides(lib):
    _, a = _call(lib, N=0)
    for name in ('frames', 'stack_in', 'stack_out'):
        assert _call(lib, **{name: a[name] + 2})[0] == -1, name
    # in place needs one stride for both sides
    assert _call(lib, stack_out=a['stack_in'], in_stride=STACK, out_stride=2 * STACK)[0] == -1


def test_rollout_frames_accepts_an_empty_batch(lib):
    # N = 0 with otherwise valid arguments: nothing to launch, no error (so the
    # rejections above are about the argument they name)
    assert _call(lib, N=0)[0] == 0
    assert _call(lib, N=0, stack_in=None, in_stride=0)[0] == 0  # no stack_in: its stride is not looked at


@pytest.mark.parametrize('terminated', [
    [False] * 6,
    [True] * 6,
    [True, False, False, False, False, False],
    [False, False, False, False, False, True],
    [False, True, True, False, True, False],
])
def test_slot_planner(terminated):
    from actorcritic.envs.atari.wrappers import plan_host_step
    N = len(terminated)
    step_slot, reset_slot, K = plan_host_step(terminated)
    assert step_slot.dtype == np.int32 and reset_slot.dtype == np.int32
    assert K == sum(terminated)
    assert list(step_slot) == list(range(N))  # the step frames: slots 0..N-1
    # the reset frames: packed behind them in env order, -1 where the env goes on
    want, k = [], 0
    for flag in terminated:
        want.append(N + k if flag else -1)
        k += int(flag)
    assert list(reset_slot) == want
    assert max(max(step_slot), max(reset_slot)) < N + K  # what a step uploads: N + K frames


class _Adaptor(object):
    host_stepped = True
    num_envs = 3
    observation_space = 'obs-space'
    action_space = 'act-space'

    def __init__(self):
        self.calls = []

    def reset(self):
        self.calls.append('reset')
        return 'stacks'

    def step(self, actions):
        self.calls.append(('step', list(actions)))
        return 'next'

    def close(self):
        self.calls.append('close')


def test_multi_env_recognises_the_host_stepped_adaptor():
    from actorcritic.multi_env import MultiEnv
    adaptor = _Adaptor()
    m = MultiEnv(adaptor)
    assert m.batched is adaptor and m.envs is adaptor
    assert (m.num_envs, m.observation_space, m.action_space) == (3, 'obs-space', 'act-space')
    assert m.reset() == 'stacks' and m.step([0, 1, 2]) == 'next'
    m.close()
    assert adaptor.calls == ['reset', ('step', [0, 1, 2]), 'close']


def test_multi_env_on_a_plain_list_still_auto_resets():
    from actorcritic.multi_env import MultiEnv, _AutoResetWrapper

    class Env(object):
        observation_space = action_space = None
        host_stepped = True  # on a member env the marker means nothing

        def reset(self):
            return 0

        def step(self, a):
            return a, 0.0, False, {}

    m = MultiEnv([Env(), Env()])
    try:
        assert m.batched is None
        assert all(isinstance(e, _AutoResetWrapper) for e in m.envs)
        assert m.step([5, None])[0] == [5, None]
    finally:
        m.close()


def test_host_atari_envs_is_marked_and_make_atari_env_passes_preprocess_through():
    import inspect
    from actorcritic.envs.atari import wrappers
    assert wrappers.HostAtariEnvs.host_stepped is True
    assert inspect.signature(wrappers.make_atari_env).parameters['preprocess'].default is True
