"""Input families of the value-domain tests (test_gpu_value_domain.py,
test_value_domain_host.py): images, weights and head gradients away from the one
distribution the other accuracy tests draw from (He-Gaussian weights, uniformly random
bytes, randn / B head gradients).

Plain numpy / torch on the CPU: no GPU, no libacmi.  Everything is a pure function of
its arguments (a seed where something is drawn).  Images are [B,84,84,4] uint8 torch
tensors, weights flat float32 torch tensors in the parameter layout of
oracle.param_offsets, head gradients [B, A+1] float32 torch tensors.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
import oracle  # noqa: E402

IMAGE_FAMILIES = ('zeros', 'full', 'catch', 'breakout', 'one_pixel', 'binary', 'saturating', 'random')
LAYERS = ('conv1', 'conv2', 'conv3', 'fc4')
WEIGHT_FAMILIES = (('base',) + tuple('%s*2^%d' % (l, k) for l in LAYERS for k in (6, -6)) +
                   ('outlier', 'heavy_tail', 'dead_half', 'dead_conv1', 'zero_bias'))
DHEAD_FAMILIES = ('base', 'outlier_row', 'half_zero', 'zero', 'value_only', 'policy_only', '*2^-40', '*2^20')

# the ranges of the wide families (test_value_domain_host.py holds each to the
# non-vacuity condition: plain float32 arithmetic of the reference formulas alone
# stays below every block's tolerance)
OUTLIER_LOG2 = 10
HEAVY_TAIL_SIGMA = 2.0
# `binary` pixels are 0 or BINARY_LEVEL.  Level 1 is past what conv1's pixel operand
# holds (f16x2.hpp u8x8_to_f16: the bytes enter the MFMA as f16 subnormals, which its
# adder does not normalise -- a batch lit only by bytes below ~8 loses the low bits of
# the weight gradient; measured in test_gpu_value_domain.py's docstring), so the case
# sits at the smallest level that is a power of two and holds the tolerance with room.
BINARY_LEVEL = 16


# ---------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------
def rand_params(A, C3, seed=0, scale=1.0):
    """test_gpu_kernels.rand_params on the CPU, without the library: the same draws
    (He-scaled Gaussian weights, biases 0.1 N(0,1)) in the same order."""
    g = torch.Generator().manual_seed(seed)
    off, n = oracle.param_offsets(A, C3)
    p = torch.empty(n, dtype=torch.float32)
    fans = [256, 1, 512, 1, 576, 1, 49 * C3, 1, 512, 1, 512, 1]
    for o, e, f in zip(off, off[1:] + [n], fans):
        p[o:e] = torch.randn(e - o, generator=g) * (scale * (2.0 / f) ** 0.5 if f > 1 else 0.1)
    return p


def blocks(params, A, C3):
    """The 12 blocks (views of params): w1 [256,32], b1, w2 [512,64], b2, w3 [576,C3],
    b3, w4 [49*C3,512], b4, wp [512,A], bp, wv [512,1], bv."""
    off, n = oracle.param_offsets(A, C3)
    shapes = [(256, 32), (32,), (512, 64), (64,), (576, C3), (C3,), (49 * C3, 512), (512,), (512, A), (A,), (512, 1),
              (1,)]
    return [params[o:e].view(s) for o, e, s in zip(off, off[1:] + [n], shapes)]


def weights(family, A, C3, seed):
    """One weight family (WEIGHT_FAMILIES) from rand_params(A, C3, seed)."""
    p = rand_params(A, C3, seed)
    b = blocks(p, A, C3)
    if family == 'base':
        pass
    elif '*2^' in family:  # one layer's W and b scaled by a power of two
        layer, k = family.split('*2^')
        l = LAYERS.index(layer)
        b[2 * l].mul_(2.0 ** int(k))
        b[2 * l + 1].mul_(2.0 ** int(k))
    elif family == 'outlier':  # one weight of each conv layer far above the rest
        g = torch.Generator().manual_seed(seed + 1)
        for l in range(3):
            w = b[2 * l].view(-1)
            i = int(torch.randint(0, w.numel(), (1,), generator=g))
            w[i] = 2.0 ** OUTLIER_LOG2 * w.abs().max()
    elif family == 'heavy_tail':  # log-normal magnitudes on every weight
        g = torch.Generator().manual_seed(seed + 2)
        for l in range(6):
            b[2 * l].mul_(torch.exp(HEAVY_TAIL_SIGMA * torch.randn(b[2 * l].shape, generator=g)))
    elif family == 'dead_half':  # conv1 channels 0..15 never fire
        b[0][:, :16] = -b[0][:, :16].abs()
        b[1][:16] = -b[1][:16].abs()
    elif family == 'dead_conv1':  # no conv1 channel fires: the a1 bound is 0
        b[0].copy_(-b[0].abs())
        b[1].copy_(-b[1].abs())
    elif family == 'zero_bias':
        for l in range(6):
            b[2 * l + 1].zero_()
    else:
        raise ValueError(family)
    return p


def conv1_bound(params, A, C3):
    """float64 B1[c] = sum_k max(W1[k][c], 0) + max(b1[c], 0) (band.hpp), the channel
    c* of the largest positive weight mass, and that mass per channel."""
    b = blocks(params, A, C3)
    mass = b[0].double().clamp(min=0).sum(0)
    return mass + b[1].double().clamp(min=0), int(mass.argmax()), mass


# ---------------------------------------------------------------------------
# images
# ---------------------------------------------------------------------------
def game_stacks(game, B, seed):
    """B frame stacks of HostGame(game) under random actions, stacked by the host
    FrameStackWrapper.  Image 0 is a stack straight after a reset (one frame four
    times), image 1 a stack straight after a terminal (the three old channels zero);
    the others are taken 1..59 steps into play (episodes restart on the way)."""
    from actorcritic.envs.atari.wrappers import FrameStackWrapper
    from actorcritic.envs.games.host import GAME_ACTIONS, HostGame
    rng = np.random.default_rng(seed)
    out = np.empty((B, 84, 84, 4), np.uint8)
    for i in range(B):
        env = FrameStackWrapper(HostGame(game, seed=seed, env_id=i), 4)
        s = env.reset()
        steps = 0 if i == 0 else (10 ** 6 if i == 1 else int(rng.integers(1, 60)))
        for t in range(steps):
            s, _, terminal, _ = env.step(int(rng.integers(0, GAME_ACTIONS[game])))
            if terminal:
                if i == 1:
                    break
                if t + 1 < steps:
                    s = env.reset()
        out[i] = s
    return torch.from_numpy(out)


def is_reset_stack(img):
    """One nonzero frame four times."""
    return bool(img.any()) and all(torch.equal(img[..., c], img[..., 3]) for c in range(3))


def is_post_terminal_stack(img):
    """The three old channels zero, the newest frame not."""
    return bool(img[..., 3].any()) and not bool(img[..., :3].any())


# a pixel only conv1's last output column reads: column 19 covers x = 76..83, column 18
# x = 72..79, so x >= 80 belongs to column 19 alone
ONE_PIXEL_POSITIONS = [(0, 0, 0), (83, 83, 3), (40, 82, 1), (10, 10, 0), (10, 10, 1), (10, 10, 2), (10, 10, 3)]


def one_pixel(B, seed):
    rng = np.random.default_rng(seed)
    out = np.zeros((B, 84, 84, 4), np.uint8)
    for i in range(B):
        y, x, c = ONE_PIXEL_POSITIONS[i] if i < len(ONE_PIXEL_POSITIONS) else (
            int(rng.integers(0, 84)), int(rng.integers(0, 84)), int(rng.integers(0, 4)))
        out[i, y, x, c] = 255
    return torch.from_numpy(out)


def saturating(params, A, C3, B, seed):
    """Half the batch (the even images): patch (0,0) holds 255 where W1[:, c*] > 0, all
    else 0, so a1[0,0,c*] = sum_k max(W1[k][c*], 0) + b1[c*], which is the bound B1[c*]
    when b1[c*] >= 0.  The odd images are Catch stacks."""
    _, cstar, _ = conv1_bound(params, A, C3)
    w = blocks(params, A, C3)[0][:, cstar].view(8, 8, 4)  # rows (kh, kw, c)
    out = game_stacks('catch', B, seed)
    out[0::2] = 0
    out[0::2, :8, :8, :] = (w > 0).to(torch.uint8) * 255
    return out


def images(family, B, seed, params=None, A=None, C3=None):
    """One image family (IMAGE_FAMILIES); 'saturating' needs the weights."""
    if family == 'zeros':
        return torch.zeros(B, 84, 84, 4, dtype=torch.uint8)
    if family == 'full':
        return torch.full((B, 84, 84, 4), 255, dtype=torch.uint8)
    if family in ('catch', 'breakout'):
        return game_stacks(family, B, seed)
    if family == 'one_pixel':
        return one_pixel(B, seed)
    if family == 'binary':
        return BINARY_LEVEL * torch.randint(0, 2, (B, 84, 84, 4), generator=torch.Generator().manual_seed(seed),
                                            dtype=torch.uint8)
    if family == 'saturating':
        return saturating(params, A, C3, B, seed)
    if family == 'random':
        return torch.randint(0, 256, (B, 84, 84, 4), generator=torch.Generator().manual_seed(seed),
                             dtype=torch.uint8)
    raise ValueError(family)


# ---------------------------------------------------------------------------
# head gradients
# ---------------------------------------------------------------------------
def dheads(family, B, A, seed):
    """One head-gradient family (DHEAD_FAMILIES): [B, A+1] f32, column A the value's."""
    d = torch.randn(B, A + 1, generator=torch.Generator().manual_seed(seed)) / B
    if family == 'base':
        pass
    elif family == 'outlier_row':
        d[B // 3] *= 2.0 ** 12
    elif family == 'half_zero':
        d[0::2] = 0.0
    elif family == 'zero':
        d.zero_()
    elif family == 'value_only':
        d[:, :A] = 0.0
    elif family == 'policy_only':
        d[:, A] = 0.0
    elif family.startswith('*2^'):
        d *= 2.0 ** int(family[3:])
    else:
        raise ValueError(family)
    return d


def inputs(case_inputs, A, C3, B, seed):
    """(images family, weights family, dhead family) -> (obs u8, params f32, dhead f32),
    all on the CPU."""
    img, wfam, dfam = case_inputs
    params = weights(wfam, A, C3, seed)
    obs = images(img, B, seed + 10, params, A, C3)
    return obs, params, dheads(dfam, B, A, seed + 20)
