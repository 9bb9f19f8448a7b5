"""Shapes, frame families and references for the Atari frame kernels (csrc/atari.hip):
atari_frames_kernel (acmi_atari_preprocess / acmi_atari_stack) and atari_rollout_kernel
(acmi_atari_rollout_frames), each compiled in a <3,3> form (run lengths fixed at 3) and a
<0,0> form (runs of up to 8 entries taken from the table).  numpy and the oracle only:
tests/test_atari_frame_cases_host.py proves the claims made here on the CPU,
tests/test_gpu_atari_shapes.py runs the kernels.

References.  The kernels are byte work in a fixed float32 order, so the GPU tests are
bit-exact against oracle.atari_preprocess / oracle.atari_stack.  That oracle is itself a
restatement (of cv2's tables), so at the shapes used here it is guarded by an independent
float64 area integral (integral_resize below, which does not use oracle.area_tables):
destination pixel (dy, dx) is the mean of the gray image over
[dy*sy, (dy+1)*sy) x [dx*sx, (dx+1)*sx), s = size / 84.

Bound of |oracle - integral| for one pixel (oracle_bound):
  * 0.5: the oracle rounds to an integer, half to even;
  * float32: u = 2^-24.  One destination pixel with runs of ny rows and nx columns is
        sum_j f32(beta_j) * (sum_k S * f32(alpha_k))
    with every product and every add rounded: per (j, k) the weight's conversion, the
    product and the add (3 ny nx roundings), per j the same three for beta (3 ny).  Every
    intermediate is at most 255 (1 + small), so each rounding moves the result by at most
    255 u:  3 (ny nx + ny) * 255 u  with the longest runs of the shape;
  * tables: cv2 drops a leading or trailing piece of a run that is at most 1e-3 wide and
    clips the last cell to the image.  A cell boundary is d * size / 84, whose fractional
    part is a multiple of 1/84 = 0.0119: it is either 0 or more than ten times the
    threshold, so the only pieces ever dropped or clipped are those that exact arithmetic
    makes 0 and the table's doubles make non-zero.  scale = 1 / (84 / size) carries two
    double roundings, d * scale a third, + scale a fourth, on values of at most 504:
    a boundary is off by at most eb = 4 * 2^-53 * 504 = 2.2e-13.  Per axis that moves the
    two end weights by eb each, every weight by eb relative (the divisor `cell`), and
    drops at most two pieces of eb: at most 5 eb of weight, 10 eb for both axes, times 255
    = 5.7e-10.
Measured on the CPU (test_oracle_stays_within_its_bound_of_the_integral, over all frame
families, single frames and pairs): worst |oracle - integral| - 0.5 per shape beside the
bound's excess over 0.5 --
    shape      worst excess   bound - 0.5
    210x160     2.6e-12        5.5e-04
    100x92     -8.7e-04        5.5e-04
    84x88       2.6e-12        1.4e-04
    168x160     2.7e-12        3.6e-04
    250x160     2.9e-12        7.3e-04
    100x320     2.9e-12        8.2e-04
    256x160     2.8e-12        7.3e-04
    84x484     -4.1e-03        3.6e-04
    487x84     -1.0e-03        6.4e-04
(the 3e-12 are exact ties: the integral is k + 0.5 up to its own double roundings and the
oracle rounds them half to even, as cv2 does).  The oracle stays within the bound at
every shape.
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
import oracle  # noqa: E402

OUT = 84
K_MAX_TAB = 8          # atari.hip kMaxTab
BANDS, BAND_ROWS = 4, 21
AREA_RUN_BYTES = 4 + 4 + 4 * K_MAX_TAB  # struct AreaRun {int first, count; float alpha[8];}
LDS_LIMIT = 64 * 1024
MAX_AREA = 40960
U32 = 2.0 ** -24
STACK = 4 * OUT * OUT

# (H, W, fixed3, longest y run, longest x run, why the shape is here)
SHAPES = [
    (210, 160, True, 3, 3, "the workload's shape"),
    (100, 92, True, 3, 3, 'small, runs of 3 both ways (it was once labelled generic)'),
    (84, 88, True, 1, 2, 'smallest; y scale exactly 1.0 (runs of 1)'),
    (168, 160, True, 2, 3, 'integer ratio in y only: accepted, y weights exactly 0.5'),
    (250, 160, False, 4, 3, 'generic through y alone'),
    (100, 320, False, 3, 5, 'generic through x alone'),
    (256, 160, False, 4, 3, 'H*W == 40960, the bound itself'),
    (84, 484, False, 1, 7, 'minimum H, largest W that fits; x runs of 7'),
    (487, 84, False, 7, 1, 'largest H that fits, minimum W; y runs of 7, most source rows per band'),
]
SHAPE_IDS = ['{}x{}-{}'.format(s[0], s[1], 'fixed3' if s[2] else 'generic') for s in SHAPES]
HW = [(s[0], s[1]) for s in SHAPES]

# acmi_atari_rollout_frames' table (has step frame, has reset frame, terminal flag): every
# row, the terminal flag both ways (it only matters where the env stepped)
CASES = [(True, False, 0), (True, False, 1), (True, True, 0), (True, True, 1), (False, True, 0), (False, True, 1),
         (False, False, 1)]
ROLLOUT_ROWS = {(True, False): 'step', (True, True): 'reset-and-step', (False, True): 'reset', (False, False): 'idle'}

# what tests/test_gpu_atari_shapes.py runs: (kernel, mode, H, W).  The frames kernel's modes
# are its `mode` argument (0 gray, 1 stack step, 2 stack reset); the rollout kernel's are
# the rows of its table.  The host test turns (H, W) into the form through acmi_atari_plan.
GPU_COMBOS = [('frames', m, H, W) for H, W in HW for m in (0, 1, 2)] + \
             [('rollout', r, H, W) for H, W in HW for r in sorted(set(ROLLOUT_ROWS.values()))]


def allowed(H, W):
    """The documented rule (include/acmi.h): sides in [84, 504], W a multiple of 4,
    H*W <= 40960, not both sides multiples of 84."""
    return (OUT <= H <= 6 * OUT and OUT <= W <= 6 * OUT and W % 4 == 0 and H * W <= MAX_AREA
            and not (H % OUT == 0 and W % OUT == 0))


@functools.lru_cache(maxsize=None)
def tables(ssize):
    return oracle.area_tables(ssize)


def max_run(ssize):
    return max(len(a) for _, a in tables(ssize))


def band_source_rows(H, band):
    """Source rows band `band` (output rows 21*band .. 21*band+20) stages: first source row
    of its first output row through last source row of its last."""
    t = tables(H)
    first, last = t[band * BAND_ROWS], t[band * BAND_ROWS + BAND_ROWS - 1]
    return first[0], last[0] + len(last[1]) - 1


# ---------------------------------------------------------------------------
# frame families: (name, last, prev) per shape; prev is the frame before `last` that the
# frameskip max-pools with it (a single-frame case uses `last` alone)
# ---------------------------------------------------------------------------
# mid values at which the gray's rounding term decides the byte: (v * c + 8192) >> 14 differs
# from (v * c) >> 14.  255 does so for G only (149.68); 127 for R (37.97) and G (74.55), 128
# for B (14.59)
PURE = [('R255', 0, 255), ('G255', 1, 255), ('B255', 2, 255), ('Rmid', 0, 127), ('Gmid', 1, 127), ('Bmid', 2, 128)]


# (the order the tests batch them in: eight envs a launch, so the pair and the pattern ride
# in the first launch with the first pure-channel frames)
FAMILY_NAMES = ['random', 'zeros', 'full', 'max-pair', 'two-level'] + [p[0] for p in PURE]


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def family_frames(H, W):
    rng = np.random.default_rng(1000 * H + W)
    fams = [('random', rng.integers(0, 256, (H, W, 3), dtype=np.uint8),
             rng.integers(0, 256, (H, W, 3), dtype=np.uint8)),
            ('zeros', np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.uint8)),
            ('full', np.full((H, W, 3), 255, np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8))]
    for name, ch, v in PURE:
        f = np.zeros((H, W, 3), np.uint8)
        f[..., ch] = v
        fams.append((name, f, np.zeros((H, W, 3), np.uint8)))
    # two levels, edges every 3 rows and 5 columns: no multiple of any scale here but 1.0, so
    # they fall inside resampling cells; prev is the pattern moved by (1, 2)
    yy, xx = np.mgrid[0:H, 0:W]
    two = np.where(((yy // 3 + xx // 5) % 2) == 1, 255, 0).astype(np.uint8)
    two2 = np.where((((yy + 1) // 3 + (xx + 2) // 5) % 2) == 1, 255, 0).astype(np.uint8)
    fams.append(('two-level', np.repeat(two[..., None], 3, -1), np.repeat(two2[..., None], 3, -1)))
    # neither frame dominates: bytes alternate high / low along the row, opposite in the two
    # frames (3 W bytes a row, so the phase also alternates between the dwords of a row)
    hi = rng.integers(200, 256, (H, W * 3), dtype=np.uint8)
    lo = rng.integers(0, 56, (H, W * 3), dtype=np.uint8)
    even = (np.arange(W * 3) % 2 == 0)[None, :]
    fams.append(('max-pair', np.where(even, hi, lo).reshape(H, W, 3), np.where(even, lo, hi).reshape(H, W, 3)))
    by = {n: (a, b) for n, a, b in fams}
    return tuple((n, _ro(np.ascontiguousarray(by[n][0])), _ro(np.ascontiguousarray(by[n][1]))) for n in FAMILY_NAMES)



@functools.lru_cache(maxsize=None)
def oracle_gray(H, W):
    """name -> (oracle.atari_preprocess(last), oracle.atari_preprocess(last, prev))."""
    return {n: (_ro(oracle.atari_preprocess(a)), _ro(oracle.atari_preprocess(a, b))) for n, a, b in family_frames(H, W)}


# ---------------------------------------------------------------------------
# the float64 area integral
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def integral_weights(ssize):
    """[84][ssize] float64: the overlap of [d*s, (d+1)*s) with the unit cell [p, p+1) of every
    source coordinate, over s (s = ssize / 84)."""
    s = ssize / float(OUT)
    d = np.arange(OUT, dtype=np.float64)[:, None]
    p = np.arange(ssize, dtype=np.float64)[None, :]
    lo, hi = d * ssize / OUT, (d + 1) * ssize / OUT
    return np.clip(np.minimum(hi, p + 1) - np.maximum(lo, p), 0.0, None) / s


def integral_resize(gray):
    H, W = gray.shape
    return integral_weights(H) @ gray.astype(np.float64) @ integral_weights(W).T


def oracle_bound(H, W):
    """(0.5, float32 term, table term) of the module docstring."""
    ny, nx = max_run(H), max_run(W)
    eb = 4 * 2.0 ** -53 * 6 * OUT
    return 0.5, 3 * (ny * nx + ny) * 255 * U32, 10 * eb * 255


# ---------------------------------------------------------------------------
# one launch of acmi_atari_rollout_frames per shape: the seven rows over five frames
# ---------------------------------------------------------------------------
def rollout_expected(stack, G, R, term):
    """One env's row of the table, through the oracle's FrameStackWrapper."""
    if G is None and R is None:
        return stack
    if G is None:
        return oracle.atari_stack(None, R, reset=True)
    if R is not None:
        stack = oracle.atari_stack(None, R, reset=True)
    return oracle.atari_stack(stack, G, terminal=term)


@functools.lru_cache(maxsize=None)
def rollout_case(H, W):
    """Five distinct frames (random, full, two-level, max-pair, random prev) over
    nslots = 2N slots, one env per row of CASES in a drawn order."""
    fams = {n: (a, b) for n, a, b in family_frames(H, W)}
    gray = oracle_gray(H, W)
    distinct = [fams['random'][0], fams['full'][0], fams['two-level'][0], fams['max-pair'][0], fams['random'][1]]
    grays = [gray['random'][0], gray['full'][0], gray['two-level'][0], gray['max-pair'][0],
             _ro(oracle.atari_preprocess(fams['random'][1]))]
    N = len(CASES)
    rng = np.random.default_rng(H * 7 + W)
    which = rng.integers(0, 5, 2 * N)
    which[:5] = rng.permutation(5)
    cases = [CASES[i] for i in rng.permutation(N)]
    step = np.array([rng.integers(0, 2 * N) if c[0] else -1 - rng.integers(0, 3) for c in cases], np.int32)
    reset = np.array([rng.integers(0, 2 * N) if c[1] else -1 - rng.integers(0, 3) for c in cases], np.int32)
    term = np.array([c[2] for c in cases], np.uint8)
    stacks = rng.integers(0, 256, (N, OUT, OUT, 4), dtype=np.uint8)
    want = [rollout_expected(stacks[n], grays[which[step[n]]] if step[n] >= 0 else None,
                             grays[which[reset[n]]] if reset[n] >= 0 else None, bool(term[n])) for n in range(N)]
    return dict(H=H, W=W, N=N, frames=_ro(np.stack([distinct[i] for i in which])),
                grays=[grays[i] for i in which], step=_ro(step), reset=_ro(reset), term=_ro(term),
                stacks=_ro(stacks), want=_ro(np.stack(want)), cases=cases)
