"""CPU tests of the device games' cuts: episodic life, the step cap and
truncation in the rule book (HostGame), the C-ABI of acmi_game_step_cuts /
acmi_returns_trunc / acmi_gae_trunc, and the oracle of the truncation-aware targets: a
numpy float32 restatement in the kernels' operation order, cross-checked against a
float64 recursion.  tests/test_gpu_game_cuts.py compares the kernels with what is here
(CutsReplay, the restatements, the target cases)."""
import ctypes
import os
import re

import numpy as np
import pytest

from actorcritic import _lib
from actorcritic.envs.games import host
from actorcritic.envs.games.host import HostGame
from actorcritic.objectives import gamma_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('acmi_game_step_cuts', 'acmi_returns_trunc', 'acmi_gae_trunc')
NAN_BITS = 0x7fc00000
BX, BY, VX, VY, PX, LIVES, B0 = range(7)
GAMMA = 0.99
TARGET_SHAPES = ((1, 1), (3, 5), (65, 20))  # 65 crosses the GAE kernel's 64-thread block


# -- the targets' oracle ----------------------------------------------------------------
def returns_trunc_f32(rewards, terminals, truncated, values, v_boot, gamma):
    """float32 restatement of acmi_returns_trunc: (targets, advantages).  The sum runs
    over ascending i to the first terminal `stop` at or after t; the bootstrap term is
    boot_pow[stop+1-t] * V_{stop+1} when stop is a truncated terminal, boot_pow[T-t] *
    v_boot without a terminal, 0 otherwise (V_T = v_boot)."""
    r = np.asarray(rewards, np.float32)
    d, tr = np.asarray(terminals, bool), np.asarray(truncated, bool)
    v, vb = np.asarray(values, np.float32).reshape(r.shape), np.asarray(v_boot, np.float32)
    N, T = r.shape
    gp, bp = gamma_tables(gamma, T)
    tgt = np.zeros((N, T), np.float32)
    for n in range(N):
        nxt = T
        for t in range(T - 1, -1, -1):
            if d[n, t]:
                nxt = t
            stop = nxt if nxt < T else T - 1
            acc = np.float32(0)
            for i in range(t, stop + 1):
                acc = np.float32(acc + np.float32(r[n, i] * gp[i - t]))
            if nxt == T:
                boot = np.float32(bp[T - t] * vb[n])
            elif tr[n, stop]:
                boot = np.float32(bp[stop + 1 - t] * (v[n, stop + 1] if stop + 1 < T else vb[n]))
            else:
                boot = np.float32(0)
            tgt[n, t] = np.float32(acc + boot)
    return tgt, (tgt - v).astype(np.float32)


def gae_trunc_f32(rewards, terminals, truncated, values, v_boot, gamma, lam):
    """float32 restatement of acmi_gae_trunc: (targets, advantages).  live = d_t == 0,
    boot = live or trunc_t; delta_t = (r_t + (boot ? gamma V_{t+1} : 0)) - V_t,
    A_t = delta_t + (live ? gamma lambda A_{t+1} : 0), target_t = A_t + V_t."""
    r = np.asarray(rewards, np.float32)
    d, tr = np.asarray(terminals, bool), np.asarray(truncated, bool)
    v, vb = np.asarray(values, np.float32).reshape(r.shape), np.asarray(v_boot, np.float32)
    g, gl = np.float32(gamma), np.float32(np.float32(gamma) * np.float32(lam))
    N, T = r.shape
    adv, tgt = np.zeros((N, T), np.float32), np.zeros((N, T), np.float32)
    zero = np.float32(0)
    for n in range(N):
        next_v, last = vb[n], zero
        for t in range(T - 1, -1, -1):
            live = not d[n, t]
            boot = live or tr[n, t]
            delta = np.float32(np.float32(r[n, t] + (np.float32(g * next_v) if boot else zero)) - v[n, t])
            last = np.float32(delta + (np.float32(gl * last) if live else zero))
            adv[n, t] = last
            tgt[n, t] = np.float32(last + v[n, t])
            next_v = v[n, t]
    return tgt, adv


def targets_trunc_f64(rewards, terminals, truncated, values, v_boot, gamma, lam=None):
    """The float64 recursion: n-step (lam None) or GAE(lam) targets and advantages.  A
    terminal cuts the return; a truncated one restarts it from V of the next step."""
    r = np.asarray(rewards, np.float64)
    d = np.asarray(terminals, bool)
    tr = np.asarray(truncated, bool) & d  # read only where terminals is set
    v, vb = np.asarray(values, np.float64).reshape(r.shape), np.asarray(v_boot, np.float64)
    N, T = r.shape
    tgt, adv = np.zeros((N, T)), np.zeros((N, T))
    for n in range(N):
        ret, next_v, last = vb[n], vb[n], 0.0
        for t in range(T - 1, -1, -1):
            if d[n, t]:
                ret = next_v if tr[n, t] else 0.0
            ret = r[n, t] + gamma * ret
            keep = 0.0 if d[n, t] and not tr[n, t] else 1.0
            live = 0.0 if d[n, t] else 1.0
            last = r[n, t] + gamma * next_v * keep - v[n, t] + gamma * (lam or 0.0) * live * last
            tgt[n, t], adv[n, t] = (ret, ret - v[n, t]) if lam is None else (last + v[n, t], last)
            next_v = v[n, t]
    return tgt, adv


def random_case(N, T, seed=0, zero_trunc=False):
    """(rewards, terminals, truncated, values, v_boot): truncated is set at random, also
    where terminals is not (there it is ignored)."""
    rng = np.random.default_rng([seed, N, T])
    r = rng.choice([-1.0, 0.0, 1.0], size=(N, T)).astype(np.float32)
    d = (rng.random((N, T)) < 0.15).astype(np.uint8)
    tr = np.zeros((N, T), np.uint8) if zero_trunc else (rng.random((N, T)) < 0.5).astype(np.uint8)
    v = rng.normal(0, 1, size=(N, T)).astype(np.float32)
    vb = rng.normal(0, 1, size=N).astype(np.float32)
    return r, d, tr, v, vb


def hand_case():
    """(3, 5) with hand-placed flags.  Env 0: truncation at t = 0 and at t = T-1 (which
    uses v_boot).  Env 1: two truncated cuts in consecutive steps.  Env 2: a plain
    terminal next to a truncated one, and truncated = 1 where terminals = 0 (ignored)."""
    r, _, _, v, vb = random_case(3, 5, seed=7)
    r[:] = [[1, 0, -1, 1, 1], [0, 1, 1, -1, 0], [1, 1, 0, 1, -1]]
    d = np.array([[1, 0, 0, 0, 1], [0, 1, 1, 0, 0], [0, 0, 1, 1, 0]], np.uint8)
    tr = np.array([[1, 0, 0, 0, 1], [0, 1, 1, 0, 0], [1, 0, 0, 1, 1]], np.uint8)
    return r, d, tr, v, vb


def f64_bound(ref):
    """The float32-vs-float64 tolerance of tests/test_gpu_parity.py (targets there:
    1e-5 * max(1, max |reference|))."""
    return 1e-5 * max(1.0, np.abs(ref).max())


TARGET_CASES = [('random-%dx%d' % s, lambda s=s: random_case(*s)) for s in TARGET_SHAPES] + [('hand', hand_case)]


@pytest.mark.parametrize('lam', [None, 0.95])
@pytest.mark.parametrize('name,case', TARGET_CASES, ids=[c[0] for c in TARGET_CASES])
def test_float32_restatement_agrees_with_the_float64_recursion(name, case, lam):
    r, d, tr, v, vb = case()
    if lam is None:
        t32, a32 = returns_trunc_f32(r, d, tr, v, vb, GAMMA)
    else:
        t32, a32 = gae_trunc_f32(r, d, tr, v, vb, GAMMA, lam)
    t64, a64 = targets_trunc_f64(r, d, tr, v, vb, GAMMA, lam)
    assert np.abs(t32 - t64).max() <= f64_bound(t64)
    assert np.abs(a32 - a64).max() <= f64_bound(a64)


@pytest.mark.parametrize('shape', TARGET_SHAPES)
def test_restatements_without_truncation_are_the_existing_oracles(shape):
    """truncated all zero: the float32 restatements of acmi_returns / acmi_gae, bit for bit."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import oracle
    r, d, tr, v, vb = random_case(*shape, zero_trunc=True)
    t32, a32 = returns_trunc_f32(r, d, tr, v, vb, GAMMA)
    want = oracle.targets_f32(r, d, vb, GAMMA)
    assert np.array_equal(t32, want) and np.array_equal(a32, (want - v).astype(np.float32))
    for got, ref in zip(gae_trunc_f32(r, d, tr, v, vb, GAMMA, 0.95), oracle.gae_f32(r, d, v, vb, GAMMA, 0.95)):
        assert np.array_equal(got, ref)


def test_hand_case_truncations_change_exactly_the_flagged_terminals():
    """What the flags mean, in float64: at a truncated terminal the one-step target is
    r + gamma V(next), at a plain one it is r; a flag without a terminal changes nothing."""
    r, d, tr, v, vb = hand_case()
    r, v, vb = r.astype(np.float64), v.astype(np.float64), vb.astype(np.float64)
    tgt, _ = targets_trunc_f64(r, d, tr, v, vb, GAMMA)
    assert tgt[0, 0] == r[0, 0] + GAMMA * v[0, 1]
    assert tgt[0, 4] == r[0, 4] + GAMMA * vb[0]
    assert tgt[1, 1] == r[1, 1] + GAMMA * v[1, 2] and tgt[1, 2] == r[1, 2] + GAMMA * v[1, 3]
    assert tgt[2, 2] == r[2, 2] and tgt[2, 3] == r[2, 3] + GAMMA * v[2, 4]
    plain, _ = targets_trunc_f64(r, d, np.zeros_like(tr), v, vb, GAMMA)
    assert np.array_equal(tgt[2, 4:], plain[2, 4:])  # t = 4: no terminal, the flag is ignored
    assert tgt[2, 0] == r[2, 0] + GAMMA * (r[2, 1] + GAMMA * r[2, 2])  # t = 0: the flag there is ignored too


# -- the wrappers above a game with cuts, restated on arrays -------------------------------
class CutsReplay(object):
    """N HostGame with cuts behind the lazy auto-reset, the 4-frame stack (roll, zero-fill
    on a terminal, the reset frame 4x) and the whole-game episode total: what
    acmi_game_step_cuts must produce.  done holds the stepper's codes (0 running, 1 game
    over, 2 life lost); events counts, per env, the life-loss terminals, the restack steps
    after them, the truncations and the reset steps after a game over."""

    def __init__(self, game, N, seed=0, env_offset=0, episodic_life=False, max_episode_steps=None):
        self.games = [HostGame(game, seed=seed, env_id=env_offset + n, episodic_life=episodic_life,
                               max_episode_steps=max_episode_steps) for n in range(N)]
        self.stacks = np.stack([np.repeat(g.reset(), 4, axis=-1) for g in self.games])
        self.done = np.zeros(N, np.uint8)
        self.total = np.zeros(N, np.float32)
        self.events = [dict(life_cut=0, restack=0, truncation=0, reset=0, game_over=0) for _ in range(N)]

    def step(self, actions):
        N = len(self.games)
        rew, term, trunc = np.zeros(N, np.float32), np.zeros(N, np.uint8), np.zeros(N, np.uint8)
        ep = np.full(N, NAN_BITS, np.uint32)
        for n, g in enumerate(self.games):
            if self.done[n]:
                before = (g.episode, g.steps, g.state.tobytes())
                self.stacks[n] = np.repeat(g.reset(), 4, axis=-1)
                if self.done[n] == 1:
                    self.total[n] = 0
                    self.events[n]['reset'] += 1
                else:  # the game went on in place
                    assert before == (g.episode, g.steps, g.state.tobytes())
                    self.events[n]['restack'] += 1
            frame, r, t, info = g.step(int(actions[n]))
            over = info.get('game_over', t)
            self.stacks[n] = np.roll(self.stacks[n], -1, axis=-1)
            if t:
                self.stacks[n].fill(0)
            self.stacks[n][..., -1:] = frame
            self.total[n] += np.float32(r)
            rew[n], term[n], trunc[n] = r, t, info.get('truncated', False)
            if over:
                ep[n] = self.total[n:n + 1].view(np.uint32)[0]
            self.done[n] = 1 if over else (2 if t else 0)
            self.events[n]['life_cut'] += bool(t and not over)
            self.events[n]['truncation'] += int(trunc[n])
            self.events[n]['game_over'] += bool(over)
        return self.stacks.copy(), rew, term, trunc, ep

    def state(self):
        g = self.games
        return (np.array([x.episode for x in g], np.int32), np.array([x.steps for x in g], np.int32),
                np.where(self.done == 1, np.float32(0), self.total).astype(np.float32), self.done.copy(),
                np.stack([x.state for x in g]))


def cuts_script(game, steps, N, seed):
    """Seeded actions, out-of-range ones (-1 and past the own count) included."""
    own = 3 if game == 'catch' else 4
    return np.random.RandomState(seed).randint(-1, own + 3, size=(steps, N)).astype(np.int32)


# the GPU stepper test's Breakout run: episodic life under a 60-step cap
CUTS_SEED, CUTS_SCRIPT_SEED, CUTS_MAX_STEPS, CUTS_CAP = 11, 3, 400, 60


def breakout_cuts_steps(N, env_offset):
    """The shortest prefix of the script whose host trace holds, for every env, a life-loss
    terminal, the restack step after it, a truncation and the reset step after that."""
    actions = cuts_script('breakout', CUTS_MAX_STEPS, N, CUTS_SCRIPT_SEED)
    ref = CutsReplay('breakout', N, seed=CUTS_SEED, env_offset=env_offset, episodic_life=True,
                     max_episode_steps=CUTS_CAP)
    after_trunc = np.zeros(N, int)
    was_trunc = np.zeros(N, bool)
    for s in range(CUTS_MAX_STEPS):
        resets = np.array([ev['reset'] for ev in ref.events])
        _, _, _, trunc, _ = ref.step(actions[s])
        after_trunc += was_trunc & (np.array([ev['reset'] for ev in ref.events]) > resets)
        was_trunc = trunc != 0
        if all(min(ev['life_cut'], ev['restack'], ev['truncation']) >= 1 for ev in ref.events) and \
                after_trunc.min() >= 1:
            return s + 1, ref.events
    return None, ref.events


@pytest.mark.parametrize('N,env_offset', [(1, 0), (3, 5)])
def test_breakout_cuts_script_covers_the_interesting_steps(N, env_offset):
    S, events = breakout_cuts_steps(N, env_offset)
    assert S is not None and S <= CUTS_MAX_STEPS, events


# -- the rules ---------------------------------------------------------------------------
PARKED_SCRIPT = np.random.RandomState(5).randint(0, 2, size=400)  # NOOP / FIRE: the paddle stays at 36


def _trace(game):
    """The game under PARKED_SCRIPT, reset on its own terminals: per step (frame, reward,
    state), and per step (terminal, game over, episode)."""
    out, flags = [], []
    out.append(game.reset().tobytes())
    for a in PARKED_SCRIPT:
        f, r, t, info = game.step(a)
        out.append((f.tobytes(), r, game.state.tobytes()))
        flags.append((t, info.get('game_over', t), game.episode))
        if t:
            out.append(game.reset().tobytes())
    return out, flags


def test_episodic_life_changes_only_the_terminal():
    life, life_flags = _trace(HostGame('breakout', seed=9, env_id=4, episodic_life=True))
    cuts = sum(1 for t, over, _ in life_flags if t and not over)
    overs = sum(1 for _, over, _ in life_flags if over)
    assert cuts >= 2 and overs >= 1, (cuts, overs)
    plain, plain_flags = _trace(HostGame('breakout', seed=9, env_id=4))
    # the plain game resets at its game overs only: drop the in-place resets' frames from the
    # episodic one, then the two traces are the same
    it = iter(life_flags)
    kept, i = [life[0]], 1
    for t, over, _ in it:
        kept.append(life[i])
        i += 1
        if t:
            if over:
                kept.append(life[i])
            i += 1
    assert kept == plain
    assert [over for _, over, _ in life_flags] == [t for t, _, _ in plain_flags]
    # episode advances only on game over
    episode = 0
    for (t, over, k), (_, _, k_plain) in zip(life_flags, plain_flags):
        assert k == episode == k_plain
        episode += bool(over)


def test_reset_after_a_life_loss_continues_in_place():
    g = HostGame('breakout', seed=1, env_id=0, episodic_life=True)
    g.reset()
    s = g.state
    s[[BX, BY, VX, VY, PX]] = (0, 78, 1, 2, 60)
    g.set_state(s)
    g.steps = 17
    f, r, term, info = g.step(0)
    assert term and info == {'truncated': False, 'game_over': False} and g.state[LIVES] == 2
    state, steps, episode = g.state.copy(), g.steps, g.episode
    again = g.reset()
    assert np.array_equal(again, g.render()) and np.array_equal(again, f)
    assert np.array_equal(g.state, state) and g.steps == steps == 18 and g.episode == episode
    _, _, term, info = g.step(0)
    assert not term and g.steps == 19
    # the last life is a game over, and the reset after it starts the next episode
    s = g.state
    s[[BX, BY, VX, VY, LIVES]] = (0, 78, 1, 2, 1)
    g.set_state(s)
    _, _, term, info = g.step(0)
    assert term and info == {'truncated': False, 'game_over': True}
    g.reset()
    assert g.episode == episode + 1 and g.steps == 0 and g.state[LIVES] == 3


def test_breakout_step_cap_truncates():
    g = HostGame('breakout', seed=2, env_id=1, max_episode_steps=30)
    g.reset()
    for t in range(1, 31):
        s = g.state
        _, r, term, info = g.step(2 if s[PX] + 5 < s[BX] else (3 if s[PX] + 5 > s[BX] else 0))
        if t < 30:
            assert not term and info == {'truncated': False, 'game_over': False}, t
    assert term and info == {'truncated': True, 'game_over': True}
    assert g.state[LIVES] == 3 and any(g.state[B0:B0 + 3])
    g.reset()
    assert g.episode == 1 and g.steps == 0


def test_catch_step_cap():
    g = HostGame('catch', seed=3, env_id=0, max_episode_steps=7)
    g.reset()
    for t in range(1, 8):
        _, r, term, info = g.step(0)
        assert r == 0.0 and term == (t == 7) and info == {'truncated': t == 7, 'game_over': t == 7}
    g = HostGame('catch', seed=3, env_id=0, max_episode_steps=19)  # its own terminal at the cap step
    g.reset()
    for t in range(1, 20):
        _, r, term, info = g.step(0)
    assert term and r in (-1.0, 1.0) and info == {'truncated': False, 'game_over': True}
    g = HostGame('catch', seed=3, env_id=0, episodic_life=True)  # one life: nothing changes
    g.reset()
    for t in range(1, 20):
        _, r, term, info = g.step(0)
        assert term == (t == 19) and info == {'truncated': False, 'game_over': t == 19}


def test_life_lost_on_the_cap_step_is_not_a_truncation():
    def at_the_cap(**kw):
        g = HostGame('breakout', seed=1, env_id=0, max_episode_steps=30, **kw)
        g.reset()
        s = g.state
        s[[BX, BY, VX, VY, PX]] = (0, 78, 1, 2, 60)
        g.set_state(s)
        g.steps = 29
        return g, g.step(0)
    g, (_, _, term, info) = at_the_cap(episodic_life=True)
    assert g.state[LIVES] == 2 and term and info == {'truncated': False, 'game_over': True}
    g.reset()  # a game over all the same: the next episode
    assert g.episode == 1 and g.steps == 0 and g.state[LIVES] == 3
    g, (_, _, term, info) = at_the_cap()  # without episodic life the cap alone ended it
    assert g.state[LIVES] == 2 and term and info == {'truncated': True, 'game_over': True}


def test_defaults_are_unchanged():
    def run(game, **kw):
        g = HostGame(game, seed=9, env_id=4, **kw)
        out = [g.reset().tobytes()]
        for a in np.random.RandomState(0).randint(0, 6, size=300):
            f, r, term, info = g.step(a)
            assert info == {} or kw
            out.append((f.tobytes(), r, term, g.state.tobytes(), g.episode, g.steps))
            if term:
                out.append(g.reset().tobytes())
        return out
    for game in ('catch', 'breakout'):
        assert run(game) == run(game, episodic_life=False, max_episode_steps=None)
    # the cap at its default value is today's game, with the flags in info
    assert run('breakout') == run('breakout', max_episode_steps=host.BREAKOUT_MAX_STEPS)
    g = HostGame('breakout')
    assert g.episodic_life is False and g.max_episode_steps is None
    for bad in (0, 2001, -1, 2.5, True, '7'):
        with pytest.raises(ValueError):
            HostGame('catch', max_episode_steps=bad)


# -- the C-ABI ----------------------------------------------------------------------------
def test_new_entry_points_are_declared_bound_and_exported(lib):
    src = open(os.path.join(ROOT, 'include', 'acmi.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(acmi_[a-z0-9_]+)\s*\(', src))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.EXPORTED, name
        assert hasattr(lib, name), name
    assert 'acmi_game_rules_t' in src and ctypes.sizeof(_lib.GameRules) == 8


def test_step_cuts_argument_errors(lib):
    one = ctypes.c_void_p(16)  # a non-null pointer no call gets as far as using
    def state(game=0, vars_=one):
        return _lib.GameState(one, one, one, one, vars_, game)
    def step(st, rules=(0, 0), N=1, in_stride=28224, out_stride=28224, ld=1, actions=one, trunc=one):
        r = ctypes.byref(_lib.GameRules(*rules)) if rules is not None else None
        return lib.acmi_game_step_cuts(ctypes.byref(st), r, N, 0, 0, actions, one, in_stride, one, out_stride, one,
                                       one, trunc, one, ld, None)
    ok = state()
    assert step(ok, rules=None) == _lib.ERR_ARG
    assert step(ok, rules=(0, -1)) == _lib.ERR_ARG
    assert step(ok, rules=(0, 2001)) == _lib.ERR_ARG
    assert step(ok, rules=(2, 0)) == _lib.ERR_ARG
    assert step(ok, rules=(-1, 0)) == _lib.ERR_ARG
    assert b'acmi_game_step_cuts' in lib.acmi_last_error()
    # acmi_game_step's own
    for bad in (state(game=2), state(game=-1), state(vars_=None)):
        assert step(bad) == _lib.ERR_ARG
    assert step(ok, N=-1) == _lib.ERR_ARG
    assert step(ok, in_stride=28224 + 8) == _lib.ERR_ARG
    assert step(ok, out_stride=28208) == _lib.ERR_ARG
    assert step(ok, ld=0) == _lib.ERR_ARG
    assert step(ok, actions=None) == _lib.ERR_ARG
    assert lib.acmi_game_step_cuts(None, ctypes.byref(_lib.GameRules(0, 0)), 1, 0, 0, one, one, 28224, one, 28224,
                                   one, one, one, one, 1, None) == _lib.ERR_ARG
    # nothing to do is not an error (and launches nothing); truncated may be null
    for rules in ((0, 0), (1, 2000), (1, 1)):
        assert step(ok, rules=rules, N=0) == 0 and step(ok, rules=rules, N=0, trunc=None) == 0


def test_trunc_targets_argument_errors(lib):
    one = ctypes.c_void_p(16)
    ret = lambda N=1, T=1, trunc=one: lib.acmi_returns_trunc(one, one, trunc, one, one, N, T, one, one, one, one,
                                                             None)
    gae = lambda N=1, T=1, trunc=one, lam=0.95: lib.acmi_gae_trunc(one, one, trunc, one, one, N, T, 0.99, lam, one,
                                                                   one, None)
    assert ret(trunc=None) == _lib.ERR_ARG and gae(trunc=None) == _lib.ERR_ARG
    assert ret(T=0) == _lib.ERR_ARG and gae(T=0) == _lib.ERR_ARG and ret(N=-1) == _lib.ERR_ARG
    assert gae(lam=1.5) == _lib.ERR_ARG
    assert b'acmi_gae_trunc' in lib.acmi_last_error()
    assert ret(N=0) == 0 and gae(N=0) == 0


def test_python_surface_needs_no_gpu():
    import inspect
    from actorcritic import spaces
    from actorcritic.envs import games
    from actorcritic.examples.atari import a2c_acktr, ppo
    from actorcritic.model import ActorCriticModel
    for fn in (a2c_acktr.train_a2c_acktr, ppo.train_ppo, a2c_acktr.create_game_environments,
               games.DeviceGameEnvs.__init__):
        p = inspect.signature(fn).parameters
        assert p['episodic_life'].default is False and p['max_episode_steps'].default is None
    assert games.DeviceGameEnvs.fused_step is False

    class Model(ActorCriticModel):
        pass
    m = Model(spaces.Box(low=0, high=255, shape=(84, 84, 4), dtype=np.uint8), spaces.Discrete(4))
    ph = m.truncations_placeholder
    assert ph.name == 'truncations' and np.dtype(ph.dtype) == np.bool_ and ph.shape == (None, None)
    assert ph is not m.terminals_placeholder

    class Envs(object):
        episodic_life = True
    with pytest.raises(ValueError):
        games.evaluate(None, Envs(), 1, uniform=True)
