"""The rule book of the device games: Catch and Breakout on the host.

:class:`HostGame` is a gym-like single env in pure Python integers + numpy.  It is
normative: the HIP stepper (csrc/games.hip, ``acmi_game_step``) reproduces its frames,
rewards, terminals and state vector bit for bit (tests/test_gpu_games.py), and it runs
on the list path as any host env does (FrameStackWrapper, EpisodeInfoWrapper, MultiEnv).

Both games draw straight into the 84x84 u8 field the tower reads: no RGB frame, no
resize, background 0.  Coordinates are (x, y) = (column, row) of an object's top-left
pixel.  The state is STATE_INTS int32 (``HostGame.state``):

    0 bx   1 by   2 vx   3 vy   4 px (paddle)   5 lives   6..8 bricks   9..11 zero

Brick row r (0..5), column c (0..11) is bit 12*(r % 2) + c of word 6 + r // 2.  Catch
keeps vy = 4, lives = 1 and no bricks.

The start of episode k of global env e is a pure function of (seed, e, k): the hash
key4(seed, e, k, tag) of csrc/common.hpp with a tag per game (and per remaining life
for Breakout's respawn).

Catch (own actions 0 NOOP, 1 RIGHT, 2 LEFT):
    ball 4x4 of 255 from y = 0, x = 4*(h % 21), vx = 4*((h >> 8) % 3 - 1); paddle 12x4
    of 200 at y = 80 from x = 36, +-4 a step, clamped to [0, 72].  A step: the paddle
    moves; the ball flips vx if x + vx leaves [0, 80], then x += vx, y += 4; at y == 76
    (step 19) the episode ends with +1 if x - px is 0, 4 or 8, else -1.

Breakout (own actions 0 NOOP, 1 FIRE = NOOP, 2 RIGHT, 3 LEFT):
    6 x 12 bricks of 7x3 px, row r at y = 12 + 3r with brightness 100 + 20r; paddle
    12x2 of 200 at y = 80 from x = 36, +-4 a step, clamped to [0, 72]; ball 2x2 of 255.
    A (re)spawn with `lives` left draws h = key4(seed, e, k, tag + lives): bx = 2*(h % 42),
    by = 40, vx = (-2, -1, 1, 2)[(h >> 8) & 3], vy = +2; the paddle stays where it is.
    A step, in this order:
      1. the paddle moves;
      2. vx flips if bx + vx leaves [0, 82], then bx += vx;
      3. vy flips if by + vy < 0 (the ceiling), then by += vy;
      4. brick: the probe pixel is (bx, by) going up and (bx, by + 1) going down; if it
         lies in a brick that is still there, that brick goes, reward +1, vy flips;
      5. paddle: if vy > 0 and by == 78 and -1 <= bx - px <= 11 (the ball sits on the
         paddle), vy = -2 and vx = (-2, -1, 1, 2)[(bx - px + 1) * 4 // 13];
      6. if by >= 80 the ball is lost: lives -= 1 and, if any are left, it respawns;
      7. terminal when lives == 0, no brick is left, or this was step 2000.

Actions at or past a game's own count act as NOOP.  The ball is drawn over the paddle,
the paddle over the bricks.

Cuts (``HostGame(..., episodic_life=False, max_episode_steps=None)``; the stepper's
``acmi_game_step_cuts``).  The flag that tells the learner "cut the return here" is not
the flag that says "the game restarts", and a cut may or may not keep its bootstrap:

    cap        = max_episode_steps (1..2000, either game), else the game's own
                 (Breakout 2000, Catch none);
    life_lost  = lives decreased in this step;
    game_over  = the game's own end (Catch: by == 76; Breakout: lives == 0 or no brick
                 left) or steps >= cap;
    terminal   = game_over or (episodic_life and life_lost);
    truncated  = steps >= cap and the game's own end has not fired and not
                 (episodic_life and life_lost): the cap alone ended the episode, and the
                 learner should still bootstrap from the value of the next observation.

With an option on, step()'s info is {'truncated': bool, 'game_over': bool}; with none it
stays {} and everything is as before.  reset() after a terminal that was not game_over
CONTINUES IN PLACE: the state, ``steps`` and ``episode`` are untouched and it returns
render() of the respawned ball (a frame stack above it restarts from that frame).  This
is deliberately not the NOOP step of the reference's AtariEpisodicLifeWrapper
(envs/atari/wrappers.py:89-117), and the whole contract rests on it: under the same
actions an ``episodic_life=True`` game produces exactly the frames, rewards and state
vectors of the plain game; only ``terminal`` differs, and what the wrappers above do with
it.  Catch has one life, so ``episodic_life`` changes nothing there.  The device stepper
has EpisodeInfoWrapper inside the life cut, as the reference chain does: its episode
totals are whole-game totals at a game over.  (An EpisodeInfoWrapper put around an
``episodic_life=True`` HostGame on the list path sees that game's terminals and so totals
per life.)

Mixed batches.  A batch may hold both games, env by env (:func:`game_pattern`; the
stepper's ``acmi_game_step_mixed``): it is N HostGame of different games, and nothing
couples them.  An env's trace is a pure function of (seed, global env id, its game, its
actions), whatever its neighbours play: the hash keys hold the game's tag, and a
'+'-pattern assigns the game by the global env id, so a data-parallel shard plays what
the same envs play in one large batch.
"""

import numpy as np

from actorcritic import spaces

STATE_INTS = 12
GAMES = ('catch', 'breakout')
GAME_ACTIONS = {'catch': 3, 'breakout': 4}
CATCH_TAG = 0xCA7C0000
BREAKOUT_TAG = 0xB4EA0000
BREAKOUT_MAX_STEPS = 2000
_M32 = 0xFFFFFFFF


def mix32(x):
    """lowbias32 finaliser on a Python int (csrc/common.hpp mix32)."""
    x &= _M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & _M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & _M32
    x ^= x >> 16
    return x


def key4(a, b, c, d):
    h = mix32((a & _M32) ^ 0x9e3779b9)
    h = mix32(h ^ (b & _M32))
    h = mix32(h ^ (c & _M32))
    return mix32(h ^ (d & _M32))


def game_id(game):
    """Index of a device game ('catch' -> 0, 'breakout' -> 1); ints pass through."""
    if isinstance(game, (int, np.integer)) and 0 <= int(game) < len(GAMES):
        return int(game)
    if game in GAMES:
        return GAMES.index(game)
    raise ValueError('unknown game {!r}: one of {}'.format(game, GAMES))


def game_pattern(game, num_envs, env_offset=0):
    """The game of every env of a batch -> tuple of num_envs names.

    game: a name or id (every env plays it); a '+'-joined string of names such as
    'catch+breakout', under which GLOBAL env e = env_offset + n plays names[e % len(names)]
    (a game follows the global env id, as an episode's start does, so shards agree with
    the whole batch); or an explicit sequence of num_envs names or ids.  ValueError for
    anything else: an unknown name, an empty part, a wrong length."""
    num_envs, env_offset = int(num_envs), int(env_offset)
    if num_envs < 0 or env_offset < 0:
        raise ValueError('num_envs and env_offset must not be negative')
    if isinstance(game, str):
        names = tuple(GAMES[game_id(part)] for part in game.split('+'))  # ('' raises in game_id)
        return tuple(names[(env_offset + n) % len(names)] for n in range(num_envs))
    if isinstance(game, (int, np.integer)):
        return (GAMES[game_id(game)],) * num_envs
    if isinstance(game, (list, tuple, np.ndarray)):
        if len(game) != num_envs:
            raise ValueError('{} games for {} envs'.format(len(game), num_envs))
        return tuple(GAMES[game_id(g)] for g in game)
    raise ValueError('game must be a name, an id, a \'+\'-joined string or a sequence, got {!r}'.format(game))


def env_game_ids(game, num_envs, env_offset=0):
    """The game id of every env of a batch (game_pattern's arguments) -> tuple of num_envs ints:
    what DeviceGameEnvs steps by, and the groups of a per-game ReturnNormalizer."""
    return tuple(game_id(g) for g in game_pattern(game, num_envs, env_offset))


def check_max_episode_steps(max_episode_steps):
    """None (the game's own cap) or an int in 1..2000; ValueError otherwise."""
    if max_episode_steps is None:
        return None
    if isinstance(max_episode_steps, bool) or not isinstance(max_episode_steps, (int, np.integer)) or \
            not 1 <= int(max_episode_steps) <= BREAKOUT_MAX_STEPS:
        raise ValueError('max_episode_steps must be None or an int in 1..{}, got {!r}'.format(
            BREAKOUT_MAX_STEPS, max_episode_steps))
    return int(max_episode_steps)


class HostGame(object):
    """One game on the host.  reset() -> frame [84, 84, 1] u8; step(a) -> (frame, reward,
    terminal, info).  Every reset() starts the next episode (0, 1, ...), as the device
    stepper's lazy auto-reset does -- except after a life-loss terminal under
    ``episodic_life``, where the game continues in place (module docstring, "Cuts")."""

    def __init__(self, game, seed=0, env_id=0, episodic_life=False, max_episode_steps=None):
        self.game = GAMES[game_id(game)]
        self.episodic_life = bool(episodic_life)
        self.max_episode_steps = check_max_episode_steps(max_episode_steps)
        self._cap = self.max_episode_steps
        if self._cap is None and self.game == 'breakout':
            self._cap = BREAKOUT_MAX_STEPS
        self._continue = False  # the last terminal was not a game over: reset() continues in place
        self.seed = int(seed) & _M32
        self.env_id = int(env_id)
        self.num_own_actions = GAME_ACTIONS[self.game]
        self.action_space = spaces.Discrete(self.num_own_actions)
        self.observation_space = spaces.Box(low=0, high=255, shape=(84, 84, 1), dtype=np.uint8)
        self.episode = -1
        self.steps = 0
        self.bx = self.by = self.vx = self.vy = self.px = self.lives = 0
        self.bricks = [0, 0, 0]

    # -- state -------------------------------------------------------------------
    @property
    def state(self):
        s = np.zeros(STATE_INTS, np.int32)
        s[:6] = (self.bx, self.by, self.vx, self.vy, self.px, self.lives)
        s[6:9] = self.bricks
        return s

    def set_state(self, state):
        """Loads a state vector (tests place the ball and the paddle with it)."""
        s = [int(v) for v in state]
        self.bx, self.by, self.vx, self.vy, self.px, self.lives = s[:6]
        self.bricks = s[6:9]

    def _spawn_ball(self):
        if self.game == 'catch':
            h = key4(self.seed, self.env_id, self.episode, CATCH_TAG)
            self.bx, self.by = 4 * (h % 21), 0
            self.vx, self.vy = 4 * ((h >> 8) % 3 - 1), 4
        else:
            h = key4(self.seed, self.env_id, self.episode, BREAKOUT_TAG + self.lives)
            self.bx, self.by = 2 * (h % 42), 40
            self.vx, self.vy = (-2, -1, 1, 2)[(h >> 8) & 3], 2

    # -- gym-like API --------------------------------------------------------------
    def reset(self):
        if self._continue:
            self._continue = False
            return self.render()
        self.episode += 1
        self.steps = 0
        self.px = 36
        if self.game == 'catch':
            self.lives, self.bricks = 1, [0, 0, 0]
        else:
            self.lives, self.bricks = 3, [0xFFFFFF] * 3
        self._spawn_ball()
        return self.render()

    def step(self, action):
        if self.episode < 0:
            raise ValueError('step() before reset()')
        a = int(action)
        if not 0 <= a < self.num_own_actions:
            a = 0
        self.steps += 1
        lives = self.lives
        reward, own = self._catch(a) if self.game == 'catch' else self._breakout(a)
        capped = self._cap is not None and self.steps >= self._cap
        game_over = own or capped
        life_cut = self.episodic_life and self.lives < lives
        terminal = game_over or life_cut
        self._continue = terminal and not game_over
        info = {}
        if self.episodic_life or self.max_episode_steps is not None:
            info = {'truncated': bool(capped and not own and not life_cut), 'game_over': bool(game_over)}
        return self.render(), float(reward), bool(terminal), info

    def _catch(self, a):
        if a == 1:
            self.px = min(self.px + 4, 72)
        elif a == 2:
            self.px = max(self.px - 4, 0)
        if not 0 <= self.bx + self.vx <= 80:
            self.vx = -self.vx
        self.bx += self.vx
        self.by += 4
        if self.by != 76:
            return 0, False
        return (1 if self.bx - self.px in (0, 4, 8) else -1), True

    def _breakout(self, a):
        reward = 0
        if a == 2:
            self.px = min(self.px + 4, 72)
        elif a == 3:
            self.px = max(self.px - 4, 0)
        if not 0 <= self.bx + self.vx <= 82:
            self.vx = -self.vx
        self.bx += self.vx
        if self.by + self.vy < 0:
            self.vy = -self.vy
        self.by += self.vy
        cy = self.by + (1 if self.vy > 0 else 0)
        if 12 <= cy < 30:
            r, c = (cy - 12) // 3, self.bx // 7
            bit = 1 << (12 * (r % 2) + c)
            if self.bricks[r // 2] & bit:
                self.bricks[r // 2] &= ~bit
                reward = 1
                self.vy = -self.vy
        off = self.bx - self.px
        if self.vy > 0 and self.by == 78 and -1 <= off <= 11:
            self.vy = -2
            self.vx = (-2, -1, 1, 2)[(off + 1) * 4 // 13]
        if self.by >= 80:
            self.lives -= 1
            if self.lives > 0:
                self._spawn_ball()
        return reward, self.lives == 0 or not any(self.bricks)  # (the step cap: step())

    def render(self):
        f = np.zeros((84, 84, 1), np.uint8)
        if self.game == 'breakout':
            for r in range(6):
                for c in range(12):
                    if self.bricks[r // 2] >> (12 * (r % 2) + c) & 1:
                        f[12 + 3 * r:15 + 3 * r, 7 * c:7 * c + 7] = 100 + 20 * r
        ph, bs = (4, 4) if self.game == 'catch' else (2, 2)
        f[80:80 + ph, self.px:self.px + 12] = 200
        f[self.by:self.by + bs, self.bx:self.bx + bs] = 255
        return f

    def close(self):
        pass
