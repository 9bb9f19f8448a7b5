"""Device games: small real games that step and render on the GPU.

:class:`DeviceGameEnvs` is a batch of Catch or Breakout envs (or of both, env by env:
"mixed") behind ``acmi_game_step`` (csrc/games.hip): one HIP workgroup per env advances
the game's integer state and draws the new 84x84 frame straight into the 4-frame stack, with the synthetic stepper's
wrapper semantics (lazy auto-reset, FrameStackWrapper, EpisodeInfoWrapper).  It
duck-types :class:`actorcritic.envs.atari.wrappers.SyntheticAtariEnvs`, so ``MultiEnv``
and ``MultiEnvAgent`` put it on the device rollout; the rules are those of
:class:`actorcritic.envs.games.host.HostGame`, bit for bit.

:func:`evaluate` plays whole episodes forward-only and returns their returns;
:func:`returns_by_game` splits those of a mixed batch by game.
"""

import ctypes

import numpy as np
import torch

from actorcritic import _lib, _ops, spaces
from actorcritic._engine import OBS_BYTES
from actorcritic.envs.atari.wrappers import (ENV_KIND_GAMES, EpisodeInfoBatch, _mask_tensor, action_mask_bits,
                                             check_env_identity, load_env_arrays)
from actorcritic.envs.games.host import (GAME_ACTIONS, GAMES, STATE_INTS, HostGame, check_max_episode_steps,
                                         env_game_ids, game_id, game_pattern)

__all__ = ['DeviceGameEnvs', 'HostGame', 'evaluate', 'returns_by_game', 'game_pattern', 'GAMES', 'GAME_ACTIONS']

MAX_ACTIONS = 64  # the layout's widest policy head


class DeviceGameEnvs(object):
    """A batch of device games with frame stacking, on one GPU.

    Args:
        game: 'catch' or 'breakout' (or its id); or whatever else
            :func:`actorcritic.envs.games.host.game_pattern` takes: a '+'-joined string such
            as 'catch+breakout' (global env e plays names[e % len(names)]) or a sequence of
            num_envs names or ids.  More than one distinct game makes a MIXED batch (below).
        num_envs: environments on this device.
        num_actions: size of the Discrete action space; default the game's own count
            (catch 3, breakout 4; mixed: the largest, 4).  A wider head (up to 64) is allowed:
            the actions past the own set step as NOOP, and up to 32 ``legal_action_masks`` holds the own
            set as one word per env (``MultiEnvAgent(mask_actions=True)``).
        seed: game seed (an episode's start is a pure function of seed, env, episode).
        env_offset: global id of the first env (data-parallel shards use rank*num_envs).
        episodic_life: a lost life is a terminal for the learner; the game goes on in place
            and resets only when it is really over (host.py, "Cuts").
        max_episode_steps: step cap, 1..2000 (either game); None: the game's own (Breakout
            2000, Catch none).  A terminal that the cap alone caused is a truncation.

    With either option set the envs step through ``acmi_game_step_cuts`` and
    ``emits_truncations`` is True: ``step_into(..., trunc_ptr=)`` writes one truncation byte
    per env beside the terminals (the rollout: ``MultiEnvAgent.last_truncations``), and the
    batched ``step()`` leaves them in ``last_truncations`` ([N] bool device tensor; None for
    envs that emit none).  ``episode_rewards`` stay whole-game totals, at a game over only.

    A single-game batch, however spelled, has ``is_mixed`` False and no ``games`` tensor, and
    steps through the entry points above.  A mixed batch steps through
    ``acmi_game_step_mixed`` -- the same kernel, one launch, the game read per env -- and has:
    ``games`` (names per env), ``game_ids`` (ints per env), ``games_tensor`` (device u8 [N]),
    ``own_action_counts`` (numpy [N]); ``game`` is the '+'-joined distinct names in id order,
    ``game_id`` None, ``num_own_actions`` the largest own count; ``legal_action_masks``
    holds every env's own set (4-action head: catch 0b0111, breakout 0b1111).  The rules
    apply to every env.  ``bad_envs`` (device int32 [1]) counts envs whose id the kernel
    refused; ids are validated here, so it stays 0.

    ``fused_step=True`` (opt-in) puts the envs on the rollout's fused step
    (``acmi_rollout_step_games``: heads, draw, game step and the next step's conv tower in
    one kernel per env), bit-identical to the default three-call chain; ``step_into``,
    ``step`` and :func:`evaluate` are unchanged.  The instance then owns the zeroed
    pending buffer of the split form (``_pend``), which ``reset_into`` clears.

    ``state_dict()`` / ``load_state_dict(d)``: what the next step reads --
    episode, step, total, done, vars, the gym-like API's stack, and ``bad_envs`` when mixed -- as
    CPU tensors, beside what the envs ARE (kind, num_envs, env_offset, seed, num_actions, the
    per-env game ids, episodic_life, max_episode_steps; ints and one int64 tensor).  Loading
    into envs that differ in any of those is a ValueError naming the field.  ``fused_step`` is
    free to differ: the fused step is bit-identical to the chain, so a state saved under one
    resumes under the other.  Between two complete rollouts nothing is pending: ``state_dict``
    checks that every ``_pend`` flag is zero (RuntimeError otherwise) and saves none of it;
    loading zeroes ``_pend``, as ``reset_into`` does.
    """

    # Off unless asked for (the keyword): the rollout steps these envs through forward +
    # sampler + step_into, see agents._RolloutBuffers; True: through rollout_step below
    fused_step = False

    def __init__(self, game, num_envs, num_actions=None, seed=0, env_offset=0, device=None, episodic_life=False,
                 max_episode_steps=None, fused_step=False):
        _lib.require_gpu()
        self.episodic_life = bool(episodic_life)
        self.max_episode_steps = check_max_episode_steps(max_episode_steps)
        self.emits_truncations = self.episodic_life or self.max_episode_steps is not None
        self._rules = _lib.GameRules(int(self.episodic_life), self.max_episode_steps or 0)
        self.last_truncations = None
        self.num_envs = int(num_envs)
        self.env_offset = int(env_offset)
        names = game_pattern(game, self.num_envs, self.env_offset)
        # every env's id, mixed or not (a per-game ReturnNormalizer's groups: return_norm.groups_for_envs)
        self.env_game_ids = env_game_ids(game, self.num_envs, self.env_offset)
        distinct = sorted(set(self.env_game_ids))
        self.is_mixed = len(distinct) > 1
        if self.is_mixed:
            self.games = names
            self.game_ids = self.env_game_ids
            self.own_action_counts = np.array([GAME_ACTIONS[g] for g in names], np.int64)
            self.game_id = None
            self.game = '+'.join(GAMES[i] for i in distinct)
            self.num_own_actions = int(self.own_action_counts.max())
        else:
            self.game_id = distinct[0] if distinct else game_id(game)
            self.game = GAMES[self.game_id]
            self.num_own_actions = GAME_ACTIONS[self.game]
        num_actions = self.num_own_actions if num_actions is None else int(num_actions)
        if not self.num_own_actions <= num_actions <= MAX_ACTIONS:
            raise ValueError('num_actions={} outside [{}, {}] for {}'.format(num_actions, self.num_own_actions,
                                                                             MAX_ACTIONS, self.game))
        self.seed = int(seed) & 0xFFFFFFFF
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.observation_space = spaces.Box(low=0, high=255, shape=(84, 84, 4), dtype=np.uint8)
        self.action_space = spaces.Discrete(num_actions)
        lib = _lib.load()
        if int(lib.acmi_game_state_ints()) != STATE_INTS or \
                int(lib.acmi_game_state_bytes()) != ctypes.sizeof(_lib.GameState):
            raise ImportError('libacmi game state layout mismatch')
        N = self.num_envs
        z = lambda dt: torch.zeros(N, dtype=dt, device=self.device)
        self._episode, self._step = z(torch.int32), z(torch.int32)
        self._total, self._done = z(torch.float32), z(torch.uint8)
        self._vars = torch.zeros((N, STATE_INTS), dtype=torch.int32, device=self.device)
        self.legal_action_masks = None
        if num_actions <= _lib.MASK_MAX_ACTIONS:
            counts = self.own_action_counts if self.is_mixed else [self.num_own_actions] * N
            self.legal_action_masks = _mask_tensor([action_mask_bits(range(int(c)), num_actions) for c in counts],
                                                   self.device)
        if self.is_mixed:
            self.games_tensor = torch.tensor(self.game_ids, dtype=torch.uint8, device=self.device)
            self.bad_envs = torch.zeros(1, dtype=torch.int32, device=self.device)
            self._games_base, self._bad_ptr = self.games_tensor.data_ptr(), self.bad_envs.data_ptr()
        self._states = {}
        self.state = self.range_state(0)
        if fused_step:
            self.fused_step = True
            # post-step states of the split form (B <= 64), committed by the next step's fc4
            # launch; an entry is int32 x acmi_game_pend_ints(), a multiple of 16 bytes
            self._pend_ints = int(lib.acmi_game_pend_ints())
            self._pend = torch.zeros((N, self._pend_ints), dtype=torch.int32, device=self.device)
            # an entry's flag word (games.hpp GamePend: k, t, total, done, vars[STATE_INTS], flag, 3 pads)
            self._pend_flag = 4 + STATE_INTS
            if self._pend_ints != self._pend_flag + 4:
                raise ImportError('libacmi pending entry layout mismatch')
        self._obs = torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=self.device)

    def _stream(self):
        return _lib.stream_handle(self.device)

    def range_state(self, n0):
        """GameState of envs n0.. (pointers at env n0)."""
        st = self._states.get(n0)
        if st is None:
            st = _lib.GameState(self._episode[n0:].data_ptr(), self._step[n0:].data_ptr(),
                                self._total[n0:].data_ptr(), self._done[n0:].data_ptr(),
                                self._vars[n0:].data_ptr(), 0 if self.game_id is None else self.game_id)
            self._states[n0] = st
        return st

    def state_arrays(self):
        """Host copies of the per-env state: episode, step, total, done, vars [N, K]."""
        return tuple(t.cpu().numpy() for t in (self._episode, self._step, self._total, self._done, self._vars))

    def reset_into(self, obs_ptr, stride=OBS_BYTES):
        if self.fused_step:  # a stale entry must never be committed over the reset state
            self._pend.zero_()
        if self.is_mixed:
            _lib.call('acmi_game_reset_mixed', ctypes.byref(self.state), self._games_base, self.num_envs,
                      self.env_offset, self.seed, ctypes.c_void_p(obs_ptr), stride, self._bad_ptr, self._stream())
            return
        _lib.call('acmi_game_reset', ctypes.byref(self.state), self.num_envs, self.env_offset, self.seed,
                  ctypes.c_void_p(obs_ptr), stride, self._stream())

    def step_into(self, actions_ptr, obs_in_ptr, in_stride, obs_out_ptr, out_stride, rew_ptr, term_ptr, ep_ptr, ld,
                  trunc_ptr=None):
        self.step_range_into(0, self.num_envs, actions_ptr, obs_in_ptr, in_stride, obs_out_ptr, out_stride, rew_ptr,
                             term_ptr, ep_ptr, ld, trunc_ptr)

    def step_range_into(self, n0, n, actions_ptr, obs_in_ptr, in_stride, obs_out_ptr, out_stride, rew_ptr,
                        term_ptr, ep_ptr, ld, trunc_ptr=None):
        """step_into for envs n0 .. n0+n-1 only (every pointer already at env n0).
        trunc_ptr: u8 truncations, laid out as the terminals (envs with ``emits_truncations``)."""
        if not (0 <= n0 and 0 <= n and n0 + n <= self.num_envs):
            raise ValueError('envs {} .. {} outside the batch of {}'.format(n0, n0 + n - 1, self.num_envs))
        if self.is_mixed:  # (rules {0, 0}: acmi_game_step's; the games pointer moves with the state, a byte an env)
            if trunc_ptr is not None and not self.emits_truncations:
                raise ValueError('these envs emit no truncations (episodic_life / max_episode_steps are off)')
            _lib.call('acmi_game_step_mixed', ctypes.byref(self.range_state(n0)), self._games_base + n0,
                      ctypes.byref(self._rules), n, self.env_offset + n0, self.seed, ctypes.c_void_p(actions_ptr),
                      ctypes.c_void_p(obs_in_ptr), in_stride, ctypes.c_void_p(obs_out_ptr), out_stride,
                      ctypes.c_void_p(rew_ptr), ctypes.c_void_p(term_ptr), ctypes.c_void_p(trunc_ptr),
                      ctypes.c_void_p(ep_ptr), ld, self._bad_ptr, self._stream())
            return
        if self.emits_truncations:
            _lib.call('acmi_game_step_cuts', ctypes.byref(self.range_state(n0)), ctypes.byref(self._rules), n,
                      self.env_offset + n0, self.seed, ctypes.c_void_p(actions_ptr), ctypes.c_void_p(obs_in_ptr),
                      in_stride, ctypes.c_void_p(obs_out_ptr), out_stride, ctypes.c_void_p(rew_ptr),
                      ctypes.c_void_p(term_ptr), ctypes.c_void_p(trunc_ptr), ctypes.c_void_p(ep_ptr), ld,
                      self._stream())
            return
        if trunc_ptr is not None:
            raise ValueError('these envs emit no truncations (episodic_life / max_episode_steps are off)')
        _lib.call('acmi_game_step', ctypes.byref(self.range_state(n0)), n, self.env_offset + n0, self.seed,
                  ctypes.c_void_p(actions_ptr), ctypes.c_void_p(obs_in_ptr), in_stride, ctypes.c_void_p(obs_out_ptr),
                  out_stride, ctypes.c_void_p(rew_ptr), ctypes.c_void_p(term_ptr), ctypes.c_void_p(ep_ptr), ld,
                  self._stream())

    def rollout_step(self, net, obs, img_stride, n0, n, acts, act_img_stride, io, stream, legal=None,
                     trunc_ptr=None):
        """The fused rollout step of envs n0 .. n0+n-1 (``fused_step=True`` envs): ``io`` is
        the _lib.RolloutIO the rollout built for them (its ``state`` is not read); the game
        state, games and pending pointers go with n0, as in step_range_into."""
        if not self.fused_step:
            raise ValueError('these envs were built without fused_step=True')
        if not (0 <= n0 and 0 <= n and n0 + n <= self.num_envs):
            raise ValueError('envs {} .. {} outside the batch of {}'.format(n0, n0 + n - 1, self.num_envs))
        if trunc_ptr is not None and not self.emits_truncations:
            raise ValueError('these envs emit no truncations (episodic_life / max_episode_steps are off)')
        gio = _lib.RolloutGameIO(io, self.range_state(n0), self._games_base + n0 if self.is_mixed else None,
                                 self._rules, trunc_ptr, self._bad_ptr if self.is_mixed else None,
                                 self._pend.data_ptr() + 4 * self._pend_ints * n0)
        _ops.rollout_step_games(net, obs, img_stride, n, acts, act_img_stride, gio, stream, legal=legal)

    # -- gym-like batched API (as SyntheticAtariEnvs) ---------------------------
    def reset(self):
        self.reset_into(self._obs.data_ptr())
        return self._obs.clone()

    def step(self, actions):
        """actions: [N] ints -> (obs [N,84,84,4] u8, rewards [N], terminals [N] bool, EpisodeInfoBatch);
        the step's truncations ([N] bool) are left in ``last_truncations`` (class docstring)."""
        a = actions if isinstance(actions, torch.Tensor) else torch.as_tensor(np.asarray(actions))
        a = a.to(device=self.device, dtype=torch.int32).contiguous()
        N = self.num_envs
        rew = torch.empty(N, dtype=torch.float32, device=self.device)
        term = torch.empty(N, dtype=torch.uint8, device=self.device)
        ep = torch.empty(N, dtype=torch.float32, device=self.device)
        trunc = torch.empty(N, dtype=torch.uint8, device=self.device) if self.emits_truncations else None
        self.step_into(a.data_ptr(), self._obs.data_ptr(), OBS_BYTES, self._obs.data_ptr(), OBS_BYTES,
                       rew.data_ptr(), term.data_ptr(), ep.data_ptr(), 1,
                       trunc_ptr=None if trunc is None else trunc.data_ptr())
        self.last_truncations = None if trunc is None else trunc.view(torch.bool)
        return self._obs.clone(), rew, term.view(torch.bool), EpisodeInfoBatch(ep[:, None])

    # -- run state (class docstring) ----------------------------------------------
    def _identity(self):
        return {'kind': ENV_KIND_GAMES, 'num_envs': self.num_envs, 'env_offset': self.env_offset,
                'seed': self.seed, 'num_actions': int(self.action_space.n),
                'game_ids': torch.tensor([int(i) for i in self.env_game_ids], dtype=torch.int64),
                'episodic_life': int(self.episodic_life), 'max_episode_steps': int(self.max_episode_steps or 0)}

    def _state_tensors(self):
        out = {'episode': self._episode, 'step': self._step, 'total': self._total, 'done': self._done,
               'vars': self._vars, 'obs': self._obs}
        if self.is_mixed:
            out['bad_envs'] = self.bad_envs
        return out

    def state_dict(self):
        if self.fused_step and bool(self._pend[:, self._pend_flag].any()):  # (one host read)
            raise RuntimeError('a game state is still pending (a rollout was abandoned between two fused steps): '
                               'the env state is whole only after a complete rollout or a reset')
        out = self._identity()
        out.update({k: v.detach().cpu().clone() for k, v in self._state_tensors().items()})
        return out

    def load_state_dict(self, state):
        check_env_identity(state, self._identity())
        load_env_arrays(state, self._state_tensors())
        if self.fused_step:  # (as reset_into: a stale entry must never be committed over the loaded state)
            self._pend.zero_()

    def close(self):
        pass


def evaluate(model, envs, episodes_per_env, greedy=True, seed=0, uniform=False, return_actions=False,
             max_steps=None):
    """Plays ``envs`` (a :class:`DeviceGameEnvs`, reset here -- not the one a training
    agent is stepping) with ``model``'s policy, forward only: tower forward, sampler
    (the mode of the policy with ``greedy``, else a draw keyed by ``seed``), step_into;
    no activations are kept for an update.

    Counts exactly the first ``episodes_per_env`` finished episodes of EVERY env
    (whichever episodes finish first would favour short ones) and returns their returns,
    a float32 device tensor [num_envs, episodes_per_env].

    uniform: the actions are drawn uniformly from the game's own set on the host
        (np.random.RandomState(seed)) and the model is not run (it may be None): the
        random baseline.  In a mixed batch every env draws from ITS game's own set.
    return_actions: also returns the actions taken, int32 [steps, num_envs].
    max_steps: give up (RuntimeError) after that many steps; default
        episodes_per_env * 2001 (Breakout's step cap + the reset step).

    ``envs`` with ``episodic_life=True`` raise ValueError: the episode count here is a count
    of terminals, and a life cut is not the end of a game.  (``max_episode_steps`` is fine:
    a truncated game is over and reports its total.)

    A mixed batch (``envs.is_mixed``): the Catch envs play on past their count while the
    Breakout envs finish (column E of the scratch takes those); :func:`returns_by_game`
    splits the result.  A model that holds per-env legal-action masks must hold exactly
    ``envs.legal_action_masks`` (ValueError otherwise): masks are indexed by env, and a
    batch composed differently from the one they were made for would use the wrong sets.
    """
    if getattr(envs, 'episodic_life', False):
        raise ValueError('evaluate() counts terminals as finished games: build the evaluation envs without '
                         'episodic_life')
    N, E = envs.num_envs, int(episodes_per_env)
    if E < 1:
        raise ValueError('episodes_per_env must be at least 1')
    dev = envs.device
    limit = int(max_steps) if max_steps is not None else E * 2001
    obs = torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=dev)
    actions = torch.zeros(N, dtype=torch.int32, device=dev)
    rew = torch.zeros(N, dtype=torch.float32, device=dev)
    term = torch.zeros(N, dtype=torch.uint8, device=dev)
    ep = torch.zeros(N, dtype=torch.float32, device=dev)
    returns = torch.zeros((N, E + 1), dtype=torch.float32, device=dev)  # column E: episodes past the count
    count = torch.zeros(N, dtype=torch.int64, device=dev)
    rows = torch.arange(N, device=dev)
    taken = []
    rng = np.random.RandomState(seed) if uniform else None
    eng = None if uniform else model.engine
    mixed = getattr(envs, 'is_mixed', False)
    if mixed and eng is not None and eng.masks is not None:
        own = envs.legal_action_masks
        if own is None or own.numel() != eng.masks.numel() or \
                not torch.equal(own.view(torch.int32).to(eng.masks.device), eng.masks):
            raise ValueError('the model\'s legal-action masks are not those of this mixed batch ({}): masks are '
                             'per env, so evaluate on a batch composed like the one they were set for, or clear '
                             'them (set_action_masks(None))'.format(envs.game))
    if eng is not None:
        acts = eng.activations(N, 'evaluate')
        saved_counter = eng.sample_counter
    envs.reset_into(obs.data_ptr())
    steps = 0
    try:
        while True:
            if uniform:
                high = envs.own_action_counts if mixed else envs.num_own_actions
                actions.copy_(torch.from_numpy(rng.randint(0, high, size=N).astype(np.int32)))
            else:
                eng.forward(obs.data_ptr(), N, acts.struct, want_value=False)
                eng.sample_counter = steps  # (a draw is keyed by seed, stream 1 and the step)
                eng.sample(acts.logits, N, actions, mode=bool(greedy), seed=int(seed) & 0xFFFFFFFF, stream_id=1)
            if return_actions:
                taken.append(actions.clone())
            envs.step_into(actions.data_ptr(), obs.data_ptr(), OBS_BYTES, obs.data_ptr(), OBS_BYTES, rew.data_ptr(),
                           term.data_ptr(), ep.data_ptr(), 1)
            done = term != 0
            slot = torch.where(done, count.clamp(max=E), torch.full_like(count, E))
            returns[rows, slot] = torch.where(done, ep, returns[rows, slot])
            count += done
            steps += 1
            # one host wait per step; Catch finishes every env at the same step
            if bool((count >= E).all()):
                break
            if steps >= limit:
                raise RuntimeError('evaluate: {} steps without {} finished episodes in every env'.format(steps, E))
    finally:
        if eng is not None:
            eng.sample_counter = saved_counter  # evaluation does not move the training RNG
    if eng is not None:
        eng.check_bad_rows()
    out = returns[:, :E].contiguous()
    if return_actions:
        return out, torch.stack(taken)
    return out


def returns_by_game(envs, returns):
    """Splits evaluate()'s returns [num_envs, E] by game -> {name: tensor [envs of that game, E]},
    in id order; a single-game batch gives one entry."""
    if returns.shape[0] != envs.num_envs:
        raise ValueError('returns of {} envs for a batch of {}'.format(returns.shape[0], envs.num_envs))
    if not getattr(envs, 'is_mixed', False):
        return {envs.game: returns}
    ids = np.asarray(envs.game_ids)
    out = {}
    for i, name in enumerate(GAMES):
        rows = np.nonzero(ids == i)[0]
        if rows.size:
            out[name] = returns[torch.as_tensor(rows, device=returns.device)]
    return out
