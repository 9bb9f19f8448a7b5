"""Agents (reference: actorcritic/agents.py:6-257).

``MultiEnvAgent.interact`` returns the reference's 6-tuple in batch-major [env, step]
layout.  With a batched device env and an :class:`AtariModel` it runs the whole
T-step rollout on the GPU: per step one strided tower forward that writes its
activations straight into the update's [N*T] buffers (row n*T + t), one sampling
kernel, one stepper kernel that writes the next stacked frame into the [N, T+1]
observation buffer — no host copies, no Python lists.  Host-stepped envs behind a
HostAtariEnvs adaptor keep the same device buffers (_interact_host): the envs step on
the host between the sampler and one frame kernel that writes the next stacks.  Anything
else takes the reference's list-based loop.

Two opt-in variants, bit-identical to the one-chain rollout (test_two_stream_rollout_
is_bit_identical, and across updates test_rollout_variants_give_identical_updates):
ACMI_ROLLOUT_SPLIT=1 runs the two env halves as two chains on two HIP streams (the
sampler keys its RNG by the global row, its row_offset, the stepper by the global
env id); ACMI_ROLLOUT_GRAPH=1 captures the rollout once as a hipGraph and replays it (the
RNG counter read from device memory, the sampler's counter_dev).  Neither is faster on one
MI355X (same lease, two rounds each: 512 x 20 2.68 vs 2.69-2.70 M env-steps/s split on /
off; 1024 x 20 bf16 2.72-2.75 M both): the per-step kernels are GPU-bound and the host
keeps up.  They are kept for hosts where launch overhead is not hidden.  (An earlier
+6 % for the split came from a race, since fixed: half 1 read the conv tower's prepared
weights while half 0's step 0 was re-making them after an update.)
"""

import ctypes
import os
import time

from abc import ABCMeta, abstractmethod

import torch

from actorcritic import _lib, _ops
from actorcritic._engine import OBS_BYTES
from actorcritic.episode_stats import EpisodeStats
from actorcritic.return_norm import own_or_for_envs


class Agent(object, metaclass=ABCMeta):
    @abstractmethod
    def interact(self, session):
        pass


class SingleEnvAgent(Agent):
    """One env, multiple steps; list-based (agents.py:50-131)."""

    def __init__(self, env, model, num_steps):
        self._env = env
        self._model = model
        self._num_steps = num_steps
        self._observation = None

    def interact(self, session):
        observation_steps, action_steps, reward_steps, terminal_steps, info_steps = [], [], [], [], []
        next_observation = self._observation
        if next_observation is None:
            next_observation = self._env.reset()
        for _ in range(self._num_steps):
            observation_steps.append(next_observation)
            action = self._model.sample_actions([[next_observation]], session)[0]
            next_observation, reward, terminal, info = self._env.step(action)
            action_steps.append(action)
            reward_steps.append(reward)
            terminal_steps.append(terminal)
            info_steps.append(info)
        self._observation = next_observation
        return ([observation_steps], [action_steps], [reward_steps], [terminal_steps], [next_observation],
                [info_steps])


class _RolloutBuffers(object):
    def __init__(self, engine, N, T, env=None):
        dev = engine.device
        self.N, self.T = N, T
        self.obs = torch.zeros((N, T, 84, 84, 4), dtype=torch.uint8, device=dev)
        self.next_obs = torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=dev)
        self.actions_tn = torch.zeros((T, N), dtype=torch.int32, device=dev)
        self.actions = torch.zeros((N, T), dtype=torch.int32, device=dev)
        self.rewards = torch.zeros((N, T), dtype=torch.float32, device=dev)
        self.terminals = torch.zeros((N, T), dtype=torch.uint8, device=dev)
        self.episode_rewards = torch.zeros((N, T), dtype=torch.float32, device=dev)
        # terminals the step cap alone caused (the targets keep their bootstrap): filled by
        # envs that say ``emits_truncations`` (envs.games.DeviceGameEnvs with an option on)
        self.truncations = torch.zeros((N, T), dtype=torch.uint8, device=dev)
        self.emits_truncations = bool(getattr(env, 'emits_truncations', False))
        self.acts = engine.activations(N * T, 'rollout')
        self.bad_host = torch.zeros(2, dtype=torch.int32, pin_memory=True)  # (engine._bad_counts)
        self.bad_event = None
        # two-chain rollout: env halves on the current stream and a side stream,
        # each with its own forward workspace (fc4 split-K slabs)
        self.halves = (os.environ.get('ACMI_ROLLOUT_SPLIT', '0') == '1' and N >= 256 and N % 2 == 0)
        self.side = torch.cuda.Stream(device=dev) if self.halves else None
        need = int(_lib.load().acmi_forward_ws_floats(N // 2 if self.halves else N))
        self.ws = [torch.zeros(max(need, 1), dtype=torch.float32, device=dev) for _ in range(2)]
        self.use_graph = os.environ.get('ACMI_ROLLOUT_GRAPH', '0') == '1'
        # the fused step (acmi_rollout_step) takes up to 31 actions; wider action sets
        # step unfused: forward + sampler + env step, the ACMI_ROLLOUT_FUSED=0 path.
        # So does an env that says ``fused_step = False`` (envs.games.DeviceGameEnvs
        # unless built with fused_step=True); no such attribute = fused
        self.fused = (os.environ.get('ACMI_ROLLOUT_FUSED', '1') != '0' and
                      engine.A <= _lib.ROLLOUT_STEP_MAX_ACTIONS and
                      bool(getattr(env, 'fused_step', True)))
        # step fusion: step t's tail also runs step t+1's conv tower (needs the
        # fused tower: x3 gemm mode, checked once per rollout, and prepared weights)
        self.fuse_steps = self.fused and os.environ.get('ACMI_ROLLOUT_FUSE_STEPS', '1') != '0'
        self.graph, self.graph_key, self.warm = None, None, False
        self.ctr_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.host = None  # _HostRolloutBuffers, made by the first host-stepped rollout


class _HostRolloutBuffers(object):
    """What a rollout over host-stepped envs adds to _RolloutBuffers."""

    def __init__(self, dev, N, T):
        # row t: the N actions of step t, then that step's count of non-finite logit rows
        self.act_bad = torch.zeros((T, N + 1), dtype=torch.int32, device=dev)
        self.act_bad_host = torch.zeros(N + 1, dtype=torch.int32, pin_memory=True)
        self.event = torch.cuda.Event()
        self.rewards = torch.zeros((N, T), dtype=torch.float32, pin_memory=True)
        self.terminals = torch.zeros((N, T), dtype=torch.uint8, pin_memory=True)
        self.episode_rewards = torch.zeros((N, T), dtype=torch.float32, pin_memory=True)


class MultiEnvAgent(Agent):
    """Multiple envs (MultiEnv), multiple steps (agents.py:134-228)."""

    def __init__(self, multi_env, model, num_steps, copy_batches=False, mask_actions=False, episode_stats=None):
        """mask_actions: take the batched env's ``legal_action_masks`` (one word per env)
        and set them on the model (AtariModel.set_action_masks): every action is then
        drawn from its env's legal set, and the losses / K-FAC statistics of that model
        run over it.  Off by default.  (Every rollout form follows the masks the model
        holds, however they were set.)
        episode_stats: an episode_stats.EpisodeStats, or True for ``EpisodeStats.for_envs(multi_env)``:
        after every complete rollout the agent adds the rollout's episode rewards to it (device
        paths: two launches on the engine's stream, no host wait; the list path: on the host);
        ``agent.episode_stats`` is the object, its state part of ``run_state()``.  None (default):
        nothing is allocated and the rollout runs as it always did."""
        self._env = multi_env
        self._model = model
        self._num_steps = num_steps
        self._observations = None
        self._bufs = None
        self._copy = bool(copy_batches)
        self._mask_actions = bool(mask_actions)
        # the last rollout's truncations, [N, T] bool on the device (the feed of
        # model.truncations_placeholder); None for envs that emit none
        self.last_truncations = None
        if not isinstance(episode_stats, (EpisodeStats, bool, type(None))):
            raise TypeError('episode_stats: an EpisodeStats or True, got {}'.format(type(episode_stats).__name__))
        self.episode_stats = own_or_for_envs(episode_stats, EpisodeStats, multi_env)
        if self.episode_stats is not None and self.episode_stats.num_envs != multi_env.num_envs:
            raise ValueError('episode_stats of {} envs for an agent of {}'.format(self.episode_stats.num_envs,
                                                                               multi_env.num_envs))
        if self._mask_actions:
            masks = getattr(getattr(multi_env, 'batched', None), 'legal_action_masks', None)
            if masks is None:
                raise ValueError('mask_actions=True needs a batched env with legal_action_masks '
                                 '(SyntheticAtariEnvs(games=...) or HostAtariEnvs(legal_actions=...))')
            model.set_action_masks(masks)

    def _fast(self):
        return getattr(self._env, 'batched', None) is not None and hasattr(self._model, 'engine')

    def interact(self, session):
        """One T-step rollout -> (observations [N,T,...], actions [N,T], rewards [N,T],
        terminals [N,T], next_observations [N,...], infos) (agents.py:157-228).

        Device rollout aliasing: the returned tensors are the agent's persistent
        rollout buffers and the NEXT interact() overwrites them in place (the
        reference returns fresh lists every call).  A caller that keeps a batch
        across calls (logging, replay, comparing rollouts) clones it, or constructs
        the agent with ``copy_batches=True`` to receive fresh tensors every call."""
        if self._fast():
            return self._interact_device()
        return self._interact_lists(session)

    # -- reference semantics (host lists) ---------------------------------------
    def _interact_lists(self, session):
        observation_steps, action_steps, reward_steps, terminal_steps, info_steps = [], [], [], [], []
        next_observations = self._observations
        if next_observations is None:
            next_observations = self._env.reset()
        for _ in range(self._num_steps):
            observation_steps.append(next_observations)
            batch_next_observations = transpose_list([next_observations])
            actions = self._model.sample_actions(batch_next_observations, session)
            next_observations, rewards, terminals, infos = self._env.step(actions)
            action_steps.append(actions)
            reward_steps.append(rewards)
            terminal_steps.append(terminals)
            info_steps.append(infos)
        self._observations = next_observations
        infos = transpose_list(info_steps)
        if self.episode_stats is not None:
            from actorcritic.envs.atari.wrappers import EpisodeInfoWrapper
            self.episode_stats.update(EpisodeInfoWrapper.get_episode_rewards_from_info_batch(infos))
        return (transpose_list(observation_steps), transpose_list(action_steps), transpose_list(reward_steps),
                transpose_list(terminal_steps), next_observations, infos)

    # -- device rollout ------------------------------------------------------------
    def _rollout_halves(self, eng, env, rb, N, T, A, seed, dev_ctr=False):
        """The T-step rollout as one chain (rb.halves False) or as the two env halves'
        chains on the current stream and rb.side."""
        main = torch.cuda.current_stream(eng.device)
        if not rb.fused:  # (the fused step 0 reads next_obs in place and files it into obs[:, 0])
            rb.obs[:, 0].copy_(rb.next_obs)
        # the tower's prepared weights are re-made on the first use after an update:
        # here, on this stream ahead of the fork (half 1 on rb.side would otherwise
        # read them before half 0's step 0 re-made them); always when capturing a
        # graph, so that every replay re-prepares from the updated parameters
        eng.net(force_prepare=dev_ctr)
        if rb.halves:
            rb.side.wait_stream(main)
        N2 = N // 2 if rb.halves else N
        # step fusion is decided once per rollout: a gemm mode switched mid-rollout must
        # not let step t skip a tower that step t-1's tail never ran
        fuse = bool(rb.fused and rb.fuse_steps and eng.lib.acmi_get_gemm_mode() == _lib.GEMM_X3)
        for t in range(T):
            _half_step(eng, env, rb, 0, N2, T, A, t, seed, dev_ctr, fuse)
            if rb.halves:
                with torch.cuda.stream(rb.side):
                    _half_step(eng, env, rb, 1, N2, T, A, t, seed, dev_ctr, fuse)
            if not dev_ctr:
                eng.sample_counter += 1
        if rb.halves:
            main.wait_stream(rb.side)
        if not rb.fused:  # (the fused tail writes actions [N, T] itself)
            rb.actions.copy_(rb.actions_tn.t())

    def _rollout_graph(self, eng, env, rb, N, T, A, seed):
        """The two-chain rollout as one hipGraph (torch.cuda.CUDAGraph over the
        libacmi launches): captured on the second rollout with these buffers, then
        replayed -- ~280 launches per rollout stop costing host time.  Everything
        that differs between rollouts lives in device memory (observations, env
        states, parameters updated in place); the RNG counter is refreshed in
        rb.ctr_dev before each replay."""
        # everything the captured launches bake in: buffers, env, seed, rank, and the
        # arithmetic modes / step fusion that chose the captured kernels
        lib = eng.lib
        key = (eng.params.data_ptr(), id(env), seed, eng.rank, int(lib.acmi_get_gemm_mode()),
               int(lib.acmi_get_forward_mode()), bool(rb.fuse_steps),
               None if eng.masks is None else eng.masks.data_ptr())
        if rb.graph is None or rb.graph_key != key:
            if not rb.warm:  # first rollout eager: loads the code objects, sizes workspaces
                rb.warm = True
                self._rollout_halves(eng, env, rb, N, T, A, seed)
                return
            rb.ctr_dev.fill_(eng.sample_counter & 0xFFFFFFFF)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._rollout_halves(eng, env, rb, N, T, A, seed, dev_ctr=True)
            rb.graph, rb.graph_key = g, key
        else:
            rb.ctr_dev.fill_(eng.sample_counter & 0xFFFFFFFF)
        rb.graph.replay()
        eng.sample_counter += T

    def _interact_device(self):
        eng = self._model.engine
        env = self._env.batched
        N, T = env.num_envs, self._num_steps
        if self._bufs is None or self._bufs.N != N or self._bufs.T != T:
            self._bufs = _RolloutBuffers(eng, N, T, env)
        rb = self._bufs
        if getattr(env, 'host_stepped', False):
            return self._interact_host(eng, env, rb, N, T)
        if rb.bad_event is not None:  # deferred NaN-logit check of the previous rollout
            t_wait = time.perf_counter()
            rb.bad_event.synchronize()
            self.last_sync_wait = time.perf_counter() - t_wait  # (bench.py's host-time split)
            if int(rb.bad_host[0]) > 0 or int(rb.bad_host[1]) > 0:
                eng.check_bad_rows()
        if self._observations is None:
            env.reset_into(rb.next_obs.data_ptr())
        seed = (self._model._random_seed or 0) & 0xFFFFFFFF
        if rb.use_graph:
            self._rollout_graph(eng, env, rb, N, T, eng.A, seed)
        else:
            self._rollout_halves(eng, env, rb, N, T, eng.A, seed)
        rb.bad_host.copy_(eng._bad_counts, non_blocking=True)
        rb.bad_event = torch.cuda.Event()
        rb.bad_event.record()
        return self._batch(eng, rb, N, T)

    def _interact_host(self, eng, env, rb, N, T):
        """The device rollout over host-stepped envs (HostAtariEnvs): per step one strided
        forward into the update's activation rows, one sampling kernel, ONE host wait (the
        D2H of the N actions and the bad-row counter), the envs' host step, and one upload
        + acmi_atari_rollout_frames launch that writes the next stacks into obs[:, t+1].
        Rewards / terminals / episode rewards gather in pinned [N, T] arrays and are
        uploaded once.  The fused step, graph capture and the two-halves split of the
        synthetic stepper do not apply: one chain, any action count."""
        if rb.host is None:
            rb.host = _HostRolloutBuffers(eng.device, N, T)
        hb = rb.host
        if self._observations is None:
            env.reset_into(rb.next_obs.data_ptr())
        A = eng.A
        legal = _mask_rows(eng, N)
        stream = eng.stream()
        obs0 = rb.obs.data_ptr()
        seed = (self._model._random_seed or 0) & 0xFFFFFFFF
        rb.obs[:, 0].copy_(rb.next_obs)
        hb.act_bad.zero_()
        rewards, terminals, episode_rewards = hb.rewards.numpy(), hb.terminals.numpy(), hb.episode_rewards.numpy()
        for t in range(T):
            src = obs0 + t * OBS_BYTES
            eng.forward(src, N, rb.acts.view(t, T), want_value=True, img_stride=T * OBS_BYTES, act_stride=T)
            row = hb.act_bad[t]  # [actions of step t (N) | rows with non-finite logits (1)]
            _ops.sample_actions(rb.acts.logits.data_ptr() + 4 * t * A, T * A, N, A, seed, 0, eng.sample_counter,
                                eng.rank * N, row.data_ptr(), row.data_ptr() + 4 * N, stream, legal=legal)
            eng.sample_counter += 1
            hb.act_bad_host.copy_(row, non_blocking=True)
            hb.event.record()
            hb.event.synchronize()  # the step's only host wait
            got = hb.act_bad_host.numpy()
            if got[N] != 0:  # no env sees an action of -1
                eng._bad_rows += int(got[N])
                eng.check_bad_rows()
            rewards[:, t], terminals[:, t], episode_rewards[:, t] = env.host_step(got[:N])
            if t + 1 < T:
                dst, dstride = src + OBS_BYTES, T * OBS_BYTES
            else:
                dst, dstride = rb.next_obs.data_ptr(), OBS_BYTES
            env.stack_into(src, T * OBS_BYTES, dst, dstride)
        rb.actions.copy_(hb.act_bad[:, :N].t())
        rb.rewards.copy_(hb.rewards, non_blocking=True)
        rb.terminals.copy_(hb.terminals, non_blocking=True)
        rb.episode_rewards.copy_(hb.episode_rewards, non_blocking=True)
        return self._batch(eng, rb, N, T)

    # -- run state -----------------------------------------------------
    def _stateful_env(self):
        """The batched device env whose state a run state holds; ValueError for the others."""
        if not self._fast():
            raise ValueError('a run state needs a batched device env: the list path keeps its state in host envs')
        env = self._env.batched
        if getattr(env, 'host_stepped', False) or not hasattr(env, 'state_dict'):
            raise ValueError('{} has no run state: host-stepped envs keep their state in the host envs'
                             .format(type(env).__name__))
        return env

    def run_state(self):
        """What the next ``interact()`` reads beside the model, between two complete rollouts:
        ``{'next_obs': [N,84,84,4] u8, 'sample_counter': int, 'env': the batched env's
        state_dict()}`` and, with episode statistics, ``'episode_stats'``: their ``state_dict()``;
        CPU tensors and plain ints.  Waits for the engine's stream (and the
        side stream of the two-halves form).  ValueError before the first ``interact()`` and
        for host-stepped or list-path envs.  The rollout length is not part of it."""
        env = self._stateful_env()
        rb = self._bufs
        if self._observations is None or rb is None:
            raise ValueError('run_state() before the first interact(): the envs have not been reset')
        eng = self._model.engine
        torch.cuda.current_stream(eng.device).synchronize()
        if rb.side is not None:
            rb.side.synchronize()
        state = {'next_obs': rb.next_obs.detach().cpu().clone(), 'sample_counter': int(eng.sample_counter),
                 'env': env.state_dict()}
        if self.episode_stats is not None:  # (the interval's accumulators and the running episodes' lengths)
            state['episode_stats'] = self.episode_stats.state_dict()
        return state

    def load_run_state(self, state):
        """Continues from a ``run_state()``: fills ``next_obs`` (making the rollout buffers for
        (N, this agent's T) if need be) and marks the envs as reset, so that no ``reset_into``
        follows; sets the engine's ``sample_counter``; loads the env state (ValueError when the
        envs are not the saved ones); with episode statistics, loads ``state['episode_stats']``
        (ValueError when it is missing or of other groups).  Load the model checkpoint first
        (checkpoint.load)."""
        env = self._stateful_env()
        if self.episode_stats is not None and 'episode_stats' not in state:
            raise ValueError('run state: no episode_stats for the agent\'s EpisodeStats')
        eng = self._model.engine
        N, T = env.num_envs, self._num_steps
        nxt = state['next_obs']
        if not torch.is_tensor(nxt) or tuple(nxt.shape) != (N, 84, 84, 4) or nxt.dtype != torch.uint8:
            raise ValueError('run state: next_obs is not the [{}, 84, 84, 4] uint8 stacks of these envs'.format(N))
        env.load_state_dict(state['env'])
        if self._bufs is None or self._bufs.N != N or self._bufs.T != T:
            self._bufs = _RolloutBuffers(eng, N, T, env)
        self._bufs.next_obs.copy_(nxt.to(eng.device))
        self._observations = self._bufs.next_obs
        eng.sample_counter = int(state['sample_counter'])
        if self.episode_stats is not None:
            self.episode_stats.load_state_dict(state['episode_stats'])

    def _batch(self, eng, rb, N, T):
        """interact()'s 6-tuple from the rollout buffers, registered for the update."""
        from actorcritic.envs.atari.model import ForwardOut
        from actorcritic.envs.atari.wrappers import EpisodeInfoBatch
        self._observations = rb.next_obs
        if self.episode_stats is not None:  # (after everything the rollout joined on this stream)
            self.episode_stats.update(rb.episode_rewards, eng.stream())
        out = (rb.obs, rb.actions, rb.rewards, rb.terminals.view(torch.bool), rb.next_obs, rb.episode_rewards)
        trunc = rb.truncations.view(torch.bool) if rb.emits_truncations else None
        if self._copy:
            out = tuple(x.clone() for x in out)
            trunc = None if trunc is None else trunc.clone()
        self.last_truncations = trunc
        obs = out[0]
        # the update re-uses the rollout activations for exactly these observations
        fwd = ForwardOut(eng, rb.acts, N, T, obs.view(N * T, 84, 84, 4))
        eng.register_rollout(obs, fwd)
        return out[:5] + (EpisodeInfoBatch(out[5]),)


def _trunc_arg(rb, row):
    """step_into's keyword for the truncation byte of batch element ``row`` (the
    terminals' layout), for envs that emit truncations; none otherwise."""
    return {'trunc_ptr': rb.truncations.data_ptr() + row} if rb.emits_truncations else {}


def _mask_rows(eng, N):
    """Device address of the engine's per-env legal-action words (None: no masks);
    ValueError unless there is one word per env of the rollout."""
    if eng.masks is None:
        return None
    return eng.row_masks(N).data_ptr()


def _half_step(eng, env, rb, h, N2, T, A, t, seed, dev_ctr=False, fuse=False):
    """Rollout step t of env half h (envs h*N2 .. h*N2+N2-1) on the current stream.
    dev_ctr: the sampler's RNG counter is rb.ctr_dev + t (graph capture) instead of
    the host eng.sample_counter.  fuse: step fusion for the whole rollout (decided
    once by the caller, so tower_done at step t means step t-1 passed next_acts)."""
    n0 = h * N2
    row = n0 * T + t
    obs0 = rb.obs.data_ptr()
    src = obs0 + row * OBS_BYTES
    acts = rb.acts.view(row, T, ws_rows=N2)
    acts.ws = rb.ws[h].data_ptr()
    acts.ws_floats = rb.ws[h].numel()
    act_t = rb.actions_tn[t].data_ptr() + 4 * n0
    # the sampler's RNG is keyed by the global env row (stream 0): env shards over
    # ranks draw exactly what one process stepping all envs would
    row0 = eng.rank * rb.N + n0
    legal = _mask_rows(eng, rb.N)
    if legal is not None:
        legal += 4 * n0  # (the env half's words)
    if dev_ctr:
        ctr_dev, ctr = _lib.c_vp(rb.ctr_dev.data_ptr()), t
    else:
        ctr_dev, ctr = None, eng.sample_counter & 0xFFFFFFFF
    if t + 1 < T:
        dst, dstride = src + OBS_BYTES, T * OBS_BYTES
    else:
        dst, dstride = rb.next_obs.data_ptr() + n0 * OBS_BYTES, OBS_BYTES
    rew, term, ep = rb.rewards.data_ptr() + 4 * row, rb.terminals.data_ptr() + row, \
        rb.episode_rewards.data_ptr() + 4 * row
    if rb.fused:  # tower + fused heads/sample/env-step tail (acmi_rollout_step)
        # step fusion: step t's tower ran in step t-1's tail; step t's tail runs
        # step t+1's tower (not the last step's: the bootstrap forward is the update's)
        nxt = rb.acts.view(row + 1, T, ws_rows=N2) if fuse and t + 1 < T else None
        # step 0 reads the previous rollout's final stacks (next_obs) in place and
        # copies them into obs[:, 0] (the batch's step-0 rows) as it goes
        src_t, sstride = (rb.next_obs.data_ptr() + n0 * OBS_BYTES, OBS_BYTES) if t == 0 else (src, T * OBS_BYTES)
        # actions straight into the [N, T] batch (element b at [b*T], like the rewards)
        act_nt = rb.actions.data_ptr() + 4 * row
        # an env with a fused step of its own (envs.games.DeviceGameEnvs) brings its
        # entry point and the rest of its io: rollout_step; the others acmi_rollout_step
        own = getattr(env, 'rollout_step', None)
        io = _lib.RolloutIO(seed, 0, ctr, ctr_dev, row0, act_nt, eng._bad_rows.data_ptr(),
                            _lib.EnvState() if own else env.range_state(n0),
                            env.env_offset + n0, env.seed, dst, dstride, rew, term, ep, T,
                            1 if fuse and t > 0 else 0, ctypes.addressof(nxt) if nxt is not None else None, T,
                            src if t == 0 else None)
        if own:
            own(eng.net(), src_t, sstride, n0, N2, acts, T, io, eng.stream(), legal=legal, **_trunc_arg(rb, row))
        else:
            _ops.rollout_step(eng.net(), src_t, sstride, N2, acts, T, io, eng.stream(), legal=legal)
        return
    eng.forward(src, N2, acts, want_value=True, img_stride=T * OBS_BYTES, act_stride=T)
    _ops.sample_actions(rb.acts.logits.data_ptr() + 4 * row * A, T * A, N2, A, seed, 0, ctr, row0, act_t,
                        eng._bad_rows.data_ptr(), eng.stream(), legal=legal, counter_dev=ctr_dev)
    env.step_range_into(n0, N2, act_t, src, T * OBS_BYTES, dst, dstride, rew, term, ep, T, **_trunc_arg(rb, row))


def transpose_list(values):
    """Transposes a list of lists (agents.py:231-257): [[1,2],[3,4]] -> [[1,3],[2,4]]."""
    return [list(row) for row in zip(*values)]
