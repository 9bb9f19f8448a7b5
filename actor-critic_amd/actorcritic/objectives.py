"""Objectives (reference: actorcritic/objectives.py:10-214).

:class:`A2CObjective` keeps the reference's maths — n-step discounted targets with
terminal cuts and a bootstrap from V(s_T) (objectives.py:123-126, closures :178-214),
stop-gradient advantage (:128-130), no advantage normalisation, policy loss
``-(mean(adv*log pi) + beta*mean(H))`` (:132-149) and baseline loss
``mean((target-V)^2/2)`` (:151-154) — evaluated by libacmi (acmi_returns,
acmi_a2c_loss).  The py_func discount-matrix closures become one reverse scan per
env whose gamma tables are the exact float32 values the closures produce.

Two options go beyond the reference (BASELINE.json's north_star names them; both
off by default, so the defaults are the reference's objective): ``gae_lambda``
(GAE(lambda) targets/advantages, acmi_gae; lambda = 1 is the n-step target in
exact arithmetic) and ``normalize_advantages`` (batch-normalised advantages for
the policy loss, acmi_adv_moments / acmi_adv_normalize; under data parallelism
the moments are summed over ranks, so every rank normalises with the global
batch's mean and std).

Time limits (beyond the reference as well): when ``model.truncations_placeholder`` is
fed (bool [env, step]: the terminals that a step cap alone caused, ``MultiEnvAgent.
last_truncations``), those terminals still cut the return but keep the bootstrap from
the value of the next observation -- row t+1 of the batch, or the bootstrap row at
t = T-1 -- through the truncating forms of acmi_returns / acmi_gae (_ops.targets).
Unfed, every terminal cuts it.

Reward scaling (beyond the reference as well, off by default): ``normalize_returns`` takes a
:class:`actorcritic.return_norm.ReturnNormalizer`; the targets are then formed from the
rewards scaled by the running std of the discounted return of each env's group (game) --
acmi_retnorm_scan, the moments summed over ranks, acmi_retnorm_apply -- written to a buffer
of the update state; the fed tensor is not written.  The statistics advance once per
``session.run`` that evaluates the targets (PPO's epochs and minibatches reuse them) -- also
in a run that fetches only ``target_values``, unless the normalizer is ``frozen``.
``normalized_rewards`` and ``return_stats`` are fetchable.

:class:`PPOObjective` (also beyond the reference) shares those targets and
advantages and replaces the loss by PPO's clipped surrogate (acmi_ppo_loss); its
``optimize_shared`` op takes several epochs of minibatch gradient steps per
``session.run`` (:class:`PPOOptimizeOp`), over env slices of the batch or -- through a
device row gather (acmi_gather_rows) -- over per-row shuffled minibatches.

:class:`VTraceObjective` (beyond the reference as well) keeps A2C's losses and replaces the targets by
V-trace's (acmi_vtrace; actorcritic/vtrace.py states them): importance weights of the current policy against
the one that acted, ``model.behaviour_log_probs_placeholder`` or the batch's own forward, correct targets and
advantages, so that its ``optimize_shared`` op may take several gradient steps per batch
(:class:`VTraceOptimizeOp`, over env slices) and re-forms the targets at each.
"""

from abc import ABCMeta, abstractmethod

import numpy as np
import torch

from actorcritic import _lib, _ops
from actorcritic.session import Node, as_node


def gamma_tables(gamma, T):
    """gamma_pow[k] = f32(gamma)**f32(k) (numpy float32 power: the D-matrix entries of
    objectives.py:183-187); boot_pow[k] = k-fold sequential float32 product (the
    float32 cumprod of objectives.py:211)."""
    g = np.float32(gamma)
    gp = (g ** np.arange(T, dtype=np.float32)).astype(np.float32)
    bp = np.ones(T + 1, np.float32)
    for k in range(1, T + 1):
        bp[k] = np.float32(bp[k - 1] * g)
    return gp, bp


class ActorCriticObjective(object, metaclass=ABCMeta):
    @property
    @abstractmethod
    def policy_loss(self):
        pass

    @property
    @abstractmethod
    def baseline_loss(self):
        pass

    def optimize_separate(self, policy_optimizer, baseline_optimizer, policy_kwargs=None, baseline_kwargs=None):
        """Separate optimisation of the two losses (objectives.py:31-54) is not supported for the
        shared-trunk Atari model on this engine (out of the hot-path scope)."""
        raise NotImplementedError('optimize_separate is not supported; use optimize_shared')

    def optimize_shared(self, optimizer, baseline_loss_weight=0.5, **kwargs):
        """optimizer.minimize(policy_loss + baseline_loss_weight * baseline_loss) (objectives.py:56-79)."""
        shared_loss = SharedLoss(self, baseline_loss_weight)
        return optimizer.minimize(shared_loss, **kwargs)


class SharedLoss(Node):
    """policy_loss + w * baseline_loss: the differentiable loss of optimize_shared."""

    def __init__(self, objective, weight):
        self.objective = objective
        self.weight = float(weight)
        self.name = 'shared_loss'
        objective._vcoef = self.weight

    def _eval(self, ctx):
        # the loss vector itself: the update needs only its kernels to have run (the
        # gradient comes from acmi_a2c_loss's dhead), and a fetched value is formed
        # by _finalize -- no two device launches per update for the scalar
        return ctx.eval(self.objective._loss_node)

    def _finalize(self, ctx, value):
        loss = self.objective._loss_node.scalars(ctx)
        return loss[0] + self.weight * loss[1]


class _Targets(Node):
    name = 'target_values'

    def __init__(self, objective):
        self.objective = objective

    def _eval(self, ctx):
        obj = self.objective
        model = obj._model
        eng = model.engine
        fwd = ctx.eval(model._forward)
        boot = ctx.eval(model._bootstrap_forward)
        N, T = fwd.batch, fwd.steps
        if boot.batch != N:
            raise ValueError('bootstrap observations must have one row per environment ({} != {})'
                             .format(boot.batch, N))
        rewards = _device(ctx.eval(model.rewards_placeholder), torch.float32, eng.device).reshape(N, T)
        terminals = _device_bool_u8(ctx.eval(model.terminals_placeholder), eng.device).reshape(N, T)
        st = eng.update_state(N * T)
        trunc = ctx.feeds.get(model.truncations_placeholder)
        if trunc is not None:  # time limits: those terminals keep their bootstrap (module docstring)
            trunc = _device_bool_u8(trunc, eng.device).reshape(N, T)
        if obj._retnorm is not None:  # per-game reward scaling: once per run (this node is memoised)
            rewards = obj._retnorm.normalize(rewards, terminals, obj._gamma, st.reward_buffer(N, T), eng.stream(),
                                             eng.world_size)
        self._launch(ctx, st, fwd, boot, rewards, terminals, trunc)
        if obj._normalize:
            _normalize_advantages(eng, st.adv, N * T, obj._adv_eps)
        st.fwd = fwd
        return st

    def _launch(self, ctx, st, fwd, boot, rewards, terminals, trunc):
        """st.targets, st.adv <- the targets and advantages of the [N][T] batch."""
        obj = self.objective
        eng = obj._model.engine
        N, T = fwd.batch, fwd.steps
        tables = obj._tables(T, eng.device) if obj._gae_lambda is None else None
        _ops.targets(rewards, terminals, fwd.flat_value, boot.flat_value, N, T, obj._gamma, obj._gae_lambda, tables,
                     st.targets, st.adv, eng.stream(), truncated=trunc)


class _ReturnStats(Node):
    """The normalizer's stats ([G][3] f64: count, mean, M2) after this run's targets."""
    name = 'return_stats'

    def __init__(self, objective):
        self.objective = objective

    def _eval(self, ctx):
        obj = self.objective
        if obj._retnorm is None:
            raise ValueError('return_stats needs an objective built with normalize_returns=')
        ctx.eval(obj._targets_node)
        return obj._retnorm.stats.clone()


def _check_normalizer(normalize_returns):
    from actorcritic.return_norm import ReturnNormalizer
    if normalize_returns is not None and not isinstance(normalize_returns, ReturnNormalizer):
        raise TypeError('normalize_returns takes a ReturnNormalizer or None, got {!r}'.format(normalize_returns))
    return normalize_returns


def _check_diagnostics(diagnostics):
    from actorcritic.update_diag import UpdateDiagnostics
    if diagnostics is not None and not isinstance(diagnostics, UpdateDiagnostics):
        raise TypeError('diagnostics takes an UpdateDiagnostics or None, got {!r}'.format(diagnostics))
    return diagnostics


def _normalize_advantages(eng, adv, M, eps):
    """adv <- (adv - mean) / (std + eps) over the global batch (all ranks)."""
    ws = getattr(eng, '_adv_ws', None)
    need = int(eng.lib.acmi_adv_moments_ws_doubles(M))
    if ws is None or ws.numel() < need:
        ws = torch.zeros(need, dtype=torch.float64, device=eng.device)
        eng._adv_ws = ws
        eng._adv_moments = torch.zeros(2, dtype=torch.float64, device=eng.device)
    mom = eng._adv_moments
    _lib.call('acmi_adv_moments', _lib.ptr(adv), M, _lib.ptr(ws), _lib.ptr(mom), eng.stream())
    if eng.world_size > 1:
        from actorcritic import parallel
        parallel.allreduce_sum_(mom)
    _lib.call('acmi_adv_normalize', _lib.ptr(adv), M, _lib.ptr(mom), float(M * eng.world_size), float(eps),
              eng.stream())


class _Loss(Node):
    """Loss scalars [policy, baseline, entropy] + head gradients in the update state."""
    name = 'losses'

    def __init__(self, objective):
        self.objective = objective

    def _eval(self, ctx):
        obj = self.objective
        model = obj._model
        eng = model.engine
        st = ctx.eval(obj._targets_node)
        fwd = ctx.eval(model._forward)
        actions = _device(ctx.eval(model.actions_placeholder), torch.int32, eng.device).reshape(-1)
        M = fwd.M
        if actions.numel() != M:
            raise ValueError('actions must have the shape of the observations batch [env, step]')
        st.actions = actions
        # the kernel scales the loss scalars by 1/world like dhead; they hold the
        # global means once the update's all-reduce has summed them (loss_reduced)
        st.loss_reduced = eng.world_size == 1
        st.fwd = fwd
        # with masks: over each row's legal set; bad rows count in the engine's counter
        _ops.a2c_loss(fwd.flat_logits, eng.A, fwd.flat_value, actions, st.targets, st.adv, M, eng.A,
                      float(obj._beta), float(obj._vcoef), 1.0 / eng.world_size, st.dhead, eng.ldh, st.loss_ws,
                      st.loss, eng.stream(), legal=fwd.row_masks(), bad_rows=eng._mask_bad_rows)
        return st.loss

    def scalars(self, ctx):
        """[policy, baseline, entropy] of this run as fetched: the global means when
        the run's optimize op all-reduced them, else (no update in the run) this
        rank's means -- the kernel's 1/world scale undone."""
        loss = ctx.eval(self)
        st = ctx.eval(self.objective._targets_node)
        if getattr(st, 'loss_reduced', True):
            return loss[:3]
        return loss[:3] * float(self.objective._model.engine.world_size)


class _LossScalar(Node):
    def __init__(self, loss_node, index, name):
        self.loss_node, self.index, self.name = loss_node, index, name

    def _eval(self, ctx):
        return ctx.eval(self.loss_node)[self.index]

    def _finalize(self, ctx, value):
        return self.loss_node.scalars(ctx)[self.index]


class A2CObjective(ActorCriticObjective):
    """A2C/ACKTR objective (objectives.py:82-175)."""

    def __init__(self, model, discount_factor=0.99, entropy_regularization_strength=0.01, name=None,
                 gae_lambda=None, normalize_advantages=False, advantage_epsilon=1e-8, normalize_returns=None,
                 diagnostics=None):
        """The reference's arguments (objectives.py:100); ``gae_lambda`` (None: the
        reference's n-step targets; a float in [0, 1]: GAE(lambda)), ``normalize_advantages``,
        ``normalize_returns`` (a :class:`actorcritic.return_norm.ReturnNormalizer`) and
        ``diagnostics`` (a :class:`actorcritic.update_diag.UpdateDiagnostics`: the optimize op
        records an update's diagnostics whenever the object is armed) are extensions beyond it
        (module docstring)."""
        if gae_lambda is not None and not 0.0 <= float(gae_lambda) <= 1.0:
            raise ValueError('gae_lambda must be in [0, 1] or None, got {}'.format(gae_lambda))
        self._model = model
        self._gamma = float(discount_factor)
        self._gae_lambda = None if gae_lambda is None else float(gae_lambda)
        self._normalize = bool(normalize_advantages)
        self._retnorm = _check_normalizer(normalize_returns)
        self.diagnostics = _check_diagnostics(diagnostics)
        self._adv_eps = float(advantage_epsilon)
        self._beta = float(entropy_regularization_strength)
        self._vcoef = 0.5
        self._name = name or 'A2CObjective'
        self._table_cache = {}
        self._targets_node = _Targets(self)
        self._loss_node = _Loss(self)
        self._policy_loss = _LossScalar(self._loss_node, 0, 'policy_loss')
        self._baseline_loss = _LossScalar(self._loss_node, 1, 'baseline_loss')
        self._mean_entropy = _LossScalar(self._loss_node, 2, 'mean_entropy')

    def _tables(self, T, device):
        if T not in self._table_cache:
            gp, bp = gamma_tables(self._gamma, T)
            self._table_cache[T] = (torch.from_numpy(gp).to(device), torch.from_numpy(bp).to(device))
        return self._table_cache[T]

    @property
    def model(self):
        return self._model

    @property
    def target_values(self):
        return _TargetView(self._targets_node, 'targets')

    @property
    def advantage(self):
        return _TargetView(self._targets_node, 'adv')

    @property
    def normalized_rewards(self):
        """The scaled rewards [env, step] the targets were formed from (``normalize_returns``)."""
        if self._retnorm is None:
            raise ValueError('normalized_rewards needs an objective built with normalize_returns=')
        return _TargetView(self._targets_node, 'norm_rewards')

    @property
    def return_stats(self):
        """The normalizer's per-group (count, mean, M2), [G][3] float64, after this run."""
        return _ReturnStats(self)

    @property
    def return_normalizer(self):
        """The ReturnNormalizer given as ``normalize_returns``, or None."""
        return self._retnorm

    @property
    def policy_loss(self):
        return self._policy_loss

    @property
    def baseline_loss(self):
        return self._baseline_loss

    @property
    def mean_entropy(self):
        return self._mean_entropy


def ppo_minibatch_rows(num_envs, num_steps, num_minibatches):
    """[(first row, rows)] of the ``num_minibatches`` contiguous env slices of an
    env-major [num_envs][num_steps] batch."""
    num_envs, num_minibatches = int(num_envs), int(num_minibatches)
    if num_minibatches < 1 or num_envs % num_minibatches != 0:
        raise ValueError('num_minibatches ({}) must divide the number of environments ({})'
                         .format(num_minibatches, num_envs))
    rows = num_envs // num_minibatches * int(num_steps)
    return [(j * rows, rows) for j in range(num_minibatches)]


def ppo_minibatch_order(shuffle_seed, step, num_epochs, num_minibatches):
    """The env-slice order of every epoch of one PPO update: a host generator seeded
    with (shuffle_seed, global step) draws one permutation per epoch."""
    rng = np.random.default_rng([int(shuffle_seed), int(step)])
    return [[int(j) for j in rng.permutation(int(num_minibatches))] for _ in range(int(num_epochs))]


def ppo_row_order(shuffle_seed, step, num_epochs, M):
    """The row order of every epoch of one PPO update with ``minibatch='rows'``: int32
    permutations of range(M), one per epoch, from the host generator
    :func:`ppo_minibatch_order` uses (seeded with (shuffle_seed, global step): no rank in
    it, so every data-parallel rank draws the same orders)."""
    rng = np.random.default_rng([int(shuffle_seed), int(step)])
    return [rng.permutation(int(M)).astype(np.int32) for _ in range(int(num_epochs))]


class _PPORun(object):
    """What one session.run shares between the PPO nodes."""

    def __init__(self, st, fwd, actions, bufs, masks=None):
        self.st, self.fwd, self.actions, self.bufs = st, fwd, actions, bufs
        self.masks = masks  # the rows' legal-action words (int32 bits) with masks on the engine
        self.stepped = False  # the optimize op ran: the scalars are its last step's
        self.step_st = None

    def vectors(self):
        """The batch's per-row vectors in acmi_ppo_loss's order (with legal-action masks
        on the engine the rows' words follow as a sixth)."""
        v = self.actions, self.bufs.old_logp, self.bufs.old_values, self.st.targets, self.st.adv
        return v if self.masks is None else v + (self.masks,)


class _PPOBuffers(object):
    def __init__(self, eng, M):
        z = lambda n: torch.zeros(n, dtype=torch.float32, device=eng.device)
        self.old_logp, self.old_values = z(M), z(M)
        self.eval_out = z(5)  # [policy, baseline, entropy, approx kl, clip fraction] without an update
        self.clip_frac = z(1)  # the gradient steps' clip fraction (their other scalars: UpdateState.loss)
        self.ws = {}

    def loss_ws(self, eng, M):
        if M not in self.ws:
            self.ws[M] = torch.zeros(int(eng.lib.acmi_ppo_loss_ws_floats(M)), dtype=torch.float32,
                                     device=eng.device)
        return self.ws[M]


class _PPORowBuffers(object):
    """The shuffled copy of an M-row batch that ``minibatch='rows'`` fills once per epoch
    (acmi_gather_rows): observations (M x 28224 bytes) and the five per-row vectors in
    :meth:`_PPORun.vectors`' order (``masked``: and the rows' legal-action words)."""

    def __init__(self, eng, M, masked=False):
        from actorcritic._engine import OBS_SHAPE
        dev = eng.device
        f = lambda: torch.zeros(M, dtype=torch.float32, device=dev)
        i = lambda: torch.zeros(M, dtype=torch.int32, device=dev)
        self.obs = torch.zeros((M,) + tuple(OBS_SHAPE), dtype=torch.uint8, device=dev)
        self.vecs = (i(), f(), f(), f(), f()) + ((i(),) if masked else ())
        self.dst = (_lib.c_vp * len(self.vecs))(*[v.data_ptr() for v in self.vecs])

    def gather(self, eng, run, index):
        """Row r of the copy <- row index[r] of the run's batch (one launch)."""
        from actorcritic._engine import OBS_BYTES
        M = self.obs.shape[0]
        src = run.vectors()
        assert len(src) == len(self.vecs)
        assert all(a.dtype == b.dtype and a.numel() == M for a, b in zip(src, self.vecs))
        src_ptrs = (_lib.c_vp * len(src))(*[_lib.ptr(v).value for v in src])
        _lib.call('acmi_gather_rows', _lib.ptr(run.fwd.obs), OBS_BYTES, M, _lib.ptr(index), M, _lib.ptr(self.obs),
                  OBS_BYTES, len(src), src_ptrs, self.dst, None, eng.stream())


class _PPOBatch(Node):
    """Once per run, from the batch's forward (the rollout's cached activations or a
    fresh one): old log-probabilities and values, targets and advantages."""
    name = 'ppo_batch'

    def __init__(self, objective):
        self.objective = objective

    def _eval(self, ctx):
        obj = self.objective
        model = obj._model
        eng = model.engine
        st = ctx.eval(obj._targets_node)
        fwd = st.fwd
        M = fwd.M
        actions = _device(ctx.eval(model.actions_placeholder), torch.int32, eng.device).reshape(-1)
        if actions.numel() != M:
            raise ValueError('actions must have the shape of the observations batch [env, step]')
        bufs = obj._buffers.get(M)
        if bufs is None:
            bufs = obj._buffers[M] = _PPOBuffers(eng, M)
        masks = fwd.row_masks()
        _ops.categorical(fwd.flat_logits, eng.A, M, eng.A, actions, None, bufs.old_logp, eng.stream(), legal=masks)
        bufs.old_values.copy_(fwd.flat_value)
        return _PPORun(st, fwd, actions, bufs, masks)


class _PPOLoss(Node):
    """[policy, baseline, entropy, approx_kl, clip_fraction]: of the run's last
    gradient step when its optimize op ran, else of the whole batch at the current
    parameters (ratio 1)."""
    name = 'ppo_losses'

    def __init__(self, objective):
        self.objective = objective

    def _eval(self, ctx):
        obj = self.objective
        run = ctx.eval(obj._batch_node)
        if not run.stepped:
            fwd, st, b = run.fwd, run.st, run.bufs
            obj._launch_loss(fwd, run.vectors(), 0, fwd.M, b, st.dhead, b.eval_out[:4], b.eval_out[4:])
        return run

    def scalars(self, ctx):
        run = ctx.eval(self)
        if run.stepped:  # (all-reduced with the gradients: global means)
            return torch.cat([run.step_st.loss, run.bufs.clip_frac])
        # no update in the run: this rank's means -- the kernel's 1/world scale undone
        return run.bufs.eval_out * float(self.objective._model.engine.world_size)


class _PPOScalar(Node):
    def __init__(self, loss_node, index, name):
        self.loss_node, self.index, self.name = loss_node, index, name

    def _eval(self, ctx):
        return self.loss_node.scalars(ctx)[self.index]

    def _finalize(self, ctx, value):
        return self.loss_node.scalars(ctx)[self.index]


class PPOObjective(ActorCriticObjective):
    """PPO's clipped-surrogate objective (Schulman et al. 2017), beyond the reference:

        r = pi(a|s) / pi_old(a|s),  L_pi = -(mean(min(r adv, clip(r, 1-e, 1+e) adv)) + beta mean(H)),
        L_v = mean((target - V)^2 / 2)   (``value_clip_range``: the clipped form of acmi_ppo_loss)

    with the targets and advantages of :class:`A2CObjective` (n-step or GAE(lambda),
    optionally batch-normalised) formed once per batch from the policy that collected
    it.  ``optimize_shared`` returns an op that takes ``num_epochs`` x
    ``num_minibatches`` gradient steps per ``session.run``.

    ``normalize_advantages``: True (over the batch, once), False, or 'minibatch'
    (baselines' / CleanRL's default: every gradient step normalises the advantages of
    its own rows, all ranks' together; with ``optimize_shared(minibatch='rows')`` only).
    """

    def __init__(self, model, discount_factor=0.99, entropy_regularization_strength=0.01, clip_range=0.1,
                 value_clip_range=None, gae_lambda=0.95, normalize_advantages=True, advantage_epsilon=1e-8,
                 name=None, normalize_returns=None, diagnostics=None):
        if not float(clip_range) > 0.0:
            raise ValueError('clip_range must be positive, got {}'.format(clip_range))
        if value_clip_range is not None and not float(value_clip_range) > 0.0:
            raise ValueError('value_clip_range must be positive or None, got {}'.format(value_clip_range))
        if gae_lambda is not None and not 0.0 <= float(gae_lambda) <= 1.0:
            raise ValueError('gae_lambda must be in [0, 1] or None, got {}'.format(gae_lambda))
        if isinstance(normalize_advantages, str) and normalize_advantages != 'minibatch':
            raise ValueError("normalize_advantages must be True, False or 'minibatch', got {!r}"
                             .format(normalize_advantages))
        self._model = model
        self._gamma = float(discount_factor)
        self._gae_lambda = None if gae_lambda is None else float(gae_lambda)
        # 'minibatch': every gradient step normalises its own rows (PPOOptimizeOp), the batch is left alone
        self._normalize_minibatch = normalize_advantages == 'minibatch'
        self._normalize = not self._normalize_minibatch and bool(normalize_advantages)
        self._retnorm = _check_normalizer(normalize_returns)
        self.diagnostics = _check_diagnostics(diagnostics)  # (A2CObjective's; the whole op's step and KL)
        self._adv_eps = float(advantage_epsilon)
        self._beta = float(entropy_regularization_strength)
        self._clip = float(clip_range)
        self._vclip = 0.0 if value_clip_range is None else float(value_clip_range)
        self._vcoef = 0.5
        self._name = name or 'PPOObjective'
        self._table_cache = {}
        self._buffers = {}
        self._row_buffers = {}
        self._targets_node = _Targets(self)
        self._batch_node = _PPOBatch(self)
        self._loss_node = _PPOLoss(self)
        self._scalars = {n: _PPOScalar(self._loss_node, i, n) for i, n in enumerate(
            ('policy_loss', 'baseline_loss', 'mean_entropy', 'approx_kl', 'clip_fraction'))}

    _tables = A2CObjective._tables

    def _launch_loss(self, fwd, vectors, row0, rows, bufs, dhead, loss_out, clip_frac_out):
        """acmi_ppo_loss of ``fwd``, a forward of the rows row0 .. row0+rows-1 of the batch
        whose (actions, old_logp, old_values, targets, adv) ``vectors`` are: the run's
        own (:meth:`_PPORun.vectors`) or their shuffled copy (:class:`_PPORowBuffers`);
        a sixth vector holds the rows' legal-action words: the loss over each row's legal set."""
        eng = self._model.engine
        sl = slice(row0, row0 + rows)
        actions, old_logp, old_values, targets, adv = (v[sl] for v in vectors[:5])
        legal = vectors[5][sl] if len(vectors) > 5 else None
        _ops.ppo_loss(fwd.flat_logits, eng.A, fwd.flat_value, actions, old_logp, old_values, targets, adv, rows,
                      eng.A, self._clip, self._vclip, self._beta, float(self._vcoef), 1.0 / eng.world_size, dhead,
                      eng.ldh, bufs.loss_ws(eng, rows), loss_out, clip_frac_out, eng.stream(), legal=legal,
                      bad_rows=eng._mask_bad_rows)

    def optimize_shared(self, optimizer, baseline_loss_weight=0.5, num_epochs=4, num_minibatches=4, shuffle_seed=0,
                        step_callback=None, global_step=None, minibatch='envs', **kwargs):
        """The PPO update op: per ``session.run``, ``num_epochs`` passes over the batch
        in ``num_minibatches`` gradient steps each (see :class:`PPOOptimizeOp`).

        ``minibatch='envs'`` (the default): minibatches are contiguous ENV slices of the
        env-major [N][T] batch (so ``num_minibatches`` must divide N: ValueError at run
        time otherwise); the order of the slices is permuted per epoch, the rows are not
        shuffled.  ``minibatch='rows'``: every epoch shuffles all N*T rows (a device
        gather into a second copy of the batch) and cuts the shuffled batch into
        ``num_minibatches`` equal parts (``num_minibatches`` must divide N*T)."""
        from actorcritic.kfac_utils import KfacOptimizer
        if isinstance(optimizer, KfacOptimizer):
            raise NotImplementedError('PPOObjective takes first-order optimizers only: K-FAC statistics of the '
                                      'clipped surrogate are not implemented')
        if kwargs:
            raise TypeError('unexpected arguments {}'.format(sorted(kwargs)))
        if int(num_epochs) < 1 or int(num_minibatches) < 1:
            raise ValueError('num_epochs and num_minibatches must be at least 1')
        if minibatch not in ('envs', 'rows'):
            raise ValueError("minibatch must be 'envs' or 'rows', got {!r}".format(minibatch))
        if self._normalize_minibatch and minibatch != 'rows':
            raise ValueError("normalize_advantages='minibatch' needs minibatch='rows': an env slice is the batch's "
                             "own memory, which a per-step normalisation would overwrite")
        self._vcoef = float(baseline_loss_weight)
        return PPOOptimizeOp(self, optimizer, int(num_epochs), int(num_minibatches), int(shuffle_seed),
                             step_callback, global_step, minibatch)

    @property
    def model(self):
        return self._model

    @property
    def target_values(self):
        return _TargetView(self._targets_node, 'targets')

    @property
    def advantage(self):
        return _TargetView(self._targets_node, 'adv')

    normalized_rewards = A2CObjective.normalized_rewards
    return_stats = A2CObjective.return_stats
    return_normalizer = A2CObjective.return_normalizer

    @property
    def policy_loss(self):
        return self._scalars['policy_loss']

    @property
    def baseline_loss(self):
        return self._scalars['baseline_loss']

    @property
    def mean_entropy(self):
        return self._scalars['mean_entropy']

    @property
    def approx_kl(self):
        """mean(log pi_old(a) - log pi(a)) over the rows of the (last) gradient step."""
        return self._scalars['approx_kl']

    @property
    def clip_fraction(self):
        """Share of rows whose ratio left [1 - clip_range, 1 + clip_range]."""
        return self._scalars['clip_fraction']


class PPOOptimizeOp(Node):
    """One PPO update per ``session.run``:

    1. the batch's forward (the rollout's cached activations, else a fresh one), from
       it the old log-probabilities / values and -- once -- targets and advantages;
    2. for every epoch and every env slice, in the epoch's permuted order: the tower
       on the slice's rows with the current parameters, acmi_ppo_loss, backward,
       all-reduce, the optimizer's kernel, ``step_callback(epoch, position)``;
    3. ``global_step`` + 1 (once per run, not per gradient step).

    Env-wise minibatching (``minibatch='envs'``, the default): a slice is the
    N / num_minibatches consecutive envs' rows, read in place through pointer offsets;
    rows are not shuffled individually.  ``last_order`` holds the slice order
    of the last run, ``[epoch][position] -> slice``.  The very first step of a run
    with one minibatch re-uses the batch's forward.

    ``minibatch='rows'``: per epoch one acmi_gather_rows launch writes the batch's rows
    (observations, actions, old log-probabilities / values, targets, advantages), in
    the epoch's permutation (:func:`ppo_row_order`), into a second copy of the batch
    (:class:`_PPORowBuffers`; M x 28224 bytes of observations); gradient step k of the
    epoch then runs exactly as above on rows [k M/nmb, (k+1) M/nmb) of that copy, which
    are contiguous again.  With ``normalize_advantages='minibatch'`` each step first
    normalises its slice of the copied advantages in place (the next epoch gathers them
    afresh from the batch's).  ``last_rows`` holds the last run's permutations,
    ``[epoch] -> int32 ndarray`` (``last_order`` stays None); every step re-forwards.
    """
    name = 'ppo_optimize'

    def __init__(self, objective, optimizer, num_epochs, num_minibatches, shuffle_seed, step_callback, global_step,
                 minibatch='envs'):
        if minibatch not in ('envs', 'rows'):
            raise ValueError("minibatch must be 'envs' or 'rows', got {!r}".format(minibatch))
        self.objective, self.optimizer = objective, optimizer
        self.num_epochs, self.num_minibatches, self.shuffle_seed = num_epochs, num_minibatches, shuffle_seed
        self.step_callback = step_callback
        self.global_step = global_step
        self.minibatch = minibatch
        self.last_order = None
        self.last_rows = None
        self._runs = 0

    def _eval(self, ctx):
        obj = self.objective
        eng = obj._model.engine
        run = ctx.eval(obj._batch_node)
        step = self.global_step.value if self.global_step is not None else self._runs
        # update diagnostics (actorcritic.update_diag): of the whole op -- the step and the KL over all
        # epochs, the value statistics of the batch's forward; the gradient is the last minibatch's
        diag = obj.diagnostics if obj.diagnostics is not None and obj.diagnostics.armed else None
        if diag is not None:
            diag.before_update(eng, run.fwd, run.st)
        if self.minibatch == 'rows':
            st = self._epochs_of_rows(ctx, run, step)
        else:
            st = self._epochs_of_env_slices(ctx, run, step)
        if diag is not None:
            from actorcritic.nn import _innermost
            diag.after_update(eng, run.fwd, st.grads, _innermost(self.optimizer))
        if eng.collective:  # (the other four scalars travel with the gradients)
            from actorcritic import parallel
            parallel.allreduce_sum_(run.bufs.clip_frac, force=True)
        run.stepped, run.step_st = True, st
        self._runs += 1
        if self.global_step is not None:
            self.global_step.assign(self.global_step.value + 1)
        return None

    def _step(self, ctx, run, part, vectors, row0, rows, epoch, pos):
        """One gradient step on ``part``, a forward of rows row0 .. row0+rows-1 of ``vectors``' batch."""
        obj, eng = self.objective, self.objective._model.engine
        st = eng.update_state(rows)
        obj._launch_loss(part, vectors, row0, rows, run.bufs, st.dhead, st.loss, run.bufs.clip_frac)
        eng.backward(part, st, with_stats=False)
        eng.allreduce(st, with_stats=False)
        self.optimizer._apply_dense(ctx, eng, st.grads, 0.0)
        eng.bump_version()
        if self.step_callback is not None:
            self.step_callback(epoch, pos)
        return st

    def _epochs_of_env_slices(self, ctx, run, step):
        from actorcritic.envs.atari.model import ForwardOut
        eng = self.objective._model.engine
        fwd = run.fwd
        T = fwd.steps
        slices = ppo_minibatch_rows(fwd.batch, T, self.num_minibatches)
        order = ppo_minibatch_order(self.shuffle_seed, step, self.num_epochs, self.num_minibatches)
        st = None
        for epoch, perm in enumerate(order):
            for pos, j in enumerate(perm):
                row0, rows = slices[j]
                if st is None and self.num_minibatches == 1:
                    part = fwd  # nothing has changed the parameters since the batch's forward
                else:
                    acts = eng.activations(rows, 'ppo')
                    obs = fwd.obs[row0:row0 + rows]
                    eng.forward(obs.data_ptr(), rows, acts.struct, want_value=True)
                    part = ForwardOut(eng, acts, rows // T, T, obs)
                st = self._step(ctx, run, part, run.vectors(), row0, rows, epoch, pos)
        self.last_order = order
        return st

    def _epochs_of_rows(self, ctx, run, step):
        from actorcritic.envs.atari.model import ForwardOut
        obj = self.objective
        eng = obj._model.engine
        M, nmb = run.fwd.M, self.num_minibatches
        if M % nmb != 0:
            raise ValueError('num_minibatches ({}) must divide the number of rows ({})'.format(nmb, M))
        rows = M // nmb
        order = [np.ascontiguousarray(p, dtype=np.int32) for p in
                 ppo_row_order(self.shuffle_seed, step, self.num_epochs, M)]
        for p in order:  # (host-side: the kernel would zero-fill a bad row, not fail)
            if p.shape != (M,) or (M and (p.min() < 0 or p.max() >= M)):
                raise ValueError('ppo_row_order must return indices into range({}) for every epoch'.format(M))
        # one upload for the run's epochs: a copy from pageable memory waits for the stream
        index = torch.from_numpy(np.stack(order)).to(eng.device)
        masked = run.masks is not None
        sh = obj._row_buffers.get((M, masked) if masked else M)
        if sh is None:
            sh = obj._row_buffers[(M, masked) if masked else M] = _PPORowBuffers(eng, M, masked)
        st = None
        for epoch in range(len(order)):
            sh.gather(eng, run, index[epoch])
            for k in range(nmb):
                row0 = k * rows
                if obj._normalize_minibatch:
                    _normalize_advantages(eng, sh.vecs[4][row0:row0 + rows], rows, obj._adv_eps)
                acts = eng.activations(rows, 'ppo')
                obs = sh.obs[row0:row0 + rows]
                eng.forward(obs.data_ptr(), rows, acts.struct, want_value=True)
                part = ForwardOut(eng, acts, rows, 1, obs)  # (a shuffled slice is not [env][step]-shaped)
                st = self._step(ctx, run, part, sh.vecs, row0, rows, epoch, k)
        self.last_rows = order
        return st


class _VTraceBuffers(object):
    def __init__(self, eng, M):
        z = lambda: torch.zeros(M, dtype=torch.float32, device=eng.device)
        self.behaviour_logp = z()  # the run's behaviour log-probabilities (the feed, or the batch's forward)
        self.rho = z()  # the batch's clipped weights at the batch's forward
        self.step_rho = z()  # a gradient step's, at the step's forward (row-aligned with the batch)


class _VTraceRun(object):
    """What one session.run shares between the V-trace nodes: the batch's per-row vectors (flat [N*T]) and
    its two forwards; ``step_st`` is the update state of the last gradient step of a VTraceOptimizeOp."""

    def __init__(self, fwd, boot, rewards, terminals, trunc, actions, masks, bufs):
        self.fwd, self.boot = fwd, boot
        self.rewards, self.terminals, self.trunc = rewards.reshape(-1), terminals.reshape(-1), trunc
        if trunc is not None:
            self.trunc = trunc.reshape(-1)
        self.actions, self.masks, self.bufs = actions, masks, bufs
        self.step_st = None


class _VTraceTargets(_Targets):
    """acmi_vtrace in place of acmi_returns / acmi_gae: targets, advantages and the clipped weights of the
    batch at its forward, against the run's behaviour log-probabilities."""

    def _launch(self, ctx, st, fwd, boot, rewards, terminals, trunc):
        obj = self.objective
        model = obj._model
        eng = model.engine
        M = fwd.M
        actions = _device(ctx.eval(model.actions_placeholder), torch.int32, eng.device).reshape(-1)
        if actions.numel() != M:
            raise ValueError('actions must have the shape of the observations batch [env, step]')
        bufs = obj._buffers.get(M)
        if bufs is None:
            bufs = obj._buffers[M] = _VTraceBuffers(eng, M)
        masks = fwd.row_masks()
        fed = ctx.feeds.get(model.behaviour_log_probs_placeholder)
        if fed is not None:
            fed = _device(fed, torch.float32, eng.device).reshape(-1)
            if fed.numel() != M:
                raise ValueError('behaviour log-probabilities must have the shape of the observations batch '
                                 '[env, step]')
            bufs.behaviour_logp.copy_(fed)
        else:  # the batch's own forward acted (the rollout's cached activations), or stands in for what did
            _ops.categorical(fwd.flat_logits, eng.A, M, eng.A, actions, None, bufs.behaviour_logp, eng.stream(),
                             legal=masks)
        run = st.vtrace = _VTraceRun(fwd, boot, rewards, terminals, trunc, actions, masks, bufs)
        obj._launch_vtrace(run, fwd, boot, 0, fwd.batch, st, bufs.rho)
        st.rho = bufs.rho


class _VTraceLoss(_Loss):
    """_Loss; once a VTraceOptimizeOp has stepped in the run, the scalars of its last gradient step."""

    def _stepped(self, ctx):
        return ctx.eval(self.objective._targets_node).vtrace.step_st

    def _eval(self, ctx):
        st = self._stepped(ctx)
        return st.loss if st is not None else super()._eval(ctx)

    def scalars(self, ctx):
        st = self._stepped(ctx)
        if st is not None:  # (all-reduced with the gradients: global means)
            return st.loss[:3]
        return super().scalars(ctx)


class VTraceObjective(A2CObjective):
    """A2C's losses on V-trace targets (Espeholt et al. 2018, IMPALA), beyond the reference: the actor-critic
    objective for data that the policy being updated did not collect -- several passes over one batch, actors
    whose parameters lag the learner, batches handed in from outside.  actorcritic/vtrace.py states the
    recurrence; the clipped weight rho sits inside the advantage, so the loss, its gradient and every
    optimizer are :class:`A2CObjective`'s (acmi_a2c_loss), K-FAC included for a single pass.

    The behaviour policy's log-probabilities of the taken actions are fed through
    ``model.behaviour_log_probs_placeholder`` [env, step]; unfed, the batch's own forward is the behaviour
    policy (all weights 1 in a single pass: GAE(``gae_lambda``) targets, n-step returns at 1).
    ``rho_bar >= c_bar > 0`` clip the weights of the temporal-difference terms and of the trace.
    ``importance_weights`` is fetchable.  ``optimize_shared(num_epochs=, num_minibatches=)`` re-forms the
    targets at every gradient step (:class:`VTraceOptimizeOp`)."""

    def __init__(self, model, discount_factor=0.99, entropy_regularization_strength=0.01, gae_lambda=1.0,
                 rho_bar=1.0, c_bar=1.0, normalize_advantages=False, normalize_returns=None, diagnostics=None,
                 advantage_epsilon=1e-8, name=None):
        if gae_lambda is None or not 0.0 <= float(gae_lambda) <= 1.0:
            raise ValueError('gae_lambda must be in [0, 1], got {}'.format(gae_lambda))
        if not float(rho_bar) > 0.0 or not float(c_bar) > 0.0:
            raise ValueError('rho_bar and c_bar must be positive, got {} and {}'.format(rho_bar, c_bar))
        if float(rho_bar) < float(c_bar):
            raise ValueError('rho_bar ({}) must not be below c_bar ({})'.format(rho_bar, c_bar))
        super().__init__(model, discount_factor, entropy_regularization_strength, name or 'VTraceObjective',
                         gae_lambda=gae_lambda, normalize_advantages=normalize_advantages,
                         advantage_epsilon=advantage_epsilon, normalize_returns=normalize_returns,
                         diagnostics=diagnostics)
        self._rho_bar, self._c_bar = float(rho_bar), float(c_bar)
        self._buffers = {}
        self._targets_node = _VTraceTargets(self)
        self._loss_node = _VTraceLoss(self)
        self._policy_loss = _LossScalar(self._loss_node, 0, 'policy_loss')
        self._baseline_loss = _LossScalar(self._loss_node, 1, 'baseline_loss')
        self._mean_entropy = _LossScalar(self._loss_node, 2, 'mean_entropy')

    @property
    def importance_weights(self):
        """The clipped weights rho [env, step] of the batch at its forward (all ones unfed)."""
        return _TargetView(self._targets_node, 'rho')

    def _launch_vtrace(self, run, part, boot, env0, envs, st, rho):
        """acmi_vtrace of the envs env0 .. env0+envs-1 of the run's batch: ``part`` and ``boot`` are forwards
        of exactly those envs' rows and bootstrap observations; -> st.targets, st.adv and the rows' ``rho``."""
        eng = self._model.engine
        T = run.fwd.steps
        sl = slice(env0 * T, (env0 + envs) * T)
        _ops.vtrace(part.flat_logits, eng.A, eng.A, run.actions[sl], run.bufs.behaviour_logp[sl], run.rewards[sl],
                    run.terminals[sl], part.flat_value, boot.flat_value, envs, T, self._gamma, self._gae_lambda,
                    self._rho_bar, self._c_bar, st.targets, st.adv, rho[sl], eng.stream(),
                    truncated=None if run.trunc is None else run.trunc[sl],
                    legal=None if run.masks is None else run.masks[sl], bad_rows=eng._mask_bad_rows)

    def optimize_shared(self, optimizer, baseline_loss_weight=0.5, num_epochs=1, num_minibatches=1, shuffle_seed=0,
                        step_callback=None, global_step=None, **kwargs):
        """``num_epochs = num_minibatches = 1`` (and no ``step_callback``, which the inherited op would not
        call): :class:`A2CObjective`'s op (any optimizer).  Otherwise a
        :class:`VTraceOptimizeOp`: per ``session.run``, ``num_epochs`` passes over the batch in
        ``num_minibatches`` gradient steps each, over env slices (V-trace needs whole trajectories;
        ``num_minibatches`` must divide the number of envs), first-order optimizers only."""
        if int(num_epochs) < 1 or int(num_minibatches) < 1:
            raise ValueError('num_epochs and num_minibatches must be at least 1')
        if int(num_epochs) == 1 and int(num_minibatches) == 1 and step_callback is None:
            if global_step is not None:
                kwargs['global_step'] = global_step
            return super().optimize_shared(optimizer, baseline_loss_weight, **kwargs)
        from actorcritic.kfac_utils import KfacOptimizer
        if isinstance(optimizer, KfacOptimizer):
            raise NotImplementedError('VTraceObjective takes first-order optimizers only for several gradient '
                                      'steps per batch: K-FAC runs the single pass (num_epochs = '
                                      'num_minibatches = 1)')
        if kwargs:
            raise TypeError('unexpected arguments {}'.format(sorted(kwargs)))
        self._vcoef = float(baseline_loss_weight)
        return VTraceOptimizeOp(self, optimizer, int(num_epochs), int(num_minibatches), int(shuffle_seed),
                                step_callback, global_step)


class VTraceOptimizeOp(Node):
    """Several V-trace gradient steps per ``session.run`` (multi-epoch A2C, an IMPALA-style learner):

    1. the batch's forward (the rollout's cached activations, else a fresh one) and, once, the run's
       behaviour log-probabilities (the feed, or that forward's), the scaled rewards (``normalize_returns``)
       and the batch's targets (what ``target_values`` / ``importance_weights`` fetch, and the diagnostics);
    2. for every epoch and every env slice, in the epoch's permuted order (:func:`ppo_minibatch_order`): the
       tower on the slice's rows and on its bootstrap observations with the current parameters, acmi_vtrace
       against the behaviour log-probabilities, the advantages normalised over the slice if asked,
       acmi_a2c_loss, backward, all-reduce, the optimizer's kernel, ``step_callback(epoch, position)``;
    3. ``global_step`` + 1 (once per run).

    A slice is N / num_minibatches consecutive envs -- whole trajectories -- read in place.  ``last_order``
    holds the slice order of the last run, ``[epoch][position] -> slice``.  The very first step of a run with
    one minibatch re-uses the batch's two forwards.  With one minibatch a step's update state is the batch's:
    ``target_values`` and ``advantage`` then hold the last step's."""
    name = 'vtrace_optimize'

    def __init__(self, objective, optimizer, num_epochs, num_minibatches, shuffle_seed, step_callback, global_step):
        self.objective, self.optimizer = objective, optimizer
        self.num_epochs, self.num_minibatches, self.shuffle_seed = num_epochs, num_minibatches, shuffle_seed
        self.step_callback = step_callback
        self.global_step = global_step
        self.last_order = None
        self._runs = 0

    def _eval(self, ctx):
        from actorcritic.envs.atari.model import ForwardOut
        obj = self.objective
        eng = obj._model.engine
        batch_st = ctx.eval(obj._targets_node)
        run = batch_st.vtrace
        fwd, boot = run.fwd, run.boot
        N, T, nmb = fwd.batch, fwd.steps, self.num_minibatches
        step = self.global_step.value if self.global_step is not None else self._runs
        slices = ppo_minibatch_rows(N, T, nmb)
        order = ppo_minibatch_order(self.shuffle_seed, step, self.num_epochs, nmb)
        diag = obj.diagnostics if obj.diagnostics is not None and obj.diagnostics.armed else None
        if diag is not None:  # (as PPOOptimizeOp: of the whole op; the gradient is the last step's)
            diag.before_update(eng, fwd, batch_st)
        envs = N // nmb
        st = None
        for epoch, perm in enumerate(order):
            for pos, j in enumerate(perm):
                row0, rows = slices[j]
                if st is None and nmb == 1:
                    part, pboot = fwd, boot  # nothing has changed the parameters since the batch's forwards
                else:
                    acts = eng.activations(rows, 'vtrace')
                    obs = fwd.obs[row0:row0 + rows]
                    eng.forward(obs.data_ptr(), rows, acts.struct, want_value=True)
                    part = ForwardOut(eng, acts, envs, T, obs)
                    bacts = eng.activations(envs, 'vtrace_boot')
                    bobs = boot.obs[j * envs:(j + 1) * envs]
                    eng.forward(bobs.data_ptr(), envs, bacts.struct, want_value=True)
                    pboot = ForwardOut(eng, bacts, envs, 1, bobs)
                st = self._step(ctx, run, part, pboot, j * envs, envs, epoch, pos)
        if diag is not None:
            from actorcritic.nn import _innermost
            diag.after_update(eng, fwd, st.grads, _innermost(self.optimizer))
        run.step_st = st
        self.last_order = order
        self._runs += 1
        if self.global_step is not None:
            self.global_step.assign(self.global_step.value + 1)
        return None

    def _step(self, ctx, run, part, pboot, env0, envs, epoch, pos):
        """One gradient step on the envs env0 .. env0+envs-1, forwarded as ``part`` / ``pboot``."""
        obj, eng = self.objective, self.objective._model.engine
        rows = part.M
        st = eng.update_state(rows)
        obj._launch_vtrace(run, part, pboot, env0, envs, st, run.bufs.step_rho)
        if obj._normalize:
            _normalize_advantages(eng, st.adv, rows, obj._adv_eps)
        sl = slice(env0 * part.steps, env0 * part.steps + rows)
        _ops.a2c_loss(part.flat_logits, eng.A, part.flat_value, run.actions[sl], st.targets, st.adv, rows, eng.A,
                      float(obj._beta), float(obj._vcoef), 1.0 / eng.world_size, st.dhead, eng.ldh, st.loss_ws,
                      st.loss, eng.stream(), legal=None if run.masks is None else run.masks[sl],
                      bad_rows=eng._mask_bad_rows)
        eng.backward(part, st, with_stats=False)
        eng.allreduce(st, with_stats=False)
        self.optimizer._apply_dense(ctx, eng, st.grads, 0.0)
        eng.bump_version()
        if self.step_callback is not None:
            self.step_callback(epoch, pos)
        return st


class _TargetView(Node):
    def __init__(self, node, attr):
        self.node, self.attr, self.name = node, attr, attr

    def _eval(self, ctx):
        st = ctx.eval(self.node)
        fwd = st.fwd if hasattr(st, 'fwd') else None
        v = getattr(st, self.attr)
        if fwd is not None:
            return v.reshape(fwd.batch, fwd.steps)
        return v


def _device(x, dtype, device):
    if isinstance(x, torch.Tensor):
        t = x
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return t.to(device=device, dtype=dtype).contiguous()


def _device_bool_u8(x, device):
    if isinstance(x, torch.Tensor):
        t = x
        if t.dtype == torch.bool:
            t = t.view(torch.uint8) if t.is_contiguous() else t.to(torch.uint8)
        elif t.dtype != torch.uint8:
            t = (t != 0).to(torch.uint8)
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=bool)).view(np.uint8))
    return t.to(device).contiguous()
