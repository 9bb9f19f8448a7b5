"""Update diagnostics on the device: explained variance, the step's KL, gradient and step norms.

Beyond the reference, whose scalar log holds the two losses and the entropy: what ONE update did,
per GROUP of envs (per game) where that makes sense, as double accumulators that a log line reads
with one host copy.  Opt-in (``A2CObjective(..., diagnostics=)``, ``PPOObjective(..., diagnostics=)``);
an object that is not armed launches nothing, and an armed update leaves the run the run it would
have been, bit for bit.

The maths (include/acmi.h states it for the kernels; the ``host_*`` functions restate it in numpy
float64 and are the rule book of the tests).  Rows are env-major ``[N][T]``: row m belongs to env
``m // T``; an env whose group id is >= G joins no group and counts in ``bad_envs``.

* value, ``acc[g] = (n, sum v, sum y, sum y^2, sum e, sum e^2)`` with v the value the loss read, y its
  target and ``e = f64(y) - f64(v)``; explained variance ``1 - Var(e)/Var(y)`` (:func:`explained_variance`);
* policy, ``acc[g] = (n, sum KL(old||new), sum H(new), max KL)`` over the good rows: old = the logits the
  loss read, new = a forward of the same observations after the update.  Per row in double over the
  legal set S: ``lse = mx + log(sum_S exp(z - mx))``, ``logp = z - lse``, ``p = exp(logp)``,
  ``KL = sum_S p_old (logp_old - logp_new)``, ``H = -sum_S p_new logp_new``.  Double because an ACKTR
  step's KL is around 1e-4, where float32 log-probabilities cancel to three digits.  A row with an
  empty S or a non-finite logit among its A, in either matrix, is bad: it adds nothing and counts in
  ``bad_rows``;
* segments, ``out[s] = (sum x^2, sum y^2, sum x y, sum (x-y)^2)`` over the elements
  ``[offsets[s], offsets[s+1])``: the 12 parameter blocks (acmi_param_offsets) of (gradient,
  K-FAC preconditioned gradient) and of (parameters after, parameters before).
"""

import ctypes

import numpy as np
import torch

from actorcritic import _lib
from actorcritic.return_norm import check_groups, groups_for_envs

VALUE_COLS = 6   # n, sum v, sum y, sum y^2, sum e, sum e^2
POLICY_COLS = 4  # n, sum KL, sum H | max KL
SEG_COLS = 4     # sum x^2, sum y^2, sum x y, sum (x-y)^2
LAYERS = ('conv1', 'conv2', 'conv3', 'fc4', 'fc_policy', 'fc_baseline')  # LayerCollection.EXPECTED
U = 2.0 ** -53

VALUE_KEYS = ('explained_variance', 'value_mean', 'target_mean', 'target_std')
POLICY_KEYS = ('policy_kl', 'policy_kl_max', 'policy_entropy_after')


# -- the numpy reference ------------------------------------------------------------------
def _groups(groups, N):
    return np.zeros(N, np.int64) if groups is None else np.asarray(groups).astype(np.int64).reshape(N)


def host_value_diag(values, targets, groups, num_groups):
    """-> (acc f64 [G][6], bad_envs) of values / targets f32 [N][T]."""
    v = np.ascontiguousarray(values, np.float32)
    y = np.ascontiguousarray(targets, np.float32)
    if v.ndim != 2 or v.shape != y.shape:
        raise ValueError('values and targets must be [N][T], got {} and {}'.format(v.shape, y.shape))
    N, T = v.shape
    G = int(num_groups)
    grp = _groups(groups, N)
    v64, y64 = v.astype(np.float64), y.astype(np.float64)
    e = y64 - v64
    acc = np.zeros((G, VALUE_COLS), np.float64)
    for g in range(G):
        sel = grp == g
        acc[g] = (sel.sum() * T, v64[sel].sum(), y64[sel].sum(), (y64[sel] * y64[sel]).sum(), e[sel].sum(),
                  (e[sel] * e[sel]).sum())
    return acc, int((grp >= G).sum())


def legal_columns(word, A):
    """The legal set of one row: the actions a < A whose bit is set (``word`` None: all)."""
    if word is None:
        return np.arange(A)
    return np.array([a for a in range(A) if (int(word) >> a) & 1], np.int64)


def host_policy_rows(logits_old, logits_new, legal=None, num_actions=None):
    """-> (good bool [M], KL f64 [M], H f64 [M]) of float32 logits [M][ld]; the first
    ``num_actions`` columns count (default: all), a bad row holds zeros."""
    zo, zn = np.asarray(logits_old, np.float32), np.asarray(logits_new, np.float32)
    M = zo.shape[0]
    A = zo.shape[1] if num_actions is None else int(num_actions)
    words = None if legal is None else np.asarray(legal).astype(np.int64) & 0xFFFFFFFF
    good, kl, h = np.zeros(M, bool), np.zeros(M, np.float64), np.zeros(M, np.float64)
    for m in range(M):
        S = legal_columns(None if words is None else words[m], A)
        if S.size == 0 or not (np.isfinite(zo[m, :A]).all() and np.isfinite(zn[m, :A]).all()):
            continue
        lp = []
        for z in (zo[m, S].astype(np.float64), zn[m, S].astype(np.float64)):
            mx = z.max()
            lp.append(z - (mx + np.log(np.exp(z - mx).sum())))
        good[m] = True
        kl[m] = (np.exp(lp[0]) * (lp[0] - lp[1])).sum()
        h[m] = -(np.exp(lp[1]) * lp[1]).sum()
    return good, kl, h


def host_policy_diag(logits_old, logits_new, legal, groups, num_groups, num_steps, num_actions=None):
    """-> (acc f64 [G][4], bad_envs, bad_rows) of float32 logits [N*T][ld] (T = ``num_steps``)."""
    good, kl, h = host_policy_rows(logits_old, logits_new, legal, num_actions)
    M, T, G = good.shape[0], int(num_steps), int(num_groups)
    if T < 1 or M % T:
        raise ValueError('{} rows are not [N][{}]'.format(M, T))
    grp = np.repeat(_groups(groups, M // T), T)
    acc = np.zeros((G, POLICY_COLS), np.float64)
    acc[:, 3] = -np.inf
    for g in range(G):
        sel = good & (grp == g)
        acc[g, :3] = (sel.sum(), kl[sel].sum(), h[sel].sum())
        if sel.any():
            acc[g, 3] = kl[sel].max()
    return acc, int((grp[::T] >= G).sum()), int((~good).sum())


def check_offsets(offsets, size=None):
    """ValueError unless ``offsets`` is a non-decreasing int sequence from >= 0 (to <= ``size``)."""
    off = np.asarray(offsets, np.int64).reshape(-1)
    if off.size < 2 or off[0] < 0 or (np.diff(off) < 0).any() or (size is not None and off[-1] > size):
        raise ValueError('segment offsets must be non-decreasing within the buffer, got {}'.format(off.tolist()))
    return off


def host_segment_sums(x, y, offsets):
    """-> f64 [S][4] of float32 vectors x, y (``y`` None: zeros)."""
    x64 = np.asarray(x, np.float32).reshape(-1).astype(np.float64)
    y64 = np.zeros_like(x64) if y is None else np.asarray(y, np.float32).reshape(-1).astype(np.float64)
    off = check_offsets(offsets, x64.size)
    out = np.zeros((off.size - 1, SEG_COLS), np.float64)
    for s in range(off.size - 1):
        a, b = x64[off[s]:off[s + 1]], y64[off[s]:off[s + 1]]
        d = a - b
        out[s] = ((a * a).sum(), (b * b).sum(), (a * b).sum(), (d * d).sum())
    return out


# -- derivations from an accumulator row ----------------------------------------------------
def _var(n, s, q):
    return q / n - (s / n) * (s / n)


def target_variance(row):
    """Var(y) of a value row; 0.0 when it lies within the rounding error of its own sums
    (``n Var(y) <= 4 n 2^-53 sum y^2``: a constant target must not read as a tiny variance)."""
    n, _, sy, qy = (float(x) for x in row[:4])
    if n == 0:
        return float('nan')
    var = _var(n, sy, qy)
    return 0.0 if var <= 4.0 * U * qy else var


def explained_variance(row):
    """1 - Var(e)/Var(y) of a value row (n, sum v, sum y, sum y^2, sum e, sum e^2); NaN where n or
    Var(y) is 0."""
    n, se, qe = float(row[0]), float(row[4]), float(row[5])
    var_y = target_variance(row)
    if n == 0 or not var_y > 0.0:
        return float('nan')
    return 1.0 - max(_var(n, se, qe), 0.0) / var_y


def value_scalars(row, suffix=''):
    n = float(row[0])
    nan = float('nan')
    var_y = target_variance(row)
    return {'explained_variance' + suffix: explained_variance(row),
            'value_mean' + suffix: float(row[1]) / n if n else nan,
            'target_mean' + suffix: float(row[2]) / n if n else nan,
            'target_std' + suffix: float(np.sqrt(var_y)) if n else nan}


def policy_scalars(row, suffix=''):
    n = float(row[0])
    nan = float('nan')
    return {'policy_kl' + suffix: float(row[1]) / n if n else nan,
            'policy_kl_max' + suffix: float(row[3]) if n else nan,
            'policy_entropy_after' + suffix: float(row[2]) / n if n else nan}


def reduce_policy_groups(acc):
    """The ``all`` row of a policy ``acc``: the sums summed, the maximum maximised."""
    acc = np.asarray(acc, np.float64)
    return np.concatenate([acc[:, :3].sum(axis=0), acc[:, 3:].max(axis=0)])


def layer_sums(seg):
    """[12][4] segment sums (weight, bias per layer) -> [6][4]: a layer's weight and bias summed."""
    seg = np.asarray(seg, np.float64).reshape(len(LAYERS), 2, SEG_COLS)
    return seg.sum(axis=1)


def cosine(row):
    """sum xy / sqrt(sum x^2 sum y^2) of a segment row; NaN where a norm is 0."""
    den = float(row[0]) * float(row[1])
    return float(row[2]) / float(np.sqrt(den)) if den > 0.0 else float('nan')


class UpdateDiagnostics(object):
    """The accumulators of one update and their launches.

    Args:
        groups: one group id per env of this rank (ints 0..num_groups-1).
        num_groups: G, 1..64; default max(groups) + 1.  Every rank must use the same G.
        group_names: names for the per-group log keys, or None.
        forward_rows: the post-update forward runs in chunks of at most this many rows.

    ``request()`` arms the object for the NEXT optimize op only; that op fills the accumulators
    (``record_*``; the engine hooks ``before_update`` / ``after_update``) and ``read()`` returns the
    scalar-log dict and empties them.  ``record_*`` take device tensors (the kernels) or numpy
    arrays / CPU tensors (the ``host_*`` functions): the class is testable without a GPU.
    """

    def __init__(self, groups, num_groups=None, group_names=None, forward_rows=1024):
        ids, G, self.group_names = check_groups(groups, num_groups, group_names)
        if int(forward_rows) < 1:
            raise ValueError('forward_rows must be at least 1, got {}'.format(forward_rows))
        self.num_envs, self.num_groups = len(ids), G
        self.forward_rows = int(forward_rows)
        self.groups = torch.tensor(ids, dtype=torch.uint8)
        self.armed = False
        self.updates = 0  # armed updates recorded so far
        self._res = {}    # 'value' [G][6], 'policy' [G][4], 'grad' [12][4], 'step' [12][4], 'coeff' [1]: f64
        self._dev = None  # the device buffers, made at the first armed update on a device
        self.last_acc = None  # read()'s host copy: {'value' [G][6], 'policy' [G][4], 'grad' / 'step' [12][4]}

    @classmethod
    def for_envs(cls, batched_env, forward_rows=1024):
        ids, G, names = groups_for_envs(batched_env)
        return cls(ids, num_groups=G, group_names=names, forward_rows=forward_rows)

    def request(self):
        """Arms the object: the next optimize op records its diagnostics (and disarms it)."""
        self.armed = True
        self._res = {}

    # -- recording ----------------------------------------------------------------------------
    def _buffers(self, device):
        if self._dev is None or self._dev['device'] != device:
            z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=device)
            self._dev = {'device': device, 'groups': self.groups.to(device), 'ws': None,
                         'value': z(self.num_groups, VALUE_COLS), 'policy': z(self.num_groups, POLICY_COLS),
                         'grad': None, 'step': None,
                         'bad': torch.zeros(2, dtype=torch.int32, device=device)}  # bad envs, bad rows
        return self._dev

    def _ws(self, dev, M, S):
        need = int(_lib.load().acmi_diag_ws_doubles(M, S))
        if dev['ws'] is None or dev['ws'].numel() < need:
            dev['ws'] = torch.zeros(need, dtype=torch.float64, device=dev['device'])
        return dev['ws']

    def _rows(self, M):
        if M % self.num_envs:
            raise ValueError('{} rows for diagnostics of {} envs'.format(M, self.num_envs))
        return self.num_envs, M // self.num_envs

    @staticmethod
    def _on_device(t):
        return torch.is_tensor(t) and t.is_cuda

    @staticmethod
    def _np(t):
        return t.detach().numpy() if torch.is_tensor(t) else np.asarray(t)

    def record_value(self, values, targets, stream=None):
        """The value accumulators of ``values`` / ``targets`` (float32, N*T elements, env-major)."""
        N, T = self._rows(int(values.numel() if torch.is_tensor(values) else np.size(values)))
        if self._on_device(values):
            dev = self._buffers(values.device)
            _lib.call('acmi_diag_value', _lib.ptr(values), _lib.ptr(targets), _lib.ptr(dev['groups']), N, T,
                      self.num_groups, _lib.ptr(self._ws(dev, N * T, 0)), _lib.ptr(dev['value']),
                      _lib.ptr(dev['bad'][:1]), stream if stream is not None else _lib.stream_handle(values.device))
            self._res['value'] = dev['value']
            return
        acc, _ = host_value_diag(self._np(values).reshape(N, T), self._np(targets).reshape(N, T),
                                 self.groups.numpy(), self.num_groups)
        self._res['value'] = torch.from_numpy(acc)

    def record_policy(self, logits_old, logits_new, legal=None, num_actions=None, stream=None):
        """The policy accumulators of two float32 logit matrices [N*T][ld] (rows may be padded:
        ``num_actions`` columns count, default all); ``legal``: one word per row, or None."""
        N, T = self._rows(int(logits_old.shape[0]))
        A = int(logits_old.shape[1] if num_actions is None else num_actions)
        if self._on_device(logits_old):
            dev = self._buffers(logits_old.device)
            for z in (logits_old, logits_new):
                if z.dtype != torch.float32 or z.dim() != 2 or z.stride(1) != 1 or z.shape[0] != N * T:
                    raise ValueError('logits must be float32 [N*T][ld] with unit column stride')
            _lib.call('acmi_diag_policy', ctypes.c_void_p(logits_old.data_ptr()), int(logits_old.stride(0)),
                      ctypes.c_void_p(logits_new.data_ptr()), int(logits_new.stride(0)), _lib.ptr(legal),
                      _lib.ptr(dev['groups']), N, T, A, self.num_groups, _lib.ptr(self._ws(dev, N * T, 0)),
                      _lib.ptr(dev['policy']), _lib.ptr(dev['bad'][:1]), _lib.ptr(dev['bad'][1:]),
                      stream if stream is not None else _lib.stream_handle(logits_old.device))
            self._res['policy'] = dev['policy']
            return
        words = None if legal is None else self._np(legal).reshape(-1)  # (int32 bits or uint32: the low 32 bits)
        acc, _, _ = host_policy_diag(self._np(logits_old), self._np(logits_new), words, self.groups.numpy(),
                                     self.num_groups, T, A)
        self._res['policy'] = torch.from_numpy(acc)

    def record_segments(self, which, x, y, offsets, stream=None):
        """``which`` 'grad' (x = gradient, y = the K-FAC preconditioned gradient or None) or 'step'
        (x = parameters after, y = before) over the segments of ``offsets`` (S + 1 ints; on a device
        an int64 tensor the caller has checked with :func:`check_offsets`)."""
        if which not in ('grad', 'step'):
            raise ValueError("which must be 'grad' or 'step', got {!r}".format(which))
        if self._on_device(x):
            dev = self._buffers(x.device)
            S = int(offsets.numel()) - 1
            if dev[which] is None or dev[which].shape[0] != S:
                dev[which] = torch.zeros(S, SEG_COLS, dtype=torch.float64, device=x.device)
            _lib.call('acmi_diag_segments', _lib.ptr(x), _lib.ptr(y), _lib.ptr(offsets), S,
                      _lib.ptr(self._ws(dev, 0, S)), _lib.ptr(dev[which]),
                      stream if stream is not None else _lib.stream_handle(x.device))
            self._res[which] = dev[which]
        else:
            self._res[which] = torch.from_numpy(host_segment_sums(
                self._np(x), None if y is None else self._np(y), self._np(offsets)))
        self._res[which + '_has_y'] = y is not None

    def record_coeff(self, coeff):
        """The K-FAC trust-region coefficient of the update (a 1-element tensor, left where it is)."""
        self._res['coeff'] = coeff

    def finish(self):
        """Ends an armed update: the object is disarmed, ``read()`` has something to return."""
        self.armed = False
        self.updates += 1
        self._res['done'] = True

    # -- the engine hooks (nn.OptimizeOp, objectives.PPOOptimizeOp) ----------------------------
    def before_update(self, eng, fwd, st):
        """Before the parameters change: the value accumulators from what the loss read, and a
        copy of the parameters."""
        if fwd.batch != self.num_envs:
            raise ValueError('diagnostics of {} envs for an update over {}'.format(self.num_envs, fwd.batch))
        dev = self._buffers(eng.device)
        self.record_value(fwd.flat_value, st.targets[:fwd.M], eng.stream())
        if dev.get('params_before') is None or dev['params_before'].shape != eng.params.shape:
            dev['params_before'] = torch.empty_like(eng.params)
            off = check_offsets(list(eng.layout.offsets) + [eng.layout.nparams], eng.layout.nparams)
            dev['offsets'] = torch.from_numpy(off).to(eng.device)
        dev['params_before'].copy_(eng.params)

    def forward_logits(self, eng, obs, M):
        """[M][A] logits of ``obs`` (uint8 [M][84][84][4] on the device) at the engine's current
        parameters: chunks of ``forward_rows`` through activations of the diagnostics' own."""
        dev = self._buffers(eng.device)
        out = dev.get('logits')
        if out is None or tuple(out.shape) != (M, eng.A):
            out = dev['logits'] = torch.zeros(M, eng.A, dtype=torch.float32, device=eng.device)
        from actorcritic._engine import OBS_BYTES
        for r0 in range(0, M, self.forward_rows):
            rows = min(self.forward_rows, M - r0)
            acts = eng.activations(rows, 'diagnostics')
            eng.forward(obs.data_ptr() + r0 * OBS_BYTES, rows, acts.struct, want_value=False)
            out[r0:r0 + rows].copy_(acts.logits[:rows])
        return out

    def after_update(self, eng, fwd, grads, optimizer=None):
        """After the update: KL and entropy of the new policy on the update's own observations
        against the logits the loss read, then the norms; ends the armed update."""
        dev = self._buffers(eng.device)
        new = self.forward_logits(eng, fwd.obs, fwd.M)
        legal = None if eng.masks is None else eng.row_masks(fwd.batch, fwd.steps)
        self.record_policy(fwd.flat_logits, new, legal, eng.A, eng.stream())
        kfac = _kfac_of(optimizer)
        precon = kfac.state['precon'] if kfac is not None and kfac.state is not None else None
        self.record_segments('grad', grads, precon, dev['offsets'], eng.stream())
        self.record_segments('step', eng.params, dev['params_before'], dev['offsets'], eng.stream())
        if kfac is not None and kfac.last_coeff is not None:
            self.record_coeff(kfac.last_coeff)
        self.finish()

    # -- reading --------------------------------------------------------------------------------
    def read(self):
        """-> the scalar-log dict of the last armed update; RuntimeError when there is none (the
        object was never armed, its update has not run yet, or it was read already).

        Under data parallelism a COLLECTIVE: every rank calls it at the same update.  The value
        and policy sums go through one SUM all-reduce and the KL maxima through one MAX all-reduce
        (on copies); the norms are of all-reduced quantities and need none.  Then the one host
        copy, of every accumulator at once."""
        from actorcritic import parallel
        res = self._res
        if not res.get('done'):
            raise RuntimeError('UpdateDiagnostics.read(): no armed update has been recorded (request() it '
                               'before the optimize op runs)')
        G = self.num_groups
        value, policy = res['value'].to(torch.float64), res['policy'].to(torch.float64)
        sums = torch.cat([value.reshape(-1), policy[:, :3].reshape(-1)])
        maxima = policy[:, 3].clone()
        if parallel.world_size() > 1:
            parallel.allreduce_sum_(sums)
            parallel.allreduce_max_(maxima)
        parts = [sums, maxima]
        for name in ('grad', 'step', 'coeff'):
            if name in res:
                parts.append(res[name].detach().reshape(-1).to(device=sums.device, dtype=torch.float64))
        host = torch.cat(parts).cpu().numpy()
        value = host[:G * VALUE_COLS].reshape(G, VALUE_COLS)
        at = G * VALUE_COLS
        policy = np.concatenate([host[at:at + 3 * G].reshape(G, 3), host[at + 3 * G:at + 4 * G].reshape(G, 1)],
                                axis=1)
        at += 4 * G
        segs = {}
        for name in ('grad', 'step'):
            if name in res:
                n = res[name].numel()
                segs[name] = host[at:at + n].reshape(-1, SEG_COLS)
                at += n
        coeff = float(host[at]) if 'coeff' in res else None
        self._res = {}
        self.last_acc = dict(segs, value=value, policy=policy)  # the host copy, as read (over all ranks)
        return self.log_scalars(value, policy, segs.get('grad'), segs.get('step'), coeff,
                                res.get('grad_has_y', False))

    def log_scalars(self, value, policy, grad=None, step=None, coeff=None, has_precon=False):
        """Host accumulators -> the scalar log's keys (NaN where undefined)."""
        out = value_scalars(value.sum(axis=0))
        out.update(policy_scalars(reduce_policy_groups(policy)))
        if grad is not None:
            out['grad_norm'] = float(np.sqrt(grad[:, 0].sum()))
        if step is not None:
            out['step_norm'] = float(np.sqrt(step[:, 3].sum()))
            out['param_norm'] = float(np.sqrt(step[:, 0].sum()))
        layered = lambda seg: seg is not None and seg.shape[0] == 2 * len(LAYERS)
        if layered(grad):
            for name, row in zip(LAYERS, layer_sums(grad)):
                out['grad_norm/' + name] = float(np.sqrt(row[0]))
        if layered(step):
            for name, row in zip(LAYERS, layer_sums(step)):
                out['step_norm/' + name] = float(np.sqrt(row[3]))
        if has_precon and layered(grad):
            for name, row in zip(LAYERS, layer_sums(grad)):
                out['precon_norm/' + name] = float(np.sqrt(row[1]))
            for name, row in zip(LAYERS, layer_sums(grad)):
                out['precon_cos/' + name] = cosine(row)
        if coeff is not None:
            out['kfac_coeff'] = coeff
        present = sorted(set(self.groups.tolist()))
        if self.group_names is not None and len(present) > 1:
            for g in present:
                name = self.group_names[g]
                out['explained_variance/' + name] = explained_variance(value[g])
                out['policy_kl/' + name] = policy_scalars(policy[g])['policy_kl']
        return out


def _kfac_of(optimizer):
    """The KfacOptimizer behind ``optimizer`` (itself, or None)."""
    from actorcritic.kfac_utils import KfacOptimizer
    return optimizer if isinstance(optimizer, KfacOptimizer) else None
