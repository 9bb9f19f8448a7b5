"""One function per libacmi operation that has a legal-action-mask or truncation twin.

Each takes the optional pointers (``legal``, ``bad_rows``, ``truncated``) as keywords,
picks the C entry point and splices them into its argument list: the only place in the
package that names a ``_masked`` / ``_trunc`` entry point (beside _lib's table).
Pointer arguments are contiguous tensors, device addresses (int) or None.
"""

import ctypes

from actorcritic import _lib


def _p(x):
    if x is None or isinstance(x, ctypes.c_void_p):
        return x
    return _lib.c_vp(x) if isinstance(x, int) else _lib.ptr(x)


def _call(plain, twin, head, extra, tail):
    """plain(*head, *tail); with the optional pointers given, twin(*head, *extra, *tail)."""
    if extra[0] is None:
        _lib.call(plain, *head, *tail)
    else:
        _lib.call(twin, *head, *extra, *tail)


def sample_actions(logits, ld, B, A, seed, stream_id, counter, row_offset, actions, bad_rows, stream, legal=None,
                   counter_dev=None, uniforms=None, mode=False):
    """Row m draws with the key (seed, stream_id, counter [+ *counter_dev], row_offset + m);
    ``counter`` is taken mod 2^32."""
    _call('acmi_sample_actions_dev', 'acmi_sample_actions_masked',
          (_p(logits), ld, B, A, seed, stream_id, _p(counter_dev), counter & 0xFFFFFFFF, row_offset, _p(uniforms),
           1 if mode else 0), (_p(legal),), (_p(actions), _p(bad_rows), stream))


def categorical(logits, ld, B, A, actions, entropy, log_prob, stream, legal=None):
    _call('acmi_categorical', 'acmi_categorical_masked', (_p(logits), ld, B, A, _p(actions)), (_p(legal),),
          (_p(entropy), _p(log_prob), stream))


def targets(rewards, terminals, values, v_boot, N, T, gamma, gae_lambda, tables, targets, adv, stream,
            truncated=None):
    """gae_lambda None: the n-step returns from ``tables`` = (gamma_pow, boot_pow); else GAE(lambda)."""
    if gae_lambda is None:
        names, form = ('acmi_returns', 'acmi_returns_trunc'), (_p(tables[0]), _p(tables[1]))
    else:
        names, form = ('acmi_gae', 'acmi_gae_trunc'), (gamma, gae_lambda)
    _call(*names, (_p(rewards), _p(terminals)), (_p(truncated),),
          (_p(values), _p(v_boot), N, T) + form + (_p(targets), _p(adv), stream))


def vtrace(logits, ld, A, actions, behaviour_logp, rewards, terminals, values, v_boot, N, T, gamma, gae_lambda,
           rho_bar, c_bar, targets, adv, rho, stream, truncated=None, legal=None, bad_rows=None, log_prob=None):
    """acmi_vtrace: one entry point, the optional pointers are its nullable arguments."""
    _lib.call('acmi_vtrace', _p(logits), ld, A, _p(actions), _p(behaviour_logp), _p(rewards), _p(terminals),
              _p(truncated), _p(values), _p(v_boot), N, T, gamma, gae_lambda, rho_bar, c_bar, _p(legal),
              _p(bad_rows), _p(targets), _p(adv), _p(rho), _p(log_prob), stream)


def a2c_loss(logits, ld, values, actions, targets, adv, M, A, beta, vcoef, grad_scale, dhead, ldh, ws, loss_out,
             stream, legal=None, bad_rows=None):
    _call('acmi_a2c_loss', 'acmi_a2c_loss_masked',
          (_p(logits), ld, _p(values), _p(actions), _p(targets), _p(adv), M, A, beta, vcoef, grad_scale, _p(dhead),
           ldh, _p(ws), _p(loss_out)), (_p(legal), _p(bad_rows)), (stream,))


def ppo_loss(logits, ld, values, actions, old_logp, old_values, targets, adv, M, A, clip_eps, vclip, beta, vcoef,
             grad_scale, dhead, ldh, ws, loss_out, clip_frac_out, stream, legal=None, bad_rows=None):
    _call('acmi_ppo_loss', 'acmi_ppo_loss_masked',
          (_p(logits), ld, _p(values), _p(actions), _p(old_logp), _p(old_values), _p(targets), _p(adv), M, A,
           clip_eps, vclip, beta, vcoef, grad_scale, _p(dhead), ldh, _p(ws), _p(loss_out), _p(clip_frac_out)),
          (_p(legal), _p(bad_rows)), (stream,))


def rollout_step(net, obs, img_stride, B, acts, act_img_stride, io, stream, legal=None):
    """net, acts, io: the ctypes structs (passed by reference)."""
    _call('acmi_rollout_step', 'acmi_rollout_step_masked',
          (ctypes.byref(net), _p(obs), img_stride, B, ctypes.byref(acts), act_img_stride, ctypes.byref(io)),
          (_p(legal),), (stream,))


def rollout_step_games(net, obs, img_stride, B, acts, act_img_stride, gio, stream, legal=None):
    """acmi_rollout_step_games: net, acts, gio (_lib.RolloutGameIO) by reference; legal is
    an argument of the one entry point (None: unmasked)."""
    _lib.call('acmi_rollout_step_games', ctypes.byref(net), _p(obs), img_stride, B, ctypes.byref(acts),
              act_img_stride, ctypes.byref(gio), _p(legal), stream)


def output_stats(net, B, acts, bwd, seed, row_offset, counter, g_stats, ws, ws_floats, stream, legal=None):
    """net, acts, bwd: the ctypes structs (passed by reference)."""
    _call('acmi_kfac_output_stats', 'acmi_kfac_output_stats_masked',
          (ctypes.byref(net), B, ctypes.byref(acts), ctypes.byref(bwd), seed, row_offset, counter), (_p(legal),),
          (_p(g_stats), _p(ws), ws_floats, stream))
