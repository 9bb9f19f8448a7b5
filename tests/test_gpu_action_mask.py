"""Legal-action masks on the GPU (include/acmi.h "Legal-action masks").

  * a full mask (the low A bits set) reproduces every unmasked entry point bit for bit;
  * random masks against float64 / float32 restatements written here, with the
    tolerances of the unmasked tests (test_gpu_parity.py's A2C loss / categorical test,
    test_gpu_ppo.py's PPO loss test): loss scalars rel 1e-5, head gradients rtol 1e-4 /
    atol 1e-9, value column rtol 1e-5 / atol 1e-10, entropy / log-prob rtol 1e-5 / atol
    1e-6, G factors rel 5e-5 (test_acktr_update_matches_oracle); columns outside the
    legal set are compared with == 0.0;
  * the sampler's edges, the loss kernels' bad rows, masked K-FAC head statistics;
  * the whole path through MultiEnvAgent / the objectives / the K-FAC optimizer, and
    the host-stepped rollout.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from actorcritic import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
import oracle  # noqa: E402

pytestmark = pytest.mark.gpu

BETA, VCOEF = 0.01, 0.5
EPS32, VCLIP32 = float(np.float32(0.1)), float(np.float32(0.2))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def dev_masks(words):
    return dev(np.asarray(words, np.uint32).view(np.int32))


def full_word(A):
    return (1 << A) - 1


def legal_matrix(masks, A):
    return ((np.asarray(masks, np.uint64)[:, None] >> np.arange(A, dtype=np.uint64)) & 1).astype(bool)


# ---------------------------------------------------------------------------
# restatements of the masked arithmetic
# ---------------------------------------------------------------------------
def masked_softmax64(logits, masks):
    """float64: (S, log p with -inf outside S, p with 0 outside S, H); rows with an
    empty S get lp = -inf, p = 0, H = 0."""
    z = np.asarray(logits, np.float64)
    M, A = z.shape
    S = legal_matrix(masks, A)
    zs = np.where(S, z, -np.inf)
    some = S.any(1)
    mx = np.where(some, zs.max(1, initial=-np.inf), 0.0)
    with np.errstate(over='ignore', invalid='ignore'):
        e = np.where(S, np.exp(np.where(S, z, 0.0) - mx[:, None]), 0.0)
    se = e.sum(1)
    lse = mx + np.log(np.where(some, se, 1.0))
    lp_in = np.where(S, z - lse[:, None], 0.0)
    p = np.where(S, np.exp(lp_in), 0.0)
    H = -(p * lp_in).sum(1)
    return S, np.where(S, lp_in, -np.inf), p, H


def a2c_ref(logits, values, actions, targets, adv, masks):
    """acmi_a2c_loss_masked in float64: bad rows (S empty or the action outside S) drop
    their policy and entropy terms (the means stay over all M rows) and their policy
    columns, and keep their value term."""
    S, lp, p, H = masked_softmax64(logits, masks)
    M, A = S.shape
    v, tg, ad = (np.asarray(x, np.float64) for x in (values, targets, adv))
    act = np.asarray(actions)
    ok = S[np.arange(M), np.clip(act, 0, A - 1)] & (act >= 0) & (act < A)
    lpa = np.where(ok, lp[np.arange(M), np.clip(act, 0, A - 1)], 0.0)
    onehot = np.eye(A)[np.clip(act, 0, A - 1)]
    lpf = np.where(S, lp, 0.0)
    d = -(ad[:, None] * (onehot - p) - BETA * p * (lpf + H[:, None])) / M
    return dict(policy_loss=-(np.sum(np.where(ok, ad * lpa, 0.0)) / M + BETA * np.sum(np.where(ok, H, 0.0)) / M),
                baseline_loss=np.mean((tg - v) ** 2 / 2.0), mean_entropy=np.sum(np.where(ok, H, 0.0)) / M,
                dlogits=np.where(S & ok[:, None], d, 0.0), dvalue=VCOEF * (v - tg) / M, ok=ok, S=S, lpa=lpa, H=H, p=p,
                lp=lp)


def ppo_ref(logits, values, actions, old_logp, old_values, targets, adv, masks, eps, vclip):
    """acmi_ppo_loss_masked in float64 (test_gpu_ppo.ppo_ref over the legal sets)."""
    a = a2c_ref(logits, values, actions, targets, adv, masks)
    S, ok, p, lp, H, lpa = a['S'], a['ok'], a['p'], a['lp'], a['H'], a['lpa']
    M, A = S.shape
    v, tg, ad, olp = (np.asarray(x, np.float64) for x in (values, targets, adv, old_logp))
    r = np.exp(np.where(ok, lpa - olp, 0.0))
    s1, s2 = r * ad, np.clip(r, 1.0 - eps, 1.0 + eps) * ad
    pol_on = s1 <= s2
    e1 = (v - tg) ** 2
    val_on, e = np.ones(M, bool), e1
    if vclip > 0:
        vo = np.asarray(old_values, np.float64)
        e2 = (vo + np.clip(v - vo, -vclip, vclip) - tg) ** 2
        val_on = ~((np.abs(v - vo) > vclip) & (e2 > e1))
        e = np.maximum(e1, e2)
    onehot = np.eye(A)[np.clip(actions, 0, A - 1)]
    lpf = np.where(S, lp, 0.0)
    w = np.where(pol_on, ad * r, 0.0)
    d = -(w[:, None] * (onehot - p)) / M + BETA * p * (lpf + H[:, None]) / M
    okf = ok.astype(np.float64)
    return dict(policy_loss=-(np.sum(okf * np.where(pol_on, s1, s2)) / M + BETA * np.sum(okf * H) / M),
                baseline_loss=np.mean(e / 2.0), mean_entropy=np.sum(okf * H) / M,
                approx_kl=np.sum(okf * (olp - lpa)) / M, clip_frac=np.sum(okf * (np.abs(r - 1.0) > eps)) / M,
                dlogits=np.where(S & ok[:, None], d, 0.0), dvalue=np.where(val_on, VCOEF * (v - tg), 0.0) / M, r=r)


def sample_masked_f32(logits, u, masks, mode=False):
    """The masked inverse-CDF draw in the kernel's float32 arithmetic (oracle.sample_f32
    over the legal indices, ascending; the fallback is the last legal action); -1 for an
    empty set or a non-finite logit anywhere in the row."""
    z = np.asarray(logits, np.float32)
    S = legal_matrix(masks, z.shape[1])
    out = np.empty(z.shape[0], np.int64)
    for m in range(z.shape[0]):
        idx = np.flatnonzero(S[m])
        if idx.size == 0 or not np.isfinite(z[m]).all():
            out[m] = -1
            continue
        zl = z[m, idx]
        if mode:
            out[m] = idx[int(np.argmax(zl))]
            continue
        mx = np.float32(zl.max())
        e = np.exp(zl - mx).astype(np.float32)
        se = np.float32(0)
        for v in e:
            se = np.float32(se + v)
        target = np.float32(np.float32(u[m]) * se)
        c = np.float32(0)
        y = idx[-1]
        for a, v in zip(idx, e):
            c = np.float32(c + v)
            if target < c:
                y = a
                break
        out[m] = y
    return out


def random_masks(rng, M, A):
    """Non-empty random legal sets; rows 0..7 hold a single action, rows 8..15 exclude
    action 0 and action A - 1."""
    S = rng.random((M, A)) < 0.5
    S[np.arange(M), rng.integers(0, A, M)] = True
    for m in range(8):
        S[m] = False
        S[m, (3 * m + 1) % A] = True
    S[8:16, 0] = S[8:16, A - 1] = False
    S[8:16, 1 + (np.arange(8) % (A - 2))] = True
    return (S.astype(np.uint64) << np.arange(A, dtype=np.uint64)).sum(1).astype(np.uint32), S


def loss_inputs(M, A, ld, seed, masks=None, S=None):
    """Random float32 inputs (logits [M, ld], the columns past A filled with a large
    finite value no kernel may read); with masks the actions are legal ones and rows
    16..47 carry illegal logits of +80 and 1e30."""
    rng = np.random.default_rng(seed)
    logits = np.full((M, ld), 3e38, np.float32)
    logits[:, :A] = rng.standard_normal((M, A)).astype(np.float32)
    if S is None:
        actions = rng.integers(0, A, M).astype(np.int32)
    else:
        actions = np.array([rng.choice(np.flatnonzero(S[m])) for m in range(M)], np.int32)
        for m in range(16, 48):
            bad = np.flatnonzero(~S[m])
            logits[m, bad] = np.where(np.arange(bad.size) % 2 == 0, np.float32(80.0), np.float32(1e30))
    d = dict(logits=logits, actions=actions, adv=rng.standard_normal(M).astype(np.float32),
             values=rng.standard_normal(M).astype(np.float32), targets=rng.standard_normal(M).astype(np.float32))
    d['old_values'] = (d['values'] - rng.uniform(-0.5, 0.5, M)).astype(np.float32)
    d['dlog'] = rng.uniform(-0.25, 0.35, M)  # log-ratio of the PPO cases: a third of the rows leave [0.9, 1.1]
    return d


# ---------------------------------------------------------------------------
# launchers
# ---------------------------------------------------------------------------
def run_sample(B, A, ld, L, legal, seed=5, sid=1, ctr=9, row_offset=0, u=None, mode=0, row0=0):
    """acmi_sample_actions_masked (legal given) / acmi_sample_actions_dev on rows row0 .. row0+B-1."""
    out = torch.full((B,), -7, dtype=torch.int32, device='cuda')
    bad = torch.zeros(1, dtype=torch.int32, device='cuda')
    lp = _lib.c_vp(L.data_ptr() + 4 * row0 * ld)
    up = None if u is None else _lib.c_vp(u.data_ptr() + 4 * row0)
    if legal is not None:
        _lib.call('acmi_sample_actions_masked', lp, ld, B, A, seed, sid, None, ctr, row_offset, up, mode,
                  _lib.c_vp(legal.data_ptr() + 4 * row0), _lib.ptr(out), _lib.ptr(bad), _lib.stream_handle())
    else:
        _lib.call('acmi_sample_actions_dev', lp, ld, B, A, seed, sid, None, ctr, row_offset, up, mode, _lib.ptr(out),
                  _lib.ptr(bad), _lib.stream_handle())
    return out, bad


def run_categorical(M, A, ld, L, AC, legal):
    ent, lp = torch.full((M,), 7.0, device='cuda'), torch.full((M,), 7.0, device='cuda')
    if legal is not None:
        _lib.call('acmi_categorical_masked', _lib.ptr(L), ld, M, A, _lib.ptr(AC), _lib.ptr(legal), _lib.ptr(ent),
                  _lib.ptr(lp), _lib.stream_handle())
    else:
        _lib.call('acmi_categorical', _lib.ptr(L), ld, M, A, _lib.ptr(AC), _lib.ptr(ent), _lib.ptr(lp),
                  _lib.stream_handle())
    return ent, lp


def run_a2c(lib, t, M, A, ld, ldh, legal, bad=None):
    dhead = torch.full((M, ldh), 7.0, device='cuda')  # (the kernel writes the padding zeros itself)
    ws = torch.zeros(lib.acmi_a2c_loss_ws_floats(M), device='cuda')
    out = torch.zeros(4, device='cuda')
    args = [_lib.ptr(t['logits']), ld, _lib.ptr(t['values']), _lib.ptr(t['actions']), _lib.ptr(t['targets']),
            _lib.ptr(t['adv']), M, A, BETA, VCOEF, 1.0, _lib.ptr(dhead), ldh, _lib.ptr(ws), _lib.ptr(out)]
    if legal is not None:
        _lib.call('acmi_a2c_loss_masked', *args, _lib.ptr(legal), _lib.ptr(bad), _lib.stream_handle())
    else:
        _lib.call('acmi_a2c_loss', *args, _lib.stream_handle())
    return dhead, out


def run_ppo(lib, t, M, A, ld, ldh, vclip, olp, legal, bad=None):
    dhead = torch.full((M, ldh), 7.0, device='cuda')
    ws = torch.zeros(lib.acmi_ppo_loss_ws_floats(M), device='cuda')
    out, cf = torch.zeros(4, device='cuda'), torch.zeros(1, device='cuda')
    args = [_lib.ptr(t['logits']), ld, _lib.ptr(t['values']), _lib.ptr(t['actions']), _lib.ptr(olp),
            _lib.ptr(t['old_values']), _lib.ptr(t['targets']), _lib.ptr(t['adv']), M, A, EPS32, vclip, BETA, VCOEF, 1.0,
            _lib.ptr(dhead), ldh, _lib.ptr(ws), _lib.ptr(out), _lib.ptr(cf)]
    if legal is not None:
        _lib.call('acmi_ppo_loss_masked', *args, _lib.ptr(legal), _lib.ptr(bad), _lib.stream_handle())
    else:
        _lib.call('acmi_ppo_loss', *args, _lib.stream_handle())
    return dhead, out, cf


def tensors(d):
    return {k: dev(d[k]) for k in ('logits', 'values', 'actions', 'old_values', 'targets', 'adv')}


# ---------------------------------------------------------------------------
# 1. a full mask equals the unmasked entry point, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('A', [4, 18, 32])
def test_full_mask_equals_unmasked_bit_for_bit(lib, cuda, A):
    """300 rows (one full 256-row block and a partial one), ld = A + 3: the sampler
    (counter RNG and injected uniforms, sample and mode, and in two chunks with
    row_offset), categorical, the A2C loss (ldh = A + 5: padding columns past the
    value) and the PPO loss with and without value clipping."""
    M, ld, ldh = 300, A + 3, A + 5
    d = loss_inputs(M, A, ld, seed=100 + A)
    t = tensors(d)
    L = t['logits']
    # (bits at or above A are ignored: half the words carry some)
    words = np.full(M, full_word(A), np.uint64)
    if A < 32:
        words[::2] |= np.uint64(0xFFFFFFFF) << np.uint64(A)
    legal = dev_masks((words & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    u = dev(np.random.default_rng(1).random(M).astype(np.float32))
    for uu, mode in ((None, 0), (u, 0), (None, 1)):
        ref, rbad = run_sample(M, A, ld, L, None, u=uu, mode=mode)
        got, gbad = run_sample(M, A, ld, L, legal, u=uu, mode=mode)
        assert torch.equal(got, ref) and int(gbad.item()) == int(rbad.item()) == 0, (uu is None, mode)
        lo, _ = run_sample(130, A, ld, L, legal, u=uu, mode=mode)
        hi, _ = run_sample(M - 130, A, ld, L, legal, u=uu, mode=mode, row_offset=130, row0=130)
        assert torch.equal(torch.cat([lo, hi]), ref), 'chunked'
    assert ref.min() >= 0 and ref.max() < A
    for a, b in zip(run_categorical(M, A, ld, L, t['actions'], legal), run_categorical(M, A, ld, L, t['actions'], None)):
        assert torch.equal(a, b)
    bad = torch.zeros(1, dtype=torch.int32, device=cuda)
    got, ref = run_a2c(lib, t, M, A, ld, ldh, legal, bad), run_a2c(lib, t, M, A, ld, ldh, None)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    assert not got[0][:, A + 1:].any() and got[0][:, :A + 1].abs().min() > 0
    _, lpa = run_categorical(M, A, ld, L, t['actions'], None)
    olp = lpa - dev(d['dlog'].astype(np.float32))
    for vclip in (0.0, VCLIP32):
        for a, b in zip(run_ppo(lib, t, M, A, ld, ldh, vclip, olp, legal, bad),
                        run_ppo(lib, t, M, A, ld, ldh, vclip, olp, None)):
            assert torch.equal(a, b), vclip
    assert int(bad.item()) == 0


def _net(lib, cuda, A, C3, B, seed):
    """A prepared net, a forward of B random images, and the buffers of an update."""
    params = dev(oracle.init_params(A, C3, seed=seed).astype(np.float32))
    prep = torch.empty(int(lib.acmi_conv_prep_bytes(C3)), dtype=torch.uint8, device=cuda)
    net = _lib.Net(A, C3, params.data_ptr(), prep.data_ptr())
    _lib.call('acmi_conv_prepare', ctypes.byref(net), _lib.ptr(prep), _lib.stream_handle())
    g = torch.Generator().manual_seed(seed)
    obs = torch.randint(0, 256, (B, 84, 84, 4), generator=g, dtype=torch.uint8).to(cuda)
    z = lambda *s: torch.zeros(*s, device=cuda)
    zi = lambda *s: torch.zeros(*s, dtype=torch.int32, device=cuda)
    t = dict(a1=z(B, 20, 20, 32), a2=z(B, 9, 9, 64), a3=z(B, 7, 7, C3), a4=z(B, 512), logits=z(B, A), value=z(B),
             m1=zi(B, 400), m2=zi(B, 162), m3=zi(B, 49 * C3 // 32))
    fws = z(max(1, int(lib.acmi_forward_ws_floats(B))))
    acts = _lib.Acts(t['a1'].data_ptr(), t['a2'].data_ptr(), t['a3'].data_ptr(), t['a4'].data_ptr(),
                     t['logits'].data_ptr(), t['value'].data_ptr(), A, fws.data_ptr(), fws.numel(), t['m1'].data_ptr(),
                     t['m2'].data_ptr(), t['m3'].data_ptr())
    _lib.call('acmi_forward', ctypes.byref(net), _lib.ptr(obs), 84 * 84 * 4, B, ctypes.byref(acts), 1,
              _lib.stream_handle())
    ldh = max(8, (A + 1 + 3) // 4 * 4)
    d = [z(B, 20, 20, 32), z(B, 9, 9, 64), z(B, 7, 7, C3), z(B, 512), z(B, ldh)]
    bwd = _lib.Bwd(*[x.data_ptr() for x in d], ldh)
    ws = z(int(lib.acmi_backward_ws_floats(B, A, C3)))
    keep = (params, prep, obs, t, fws, d, ws)
    return net, acts, bwd, ws, obs, t, params, keep


def _stat_layout(lib, A, C3):
    din, dout, so = (ctypes.c_int64 * 6)(), (ctypes.c_int64 * 6)(), (ctypes.c_int64 * 11)()
    tot = ctypes.c_int64()
    _lib.call('acmi_kfac_layout', A, C3, din, dout, so, ctypes.byref(tot))
    return list(dout), list(so), tot.value


def _output_stats(net, acts, bwd, ws, B, tot, legal, seed=7, row_offset=0, ctr=3):
    gstat = torch.full((tot,), 7.0, device='cuda')
    if legal is not None:
        _lib.call('acmi_kfac_output_stats_masked', ctypes.byref(net), B, ctypes.byref(acts), ctypes.byref(bwd), seed,
                  row_offset, ctr, _lib.ptr(legal), _lib.ptr(gstat), _lib.ptr(ws), ws.numel(), _lib.stream_handle())
    else:
        _lib.call('acmi_kfac_output_stats', ctypes.byref(net), B, ctypes.byref(acts), ctypes.byref(bwd), seed,
                  row_offset, ctr, _lib.ptr(gstat), _lib.ptr(ws), ws.numel(), _lib.stream_handle())
    torch.cuda.synchronize()
    return gstat


def test_full_mask_output_stats_equal_unmasked(lib, cuda):
    A, C3, B = 18, 32, 24
    net, acts, bwd, ws, obs, t, params, keep = _net(lib, cuda, A, C3, B, seed=4)
    dout, so, tot = _stat_layout(lib, A, C3)
    ref = _output_stats(net, acts, bwd, ws, B, tot, None)
    got = _output_stats(net, acts, bwd, ws, B, tot, dev_masks(np.full(B, full_word(A), np.uint32)))
    for l in range(6):  # every G block (the A part of the vector is not this call's)
        lo, n = so[5 + l], dout[l] * dout[l]
        assert torch.equal(got[lo:lo + n], ref[lo:lo + n]), l
        assert torch.isfinite(ref[lo:lo + n]).all() and ref[lo:lo + n].abs().max() > 0


GAMES = ['Freeway', 'Breakout', 'Pong', 'Seaquest', 'Assault', 'Freeway', 'Skiing', 'Tennis']


def _games(N):
    return [GAMES[n % len(GAMES)] for n in range(N)]


def _build(N, T, A=18, C3=32, games=None, mask_actions=False, seed=5):
    from actorcritic import session as sess
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.envs.atari.wrappers import SyntheticAtariEnvs
    from actorcritic.multi_env import MultiEnv
    sess.reset_default_graph()
    env = MultiEnv(SyntheticAtariEnvs(N, num_actions=A, seed=seed, games=games))
    params = oracle.init_params(A, C3, seed=1)
    # (larger policy weights than the 0.01-gain init: the draws depend on the logits)
    off, _ = oracle.param_offsets(A, C3)
    params[off[8]:off[9]] *= 60.0
    model = AtariModel(env.observation_space, env.action_space, C3, params=params, random_seed=3)
    agent = MultiEnvAgent(env, model, T, mask_actions=mask_actions)
    return env, model, agent, params


def _feed(model, data):
    obs, act, rew, term, nxt, _ = data
    return {model.observations_placeholder: obs, model.bootstrap_observations_placeholder: nxt,
            model.actions_placeholder: act, model.rewards_placeholder: rew, model.terminals_placeholder: term}


def _clone(data):
    return tuple(x.clone() if isinstance(x, torch.Tensor) else x for x in data)


def _rollouts(agent, model, k):
    """k rollouts -> [(obs, actions, rewards, terminals, next_obs, logits)] (clones)."""
    from actorcritic import session as sess
    out = []
    with sess.Session() as s:
        for _ in range(k):
            data = agent.interact(s)
            logits = model.engine.lookup_rollout(data[0]).flat_logits.clone()
            out.append(tuple(x.clone() for x in data[:5]) + (logits,))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('N', [8, 72], ids=['split-form', 'one-block-per-env'])
def test_full_mask_rollout_step_equals_unmasked(lib, cuda, monkeypatch, N):
    """The fused step (acmi_rollout_step_masked, every env's word full) against
    acmi_rollout_step on a twin env: T = 3, A = 18, mixed games -- observations, actions,
    rewards, terminals and logits of two rollouts, bit for bit."""
    monkeypatch.delenv('ACMI_ROLLOUT_FUSED', raising=False)
    T, A = 3, 18
    env, model, agent, _ = _build(N, T, A, games=_games(N))
    ref = _rollouts(agent, model, 2)
    assert agent._bufs.fused and model.engine.masks is None
    env2, model2, agent2, _ = _build(N, T, A, games=_games(N))
    model2.set_action_masks(np.full(N, full_word(A), np.uint32))
    got = _rollouts(agent2, model2, 2)
    assert agent2._bufs.fused and model2.engine.masks is not None
    for a, b in zip(got, ref):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    assert len(np.unique(ref[0][1].cpu().numpy())) > 4  # (the draws spread over the 18 actions)


# ---------------------------------------------------------------------------
# 2. random masks against float64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('A', [5, 18, 32])
def test_random_masks_match_float64(lib, cuda, A):
    """300 rows of non-empty random legal sets: single-action rows (H == 0, p == 1, zero
    policy columns), rows whose illegal logits are +80 and 1e30, rows without action 0
    and action A - 1.  Tolerances: the unmasked tests' (module docstring)."""
    M, ld, ldh = 300, A + 3, A + 5
    rng = np.random.default_rng(200 + A)
    masks, S = random_masks(rng, M, A)
    d = loss_inputs(M, A, ld, seed=300 + A, masks=masks, S=S)
    assert (S[:8].sum(1) == 1).all() and not S[8:16, 0].any() and not S[8:16, A - 1].any()
    assert (d['logits'][16:48, :A] >= 80).sum() >= 32 and (d['logits'][16:48, :A] >= 1e30).any()
    t = tensors(d)
    legal = dev_masks(masks)
    z = d['logits'][:, :A]
    ref = a2c_ref(z, d['values'], d['actions'], d['targets'], d['adv'], masks)
    assert ref['ok'].all()
    # categorical
    ent, lp = run_categorical(M, A, ld, t['logits'], t['actions'], legal)
    ent, lp = ent.cpu().numpy(), lp.cpu().numpy()
    assert np.isfinite(ent).all() and np.isfinite(lp).all()
    np.testing.assert_allclose(ent, ref['H'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(lp, ref['lpa'], rtol=1e-5, atol=1e-6)
    assert (ent[:8] == 0.0).all() and (lp[:8] == 0.0).all()
    # log-prob of an action outside S is -inf
    out_act = np.array([np.flatnonzero(~S[m])[0] if (~S[m]).any() else -1 for m in range(M)], np.int32)
    _, lp_out = run_categorical(M, A, ld, t['logits'], dev(out_act), legal)
    lp_out = lp_out.cpu().numpy()
    assert np.isneginf(lp_out[out_act >= 0]).all() and (out_act >= 0).sum() > M // 2
    # A2C
    bad = torch.zeros(1, dtype=torch.int32, device=cuda)
    dhead, out = run_a2c(lib, t, M, A, ld, ldh, legal, bad)
    dh, got = dhead.cpu().numpy(), out.cpu().numpy()
    print('a2c scalars', got[:3], ref['policy_loss'], ref['baseline_loss'], ref['mean_entropy'])
    assert np.isfinite(dh).all() and np.isfinite(got).all() and int(bad.item()) == 0
    assert got[0] == pytest.approx(ref['policy_loss'], rel=1e-5, abs=1e-7)
    assert got[1] == pytest.approx(ref['baseline_loss'], rel=1e-5)
    assert got[2] == pytest.approx(ref['mean_entropy'], rel=1e-5)
    np.testing.assert_allclose(dh[:, :A], ref['dlogits'], rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(dh[:, A], ref['dvalue'], rtol=1e-5, atol=1e-10)
    assert (dh[:, :A][~S] == 0.0).all() and not dh[:, A + 1:].any()
    assert (dh[:8, :A] == 0.0).all()  # a single legal action: p == 1, nothing to learn
    # PPO, with and without value clipping
    olp32 = (lp - d['dlog']).astype(np.float32)
    for vclip in (0.0, VCLIP32):
        pref = ppo_ref(z, d['values'], d['actions'], olp32, d['old_values'], d['targets'], d['adv'], masks, EPS32,
                       vclip)
        near = (np.abs(pref['r'] - (1 + EPS32)) < 1e-3) | (np.abs(pref['r'] - (1 - EPS32)) < 1e-3)
        if near.any():  # (no row on a clip boundary: move those to ratio 1)
            olp32 = np.where(near, lp, olp32).astype(np.float32)
            pref = ppo_ref(z, d['values'], d['actions'], olp32, d['old_values'], d['targets'], d['adv'], masks,
                           EPS32, vclip)
        dhead, out, cf = run_ppo(lib, t, M, A, ld, ldh, vclip, dev(olp32), legal, bad)
        dh, got = dhead.cpu().numpy(), out.cpu().numpy()
        print('ppo scalars', vclip, got, float(cf), [pref[k] for k in ('policy_loss', 'baseline_loss', 'mean_entropy',
                                                                         'approx_kl', 'clip_frac')])
        assert np.isfinite(dh).all() and np.isfinite(got).all() and int(bad.item()) == 0
        assert got[0] == pytest.approx(pref['policy_loss'], rel=1e-5, abs=1e-7)
        assert got[1] == pytest.approx(pref['baseline_loss'], rel=1e-5)
        assert got[2] == pytest.approx(pref['mean_entropy'], rel=1e-5)
        assert got[3] == pytest.approx(pref['approx_kl'], rel=1e-5)
        assert float(cf) == pytest.approx(pref['clip_frac'], rel=1e-5, abs=1e-7)
        np.testing.assert_allclose(dh[:, :A], pref['dlogits'], rtol=1e-4, atol=1e-9)
        np.testing.assert_allclose(dh[:, A], pref['dvalue'], rtol=1e-5, atol=1e-10)
        assert (dh[:, :A][~S] == 0.0).all() and not dh[:, A + 1:].any()
    # old_logp from the masked categorical on the same logits and mask: ratio exactly 1,
    # PPO's dhead is the masked A2C dhead bit for bit
    a2c_dhead, a2c_out = run_a2c(lib, t, M, A, ld, ldh, legal, bad)
    _, lp_d = run_categorical(M, A, ld, t['logits'], t['actions'], legal)
    dhead, out, cf = run_ppo(lib, t, M, A, ld, ldh, 0.0, lp_d, legal, bad)
    assert torch.equal(dhead, a2c_dhead)
    assert float(out[3]) == 0.0 and float(cf) == 0.0 and torch.equal(out[1:3], a2c_out[1:3])


# ---------------------------------------------------------------------------
# 3. sampler edges
# ---------------------------------------------------------------------------
def test_sampler_edges(lib, cuda):
    B, A = 4096, 18
    rng = np.random.default_rng(31)
    masks, S = random_masks(rng, B, A)
    logits = rng.standard_normal((B, A)).astype(np.float32)
    # an illegal logit as the row maximum in a third of the rows
    for m in range(0, B, 3):
        bad_cols = np.flatnonzero(~S[m])
        if bad_cols.size:
            logits[m, bad_cols[0]] = 50.0
    u = rng.random(B).astype(np.float32)
    u[:64] = 0.0
    u[64:128] = np.nextafter(np.float32(1), np.float32(0))
    L, U, legal = dev(logits), dev(u), dev_masks(masks)
    got, bad = run_sample(B, A, A, L, legal, u=U)
    got = got.cpu().numpy()
    ref = sample_masked_f32(logits, u, masks)
    np.testing.assert_array_equal(got, ref)
    assert S[np.arange(B), got].all() and int(bad.item()) == 0
    first = np.array([np.flatnonzero(S[m])[0] for m in range(B)])
    last = np.array([np.flatnonzero(S[m])[-1] for m in range(B)])
    np.testing.assert_array_equal(got[:64], first[:64])
    np.testing.assert_array_equal(got[64:128], last[64:128])
    # the counter RNG: the oracle's uniforms, and no action outside its row's mask
    got, bad = run_sample(B, A, A, L, legal, seed=5, sid=1, ctr=9)
    got = got.cpu().numpy()
    np.testing.assert_array_equal(got, sample_masked_f32(logits, oracle.sample_uniforms(5, 1, 9, B), masks))
    assert S[np.arange(B), got].all() and int(bad.item()) == 0
    # mode: the first arg-max over the legal logits
    logits2 = logits.copy()
    for m in range(1, B, 5):  # ties among the legal logits: the first one wins
        idx = np.flatnonzero(S[m])
        if idx.size >= 2:
            logits2[m, idx[-1]] = logits2[m, idx[0]] = 9.0
    got, bad = run_sample(B, A, A, dev(logits2), legal, mode=1)
    got = got.cpu().numpy()
    np.testing.assert_array_equal(got, sample_masked_f32(logits2, u, masks, mode=True))
    assert (logits2.argmax(1) != got).sum() > B // 6 and int(bad.item()) == 0
    # one empty mask and one NaN row (the NaN in an ILLEGAL column: the check covers all A)
    masks3, logits3 = masks.copy(), logits.copy()
    masks3[11] = 0
    logits3[29, np.flatnonzero(~S[29])[0] if (~S[29]).any() else 0] = np.nan
    for mode in (0, 1):
        got, bad = run_sample(B, A, A, dev(logits3), dev_masks(masks3), u=U, mode=mode)
        got = got.cpu().numpy()
        assert got[11] == -1 and got[29] == -1 and int(bad.item()) == 2
        keep = np.ones(B, bool)
        keep[[11, 29]] = False
        assert (got[keep] >= 0).all()


# ---------------------------------------------------------------------------
# 4. bad rows in the loss kernels
# ---------------------------------------------------------------------------
def test_loss_bad_rows(lib, cuda):
    """64 rows; rows 5 and 40 took an action outside their legal set, row 17 has an
    empty one: the counter reads 3, their policy columns are zero and their value
    columns unchanged, the scalars are finite and drop those rows' policy / entropy terms."""
    M, A, ld, ldh = 64, 18, 18, 20
    rng = np.random.default_rng(41)
    masks, S = random_masks(rng, M, A)
    S[5, 2] = S[40, 17] = False
    masks = (S.astype(np.uint64) << np.arange(A, dtype=np.uint64)).sum(1).astype(np.uint32)
    d = loss_inputs(M, A, ld, seed=42, masks=masks, S=S)
    d['actions'][5], d['actions'][40] = 2, 17
    masks[17], S[17] = 0, False
    bad_rows = [5, 17, 40]
    t, legal = tensors(d), dev_masks(masks)
    ref = a2c_ref(d['logits'], d['values'], d['actions'], d['targets'], d['adv'], masks)
    assert sorted(np.flatnonzero(~ref['ok'])) == bad_rows
    bad = torch.zeros(1, dtype=torch.int32, device=cuda)
    dhead, out = run_a2c(lib, t, M, A, ld, ldh, legal, bad)
    dh, got = dhead.cpu().numpy(), out.cpu().numpy()
    assert int(bad.item()) == 3
    assert np.isfinite(dh).all() and np.isfinite(got).all()
    assert (dh[bad_rows, :A] == 0.0).all()
    np.testing.assert_allclose(dh[:, A], ref['dvalue'], rtol=1e-5, atol=1e-10)
    assert (dh[bad_rows, A] != 0.0).all()
    assert got[0] == pytest.approx(ref['policy_loss'], rel=1e-5, abs=1e-7)
    assert got[1] == pytest.approx(ref['baseline_loss'], rel=1e-5)
    assert got[2] == pytest.approx(ref['mean_entropy'], rel=1e-5)
    np.testing.assert_allclose(dh[:, :A], ref['dlogits'], rtol=1e-4, atol=1e-9)
    # (dropping the rows matters: with their terms the scalars differ by far more than the bound)
    olp = (np.where(ref['ok'], ref['lpa'], 0.0) - d['dlog']).astype(np.float32)
    for vclip in (0.0, VCLIP32):
        pref = ppo_ref(d['logits'], d['values'], d['actions'], olp, d['old_values'], d['targets'], d['adv'], masks,
                       EPS32, vclip)
        near = (np.abs(pref['r'] - (1 + EPS32)) < 1e-3) | (np.abs(pref['r'] - (1 - EPS32)) < 1e-3)
        assert not near[ref['ok']].any()
        bad.zero_()
        dhead, out, cf = run_ppo(lib, t, M, A, ld, ldh, vclip, dev(olp), legal, bad)
        dh, got = dhead.cpu().numpy(), out.cpu().numpy()
        assert int(bad.item()) == 3
        assert np.isfinite(dh).all() and np.isfinite(got).all() and np.isfinite(float(cf))
        assert (dh[bad_rows, :A] == 0.0).all()
        np.testing.assert_allclose(dh[:, A], pref['dvalue'], rtol=1e-5, atol=1e-10)
        assert got[0] == pytest.approx(pref['policy_loss'], rel=1e-5, abs=1e-7)
        assert got[1] == pytest.approx(pref['baseline_loss'], rel=1e-5)
        assert got[2] == pytest.approx(pref['mean_entropy'], rel=1e-5)
        assert got[3] == pytest.approx(pref['approx_kl'], rel=1e-5)
        assert float(cf) == pytest.approx(pref['clip_frac'], rel=1e-5, abs=1e-7)
        np.testing.assert_allclose(dh[:, :A], pref['dlogits'], rtol=1e-4, atol=1e-9)
    # a NULL counter is accepted
    _lib.call('acmi_a2c_loss_masked', _lib.ptr(t['logits']), ld, _lib.ptr(t['values']), _lib.ptr(t['actions']),
              _lib.ptr(t['targets']), _lib.ptr(t['adv']), M, A, BETA, VCOEF, 1.0, _lib.ptr(dhead), ldh,
              _lib.ptr(torch.zeros(lib.acmi_a2c_loss_ws_floats(M), device=cuda)), _lib.ptr(torch.zeros(4, device=cuda)),
              _lib.ptr(legal), None, _lib.stream_handle())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# 5. masked K-FAC head statistics
# ---------------------------------------------------------------------------
def test_masked_kfac_head_statistics(lib, cuda):
    """B = 24, A = 18, C3 = 32, random per-row masks with actions 15..17 illegal in
    every row: G_pi's rows and columns 15..17 are exactly 0, G_pi and G_v match the
    float64 restatement on the kernel's own draws (its RNG key and float32 inverse CDF
    restated here), the conv / fc blocks oracle.g_factors fed those head gradients."""
    A, C3, B = 18, 32, 24
    seed, row_offset, ctr = 0x4b464143, 48, 40
    net, acts, bwd, ws, obs, t, params, keep = _net(lib, cuda, A, C3, B, seed=9)
    # (the 0.01-gain policy head gives near-uniform rows: scale the logits up in place)
    t['logits'].mul_(200.0)
    rng = np.random.default_rng(51)
    masks, S = random_masks(rng, B, A)
    S[:, 15:] = False
    S[np.arange(B), rng.integers(0, 15, B)] = True
    masks = (S.astype(np.uint64) << np.arange(A, dtype=np.uint64)).sum(1).astype(np.uint32)
    dout, so, tot = _stat_layout(lib, A, C3)
    gstat = _output_stats(net, acts, bwd, ws, B, tot, dev_masks(masks), seed, row_offset, ctr).cpu().double().numpy()
    blocks = [gstat[so[5 + l]:so[5 + l] + dout[l] ** 2].reshape(dout[l], dout[l]) for l in range(6)]
    g_pi_got, g_v_got = blocks[4], blocks[5]
    assert (g_pi_got[15:, :] == 0.0).all() and (g_pi_got[:, 15:] == 0.0).all()
    logits32 = t['logits'].cpu().numpy()
    h = oracle.key4(seed, 0, ctr, np.uint32(row_offset) + np.arange(B, dtype=np.uint32))
    y = sample_masked_f32(logits32, oracle.u01(h), masks)
    assert S[np.arange(B), y].all() and len(np.unique(y)) > 3
    _, _, p, _ = masked_softmax64(logits32, masks)
    g_pi = p - np.eye(A)[y]
    u1 = oracle.u01(oracle.mix32(h ^ np.uint32(0x68e31da4))).astype(np.float64) + 1.0 / 33554432.0
    u2 = oracle.u01(oracle.mix32(h ^ np.uint32(0xb5297a4d))).astype(np.float64)
    g_v = -(np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2))
    full = {k: t[k].cpu().double().numpy() for k in ('a1', 'a2', 'a3', 'a4', 'logits', 'value')}
    full['x'] = obs.cpu().numpy().astype(np.float64) / 255.0
    full['a3f'] = full['a3'].reshape(B, -1)
    gfac = oracle.g_factors(params.cpu().double().numpy(), full, g_pi, g_v, A, C3)
    for l in range(6):
        rel = np.abs(blocks[l] - gfac[l]).max() / np.abs(gfac[l]).max()
        print('G', l, 'rel %.2e' % rel)
        assert rel < 5e-5, ('G', l, rel)


# ---------------------------------------------------------------------------
# 6. through the API
# ---------------------------------------------------------------------------
def _n_legal(games):
    from actorcritic.envs.atari import wrappers
    return np.array([wrappers.ATARI57_ACTIONS[wrappers.game_index(g)] for g in games])


def test_api_masked_rollouts_are_legal_and_fused_equals_unfused(lib, cuda, monkeypatch):
    N, T, A = 8, 5, 18
    games = _games(N)
    nl = _n_legal(games)
    assert nl.min() == 3 and nl.max() == 18
    monkeypatch.delenv('ACMI_ROLLOUT_FUSED', raising=False)
    env, model, agent, _ = _build(N, T, A, games=games, mask_actions=True)
    assert model.action_masks.cpu().tolist() == [(1 << int(n)) - 1 for n in nl]
    fused = _rollouts(agent, model, 3)
    assert agent._bufs.fused
    for r in fused:
        act = r[1].cpu().numpy()
        assert (act >= 0).all() and (act < nl[:, None]).all()
    # (without masks the same policy does leave the legal sets)
    env0, model0, agent0, _ = _build(N, T, A, games=games)
    assert (_rollouts(agent0, model0, 1)[0][1].cpu().numpy() >= nl[:, None]).any()
    monkeypatch.setenv('ACMI_ROLLOUT_FUSED', '0')
    env2, model2, agent2, _ = _build(N, T, A, games=games, mask_actions=True)
    unfused = _rollouts(agent2, model2, 3)
    assert not agent2._bufs.fused
    for a, b in zip(fused, unfused):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    # the sampler restated on the stored logits reproduces the actions
    lg = fused[0][5].cpu().numpy().reshape(N, T, A)
    words = model.action_masks.cpu().numpy()
    for t in range(T):
        u = oracle.sample_uniforms(3, 0, t, N)
        np.testing.assert_array_equal(fused[0][1][:, t].cpu().numpy(), sample_masked_f32(lg[:, t], u, words))


def test_api_entropy_and_log_prob_follow_the_masks(lib, cuda):
    from actorcritic import session as sess
    N, T, A = 8, 5, 18
    env, model, agent, _ = _build(N, T, A, games=_games(N), mask_actions=True)
    with sess.Session() as s:
        data = agent.interact(s)
        ent, lp = s.run([model.policy.entropy, model.policy.log_prob], feed_dict=_feed(model, data))
        logits = model.engine.lookup_rollout(data[0]).flat_logits.cpu().numpy()
    words = np.repeat(model.action_masks.cpu().numpy(), T)
    S, lpr, p, H = masked_softmax64(logits, words)
    act = data[1].cpu().numpy().reshape(-1)
    np.testing.assert_allclose(np.asarray(ent).reshape(-1), H, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(np.asarray(lp).reshape(-1), lpr[np.arange(N * T), act], rtol=1e-5, atol=1e-6)
    # a fed batch of another env count is refused, naming both numbers
    with sess.Session() as s:
        with pytest.raises(ValueError, match=r'8 envs.* 6'):
            s.run(model.policy.entropy, feed_dict={model.observations_placeholder: data[0][:6].clone()})


@pytest.mark.parametrize('acktr', [False, True], ids=['a2c', 'acktr'])
def test_api_updates_leave_illegal_action_gradients_zero(lib, cuda, acktr):
    """All 8 envs on Freeway (3 legal actions) under the 18-action head: after an A2C
    (RMSProp) and an ACKTR (K-FAC, gs = 40: statistics, inverses, step) update the
    gradient entries of W_pi / b_pi for actions 3..17 are exactly 0.0, and so are the
    rows / columns 3..17 of the policy head's G factor."""
    from actorcritic import session as sess
    from actorcritic.examples.atari.a2c_acktr import create_optimizer
    from actorcritic.nn import linear_decay
    from actorcritic.objectives import A2CObjective
    N, T, A, C3 = 8, 5, 18, 32
    env, model, agent, _ = _build(N, T, A, C3, games=['Freeway'] * N, mask_actions=True)
    obj = A2CObjective(model)
    gs = sess.get_or_create_global_step()
    opt = create_optimizer(acktr, model, linear_decay(0.25, 0.025, gs, 1000) if acktr else 7e-4)
    op = obj.optimize_shared(opt, 0.5, global_step=gs)
    gs.assign(40)
    with sess.Session() as s:
        data = agent.interact(s)
        before = model.params.clone()
        pl, ent = s.run([op, obj.policy_loss, obj.mean_entropy], feed_dict=_feed(model, data))[1:]
        torch.cuda.synchronize()
        model.engine.check_bad_rows()  # no bad rows: the actions were drawn under the same masks
    assert (data[1] < 3).all()
    assert np.isfinite(float(pl)) and 0.0 < float(ent) <= np.log(3.0) + 1e-6
    eng = model.engine
    L = eng.layout
    grads = eng.update_state(N * T).grads
    w_pi = grads[L.offsets[8]:L.offsets[9]].view(512, A)
    b_pi = grads[L.offsets[9]:L.offsets[10]]
    assert (w_pi[:, 3:] == 0.0).all() and (b_pi[3:] == 0.0).all()
    assert w_pi[:, :3].abs().max() > 0 and b_pi[:3].abs().max() > 0
    assert torch.isfinite(model.params).all() and not torch.equal(before, model.params)
    if acktr:
        fac = opt.state['factors']
        g_pi = fac[L.stat_off[5 + 4]:L.stat_off[5 + 4] + A * A].view(A, A)
        assert (g_pi[3:, :] == 0.0).all() and (g_pi[:, 3:] == 0.0).all() and g_pi[:3, :3].abs().max() > 0


def test_api_ppo_rows_identity_equals_env_slices_with_masks(lib, cuda, monkeypatch):
    from actorcritic import objectives
    from actorcritic import session as sess
    from actorcritic.nn import ClipGlobalNormOptimizer, RMSPropOptimizer
    N, T, A, epochs, nmb = 8, 5, 18, 2, 2
    env, model, agent, _ = _build(N, T, A, 64, games=_games(N), mask_actions=True)
    gs = sess.get_or_create_global_step()
    obj = objectives.PPOObjective(model)
    monkeypatch.setattr(objectives, 'ppo_row_order',
                        lambda seed, step, e, M: [np.arange(M, dtype=np.int32) for _ in range(e)])
    monkeypatch.setattr(objectives, 'ppo_minibatch_order',
                        lambda seed, step, e, n: [list(range(n)) for _ in range(e)])
    scalars = ('policy_loss', 'baseline_loss', 'mean_entropy', 'approx_kl', 'clip_fraction')
    got = {}
    with sess.Session() as s:
        data = _clone(agent.interact(s))
        p0 = model.params.clone()
        for mode in ('envs', 'rows'):
            model.params.copy_(p0)
            model.engine.bump_version()
            opt = ClipGlobalNormOptimizer(RMSPropOptimizer(learning_rate=7e-4), clip_norm=0.5)
            op = obj.optimize_shared(opt, 0.5, num_epochs=epochs, num_minibatches=nmb, shuffle_seed=3,
                                     global_step=gs, minibatch=mode)
            out = s.run([op] + [getattr(obj, n) for n in scalars], feed_dict=_feed(model, data))
            torch.cuda.synchronize()
            model.engine.check_bad_rows()
            got[mode] = (model.params.clone(), [torch.as_tensor(x).cpu() for x in out[1:]])
    assert not torch.equal(got['envs'][0], p0)
    assert torch.equal(got['rows'][0], got['envs'][0])
    for name, a, b in zip(scalars, got['envs'][1], got['rows'][1]):
        assert torch.equal(a, b), name
        assert torch.isfinite(a).all(), name


def test_api_without_masks_the_rollout_is_the_unmasked_one(lib, cuda, monkeypatch):
    """mask_actions=False (the default): the agent's rollout is what the unmasked
    entry points give when called directly -- acmi_sample_actions_at on the stored
    logits and acmi_env_step of a twin env reproduce actions, observations, rewards and
    terminals bit for bit."""
    from actorcritic.envs.atari.wrappers import SyntheticAtariEnvs
    monkeypatch.delenv('ACMI_ROLLOUT_FUSED', raising=False)
    N, T, A = 8, 5, 18
    games = _games(N)
    env, model, agent, _ = _build(N, T, A, games=games, mask_actions=False)
    assert model.engine.masks is None and env.batched.legal_action_masks is not None
    obs, act, rew, term, nxt, logits = _rollouts(agent, model, 1)[0]
    twin = SyntheticAtariEnvs(N, num_actions=A, seed=5, games=games)
    cur = torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=cuda)
    twin.reset_into(cur.data_ptr())
    lg = logits.view(N, T, A)
    bad = torch.zeros(1, dtype=torch.int32, device=cuda)
    for t in range(T):
        assert torch.equal(cur, obs[:, t])
        a_t = torch.zeros(N, dtype=torch.int32, device=cuda)
        l_t = lg[:, t].contiguous()
        _lib.call('acmi_sample_actions_at', _lib.ptr(l_t), A, N, A, 3, 0, t, 0, None, 0, _lib.ptr(a_t), _lib.ptr(bad),
                  _lib.stream_handle())
        assert torch.equal(a_t, act[:, t])
        out = torch.zeros_like(cur)
        r, d, ep = (torch.zeros(N, device=cuda), torch.zeros(N, dtype=torch.uint8, device=cuda),
                    torch.zeros(N, device=cuda))
        twin.step_into(a_t.data_ptr(), cur.data_ptr(), 84 * 84 * 4, out.data_ptr(), 84 * 84 * 4, r.data_ptr(),
                       d.data_ptr(), ep.data_ptr(), 1)
        assert torch.equal(r, rew[:, t]) and torch.equal(d.bool(), term[:, t].bool())
        cur = out
    assert torch.equal(cur, nxt) and int(bad.item()) == 0


def test_api_mask_actions_needs_masks(lib, cuda):
    with pytest.raises(ValueError, match='legal_action_masks'):
        _build(4, 3, 4, games=None, mask_actions=True)


# ---------------------------------------------------------------------------
# 7. the host-stepped path
# ---------------------------------------------------------------------------
def _raw_chain(seed, A):
    from actorcritic import spaces
    from actorcritic.envs.atari import wrappers

    class ALE(oracle.FakeALE):
        action_space = spaces.Discrete(A)
        observation_space = spaces.Box(low=0, high=255, shape=(210, 160, 3), dtype=np.uint8)

    return wrappers.wrap_atari_env(ALE(seed), preprocess=False)


def test_host_stepped_rollout_draws_from_the_legal_set(lib, cuda):
    from actorcritic import session as sess
    from actorcritic.agents import MultiEnvAgent
    from actorcritic.envs.atari.model import AtariModel
    from actorcritic.envs.atari.wrappers import HostAtariEnvs, action_mask_bits
    from actorcritic.multi_env import MultiEnv
    N, T, A, C3 = 4, 4, 18, 32
    legal = [0, 1, 3, 4]
    sess.reset_default_graph()
    benv = HostAtariEnvs([_raw_chain(100 + i, A) for i in range(N)], legal_actions=[legal] * N)
    assert benv.legal_action_masks.cpu().tolist() == [action_mask_bits(legal, A)] * N
    env = MultiEnv(benv)
    params = oracle.init_params(A, C3, seed=1)
    off, _ = oracle.param_offsets(A, C3)
    params[off[8]:off[9]] *= 60.0
    model = AtariModel(env.observation_space, env.action_space, C3, params=params, random_seed=3)
    agent = MultiEnvAgent(env, model, T, mask_actions=True)
    seen = []
    step = benv.host_step
    benv.host_step = lambda actions: (seen.append(np.array(actions)), step(actions))[1]
    try:
        with sess.Session() as s:
            data = agent.interact(s)
            logits = model.engine.lookup_rollout(data[0]).flat_logits.cpu().numpy().reshape(N, T, A)
    finally:
        env.close()
    assert len(seen) == T and all(set(a.tolist()) <= set(legal) for a in seen)
    act = data[1].cpu().numpy()
    np.testing.assert_array_equal(act, np.stack(seen, 1))
    words = np.full(N, action_mask_bits(legal, A), np.uint32)
    for t in range(T):
        u = oracle.sample_uniforms(3, 0, t, N)
        np.testing.assert_array_equal(act[:, t], sample_masked_f32(logits[:, t], u, words))
    assert len(np.unique(act)) > 1
