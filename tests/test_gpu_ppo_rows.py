"""GPU tests of PPO's per-row shuffled minibatches: the row gather kernel
(acmi_gather_rows -- a copy, so every comparison is torch.equal against torch indexing)
and the update op in ``minibatch='rows'`` mode (bit-identity with the env slices under the
identity permutation, float64 parity step by step with test_gpu_ppo.py's bound,
divisibility, checkpoint resume)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from actorcritic import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import oracle  # noqa: E402
from test_gpu_ppo import F32_EPS, _build, _feed, _rmsprop, ppo_ref  # noqa: E402

pytestmark = pytest.mark.gpu

OBS_BYTES = 84 * 84 * 4
ERR_ARG = -1  # ACMI_ERR_ARG


def _addr(x):
    if x is None or isinstance(x, ctypes.c_void_p):
        return x
    if isinstance(x, torch.Tensor):
        return ctypes.c_void_p(x.data_ptr())
    return ctypes.c_void_p(int(x))


def gather(lib, obs, img_stride, src_rows, index, obs_out, out_stride, vec_src=(), vec_dst=(), bad=None):
    """acmi_gather_rows' status; obs / obs_out: tensors, raw addresses or None."""
    n = len(vec_src)
    src = (ctypes.c_void_p * max(n, 1))(*[v.data_ptr() for v in vec_src])
    dst = (ctypes.c_void_p * max(n, 1))(*[v.data_ptr() for v in vec_dst])
    rc = lib.acmi_gather_rows(_addr(obs), img_stride, src_rows, _addr(index), index.numel(), _addr(obs_out),
                              out_stride, n, src, dst, _addr(bad), _lib.stream_handle())
    torch.cuda.synchronize()
    return rc


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _vectors(src_rows, gen, cuda):
    """Five 4-byte row vectors, int32 and float32 mixed, NaN and -0.0 among the floats."""
    f = [torch.randn(src_rows, generator=gen).to(cuda) for _ in range(3)]
    f[0][0], f[1][0] = float('nan'), -0.0
    f[2][src_rows - 1] = float('nan')
    f[0][src_rows - 1] = -0.0
    i = [torch.randint(-2 ** 31, 2 ** 31 - 1, (src_rows,), generator=gen, dtype=torch.int64).to(torch.int32).to(cuda)
         for _ in range(2)]
    return [i[0], f[0], f[1], i[1], f[2]]


@pytest.mark.parametrize('src_rows,rows', [(7, 7), (50, 37), (5, 1)])
def test_gather_rows_plain(lib, cuda, src_rows, rows):
    gen = torch.Generator().manual_seed(100 + src_rows)
    obs = torch.randint(0, 256, (src_rows, 84, 84, 4), generator=gen, dtype=torch.uint8).to(cuda)
    if rows == src_rows:
        idx = torch.randperm(src_rows, generator=gen)
    else:
        idx = torch.randint(0, src_rows, (rows,), generator=gen)
        idx[-1] = src_rows - 1
        if rows > 2:
            idx[1] = idx[0]  # (a duplicate for certain) and the first / last source rows
            idx[2] = 0
            assert len(set(idx.tolist())) < rows
    index = idx.to(torch.int32).to(cuda)
    lidx = idx.to(cuda)
    vs = _vectors(src_rows, gen, cuda)

    def fresh():
        return torch.full((rows, 84, 84, 4), 0xAB, dtype=torch.uint8, device=cuda), \
            [torch.full((rows,), 7, dtype=v.dtype, device=cuda) for v in vs]

    out, vd = fresh()
    assert gather(lib, obs, OBS_BYTES, src_rows, index, out, OBS_BYTES, vs, vd) == 0
    assert torch.equal(out, obs[lidx])
    for s, d in zip(vs, vd):
        assert torch.equal(_bits(d), _bits(s)[lidx])
    # no vectors
    out, vd = fresh()
    assert gather(lib, obs, OBS_BYTES, src_rows, index, out, OBS_BYTES) == 0
    assert torch.equal(out, obs[lidx])
    # vectors only
    out, vd = fresh()
    assert gather(lib, None, 0, src_rows, index, None, 0, vs, vd) == 0
    assert bool((out == 0xAB).all())
    for s, d in zip(vs, vd):
        assert torch.equal(_bits(d), _bits(s)[lidx])


def test_gather_rows_strides_and_padding(lib, cuda):
    """Source: step t = 1 of an [N = 6][T = 3] buffer; output rows 16 bytes apart more than
    an image: the pad bytes and everything past the last row keep the guard byte."""
    gen = torch.Generator().manual_seed(7)
    N, T, GUARD = 6, 3, 0xAB
    buf = torch.randint(0, 256, (N, T, 84, 84, 4), generator=gen, dtype=torch.uint8).to(cuda)
    vec = torch.randn(N, generator=gen).to(cuda)
    idx = torch.tensor([5, 0, 3, 3, 1])
    rows, stride, tail = idx.numel(), OBS_BYTES + 16, 4096
    out = torch.full((rows * stride + tail,), GUARD, dtype=torch.uint8, device=cuda)
    vd = torch.zeros(rows, device=cuda)
    rc = gather(lib, buf.data_ptr() + OBS_BYTES, T * OBS_BYTES, N, idx.to(torch.int32).to(cuda), out, stride, [vec],
                [vd])
    assert rc == 0
    body = out[:rows * stride].view(rows, stride)
    assert torch.equal(body[:, :OBS_BYTES], buf[idx.to(cuda), 1].reshape(rows, OBS_BYTES))
    assert bool((body[:, OBS_BYTES:] == GUARD).all())
    assert bool((out[rows * stride:] == GUARD).all())
    assert torch.equal(_bits(vd), _bits(vec)[idx.to(cuda)])


def test_gather_rows_bad_indices_are_zero_filled_and_counted(lib, cuda):
    gen = torch.Generator().manual_seed(8)
    src_rows = 4
    obs = torch.randint(1, 256, (src_rows, 84, 84, 4), generator=gen, dtype=torch.uint8).to(cuda)
    vs = [torch.arange(1, src_rows + 1, dtype=torch.int32, device=cuda),
          torch.arange(1, src_rows + 1, dtype=torch.float32, device=cuda)]
    idx = [2, -1, 0, src_rows, 1]
    index = torch.tensor(idx, dtype=torch.int32, device=cuda)
    good = [r for r, i in enumerate(idx) if 0 <= i < src_rows]
    results = []
    for counted in (True, False):
        bad = torch.tensor([5], dtype=torch.int32, device=cuda) if counted else None
        out = torch.full((len(idx), 84, 84, 4), 0xCD, dtype=torch.uint8, device=cuda)
        vd = [torch.full((len(idx),), 7, dtype=v.dtype, device=cuda) for v in vs]
        assert gather(lib, obs, OBS_BYTES, src_rows, index, out, OBS_BYTES, vs, vd, bad) == 0
        for r in (1, 3):
            assert not bool(out[r].any())
            assert all(int(_bits(d)[r]) == 0 for d in vd)
        for r in good:
            assert torch.equal(out[r], obs[idx[r]])
            assert all(torch.equal(_bits(d)[r], _bits(s)[idx[r]]) for s, d in zip(vs, vd))
        if counted:
            assert int(bad) == 5 + 2
        results.append((out, vd))
    assert torch.equal(results[0][0], results[1][0])
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(results[0][1], results[1][1]))


def test_gather_rows_offsets_are_64_bit(lib, cuda):
    """A 4.3 GB source (allocated, never filled): rows whose byte offsets pass 2^31 and 2^32."""
    gen = torch.Generator().manual_seed(9)
    src_rows, picks = 152400, [152300, 0, 76100]
    assert picks[2] * OBS_BYTES > 2 ** 31 and picks[0] * OBS_BYTES > 2 ** 32
    src = torch.empty(src_rows * OBS_BYTES, dtype=torch.uint8, device=cuda).view(src_rows, OBS_BYTES)
    vec = torch.empty(src_rows, dtype=torch.int32, device=cuda)
    known = torch.randint(0, 256, (3, OBS_BYTES), generator=gen, dtype=torch.uint8).to(cuda)
    for k, i in enumerate(picks):
        src[i] = known[k]
        vec[i] = 1000 + k
    out = torch.zeros(3, OBS_BYTES, dtype=torch.uint8, device=cuda)
    vd = torch.zeros(3, dtype=torch.int32, device=cuda)
    index = torch.tensor(picks, dtype=torch.int32, device=cuda)
    assert gather(lib, src, OBS_BYTES, src_rows, index, out, OBS_BYTES, [vec], [vd]) == 0
    assert torch.equal(out, known)
    assert vd.tolist() == [1000, 1001, 1002]


def test_gather_rows_refuses_a_misaligned_image_pointer(lib, cuda):
    obs = torch.zeros(3 * OBS_BYTES + 16, dtype=torch.uint8, device=cuda)
    out = torch.full((2 * OBS_BYTES + 16,), 0xAB, dtype=torch.uint8, device=cuda)
    index = torch.tensor([1, 0], dtype=torch.int32, device=cuda)
    assert gather(lib, obs.data_ptr() + 4, OBS_BYTES, 3, index, out, OBS_BYTES) == ERR_ARG
    assert gather(lib, obs, OBS_BYTES, 3, index, out.data_ptr() + 4, OBS_BYTES) == ERR_ARG
    assert b'aligned' in lib.acmi_last_error()
    assert bool((out == 0xAB).all())  # (nothing was enqueued)


# ---------------------------------------------------------------------------
# the update op with minibatch='rows'
# ---------------------------------------------------------------------------
SCALARS = ('policy_loss', 'baseline_loss', 'mean_entropy', 'approx_kl', 'clip_fraction')


def _clone(data):
    return tuple(x.clone() if isinstance(x, torch.Tensor) else x for x in data)


def test_identity_permutation_equals_env_slices_bit_for_bit(lib, cuda, monkeypatch):
    from actorcritic import objectives
    from actorcritic import session as sess
    N, T, epochs, nmb = 4, 5, 2, 2
    env, model, agent, gs, params = _build(N, T, 4, 64)
    obj = objectives.PPOObjective(model)
    monkeypatch.setattr(objectives, 'ppo_row_order',
                        lambda seed, step, e, M: [np.arange(M, dtype=np.int32) for _ in range(e)])
    monkeypatch.setattr(objectives, 'ppo_minibatch_order',
                        lambda seed, step, e, n: [list(range(n)) for _ in range(e)])
    got = {}
    with sess.Session() as s:
        data = _clone(agent.interact(s))
        p0 = model.params.clone()
        for mode in ('envs', 'rows'):
            model.params.copy_(p0)
            model.engine.bump_version()
            op = obj.optimize_shared(_rmsprop(), 0.5, num_epochs=epochs, num_minibatches=nmb, shuffle_seed=3,
                                     global_step=gs, minibatch=mode)
            out = s.run([op] + [getattr(obj, n) for n in SCALARS], feed_dict=_feed(model, data))
            torch.cuda.synchronize()
            got[mode] = (model.params.clone(), [torch.as_tensor(x).cpu() for x in out[1:]], op)
    assert got['envs'][2].last_order == [[0, 1]] * epochs and got['envs'][2].last_rows is None
    assert got['rows'][2].last_order is None and len(got['rows'][2].last_rows) == epochs
    assert not torch.equal(got['envs'][0], p0)
    assert torch.equal(got['rows'][0], got['envs'][0])
    for name, a, b in zip(SCALARS, got['envs'][1], got['rows'][1]):
        assert torch.equal(a, b), name


FWD_RTOL = 1e-5  # the f32 forward against float64 (test_gpu_parity.py's forward tolerance)


def _take_undetermined_gates(part, gpu_acts):
    """A ReLU whose pre-activation lies within the f32 forward's error of zero has no
    determined gate: float64 and the GPU may fall on different sides, and a whole term of
    the gradient with it (met here at one conv3 unit: pre-activation 1.5e-7 in float64,
    0 on the GPU, which moved 47 conv parameters past the bound).  As in
    test_gpu_parity.py / test_gpu_bench_shard.py the float64 backward takes the GPU's gate
    -- here at those units only: the forward must agree with float64 within FWD_RTOL of
    the layer's largest activation, so a unit whose gates differ is within that of zero on
    both sides.  Everything else in ``part`` stays float64.  Returns the number taken."""
    taken = 0
    for name, g in zip(('a1', 'a2', 'a3', 'a4'), gpu_acts):
        a = part[name]
        g = g.cpu().double().numpy().reshape(a.shape)
        tol = FWD_RTOL * np.abs(a).max()
        assert np.abs(g - a).max() <= tol, ('forward', name, float(np.abs(g - a).max()), tol)
        differ = (g > 0) != (a > 0)
        assert np.all(a[differ] <= tol) and np.all(g[differ] <= tol)
        a[differ] = np.where(g[differ] > 0, np.finfo(np.float64).tiny, 0.0)
        taken += int(differ.sum())
    part['a3f'] = part['a3'].reshape(part['a3'].shape[0], -1)
    return taken


@pytest.mark.parametrize('normalize', [True, 'minibatch'], ids=['batch-norm', 'minibatch-norm'])
def test_rows_update_matches_oracle_step_by_step(lib, cuda, normalize):
    """test_ppo_update_matches_oracle_step_by_step with shuffled row minibatches: 2 epochs x 2
    minibatches of 10 of the 4 x 5 batch's 20 rows, clip-wrapped RMSProp; every step, started
    from the GPU's parameters before it, against the float64 step on obs[idx] within that
    test's per-element bound 1e-3 |delta| + 2 eps32 |p| + 1e-12.  'minibatch': the float64
    side normalises adv[idx] per step (the batch's advantages stay unnormalised).  ReLU units
    on the kink: _take_undetermined_gates."""
    from actorcritic import session as sess
    from actorcritic.objectives import PPOObjective, ppo_row_order
    N, T, A, C3, epochs, nmb, seed = 4, 5, 4, 64, 2, 2, 9
    M = N * T
    env, model, agent, gs, params = _build(N, T, A, C3)
    obj = PPOObjective(model, normalize_advantages=normalize)
    snaps, calls, fwds = [], [], []

    def callback(epoch, pos):
        calls.append((epoch, pos))
        snaps.append(model.params.clone())
        acts = model.engine.activations(M // nmb, 'ppo')  # the step's forward
        fwds.append([a.clone() for a in (acts.a1, acts.a2, acts.a3, acts.a4)])

    op = obj.optimize_shared(_rmsprop(), 0.5, num_epochs=epochs, num_minibatches=nmb, shuffle_seed=seed,
                             step_callback=callback, global_step=gs, minibatch='rows')
    with sess.Session() as s:
        data = agent.interact(s)
        assert model.engine.lookup_rollout(data[0]) is not None
        snaps.append(model.params.clone())
        step0 = gs.value
        out = s.run([op] + [getattr(obj, n) for n in SCALARS], feed_dict=_feed(model, data))
    assert gs.value == step0 + 1
    assert calls == [(e, k) for e in range(epochs) for k in range(nmb)]
    assert op.last_order is None and len(op.last_rows) == epochs
    want = ppo_row_order(seed, step0, epochs, M)
    for a, b in zip(op.last_rows, want):
        assert a.dtype == np.int32 and np.array_equal(a, b)
    rows = M // nmb
    steps = [perm[k * rows:(k + 1) * rows] for perm in op.last_rows for k in range(nmb)]

    def env_range(idx):
        lo = int(idx.min())
        return lo % T == 0 and np.array_equal(np.sort(idx), np.arange(lo, lo + len(idx)))

    assert not all(env_range(idx) for idx in steps)

    obs, act, rew, term, nxt, _ = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in data)
    obs, act = obs.reshape(-1, 84, 84, 4), act.reshape(-1)
    p0 = snaps[0].cpu().numpy().astype(np.float64)
    full = oracle.forward(p0, obs, A, C3)
    vb = oracle.forward(p0, nxt, A, C3)['value']
    tg, adv = oracle.gae_f64(rew, term, full['value'].reshape(N, T), vb, 0.99, 0.95)
    tg, adv = tg.reshape(-1), adv.reshape(-1)
    if normalize is True:
        adv = oracle.normalize_advantages(adv)
    old_logp = oracle.log_softmax(full['logits'])[np.arange(M), act]
    old_values = full['value']
    ms, mom = np.ones_like(p0), np.zeros_like(p0)
    last = None
    for k, idx in enumerate(steps):
        idx = idx.astype(np.int64)
        pb = snaps[k].cpu().numpy().astype(np.float64)
        got = snaps[k + 1].cpu().numpy().astype(np.float64)
        part = oracle.forward(pb, obs[idx], A, C3)
        print('step', k, 'gates taken from the GPU forward:', _take_undetermined_gates(part, fwds[k]))
        ad = oracle.normalize_advantages(adv[idx]) if normalize == 'minibatch' else adv[idx]
        last = ppo_ref(part['logits'], part['value'], act[idx], old_logp[idx], old_values[idx], tg[idx], ad, 0.1, 0.0)
        grads, _ = oracle.backward(pb, part, last['dlogits'], last['dvalue'], A, C3)
        rp, ms, mom = oracle.rmsprop_apply(pb, ms, mom, grads, 7e-4, 0.5)
        bound = 1e-3 * np.abs(rp - pb) + 2 * F32_EPS * np.abs(pb) + 1e-12
        err = np.abs(got - rp)
        print('step', k, 'rows', idx.tolist(), 'max err/bound', float((err / bound).max()), 'max |r-1|',
              float(np.abs(last['r'] - 1).max()))
        over = np.flatnonzero(err > bound)
        if over.size:  # where: the parameter blocks (oracle.param_offsets) and the worst elements
            off, _ = oracle.param_offsets(A, C3)
            print('  over the bound:', over.size, 'by block', np.bincount(np.searchsorted(off, over, 'right') - 1,
                                                                          minlength=len(off)).tolist())
            for i in over[np.argsort(-(err / bound)[over])[:5]]:
                print('  element', int(i), 'p', pb[i], 'delta f64', rp[i] - pb[i], 'delta gpu', got[i] - pb[i])
        assert np.all(err <= bound), 'gradient step {}'.format(k)
    assert len(steps) == epochs * nmb == len(snaps) - 1
    # the fetched scalars are the last gradient step's
    print('scalars', [float(x) for x in out[1:]], [float(last[n]) for n in ('policy_loss', 'baseline_loss',
                                                                             'mean_entropy', 'approx_kl', 'clip_frac')])
    assert out[1] == pytest.approx(last['policy_loss'], rel=1e-4, abs=1e-6)
    assert out[2] == pytest.approx(last['baseline_loss'], rel=1e-4)
    assert out[3] == pytest.approx(last['mean_entropy'], rel=1e-5)
    assert out[4] == pytest.approx(last['approx_kl'], rel=1e-2, abs=1e-6)
    assert out[5] == pytest.approx(last['clip_frac'], abs=1e-7)


def test_rows_minibatches_must_divide_the_rows_not_the_envs(lib, cuda):
    from actorcritic import session as sess
    from actorcritic.objectives import PPOObjective
    env, model, agent, gs, params = _build(4, 5, 4, 64)
    obj = PPOObjective(model)

    def run(s, data, nmb, mode):
        op = obj.optimize_shared(_rmsprop(), 0.5, num_epochs=1, num_minibatches=nmb, global_step=gs, minibatch=mode)
        s.run(op, feed_dict=_feed(model, data))
        return op

    with sess.Session() as s:
        data = _clone(agent.interact(s))
        before = model.params.clone()
        op = run(s, data, 5, 'rows')  # 5 divides 20 rows
        torch.cuda.synchronize()
        assert not torch.equal(model.params, before) and op.last_rows[0].shape == (20,)
        with pytest.raises(ValueError):
            run(s, data, 5, 'envs')  # ... but not 4 envs
        for mode in ('rows', 'envs'):
            with pytest.raises(ValueError):
                run(s, data, 3, mode)


def test_rows_adam_resume_is_bit_identical(lib, cuda, tmp_path):
    """test_ppo_adam_resume_is_bit_identical with minibatch='rows': the restored global step
    also seeds the row permutations."""
    from actorcritic import checkpoint
    from actorcritic import session as sess
    from actorcritic.examples.atari.ppo import create_optimizer
    from actorcritic.objectives import PPOObjective

    def graph():
        env, model, agent, gs, params = _build()
        opt = create_optimizer(2.5e-4)
        op = PPOObjective(model, value_clip_range=0.2).optimize_shared(
            opt, 0.5, num_epochs=2, num_minibatches=2, shuffle_seed=4, global_step=gs, minibatch='rows')
        return model, agent, gs, opt, op, params

    model, agent, gs, opt, op, params = graph()
    with sess.Session() as s:
        s.run(op, feed_dict=_feed(model, agent.interact(s)))
        first = [p.copy() for p in op.last_rows]
        data = _clone(agent.interact(s))
        path = checkpoint.save(str(tmp_path / 'Atari'), gs.value, model, opt)
        saved = {k: v.clone() for k, v in opt.slots().items()}
        s.run(op, feed_dict=_feed(model, data))
    torch.cuda.synchronize()
    uninterrupted, gs_after, order = model.params.clone(), gs.value, op.last_rows
    assert int(saved['_t'][0]) == 4 and int(opt.slots()['_t'][0]) == 8
    assert not all(np.array_equal(a, b) for a, b in zip(first, order))  # (the step seeds the order)

    model2, agent2, gs2, opt2, op2, _ = graph()
    checkpoint.load(path, model2, opt2, gs2)
    for k, v in opt2.slots().items():
        assert torch.equal(v.cpu(), saved[k].cpu()), k
    with sess.Session() as s:
        s.run(op2, feed_dict=_feed(model2, data))
    torch.cuda.synchronize()
    assert gs2.value == gs_after
    assert all(np.array_equal(a, b) for a, b in zip(op2.last_rows, order))
    assert not torch.equal(model2.params, torch.from_numpy(params).cuda())
    assert torch.equal(model2.params, uninterrupted)
