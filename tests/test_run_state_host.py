"""Run-state checkpoints on the CPU (no GPU, no kernels): the file name, the return
normaliser's carry beside its state_dict, the model checkpoint's unchanged key set, and
the rank / world-size checks of a run-state file.  The bit-for-bit
continuation itself needs the device: tests/test_gpu_run_state.py."""
import types

import pytest
import torch

from actorcritic import checkpoint
from actorcritic._engine import Layout
from actorcritic.nn import ClipGlobalNormOptimizer, RMSPropOptimizer
from actorcritic.return_norm import ReturnNormalizer


def _model(A=4, C3=64, seed=1):
    eng = types.SimpleNamespace(device=torch.device('cpu'), layout=Layout(A, C3), version=0)
    eng.bump_version = lambda: setattr(eng, 'version', eng.version + 1)
    eng.params = torch.randn(eng.layout.nparams, generator=torch.Generator().manual_seed(seed))
    return types.SimpleNamespace(params=eng.params, num_actions=A, conv3_num_filters=C3, engine=eng)


def _objective(norm):
    return types.SimpleNamespace(return_normalizer=norm)


class _Agent(object):
    """What checkpoint.save_run_state / load_run_state touch of a MultiEnvAgent."""

    def __init__(self, N=3):
        g = torch.Generator().manual_seed(N)
        self.state = {'next_obs': torch.randint(0, 256, (N, 84, 84, 4), generator=g, dtype=torch.uint8),
                      'sample_counter': 12,
                      'env': {'kind': 2, 'num_envs': N, 'step': torch.arange(N, dtype=torch.int32)}}
        self.loaded = None

    def run_state(self):
        return self.state

    def load_run_state(self, state):
        self.loaded = state


def test_run_state_path_formats_the_name():
    assert checkpoint.run_state_path('/tmp/x/Atari-Catch', 1200, 3) == '/tmp/x/Atari-Catch-1200.run3.pt'
    assert checkpoint.run_state_path('m', torch.tensor(7), 0) == 'm-7.run0.pt'


def test_carry_round_trip_and_shape_check():
    a = ReturnNormalizer([0, 1, 0, 1, 1])
    a.carry.copy_(torch.tensor([0.5, -1.25, 3.0, 0.0, 7.75]))
    saved = a.carry_state()
    assert saved.dtype == torch.float32 and saved.device.type == 'cpu' and tuple(saved.shape) == (5,)
    a.carry.zero_()  # (a copy: what was saved does not follow the normaliser)
    assert saved.tolist() == [0.5, -1.25, 3.0, 0.0, 7.75]
    b = ReturnNormalizer([0, 1, 0, 1, 1])
    b.load_carry(saved)
    assert torch.equal(b.carry, saved)
    for wrong in (saved[:4], saved[None], torch.zeros(6), saved.double()):
        with pytest.raises(ValueError):
            b.load_carry(wrong)
    assert torch.equal(b.carry, saved)
    assert set(a.state_dict()) == {'stats', 'num_groups', 'epsilon', 'clip', 'group_names'}


def test_model_checkpoint_zeroes_the_carry_and_load_carry_after_it_stays(tmp_path):
    norm = ReturnNormalizer([0, 1, 1], num_groups=2)
    norm.stats.copy_(torch.tensor([[4.0, 0.5, 2.0], [9.0, -1.0, 3.0]], dtype=torch.float64))
    norm.carry.copy_(torch.tensor([1.5, -2.0, 0.25]))
    carry = norm.carry_state()
    model = _model()
    path = checkpoint.save(str(tmp_path / 'm'), 3, model, None, objective=_objective(norm))

    fresh = ReturnNormalizer([0, 1, 1], num_groups=2)
    fresh.carry.fill_(9.0)
    fresh.load_state_dict(norm.state_dict())
    assert not fresh.carry.any()  # load_state_dict alone still zeroes it

    fresh.carry.fill_(9.0)
    checkpoint.load(path, _model(seed=2), objective=_objective(fresh))
    assert not fresh.carry.any()
    fresh.load_carry(carry)  # model checkpoint first, run state second
    assert torch.equal(fresh.carry, carry) and torch.equal(fresh.stats, norm.stats)


def test_model_checkpoint_keys_are_unchanged(tmp_path):
    model = _model()
    opt = ClipGlobalNormOptimizer(RMSPropOptimizer(learning_rate=7e-4), clip_norm=0.5)
    opt._optimizer._ms, opt._optimizer._mom = torch.ones(5), torch.zeros(5)
    norm = ReturnNormalizer([0, 0], num_groups=1)
    plain = checkpoint.save(str(tmp_path / 'a'), 1, model, opt)
    assert set(torch.load(plain, weights_only=True)) == {'params', 'global_step', 'num_actions', 'conv3_filters',
                                                         'opt/_ms', 'opt/_mom'}
    with_norm = checkpoint.save(str(tmp_path / 'b'), 2, model, opt, objective=_objective(norm))
    assert set(torch.load(with_norm, weights_only=True)) == {
        'params', 'global_step', 'num_actions', 'conv3_filters', 'opt/_ms', 'opt/_mom', 'retnorm/stats',
        'retnorm/epsilon', 'retnorm/clip'}
    # a run state beside it touches neither the model checkpoint nor the index
    before = (tmp_path / 'b-2.pt').read_bytes(), (tmp_path / 'checkpoint').read_bytes()
    norm.carry.copy_(torch.tensor([0.5, 1.5]))
    rs = checkpoint.save_run_state(str(tmp_path / 'b'), 2, _Agent(2), _objective(norm))
    assert rs == str(tmp_path / 'b-2.run0.pt')
    assert before == ((tmp_path / 'b-2.pt').read_bytes(), (tmp_path / 'checkpoint').read_bytes())
    assert sorted(p.name for p in tmp_path.iterdir()) == ['a-1.pt', 'b-2.pt', 'b-2.run0.pt', 'checkpoint']
    blob = torch.load(rs, weights_only=True)
    assert (blob['format'], blob['rank'], blob['world_size'], blob['global_step']) == (1, 0, 1, 2)
    assert all(type(blob[k]) is int for k in ('format', 'rank', 'world_size', 'global_step', 'sample_counter'))
    assert torch.equal(blob['retnorm/carry'], torch.tensor([0.5, 1.5]))


def _blob(**over):
    agent = _Agent()
    blob = dict(format=checkpoint.RUN_STATE_FORMAT, rank=0, world_size=1, global_step=40, **agent.state)
    blob['retnorm/carry'] = torch.tensor([1.0, 2.0, 3.0])
    blob.update(over)
    return blob


def test_hand_made_run_state_loads_and_wrong_rank_or_world_size_raises(tmp_path):
    path = str(tmp_path / 'm-40.run0.pt')
    torch.save(_blob(), path)
    assert set(torch.load(path, weights_only=True)) == {'format', 'rank', 'world_size', 'global_step', 'next_obs',
                                                        'sample_counter', 'env', 'retnorm/carry'}
    agent, norm = _Agent(), ReturnNormalizer([0, 0, 0])
    blob = checkpoint.load_run_state(path, agent, _objective(norm))
    assert int(blob['global_step']) == 40
    assert set(agent.loaded) == {'next_obs', 'sample_counter', 'env'}
    assert torch.equal(agent.loaded['next_obs'], _Agent().state['next_obs']) and agent.loaded['sample_counter'] == 12
    assert torch.equal(agent.loaded['env']['step'], torch.arange(3, dtype=torch.int32))
    assert norm.carry.tolist() == [1.0, 2.0, 3.0]
    # without a normaliser the carry is left alone
    checkpoint.load_run_state(path, _Agent())

    for field, value in (('rank', 1), ('world_size', 2), ('format', 99)):
        torch.save(_blob(**{field: value}), path)
        agent = _Agent()
        with pytest.raises(ValueError, match=field.replace('_', '.')):
            checkpoint.load_run_state(path, agent)
        assert agent.loaded is None  # refused before anything was loaded
    # a normaliser needs its carry: never a silent reset
    blob = _blob()
    del blob['retnorm/carry']
    torch.save(blob, path)
    agent = _Agent()
    with pytest.raises(ValueError, match='carry'):
        checkpoint.load_run_state(path, agent, _objective(ReturnNormalizer([0, 0, 0])))
    assert agent.loaded is None
