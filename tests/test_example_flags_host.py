"""The command line the two Atari examples share (examples/atari/loop.py)."""
import inspect
import os

from actorcritic.examples.atari import a2c_acktr, ppo
from actorcritic.examples.atari.loop import parse_flags, result_paths


def test_no_flags_are_the_train_functions_defaults():
    flags = parse_flags([])
    assert flags == dict(game=None, mask_actions=False, episodic_life=False, max_episode_steps=None,
                         normalize_returns=False, fused_games=False, run_state=False, episode_stats=False,
                         diagnostics=False, checkpoint_every=100)
    for fn in (a2c_acktr.train_a2c_acktr, ppo.train_ppo):
        params = inspect.signature(fn).parameters
        assert {k: params[k].default for k in flags} == flags


def test_every_flag():
    flags = parse_flags('--game catch+breakout --mask-actions --episodic-life --max-episode-steps 50 '
                        '--normalize-returns --fused-games --run-state --episode-stats --diagnostics '
                        '--checkpoint-every 7'.split())
    assert flags == dict(game='catch+breakout', mask_actions=True, episodic_life=True, max_episode_steps=50,
                         normalize_returns=True, fused_games=True, run_state=True, episode_stats=True,
                         diagnostics=True, checkpoint_every=7)
    assert parse_flags(['--checkpoint-every', '3', '--game', 'catch'])['game'] == 'catch'


def test_result_paths(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    root = str(tmp_path / 'results')
    assert result_paths(None) == ('BreakoutNoFrameskip-v4', root + '/checkpoints/BreakoutNoFrameskip-v4',
                                  root + '/summaries/BreakoutNoFrameskip-v4')
    env_id, checkpoint_path, summary_path = result_paths('catch', '-ppo')
    assert env_id == 'DeviceGame-catch'
    assert checkpoint_path == root + '/checkpoints-ppo/DeviceGame-catch'
    assert summary_path == root + '/summaries-ppo/DeviceGame-catch'
    assert os.path.isdir(checkpoint_path) and os.path.isdir(summary_path)
