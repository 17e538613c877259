"""Connect Four on the host (no GPU): `games.ConnectFourEnv` against the hand-written games of connect4_cases.py, the numpy model of the
device step against the env, every planted mistake caught by a named case, uniformly random play, and the declarations."""
import json
import os
import re

import numpy as np
import pytest

import connect4_cases as cc
from helpers import REPO

SHAPE_KEYS = ('S', 'T', 'F')


def _env(shape, stack_history=4):
    from muzero_amd.games import ConnectFourEnv

    rows, cols, win = cc.SHAPES[shape]
    return ConnectFourEnv(rows, cols, win, stack_history)


def _play_case(case, stack_history):
    """Plays the case on the host env, checking every ply: reward, done, mask, observation (from board snapshots), counters."""
    rows, cols, win = cc.SHAPES[case['shape']]
    env = _env(case['shape'], stack_history)
    assert env.observation_shape == (2 * stack_history + 1, rows, cols) and env.num_actions == cols + 1
    obs = env.reset()
    snaps = {1: [], 2: []}
    assert np.array_equal(obs, cc.observation_from_boards(snaps, 1, stack_history, rows, cols)) and obs.dtype == np.int8
    last = len(case['moves']) - 1
    for ply, a in enumerate(case['moves']):
        mover = 1 + ply % 2
        assert env.current_player == mover
        assert env.steps == ply and not env.is_game_over
        obs, reward, done, _ = env.step(a)
        if a < cols:
            snaps[mover].insert(0, env.board.copy())
        assert reward == (case['reward'] if ply == last else 0.0), (case['name'], ply)
        assert done == (case['done'] if ply == last else False), (case['name'], ply)
        assert env.steps == ply + 1 and env.is_game_over == done
        to_play = mover if done else 3 - mover  # the side to move switches only if the game is not over
        assert env.current_player == to_play and env.opponent_player == 3 - to_play
        assert np.array_equal(obs, cc.observation_from_boards(snaps, to_play, stack_history, rows, cols)), (case['name'], ply)
        legal = [c for c in range(cols) if env.board[0, c] == 0]
        if case['masks'] is not None:
            assert legal == case['masks'][ply], (case['name'], ply)
        assert np.array_equal(np.flatnonzero(env.actions_mask), legal + [cols]), (case['name'], ply)  # resign is always legal
    assert np.array_equal(env.board, cc.board_array(case['board'])), case['name']
    assert env.winner == case['winner'] and env.loser == (None if case['winner'] is None else 3 - case['winner'])
    return env


@pytest.mark.parametrize('stack_history', [1, 4])
@pytest.mark.parametrize('shape', SHAPE_KEYS)
def test_scripted_games_on_the_host_env(shape, stack_history):
    names = [c['name'] for c in cc.cases(shape)]
    for need in ('vertical_earliest_win', 'both_rays_needed', 'diag_up_last_top', 'diag_up_last_bottom', 'diag_down_last_top', 'diag_down_last_bottom',
                 'wrap_horizontal', 'wrap_diag_up', 'wrap_diag_down', 'column_fills', 'draw_full_board', 'win_on_last_cell', 'resign_black', 'resign_white'):
        assert need in names, need
    for case in cc.cases(shape):
        env = _play_case(case, stack_history)
        if case['done']:
            with pytest.raises(RuntimeError):
                env.step(int(np.flatnonzero(env.actions_mask)[0]))


@pytest.mark.parametrize('shape', SHAPE_KEYS)
def test_wrap_cases_hold_consecutive_bits_and_earliest_win_sits_on_the_gate(shape):
    """What the cases claim about themselves: the near-misses really are num_to_win stones of one colour on equally spaced bit positions
    (spacing 1, cols - 1, cols + 1) that cross a row edge, and the earliest win falls on ply 2 * (num_to_win - 1)."""
    rows, cols, win = cc.SHAPES[shape]
    for name, step, dc in (('wrap_horizontal', 1, 1), ('wrap_diag_up', cols - 1, -1), ('wrap_diag_down', cols + 1, 1)):
        b = cc.board_array(cc.case(shape, name)['board']).reshape(-1)
        runs = [p for colour in (1, 2) for p in range(rows * cols - (win - 1) * step) if all(b[p + k * step] == colour for k in range(win))]
        assert runs, name
        # on a real line the column moves by dc per stone; here it jumps across the edge
        assert all(any((p + k * step) % cols != p % cols + k * dc for k in range(win)) for p in runs), name
    assert len(cc.case(shape, 'vertical_earliest_win')['moves']) - 1 == 2 * (win - 1)
    assert len(cc.case(shape, 'draw_full_board')['moves']) == rows * cols == len(cc.case(shape, 'win_on_last_cell')['moves'])


def test_full_column_and_bad_actions_raise():
    env = _env('S')
    for a in (2, 2, 2, 2):
        env.step(a)
    with pytest.raises(ValueError):
        env.step(2)
    with pytest.raises(ValueError):
        env.step(6)
    with pytest.raises(ValueError):
        env.step(-1)
    from muzero_amd.games import BoardGameEnv, ConnectFourEnv

    assert isinstance(env, BoardGameEnv) and env.name == 'ConnectFour'
    with pytest.raises(ValueError):
        ConnectFourEnv(4, 5, 6)


def _model_vs_env(model, env, moves):
    """Steps both; returns the first difference as a string, or None.  After a finished game the env is reset, as the device resets."""
    cols = env.cols
    for ply, a in enumerate(moves):
        mover = env.current_player
        obs, reward, done, _ = env.step(a)
        try:
            out = model.step(a)
        except (IndexError, ValueError) as e:  # (a planted mistake may walk off the board)
            return f'ply {ply}: {type(e).__name__}'
        if out['reward'] != reward or out['done'] != done or out['winner'] != env.winner:
            return f'ply {ply}: reward / done / winner {out["reward"], out["done"], out["winner"]} != {reward, done, env.winner}'
        if not np.array_equal(out['board'], env.board):
            return f'ply {ply}: board'
        if out['to_play'] != env.current_player or (done and env.current_player != mover):
            return f'ply {ply}: side to move'
        if done:
            obs = env.reset()
        if model.player != env.current_player or model.steps != env.steps:
            return f'ply {ply}: player / steps after the move'
        if not np.array_equal(model.obs.reshape(obs.shape), obs.astype(np.float32)):
            return f'ply {ply}: observation'
        if not np.array_equal(model.mask, env.actions_mask.astype(np.uint8)):
            return f'ply {ply}: mask'
        if not np.array_equal(model.board.reshape(env.board.shape), env.board):
            return f'ply {ply}: board after the move'
        for pid in (1, 2):
            if not np.array_equal(model.planes[pid - 1].reshape(env.feature_planes[pid].shape), env.feature_planes[pid]):
                return f'ply {ply}: history planes'
    return None


@pytest.mark.parametrize('shape', SHAPE_KEYS)
def test_numpy_model_of_the_device_step_equals_the_host_env(shape):
    rows, cols, win = cc.SHAPES[shape]
    for case in cc.cases(shape):
        assert _model_vs_env(cc.C4Model(rows, cols, win), _env(shape), case['moves']) is None, case['name']
    # 2 000 uniformly random legal games (resign at random too), played back to back through the auto-reset
    rs = np.random.RandomState(11)
    model, env = cc.C4Model(rows, cols, win), _env(shape)
    games = 0
    while games < 2000:
        legal = np.flatnonzero(env.actions_mask)
        a = int(legal[rs.randint(len(legal))]) if rs.rand() < 0.02 else int(rs.choice(legal[:-1]))
        diff = _model_vs_env(model, env, [a])
        assert diff is None, (games, diff)
        games += env.steps == 0
    assert model.episodes == 2000


# planted mistake -> the scripted case (on S) that must catch it
PLANTED = {
    'no_guard': 'wrap_horizontal', 'gravity_high': 'vertical_earliest_win', 'diag_missing': 'diag_up_last_top', 'one_ray': 'both_rays_needed',
    'mask_early': 'column_fills', 'mask_late': 'column_fills', 'draw_first': 'win_on_last_cell', 'switch_after_end': 'vertical_earliest_win',
    'wrong_history': 'vertical_earliest_win', 'gate_off_by_one': 'vertical_earliest_win', 'resign_wrong_side': 'resign_black',
}


@pytest.mark.parametrize('bug', cc.BUGS)
def test_every_planted_mistake_is_caught_by_its_named_case(bug):
    for shape in SHAPE_KEYS:
        rows, cols, win = cc.SHAPES[shape]
        case = cc.case(shape, PLANTED[bug])
        assert _model_vs_env(cc.C4Model(rows, cols, win, bug), _env(shape), case['moves']) is not None, (bug, shape, case['name'])
    # the wrap mistake: every one of the three wrap cases catches it, on every shape
    if bug == 'no_guard':
        for shape in SHAPE_KEYS:
            rows, cols, win = cc.SHAPES[shape]
            for name in ('wrap_horizontal', 'wrap_diag_up', 'wrap_diag_down'):
                assert _model_vs_env(cc.C4Model(rows, cols, win, bug), _env(shape), cc.case(shape, name)['moves']) is not None, (shape, name)


def random_policy_stats(games=2000, seed=1):
    """Uniformly random legal play (no resign) on F: mean length and the first player's win / draw / loss shares."""
    rows, cols, win = cc.SHAPES['F']
    rs = np.random.RandomState(seed)
    env = _env('F')
    lengths, results = [], []
    for _ in range(games):
        env.reset()
        done = False
        while not done:
            _, _, done, _ = env.step(int(rs.choice(np.flatnonzero(env.actions_mask[:cols]))))
        lengths.append(env.steps)
        results.append(env.winner)
    n = float(games)
    return dict(games=games, seed=seed, rows=rows, cols=cols, num_to_win=win, mean_length=float(np.mean(lengths)), min_length=int(min(lengths)),
                max_length=int(max(lengths)), first_player_win=results.count(1) / n, draw=results.count(None) / n, first_player_loss=results.count(2) / n)


def test_uniformly_random_play_baseline():
    """The baseline of the learning numbers (profiles/connect4/random_policy.json records the same run); only what is derivable is asserted."""
    s = random_policy_stats()
    rows, cols, win = cc.SHAPES['F']
    assert abs(s['first_player_win'] + s['draw'] + s['first_player_loss'] - 1.0) < 1e-12
    assert 2 * win - 1 <= s['min_length'] <= s['mean_length'] <= s['max_length'] <= rows * cols
    rec = json.load(open(os.path.join(REPO, 'profiles', 'connect4', 'random_policy.json')))
    for k, v in s.items():
        assert rec[k] == pytest.approx(v, abs=1e-12), k


def test_config_names_and_constants():
    from muzero_amd import pipeline
    from muzero_amd import planner as pl
    from muzero_amd.config import make_connect4_config

    cfg = make_connect4_config()
    assert cfg.is_board_game and cfg.td_steps == 0 and cfg.discount == 1.0 and cfg.num_actions == 8 and cfg.input_shape == (9, 6, 7)
    assert [cfg.visit_softmax_temperature_fn(s, 0) for s in (0, 5, 6, 40)] == [1.0, 1.0, 0.1, 0.1]
    assert pipeline.board_temperature_switch(cfg) == 6
    assert pipeline.board_temperature_switch(make_connect4_config(temp_switch_steps=10)) == 10
    assert 'ConnectFour' in pipeline.DEVICE_ENVS and 'ConnectFour' in pipeline.ARENA_ENVS
    assert pipeline.resolve_self_play_envs('ConnectFour', 4) == ('device', 'ConnectFour')
    assert pipeline.resolve_self_play_envs(_env('F'), 4) == ('device', 'ConnectFour')
    assert pipeline.resolve_arena_env('ConnectFour') == 'ConnectFour' and pipeline.resolve_arena_env(_env('S')) == 'ConnectFour'
    header = open(os.path.join(REPO, 'include', 'mzplanner.h')).read()
    assert int(re.search(r'#define MZ_ENV_CONNECT4 (\d+)', header).group(1)) == pl.ENV_CONNECT4 == 8
    import ctypes

    from muzero_amd import build

    lib = ctypes.CDLL(build.build())
    for fn in ('mz_selfplay_reset_connect4', 'mz_connect4_debug_step', 'mz_connect4_debug_mask', 'mz_arena_reset_connect4'):
        assert re.search(r'^extern int ' + fn + r'\(', header, flags=re.M), fn  # declared
        assert hasattr(lib, fn), fn  # and exported
        assert fn not in pl.ABI_SYMBOLS  # (the list the two header-parsing ABI tests compare: see the header's note)
    csrc = open(os.path.join(REPO, 'muzero_amd', 'csrc', 'mz_connect4.h')).read()
    assert re.search(r'constexpr int ENV_CONNECT4 = 8;', csrc)
