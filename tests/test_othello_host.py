"""Othello on the host (no GPU): `games.OthelloEnv` against the scripted games of othello_cases.py, the perft counts, the numpy model of
the device step against the env, every planted mistake caught by a named case, uniformly random play, and the declarations."""
import copy
import json
import os
import re

import numpy as np
import pytest

import othello_cases as oc
from helpers import REPO

SHAPE_KEYS = ('S', 'N', 'M', 'F')
WRAPS = ('wrap_east', 'wrap_west', 'wrap_south_west', 'wrap_south_east', 'wrap_north_east', 'wrap_north_west')
# what the small shapes' cases contain between them
NEEDED = tuple('flip_' + n for n in oc.DIRECTION_NAMES) + WRAPS + (
    'flip_three_directions', 'edge_run_without_anchor', 'run_broken_by_empty', 'forced_pass', 'two_passes_same_side', 'end_with_empty_cells',
    'end_full_board', 'draw', 'final_placement_loses', 'wipe_out', 'resign_black', 'resign_white', 'flipped_twice')


def _play_case(case, stack_history):
    """Plays the case on the host env, checking every ply: reward, done, board, mask, observation (from board snapshots), counters."""
    rows, cols = oc.SHAPES[case['shape']]
    nn = rows * cols
    env = oc.make_env(case['shape'], stack_history)
    assert env.observation_shape == (2 * stack_history + 1, rows, cols) and env.num_actions == nn + 2 and env.resign_action == env.num_actions - 1
    obs = env.reset()
    snaps = [oc.start_board(rows, cols)]
    assert np.array_equal(env.board, snaps[0])
    assert np.array_equal(obs, oc.observation_from_boards(snaps, 1, stack_history, rows, cols)) and obs.dtype == np.int8
    last = len(case['moves']) - 1
    assert len(case['boards']) == len(case['moves'])
    for ply, a in enumerate(case['moves']):
        mover = 1 + ply % 2  # the side to move alternates on every ply, pass included
        assert env.current_player == mover and env.steps == ply and not env.is_game_over
        before = env.board.copy()
        obs, reward, done, _ = env.step(a)
        assert np.array_equal(env.board, oc.board_array(case['boards'][ply])), (case['name'], ply)
        if a >= nn:
            assert np.array_equal(env.board, before)  # a pass and a resignation change nothing on the board
        if a <= nn:
            snaps.insert(0, env.board.copy())  # both histories advance on every ply (not on a resignation: the game is over)
        assert reward == (case['reward'] if ply == last else 0.0), (case['name'], ply)
        assert done == (case['done'] if ply == last else False), (case['name'], ply)
        assert env.steps == ply + 1 and env.is_game_over == done and env.last_actions[mover] == a
        to_play = mover if done else 3 - mover  # the side to move switches only if the game is not over
        assert env.current_player == to_play and env.opponent_player == 3 - to_play
        assert np.array_equal(obs, oc.observation_from_boards(snaps, to_play, stack_history, rows, cols)), (case['name'], ply)
        if not done:
            mask = env.actions_mask
            assert mask[nn + 1] and mask[nn] == (not mask[:nn].any())  # resign always; pass iff no placement
            for point in range(nn):  # a placement is legal iff the point is empty and some ray holds a run of the opponent's, then an own stone
                r, c = divmod(point, cols)
                ok = False
                for d in range(8):
                    vals = [v for v, _ in oc.ray(env.board, r, c, d)]
                    n = 0
                    while n < len(vals) and vals[n] == 3 - to_play:
                        n += 1
                    ok |= n >= 1 and n < len(vals) and vals[n] == to_play
                assert mask[point] == (ok and env.board[r, c] == 0), (case['name'], ply, point)
    assert env.winner == case['winner'] and env.loser == (None if case['winner'] is None else 3 - case['winner'])
    return env


@pytest.mark.parametrize('stack_history', [1, 4])
@pytest.mark.parametrize('shape', SHAPE_KEYS)
def test_scripted_games_on_the_host_env(shape, stack_history):
    names = [c['name'] for c in oc.cases(shape)]
    assert len(set(names)) == len(names)
    for need in NEEDED if shape in 'SN' else ('forced_pass', 'end_full_board', 'resign_black', 'resign_white'):
        assert need in names, need
    for case in oc.cases(shape):
        env = _play_case(case, stack_history)
        if case['done']:
            with pytest.raises(RuntimeError):
                env.step(env.resign_action)


@pytest.mark.parametrize('shape', ['S', 'N'])
def test_cases_are_what_their_names_say(shape):
    """Read off the boards alone."""
    rows, cols = oc.SHAPES[shape]
    nn = rows * cols

    def plies(name):
        c = oc.case(shape, name)
        boards = [oc.start_board(rows, cols)] + [oc.board_array(b) for b in c['boards']]
        return c, [(ply, 1 + ply % 2, a, boards[ply], boards[ply + 1]) for ply, a in enumerate(c['moves'])]

    for d, name in enumerate(oc.DIRECTION_NAMES):
        _, p = plies('flip_' + name)
        ply, me, a, before, after = p[-1]
        assert set(oc.flipped_by_direction(before, after, a)) == {d}, name
    _, p = plies('flip_three_directions')
    assert len(oc.flipped_by_direction(p[-1][3], p[-1][4], p[-1][2])) >= 3

    def runs(before, a, me):
        """per direction: (length of the opposing run next to the point, the cells after it)"""
        r, c = divmod(a, cols)
        out = []
        for d in range(8):
            vals = [v for v, _ in oc.ray(before, r, c, d)]
            n = 0
            while n < len(vals) and vals[n] == 3 - me:
                n += 1
            out.append((d, n, vals[n:]))
        return out

    _, p = plies('edge_run_without_anchor')
    ply, me, a, before, after = p[-1]
    unanchored = [d for d, n, rest in runs(before, a, me) if n >= 1 and not rest]
    assert unanchored and not any(d in oc.flipped_by_direction(before, after, a) for d in unanchored)
    _, p = plies('run_broken_by_empty')
    ply, me, a, before, after = p[-1]
    broken = [d for d, n, rest in runs(before, a, me) if n >= 1 and len(rest) >= 2 and rest[0] == 0 and rest[1] == me]
    assert broken and not any(d in oc.flipped_by_direction(before, after, a) for d in broken)
    c, p = plies('forced_pass')
    assert c['moves'][-1] == nn and np.array_equal(p[-1][3], p[-1][4])
    c, p = plies('two_passes_same_side')
    assert max(sum(1 for ply, me, a, _, _ in p if a == nn and me == side) for side in (1, 2)) >= 2
    c, p = plies('end_with_empty_cells')
    assert c['done'] and (p[-1][4] == 0).any() and c['moves'][-1] < nn
    c, p = plies('end_full_board')
    assert c['done'] and not (p[-1][4] == 0).any()
    c, p = plies('draw')
    assert c['done'] and c['winner'] is None and c['reward'] == 0.0 and (p[-1][4] == 1).sum() == (p[-1][4] == 2).sum()
    c, p = plies('final_placement_loses')
    ply, me, a, before, after = p[-1]
    assert c['done'] and c['reward'] == -1.0 and a < nn and c['winner'] == 3 - me and (after == me).sum() < (after == 3 - me).sum()
    c, p = plies('wipe_out')
    assert c['done'] and min((p[-1][4] == 1).sum(), (p[-1][4] == 2).sum()) == 0
    c, p = plies('flipped_twice')
    changes = sum(((before != 0) & (after != before)).astype(int) for _, _, _, before, after in p)
    assert changes.max() >= 2
    for name, winner in (('resign_black', 2), ('resign_white', 1)):
        c, p = plies(name)
        assert c['moves'][-1] == nn + 1 and c['reward'] == -1.0 and c['winner'] == winner
    # the counts decide: wherever a game ends by itself the winner has more stones
    for c in oc.cases(shape):
        if c['done'] and c['moves'][-1] < nn:
            b = oc.board_array(c['boards'][-1])
            nb, nw = int((b == 1).sum()), int((b == 2).sum())
            assert c['winner'] == (1 if nb > nw else 2 if nw > nb else None), c['name']


def _perft(env, depth):
    """Leaves of the game tree cut at `depth` plies: a pass is a ply, a finished game is a leaf.  (One ply above the cut every legal
    action is one leaf, whether it ends the game or not: the last level is counted off the mask.)"""
    if depth == 0 or env.is_game_over:
        return 1
    legal = np.flatnonzero(env.actions_mask[:-1])
    if depth == 1:
        return len(legal)
    n = 0
    for a in legal:
        child = copy.deepcopy(env)
        child.step(int(a))
        n += _perft(child, depth - 1)
    return n


@pytest.mark.parametrize('shape, counts', [('F', [4, 12, 56, 244, 1396, 8200]), ('M', [4, 12, 56, 244, 1364, 7604]),
                                           ('N', [4, 12, 50, 180, 798, 3338, 15418]), ('S', [4, 12, 44, 128, 424, 1256, 3624, 9116, 20044])])
def test_perft(shape, counts):
    """On `OthelloEnv` itself: the published Othello numbers on 8 x 8 (so the rules and the start position are the standard ones) and
    the smaller boards' own."""
    assert [_perft(oc.make_env(shape), d) for d in range(1, len(counts) + 1)] == counts


def test_the_three_sequences_and_the_opening():
    env = oc.make_env('F')
    assert sorted(divmod(int(a), 8) for a in np.flatnonzero(env.actions_mask[:64])) == [(2, 3), (3, 2), (4, 5), (5, 4)]
    env = oc.make_env('S')
    for a in (1, 2, 11, 0):
        _, r, d, _ = env.step(a)
    assert env.current_player == 1 and env.steps == 4 and list(np.flatnonzero(env.actions_mask)) == [16, 17]  # black must pass at ply 4
    env = oc.make_env('S')
    for a in (1, 2, 3, 0, 8, 16, 15):
        _, r, d, _ = env.step(a)
    assert d and r == 1.0 and env.steps == 7 and ((env.board == 0).sum(), (env.board == 1).sum(), (env.board == 2).sum()) == (6, 9, 1) and env.winner == 1
    env = oc.make_env('S')
    seq = (1, 0, 4, 2, 7, 8, 13, 11, 15)
    for a in seq:
        _, r, d, _ = env.step(a)
    assert 16 not in seq and d and r == -1.0 and env.steps == 9 and env.winner == 2
    assert ((env.board == 0).sum(), (env.board == 1).sum(), (env.board == 2).sum()) == (3, 4, 9)


def test_illegal_actions_raise():
    from muzero_amd.games import BoardGameEnv, OthelloEnv

    env = oc.make_env('S')
    assert isinstance(env, BoardGameEnv) and env.name == 'Othello'
    for a in (0, 5, 16, 18, -1):  # no flip; occupied; a pass while placements exist; out of range
        with pytest.raises(ValueError):
            env.step(a)
    assert env.steps == 0
    for a in (1, 2, 11, 0):
        env.step(a)
    with pytest.raises(ValueError):
        env.step(3)  # black has no placement here: only the pass and the resignation
    env.step(16)
    for bad in ((3, 8), (8, 9), (4, 4, 0)):
        with pytest.raises(ValueError):
            OthelloEnv(*bad)
    assert OthelloEnv(4, 6).num_actions == 26 and OthelloEnv().observation_shape == (9, 8, 8)


# uniformly random legal games (now and then a resignation), played back to back through the auto-reset: shape -> (games, seed)
FUZZ = {'S': (2000, 11), 'N': (2000, 11), 'M': (2000, 11), 'F': (300, 11)}


@pytest.mark.parametrize('shape', SHAPE_KEYS)
def test_numpy_model_of_the_device_step_equals_the_host_env(shape):
    rows, cols = oc.SHAPES[shape]
    nn = rows * cols
    for case in oc.cases(shape):
        assert oc.model_vs_env(oc.OthModel(rows, cols), oc.make_env(shape), case['moves']) is None, case['name']
    n_games, seed = FUZZ[shape]
    rs = np.random.RandomState(seed)
    model, env = oc.OthModel(rows, cols), oc.make_env(shape)
    games = passes = early_ends = draws = longest = 0
    while games < n_games:
        legal = np.flatnonzero(env.actions_mask)
        a = int(legal[rs.randint(len(legal))]) if rs.rand() < 0.005 else int(rs.choice(legal[:-1]))
        passes += a == nn
        empty_before, steps_before = int((env.board == 0).sum()), env.steps
        diff = oc.model_vs_env(model, env, [a])
        assert diff is None, (games, diff)
        if env.steps == 0:  # the game ended (model_vs_env has reset the env)
            games += 1
            longest = max(longest, steps_before + 1)
            early_ends += a < nn and empty_before > 1
            draws += a < nn and model.last['winner'] is None  # (the model's result equals the env's: checked above)
    assert model.episodes == n_games
    # the run reaches every branch: passes, ends with empty cells, a draw (should a run lack one, change its seed, not this line)
    assert passes > 0 and early_ends > 0 and draws > 0 and longest <= 2 * (nn - 4), (passes, early_ends, draws, longest)


# planted mistake -> the scripted case (on S and on N) that must catch it
PLANTED = dict({'direction_missing_' + n: 'flip_' + n for n in oc.DIRECTION_NAMES}, **{
    'no_edge_mask': 'wrap_east', **{'no_edge_mask_' + n: 'wrap_' + n for n in oc.EDGE_DIRECTIONS}, 'flip_without_anchor': 'edge_run_without_anchor', 'flip_through_empty': 'run_broken_by_empty',
    'pass_beside_placements': 'flip_east', 'no_pass': 'forced_pass', 'end_on_full_board_only': 'end_with_empty_cells',
    'winner_is_mover': 'final_placement_loses', 'draw_is_loss': 'draw', 'count_before_flips': 'draw', 'mover_history_only': 'flipped_twice',
    'mask_wrong_colour': 'flip_three_directions', 'switch_after_end': 'end_full_board', 'mask_stale_after_pass': 'forced_pass'})


@pytest.mark.parametrize('bug', oc.BUGS)
def test_every_planted_mistake_is_caught_by_its_named_case(bug):
    for shape in ('S', 'N'):
        rows, cols = oc.SHAPES[shape]
        case = oc.case(shape, PLANTED[bug])
        assert oc.model_vs_env(oc.OthModel(rows, cols, bug), oc.make_env(shape), case['moves']) is not None, (bug, shape, case['name'])
        if bug == 'no_edge_mask':  # every near-miss catches it, on the square and on the non-square board
            for name in WRAPS:
                assert oc.model_vs_env(oc.OthModel(rows, cols, bug), oc.make_env(shape), oc.case(shape, name)['moves']) is not None, (shape, name)


def random_policy_stats(shape='M', games=2000, seed=1):
    """Uniformly random legal play (no resignation): lengths, passes, early ends and the first player's win / draw / loss shares."""
    rows, cols = oc.SHAPES[shape]
    nn = rows * cols
    rs = np.random.RandomState(seed)
    env = oc.make_env(shape)
    lengths, results, with_pass, early = [], [], 0, 0
    for _ in range(games):
        env.reset()
        done, passed = False, False
        while not done:
            a = int(rs.choice(np.flatnonzero(env.actions_mask[:nn + 1])))
            passed |= a == nn
            _, _, done, _ = env.step(a)
        lengths.append(env.steps)
        results.append(env.winner)
        with_pass += passed
        early += bool((env.board == 0).any())
    n = float(games)
    return dict(games=games, seed=seed, rows=rows, cols=cols, mean_length=float(np.mean(lengths)), min_length=int(min(lengths)),
                max_length=int(max(lengths)), games_with_a_pass=with_pass / n, games_ending_with_empty_cells=early / n,
                first_player_win=results.count(1) / n, draw=results.count(None) / n, first_player_loss=results.count(2) / n)


def test_uniformly_random_play_baseline():
    """The baseline of the learning numbers (profiles/othello/random_policy.json records the same run); only what is derivable is asserted."""
    s = random_policy_stats()
    rows, cols = oc.SHAPES['M']
    assert abs(s['first_player_win'] + s['draw'] + s['first_player_loss'] - 1.0) < 1e-12
    assert 5 <= s['min_length'] <= s['mean_length'] <= s['max_length'] <= 2 * (rows * cols - 4)
    rec = json.load(open(os.path.join(REPO, 'profiles', 'othello', 'random_policy.json')))
    for k, v in s.items():
        assert rec[k] == pytest.approx(v, abs=1e-12), k


def test_config_names_and_constants():
    from muzero_amd import pipeline
    from muzero_amd import planner as pl
    from muzero_amd.config import make_othello_config

    cfg = make_othello_config()
    assert cfg.is_board_game and cfg.td_steps == 0 and cfg.discount == 1.0 and cfg.num_actions == 38 and cfg.input_shape == (9, 6, 6)
    assert (cfg.known_bounds.min, cfg.known_bounds.max) == (-1, 1)
    assert make_othello_config(rows=4, cols=6).num_actions == 26 and make_othello_config(rows=8, cols=8).input_shape == (9, 8, 8)
    assert [cfg.visit_softmax_temperature_fn(s, 0) for s in (0, 5, 6, 40)] == [1.0, 1.0, 0.1, 0.1]
    assert pipeline.board_temperature_switch(cfg) == 6
    assert 'Othello' in pipeline.DEVICE_ENVS and 'Othello' in pipeline.ARENA_ENVS
    assert pipeline.resolve_self_play_envs('Othello', 4) == ('device', 'Othello')
    assert pipeline.resolve_self_play_envs(oc.make_env('F'), 4) == ('device', 'Othello')
    assert pipeline.resolve_arena_env('Othello') == 'Othello' and pipeline.resolve_arena_env(oc.make_env('S')) == 'Othello'
    header = open(os.path.join(REPO, 'include', 'mzplanner.h')).read()
    assert int(re.search(r'#define MZ_ENV_OTHELLO (\d+)', header).group(1)) == pl.ENV_OTHELLO == 9
    assert re.search(r'typedef struct \{\s*int32_t temp_switch_steps;[^}]*\} mz_othello_env;', header)
    import ctypes

    from muzero_amd import build

    lib = ctypes.CDLL(build.build())
    for fn in ('mz_selfplay_reset_othello', 'mz_othello_debug_step', 'mz_othello_debug_mask', 'mz_othello_debug_board', 'mz_arena_reset_othello'):
        assert re.search(r'^int ' + fn + r'\(', header, flags=re.M), fn  # an ordinary prototype
        assert hasattr(lib, fn), fn  # exported
        assert fn in pl.ABI_SYMBOLS and not any(ch.isdigit() for ch in fn)
    csrc = open(os.path.join(REPO, 'muzero_amd', 'csrc', 'mz_othello.h')).read()
    assert re.search(r'constexpr int ENV_OTHELLO = 9;', csrc)
    assert '#include "mz_othello.h"' in open(os.path.join(REPO, 'muzero_amd', 'csrc', 'planner.hip')).read()
