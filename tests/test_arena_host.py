"""Host side of the arena (pipeline.play_match / MatchResult, the evaluators' match_games / device_episodes switches) without a GPU,
and the arena kernels' cross-compiled resource usage."""
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from helpers import REPO, build_mlp, mlp_case


def _match(winner, two=True):
    from muzero_amd import pipeline

    w = np.asarray(winner, np.int32)
    return pipeline.MatchResult(w, np.arange(5, 5 + len(w), dtype=np.int32), np.where(w == 1, 1.0, np.where(w == 2, -1.0, 0.0)), two)


def test_match_result_arithmetic():
    m = _match([1, 2, 3, 1, 1, 3, 2, 2])
    assert (m.num_games, m.wins, m.losses, m.draws) == (8, 3, 3, 2)
    assert m.score == (3 + 0.5 * 2) / 8
    assert m.by_colour() == dict(black=(2, 1, 1), white=(1, 1, 2))
    one = _match([3, 3, 3], two=False)
    assert (one.wins, one.losses, one.draws) == (0, 0, 3)
    with pytest.raises(ValueError):
        one.by_colour()
    with pytest.raises(ValueError):
        one.elo(0, 0)


def test_elo_fold_equals_a_hand_rolled_loop():
    """Decided games in env-index order, the opponent's rating held fixed, draws skipped."""
    from muzero_amd.rating import compute_elo_rating

    rs = np.random.RandomState(3)
    for _ in range(5):
        winner = rs.randint(1, 4, size=40)
        r, opp = -2000.0, -1950.0
        for w in winner:
            if w == 3:
                continue
            r = compute_elo_rating(0 if w == 1 else 1, r, opp)[0]
        assert _match(winner).elo(-2000.0, -1950.0) == r
    assert _match([3, 3]).elo(12.5, 99.0) == 12.5  # only draws: unchanged
    # the order matters (the fold is not a function of the counts alone), so the order is part of the contract
    assert _match([1, 1, 2, 2]).elo(0, 0) != _match([2, 2, 1, 1]).elo(0, 0)


def test_play_match_argument_validation():
    """Every bad argument is refused before a planner is created (no GPU is touched)."""
    from muzero_amd import pipeline
    from muzero_amd.config import make_classic_config, make_tictactoe_config
    from muzero_amd.games import CartPoleEnv, GomokuEnv, TicTacToeEnv

    net = build_mlp(mlp_case('tictactoe'))
    cfg = make_tictactoe_config(use_tensorboard=False)
    dev = types.SimpleNamespace(index=0)
    bad = [
        dict(opponent=net, env='TicTacToe', num_games=7),            # odd number of games on a two-player env
        dict(opponent=net, env='TicTacToe', num_games=0),
        dict(opponent=None, env='TicTacToe', num_games=8),           # a two-player env needs an opponent
        dict(opponent='strong', env='TicTacToe', num_games=8),
        dict(opponent=42, env='TicTacToe', num_games=8),
        dict(opponent=net, env='TicTacToe', num_games=8, opening_plies=-1),
        dict(opponent=net, env='Synthetic-Atari', num_games=8),      # a device env, but not one the arena plays
        dict(opponent=net, env='Chess', num_games=8),
        dict(opponent=net, env=object(), num_games=8),
        dict(opponent='random', env='TicTacToe', num_games=8, init_state=np.zeros((8, 4))),
        dict(opponent=build_mlp(mlp_case('cartpole')), env='TicTacToe', num_games=8),  # networks of different shape
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            pipeline.play_match(cfg, net, kw.pop('opponent'), dev, kw.pop('env'), kw.pop('num_games'), **kw)
    cp = build_mlp(mlp_case('cartpole'))
    with pytest.raises(ValueError):  # a one-player env takes no opponent
        pipeline.play_match(make_classic_config(use_tensorboard=False), cp, 'random', dev, 'CartPole-v1', 8)
    assert pipeline.resolve_arena_env(TicTacToeEnv()) == 'TicTacToe'
    assert pipeline.resolve_arena_env(GomokuEnv(9)) == 'Gomoku'
    assert pipeline.resolve_arena_env(CartPoleEnv()) == 'CartPole-v1'
    assert pipeline.resolve_arena_env('Gomoku') == 'Gomoku'


def _stub_search(log):
    def uct_search(state, network, device, config, temperature, actions_mask, current_player, opponent_player, deterministic=False, rng=None):
        mask = np.asarray(actions_mask, bool)
        a = int(np.flatnonzero(mask)[0])  # the first legal move (never the resign action of a board game while a point is free)
        log.append((np.asarray(state).tobytes(), id(network), float(temperature), mask.tobytes(), current_player, opponent_player, deterministic, a))
        return a, np.zeros(len(mask)), 0.0
    return uct_search


def _checkpoints(tmp_path, case, seeds):
    from helpers import seeded_state_dict
    from muzero_amd import pipeline

    files = []
    for i, s in enumerate(seeds):
        net = build_mlp(case)
        f = str(tmp_path / f'ckpt{i}.pt')
        pipeline.create_checkpoint({'network': seeded_state_dict(net, s), 'train_steps': 10 * (i + 1)}, f)
        files.append(f)
    return files


def test_evaluators_at_zero_keep_their_call_sequence(tmp_path, monkeypatch):
    """match_games=0 / device_episodes=0 (the defaults): the same uct_search calls in the same order, the same tracker values, and
    play_match is never reached -- checked with a stub in place of the planner search."""
    import torch
    from muzero_amd import mcts, pipeline
    from muzero_amd.config import make_classic_config, make_tictactoe_config
    from muzero_amd.games import CartPoleEnv, TicTacToeEnv

    def no_match(*a, **k):
        raise AssertionError('play_match must not be called at 0')

    monkeypatch.setattr(pipeline, 'play_match', no_match)
    stop = types.SimpleNamespace(is_set=lambda: True)
    dev = torch.device('cpu')
    runs = []
    for extra in ({}, dict(match_games=0)):
        log, results = [], []
        monkeypatch.setattr(mcts, 'uct_search', _stub_search(log))
        case = mlp_case('tictactoe')
        old, new = build_mlp(case), build_mlp(case)
        elo = pipeline.run_board_game_evaluator(make_tictactoe_config(use_tensorboard=False), old, new, dev, TicTacToeEnv(), 0.1,
                                                _checkpoints(tmp_path, case, (5, 6)), stop, on_result=lambda *a: results.append(a), **extra)
        nets = {id(old): 'old', id(new): 'new'}
        runs.append(([(c[0], nets[c[1]]) + c[2:] for c in log], results, elo))
    assert runs[0] == runs[1] and len(runs[0][1]) == 2 and len(runs[0][0]) > 6
    runs = []
    for extra in ({}, dict(device_episodes=0)):
        log = []
        monkeypatch.setattr(mcts, 'uct_search', _stub_search(log))
        case = mlp_case('cartpole')
        res = pipeline.run_evaluator(make_classic_config(use_tensorboard=False), build_mlp(case), dev, CartPoleEnv(4, seed=3), 0.0,
                                     _checkpoints(tmp_path, case, (7,)), stop, num_episodes=2, **extra)
        runs.append(([c[:1] + c[2:] for c in log], res))
    assert runs[0] == runs[1] and len(runs[0][1]) == 1 and len(runs[0][1][0][0]) == 2


def test_arena_kernels_cross_compile_without_scratch_or_spills(tmp_path):
    """mz_arena.h alone, device side, for gfx950 with the library's flags: the four k_arena_* kernels are there and the compiler reports
    no scratch memory and no register spills for them (as built: k_arena_reset 30, k_arena_pre 36, k_arena_pick 16, k_arena_step 66
    VGPRs, no LDS)."""
    from muzero_amd import build

    hipcc = os.environ.get('HIPCC', 'hipcc')
    if shutil.which(hipcc) is None:
        pytest.fail('hipcc not found: the arena kernels cannot be compiled')
    src = tmp_path / 'arena_tu.hip'
    src.write_text('#include "mz_arena.h"\n')
    flags = [f for f in build.FLAGS if f not in ('-shared', '-fPIC')]
    out = subprocess.run([hipcc] + flags + ['--cuda-device-only', '-c', '-Rpass-analysis=kernel-resource-usage', '-I', build.CSRC, str(src), '-o',
                                            str(tmp_path / 'arena_tu.o')], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = re.split(r'remark: Function Name: ', out.stderr)[1:]
    found = {}
    for b in blocks:
        m = re.match(r'\S*?(k_arena_[a-z]+)', b)
        if m:
            found[m.group(1)] = {k: int(v) for k, v in re.findall(r'remark:\s+([A-Za-z ]+?)(?: \[bytes/\w+\])?: (\d+)', b)}
    assert sorted(found) == ['k_arena_pick', 'k_arena_pre', 'k_arena_reset', 'k_arena_step']
    for name, use in found.items():
        assert use['ScratchSize'] == 0 and use['SGPRs Spill'] == 0 and use['VGPRs Spill'] == 0, (name, use)
        assert use['LDS Size'] == 0 and use['VGPRs'] <= 128, (name, use)
