"""Connect Four in the arena (mz_arena_reset_connect4) on an MI355X: every ply against host `games.ConnectFourEnv` objects and the
oracle search (tests/test_gpu_arena.py's ply-by-ply check, on this game), two weight sets and the random opponent, the tally, balanced
colours, paired legal openings that never resign, frozen finished games; `play_match` and `run_board_game_evaluator` on top."""
import types

import numpy as np
import pytest
import torch

import connect4_cases as cc
from helpers import philox_uniforms, seeded_state_dict
from test_gpu_arena import _planner, _play_board_match

pytestmark = pytest.mark.gpu

BOARD_KW = dict(discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0), root_dirichlet_alpha=0.25, root_exploration_eps=0.25)
GAMES, SIMS, OPENING = 8, 8, 2


def _net(shape, seed):
    from muzero_amd.network import MuZeroBoardGameNet

    rows, cols, _ = cc.SHAPES[shape]
    net = MuZeroBoardGameNet((9, rows, cols), cols + 1, 1, 8)
    net.load_state_dict(seeded_state_dict(net, seed))
    net.eval()
    return net


def _make_env(shape):
    from muzero_amd.games import ConnectFourEnv

    class Env(ConnectFourEnv):  # (the oracle envs' step returns three values)
        def step(self, action):
            obs, reward, done, _ = super().step(action)
            return obs, reward, done

    return lambda: Env(*cc.SHAPES[shape])


@pytest.mark.parametrize('opponent', ['planner', 'random'])
@pytest.mark.parametrize('shape', ['S', 'F'])
def test_every_ply_against_host_envs_and_the_oracle(oracle, shape, opponent):
    from test_oracle_nets import _oracle_net
    from muzero_amd import planner as pl

    rows, cols, win = cc.SHAPES[shape]
    net_p, net_q = _net(shape, 41), _net(shape, 43)
    p = _planner(net_p, GAMES, 7, num_simulations=SIMS, **BOARD_KW)
    q = _planner(net_q, GAMES, 8, num_simulations=SIMS, **BOARD_KW) if opponent == 'planner' else None
    cfg = oracle.make_config(cols + 1, SIMS, 1.0, True, (-1.0, 1.0), 0.25, 0.25)
    p.arena_reset_connect4(q if q is not None else 'random', OPENING, win)
    res, openings = _play_board_match(oracle, p, q, _oracle_net(oracle, net_p, 'conv'), _oracle_net(oracle, net_q, 'conv') if q is not None else None, cfg,
                                      _make_env(shape), (9, rows, cols), OPENING, rows * cols)
    assert res['challenger_wins'] + res['opponent_wins'] + res['draws'] == GAMES and res['live'] == 0
    for t, o in enumerate(openings):  # paired, legal columns, never the resignation: legal[floor(u * n_legal)] of the pair's stream
        assert np.array_equal(o[:GAMES // 2], o[GAMES // 2:]) and (o < cols).all()
        for b in range(GAMES // 2):
            assert o[b] == int(np.floor(philox_uniforms(7, b, t, 0x60000000, 1)[0] * cols))  # (every column is legal in the first two plies)
    p.close()
    if q is not None:
        q.close()


def test_random_opponent_never_resigns():
    """Against the random opponent to the end of every game on S: every random move is a legal column, drawn as
    legal_columns[floor(u * n)] from the env's own stream, also when resignation is the only other legal action left in a column-starved
    position."""
    from muzero_amd import planner as pl

    rows, cols, win = cc.SHAPES['S']
    B = 16
    p = _planner(_net('S', 41), B, 9, capture=False, num_simulations=SIMS, **BOARD_KW)
    p.arena_reset_connect4('random', 0, win)
    seen = 0
    for t in range(rows * cols):
        p.arena_step(1)
        rec = p.arena_read_ply()
        rows_ = np.flatnonzero(rec['live'].astype(bool) & (rec['side'] == pl.SIDE_RANDOM))
        for b in rows_:
            legal = np.flatnonzero(rec['mask'][b][:cols])
            u = philox_uniforms(9, int(b), t, 0x61000000, 1)[0]
            assert rec['u'][b] == u and rec['action'][b] == legal[int(np.floor(u * len(legal)))] and rec['mask'][b][cols] == 1
        seen += len(rows_)
        if p.arena_result()['live'] == 0:
            break
    assert seen > B
    p.close()


@pytest.mark.parametrize('shape', ['S', 'F'])
def test_play_match_and_evaluator_return_the_arena_tally(shape, tmp_path):
    from muzero_amd import pipeline
    from muzero_amd import planner as pl
    from muzero_amd.config import make_connect4_config
    from muzero_amd.games import ConnectFourEnv

    rows, cols, win = cc.SHAPES[shape]
    cfg = make_connect4_config(rows=rows, cols=cols, num_to_win=win, num_simulations=SIMS)
    net_a, net_b = _net(shape, 41), _net(shape, 43)
    dev = torch.device('cuda', 0)
    m = pipeline.play_match(cfg, net_a, net_b, dev, 'ConnectFour', GAMES)
    # the same arena by hand: play_match's seeds, two opening plies
    p = _planner(net_a, GAMES, 1 + 104729, capture=False, num_simulations=SIMS, **BOARD_KW)
    q = _planner(net_b, GAMES, 1 + 130003, capture=False, num_simulations=SIMS, **BOARD_KW)
    p.arena_reset_connect4(q, 2, win)
    p.arena_step(rows * cols)
    res = p.arena_result()
    p.close()
    q.close()
    assert res['live'] == 0 and m.two_player and m.num_games == GAMES
    assert np.array_equal(m.winner, res['winner']) and np.array_equal(m.length, res['length']) and np.array_equal(m.ret, res['ret'])
    assert (m.wins, m.losses, m.draws) == (res['challenger_wins'], res['opponent_wins'], res['draws'])
    assert np.array_equal(pipeline.play_match(cfg, net_a, net_b, dev, ConnectFourEnv(rows, cols, win), GAMES).winner, m.winner)
    r = pipeline.play_match(cfg, net_a, 'random', dev, 'ConnectFour', GAMES, opening_plies=2)
    assert r.num_games == GAMES and set(np.unique(r.winner)) <= {pl.ARENA_WIN_CHALLENGER, pl.ARENA_WIN_OPPONENT, pl.ARENA_DRAW}
    # the evaluator with match_games: one checkpoint of net_a's weights against net_b
    ckpt = str(tmp_path / 'c4.ckpt')
    pipeline.create_checkpoint({'network': net_a.state_dict(), 'train_steps': 7}, ckpt)
    old, new = _net(shape, 43), _net(shape, 5)
    got = []
    stop = types.SimpleNamespace(is_set=lambda: True)
    elo = pipeline.run_board_game_evaluator(cfg, old, new, dev, ConnectFourEnv(rows, cols, win), 0.0, [ckpt], stop, initial_elo=0,
                                            on_result=lambda e, steps, ts: got.append((e, steps, ts)), match_games=GAMES, opening_plies=2)
    assert got == [(m.elo(0, 0), int(round(float(m.length.mean()))), 7)] and elo == got[0][0]
