"""Othello in the arena (mz_arena_reset_othello) on an MI355X: every ply against host `games.OthelloEnv` objects and the oracle search
(tests/test_gpu_arena.py's ply-by-ply check, on this game), two weight sets and the random opponent, the tally by the stone count,
balanced colours, paired legal openings, random moves that pass where they must and never resign, frozen finished games; `play_match`
and `run_board_game_evaluator` on top."""
import types

import numpy as np
import pytest
import torch

import othello_cases as oc
from helpers import philox_uniforms, seeded_state_dict
from test_gpu_arena import _planner, _play_board_match

pytestmark = pytest.mark.gpu

BOARD_KW = dict(discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0), root_dirichlet_alpha=0.25, root_exploration_eps=0.25)
GAMES, SIMS, OPENING = 8, 8, 2


def _net(shape, seed):
    from muzero_amd.network import MuZeroBoardGameNet

    rows, cols = oc.SHAPES[shape]
    net = MuZeroBoardGameNet((9, rows, cols), rows * cols + 2, 1, 8)
    net.load_state_dict(seeded_state_dict(net, seed))
    net.eval()
    return net


def _make_env(shape):
    from muzero_amd.games import OthelloEnv

    class Env(OthelloEnv):  # (the oracle envs' step returns three values)
        def step(self, action):
            obs, reward, done, _ = super().step(action)
            return obs, reward, done

    return lambda: Env(*oc.SHAPES[shape])


@pytest.mark.parametrize('opponent', ['planner', 'random'])
@pytest.mark.parametrize('shape', ['S', 'N'])
def test_every_ply_against_host_envs_and_the_oracle(oracle, shape, opponent):
    from test_oracle_nets import _oracle_net

    rows, cols = oc.SHAPES[shape]
    nn = rows * cols
    net_p, net_q = _net(shape, 41), _net(shape, 43)
    p = _planner(net_p, GAMES, 7, num_simulations=SIMS, **BOARD_KW)
    q = _planner(net_q, GAMES, 8, num_simulations=SIMS, **BOARD_KW) if opponent == 'planner' else None
    cfg = oracle.make_config(nn + 2, SIMS, 1.0, True, (-1.0, 1.0), 0.25, 0.25)
    p.arena_reset_othello(q if q is not None else 'random', OPENING)
    res, openings = _play_board_match(oracle, p, q, _oracle_net(oracle, net_p, 'conv'), _oracle_net(oracle, net_q, 'conv') if q is not None else None, cfg,
                                      _make_env(shape), (9, rows, cols), OPENING, 2 * (nn - 4))
    assert res['challenger_wins'] + res['opponent_wins'] + res['draws'] == GAMES and res['live'] == 0
    env = _make_env(shape)()
    first = np.flatnonzero(env.actions_mask[:nn])
    for t, o in enumerate(openings):  # paired, legal placements, never the resignation
        assert np.array_equal(o[:GAMES // 2], o[GAMES // 2:]) and (o < nn).all()
    for b in range(GAMES // 2):  # legal[floor(u * n_legal)] of the pair's stream over the start position's four placements
        assert openings[0][b] == first[int(np.floor(philox_uniforms(7, b, 0, 0x60000000, 1)[0] * len(first)))]
    p.close()
    if q is not None:
        q.close()


def _random_moves(seed, opening_plies, B=16):
    """To the end of every game on S beside host envs, every random move (opening or random opponent) checked: legal[floor(u * n)] over
    the legal placements, drawn from its own stream, or the pass where there is no placement -- never the resignation, which is legal
    throughout.  After every ply the device boards (`debug_othello_board`) equal the host envs', live and finished alike: a finished
    game's row stays its final board, flips included.  Returns (random moves, passes among them, games that ended by the count, of
    those the wipe-outs, of those the ones with empty cells left)."""
    from muzero_amd import planner as pl

    rows, cols = oc.SHAPES['S']
    nn, half = rows * cols, B // 2
    p = _planner(_net('S', 41), B, seed, capture=False, num_simulations=SIMS, **BOARD_KW)
    p.arena_reset_othello('random', opening_plies)
    envs = [_make_env('S')() for _ in range(B)]
    over = np.zeros(B, bool)
    seen = passes = counted = wiped = early = 0
    assert np.array_equal(p.debug_othello_board(), np.stack([e.board.reshape(-1) for e in envs]))
    for t in range(2 * (nn - 4)):
        p.arena_step(1)
        rec = p.arena_read_ply()
        assert np.array_equal(rec['live'].astype(bool), ~over)
        for b in np.flatnonzero(~over):
            a = int(rec['action'][b])
            assert np.array_equal(rec['mask'][b].astype(bool), envs[b].actions_mask)
            if rec['side'][b] in (pl.SIDE_RANDOM, pl.SIDE_OPENING):
                opening = rec['side'][b] == pl.SIDE_OPENING
                legal = np.flatnonzero(rec['mask'][b][:nn + 1])
                u = philox_uniforms(seed, int(b) % half if opening else int(b), t, 0x60000000 if opening else 0x61000000, 1)[0]
                assert rec['u'][b] == u and a == legal[int(np.floor(u * len(legal)))] and rec['mask'][b][nn + 1] == 1
                if a == nn:
                    assert not rec['mask'][b][:nn].any()
                    passes += 1
                seen += 1
            _, _, over[b] = envs[b].step(a)
            if over[b] and a < nn:
                counted += 1
                wiped += min((envs[b].board == 1).sum(), (envs[b].board == 2).sum()) == 0
                early += bool((envs[b].board == 0).any())
        # (a host env is not reset here, so a finished game's board is its final position: what the device must have frozen)
        assert np.array_equal(p.debug_othello_board(), np.stack([e.board.reshape(-1) for e in envs])), t
        if over.all():
            break
    res = p.arena_result()
    assert res['live'] == 0 and over.all()
    # the tally is the host envs': a game that ended by the count was decided on the final board, flips included
    col = np.where(np.arange(B) < half, 1, 2)
    w = np.array([e.winner or 0 for e in envs])
    expect = np.where(w == 0, pl.ARENA_DRAW, np.where(w == col, pl.ARENA_WIN_CHALLENGER, pl.ARENA_WIN_OPPONENT))
    assert np.array_equal(res['winner'], expect) and np.array_equal(res['length'], [e.steps for e in envs])
    p.arena_step(1)  # plies after the end change nothing
    assert np.array_equal(p.debug_othello_board(), np.stack([e.board.reshape(-1) for e in envs]))
    p.close()
    return seen, passes, counted, wiped, early


def test_random_opponent_never_resigns():
    seen = _random_moves(9, 0)[0]
    assert seen > 16


def test_random_moves_pass_where_they_must():
    """The scripted start that forces passes: every ply of the game an opening ply, so both sides draw legal[floor(u * n)] to the natural
    end of every game (an untrained net's search resigns long before a pass comes up).  53 % of uniformly random 4 x 4 games hold a
    pass; the games end by the count, with the winner read off the final board.  Seed 7 was picked on the host (the draws are Philox's,
    the rules the host env's) for a run whose frozen final boards include a wipe-out, ends with empty cells and a draw."""
    seen, passes, counted, wiped, early = _random_moves(7, 24)
    assert passes >= 1 and counted == 16 and wiped >= 1 and early >= 1, (seen, passes, counted, wiped, early)


@pytest.mark.parametrize('shape', ['S', 'N'])
def test_play_match_and_evaluator_return_the_arena_tally(shape, tmp_path):
    from muzero_amd import pipeline
    from muzero_amd import planner as pl
    from muzero_amd.config import make_othello_config
    from muzero_amd.games import OthelloEnv

    rows, cols = oc.SHAPES[shape]
    nn = rows * cols
    cfg = make_othello_config(rows=rows, cols=cols, num_simulations=SIMS)
    net_a, net_b = _net(shape, 41), _net(shape, 43)
    dev = torch.device('cuda', 0)
    m = pipeline.play_match(cfg, net_a, net_b, dev, 'Othello', GAMES)
    # the same arena by hand: play_match's seeds, two opening plies
    p = _planner(net_a, GAMES, 1 + 104729, capture=False, num_simulations=SIMS, **BOARD_KW)
    q = _planner(net_b, GAMES, 1 + 130003, capture=False, num_simulations=SIMS, **BOARD_KW)
    p.arena_reset_othello(q, 2)
    p.arena_step(2 * (nn - 4))
    res = p.arena_result()
    p.close()
    q.close()
    assert res['live'] == 0 and m.two_player and m.num_games == GAMES
    assert np.array_equal(m.winner, res['winner']) and np.array_equal(m.length, res['length']) and np.array_equal(m.ret, res['ret'])
    assert (m.wins, m.losses, m.draws) == (res['challenger_wins'], res['opponent_wins'], res['draws'])
    assert np.array_equal(pipeline.play_match(cfg, net_a, net_b, dev, OthelloEnv(rows, cols), GAMES).winner, m.winner)
    r = pipeline.play_match(cfg, net_a, 'random', dev, 'Othello', GAMES, opening_plies=2)
    assert r.num_games == GAMES and set(np.unique(r.winner)) <= {pl.ARENA_WIN_CHALLENGER, pl.ARENA_WIN_OPPONENT, pl.ARENA_DRAW}
    # the evaluator with match_games: one checkpoint of net_a's weights against net_b
    ckpt = str(tmp_path / 'othello.ckpt')
    pipeline.create_checkpoint({'network': net_a.state_dict(), 'train_steps': 7}, ckpt)
    old, new = _net(shape, 43), _net(shape, 5)
    got = []
    stop = types.SimpleNamespace(is_set=lambda: True)
    elo = pipeline.run_board_game_evaluator(cfg, old, new, dev, OthelloEnv(rows, cols), 0.0, [ckpt], stop, initial_elo=0,
                                            on_result=lambda e, steps, ts: got.append((e, steps, ts)), match_games=GAMES, opening_plies=2)
    assert got == [(m.elo(0, 0), int(round(float(m.length.mean()))), 7)] and elo == got[0][0]
