"""Go in the arena (mz_arena_reset_go) on an MI355X: every ply against host `games.GoEnv` objects and the oracle search
(tests/test_gpu_arena.py's ply-by-ply check, on this game), two weight sets and the random opponent, the tally by the area count,
balanced colours, paired openings, random moves that may pass and never resign, finished games frozen on their final boards -- captures
included -- after a two-pass end, a max_plies end and a draw; `play_match` and `run_board_game_evaluator` on top."""
import types

import numpy as np
import pytest
import torch

from helpers import philox_uniforms, seeded_state_dict
from test_gpu_arena import _planner, _play_board_match

pytestmark = pytest.mark.gpu

BOARD_KW = dict(discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0), root_dirichlet_alpha=0.25, root_exploration_eps=0.25)
GAMES, SIMS, OPENING = 8, 8, 2


def _net(rows, cols, seed):
    from muzero_amd.network import MuZeroBoardGameNet

    net = MuZeroBoardGameNet((9, rows, cols), rows * cols + 2, 1, 8)
    net.load_state_dict(seeded_state_dict(net, seed))
    net.eval()
    return net


def _make_env(rows, cols, **rules):
    from muzero_amd.games import GoEnv

    class Env(GoEnv):  # (the oracle envs' step returns three values)
        def step(self, action):
            obs, reward, done, _ = super().step(action)
            return obs, reward, done

    return lambda: Env(rows, cols, **rules)


@pytest.mark.parametrize('opponent', ['planner', 'random'])
@pytest.mark.parametrize('rows,cols,rules', [(5, 5, dict(komi2=15, max_plies=16, allow_resign=True)), (4, 6, dict(komi2=4, max_plies=14, allow_resign=False))])
def test_every_ply_against_host_envs_and_the_oracle(oracle, rows, cols, rules, opponent):
    from test_oracle_nets import _oracle_net

    nn = rows * cols
    net_p, net_q = _net(rows, cols, 41), _net(rows, cols, 43)
    p = _planner(net_p, GAMES, 7, num_simulations=SIMS, **BOARD_KW)
    q = _planner(net_q, GAMES, 8, num_simulations=SIMS, **BOARD_KW) if opponent == 'planner' else None
    cfg = oracle.make_config(nn + 2, SIMS, 1.0, True, (-1.0, 1.0), 0.25, 0.25)
    p.arena_reset_go(q if q is not None else 'random', OPENING, **rules)
    res, openings = _play_board_match(oracle, p, q, _oracle_net(oracle, net_p, 'conv'), _oracle_net(oracle, net_q, 'conv') if q is not None else None, cfg,
                                      _make_env(rows, cols, **rules), (9, rows, cols), OPENING, rules['max_plies'])
    assert res['challenger_wins'] + res['opponent_wins'] + res['draws'] == GAMES and res['live'] == 0
    for o in openings:  # paired, placements or the pass, never the resignation
        assert np.array_equal(o[:GAMES // 2], o[GAMES // 2:]) and (o <= nn).all()
    for b in range(GAMES // 2):  # legal[floor(u * n_legal)] of the pair's stream over the empty board's nn + 1 choices
        assert openings[0][b] == int(np.floor(philox_uniforms(7, b, 0, 0x60000000, 1)[0] * (nn + 1)))
    p.close()
    if q is not None:
        q.close()


def _random_moves(rows, cols, rules, seed, opening_plies, B=16):
    """To the end of every game beside host envs, every random move (opening or random opponent) checked: legal[floor(u * n)] over the
    legal placements and the pass, drawn from its own stream -- never the resignation, legal or not.  After every ply the device
    boards (`debug_go_board`) equal the host envs', live and finished alike: a finished game's row stays its final board, captures
    included.  Returns (random moves, passes among them, two-pass ends, max_plies ends, draws, capturing plies, final plies that
    captured)."""
    from muzero_amd import planner as pl

    nn, half = rows * cols, B // 2
    cap = rules['max_plies'] or 2 * nn
    p = _planner(_net(rows, cols, 41), B, seed, capture=False, num_simulations=SIMS, **BOARD_KW)
    p.arena_reset_go('random', opening_plies, **rules)
    envs = [_make_env(rows, cols, **rules)() for _ in range(B)]
    over = np.zeros(B, bool)
    seen = passes = two_pass = by_cap = draws = captures = final_captures = 0
    assert np.array_equal(p.debug_go_board(), np.stack([e.board.reshape(-1) for e in envs]))
    for t in range(cap):
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
                assert rec['u'][b] == u and a == legal[int(np.floor(u * len(legal)))] and rec['mask'][b][nn + 1] == rules['allow_resign']
                passes += a == nn
                seen += 1
            stones = np.count_nonzero(envs[b].board)
            _, _, over[b] = envs[b].step(a)
            took = a < nn and np.count_nonzero(envs[b].board) <= stones
            captures += took
            if over[b] and a <= nn:
                final_captures += took
                by_cap += envs[b].steps == cap
                two_pass += a == nn and envs[b].steps < cap
                draws += envs[b].winner is None
        # (a host env is not reset here, so a finished game's board is its final position: what the device must have frozen)
        assert np.array_equal(p.debug_go_board(), np.stack([e.board.reshape(-1) for e in envs])), t
        if over.all():
            break
    res = p.arena_result()
    assert res['live'] == 0 and over.all()
    # the tally is the host envs': a game that ended by the count was decided on the final board, captures included
    col = np.where(np.arange(B) < half, 1, 2)
    w = np.array([e.winner or 0 for e in envs])
    expect = np.where(w == 0, pl.ARENA_DRAW, np.where(w == col, pl.ARENA_WIN_CHALLENGER, pl.ARENA_WIN_OPPONENT))
    assert np.array_equal(res['winner'], expect) and np.array_equal(res['length'], [e.steps for e in envs])
    p.arena_step(1)  # plies after the end change nothing
    assert np.array_equal(p.debug_go_board(), np.stack([e.board.reshape(-1) for e in envs]))
    p.close()
    return seen, passes, two_pass, by_cap, draws, captures, final_captures


@pytest.mark.parametrize('allow_resign', [True, False])
def test_random_opponent_never_resigns(allow_resign):
    seen = _random_moves(5, 5, dict(komi2=15, max_plies=20, allow_resign=allow_resign), 9, 0)[0]
    assert seen > 16


@pytest.mark.parametrize('rows,cols,rules,seed', [(3, 3, dict(komi2=0, max_plies=14, allow_resign=True), 8),
                                                  (3, 4, dict(komi2=2, max_plies=16, allow_resign=True), 3)])
def test_frozen_final_boards_after_every_kind_of_end(rows, cols, rules, seed):
    """Every ply of the game an opening ply, so both sides draw legal[floor(u * n)] to the natural end of every game.  The seeds were
    picked on the host (the draws are Philox's, the rules the host env's) for runs that hold a two-pass end, a max_plies end, a draw
    and captures; the frozen boards are compared after every ply."""
    seen, passes, two_pass, by_cap, draws, captures, final_captures = _random_moves(rows, cols, rules, seed, rules['max_plies'])
    assert passes >= 2 and two_pass >= 2 and by_cap >= 2 and draws >= 2 and captures >= 2, (seen, passes, two_pass, by_cap, draws, captures, final_captures)


@pytest.mark.parametrize('rows,cols', [(5, 5), (4, 6)])
def test_play_match_and_evaluator_return_the_arena_tally(rows, cols, tmp_path):
    from muzero_amd import pipeline
    from muzero_amd import planner as pl
    from muzero_amd.config import make_go_config
    from muzero_amd.games import GoEnv

    rules = dict(komi2=5, max_plies=18, allow_resign=True)
    cfg = make_go_config(rows=rows, cols=cols, num_simulations=SIMS, **rules)
    net_a, net_b = _net(rows, cols, 41), _net(rows, cols, 43)
    dev = torch.device('cuda', 0)
    m = pipeline.play_match(cfg, net_a, net_b, dev, 'Go', GAMES)
    # the same arena by hand: play_match's seeds, two opening plies
    p = _planner(net_a, GAMES, 1 + 104729, capture=False, num_simulations=SIMS, **BOARD_KW)
    q = _planner(net_b, GAMES, 1 + 130003, capture=False, num_simulations=SIMS, **BOARD_KW)
    p.arena_reset_go(q, 2, **rules)
    p.arena_step(rules['max_plies'])
    res = p.arena_result()
    p.close()
    q.close()
    assert res['live'] == 0 and m.two_player and m.num_games == GAMES
    assert np.array_equal(m.winner, res['winner']) and np.array_equal(m.length, res['length']) and np.array_equal(m.ret, res['ret'])
    assert (m.wins, m.losses, m.draws) == (res['challenger_wins'], res['opponent_wins'], res['draws'])
    assert np.array_equal(pipeline.play_match(cfg, net_a, net_b, dev, GoEnv(rows, cols, **rules), GAMES).winner, m.winner)
    r = pipeline.play_match(cfg, net_a, 'random', dev, 'Go', GAMES, opening_plies=2)
    assert r.num_games == GAMES and set(np.unique(r.winner)) <= {pl.ARENA_WIN_CHALLENGER, pl.ARENA_WIN_OPPONENT, pl.ARENA_DRAW}
    # the evaluator with match_games: one checkpoint of net_a's weights against net_b
    ckpt = str(tmp_path / 'go.ckpt')
    pipeline.create_checkpoint({'network': net_a.state_dict(), 'train_steps': 7}, ckpt)
    old, new = _net(rows, cols, 43), _net(rows, cols, 5)
    got = []
    stop = types.SimpleNamespace(is_set=lambda: True)
    elo = pipeline.run_board_game_evaluator(cfg, old, new, dev, GoEnv(rows, cols, **rules), 0.0, [ckpt], stop, initial_elo=0,
                                            on_result=lambda e, steps, ts: got.append((e, steps, ts)), match_games=GAMES, opening_plies=2)
    assert got == [(m.elo(0, 0), int(round(float(m.length.mean()))), 7)] and elo == got[0][0]
