"""The arena (mz_arena_*: evaluation games in lock-step on the device, no noise, no auto-reset, two weight sets) on an MI355X: every
searched move against the oracle search, the env bookkeeping against the oracle envs, the tally, the random moves, the errors and
pipeline.play_match on top."""
import ctypes as C
import types

import numpy as np
import pytest

from helpers import build_conv, build_mlp, conv_case, mlp_case, philox_uniforms

pytestmark = pytest.mark.gpu

BOARD_KW = dict(discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0), root_dirichlet_alpha=0.25, root_exploration_eps=0.25)


def _planner(net, num_envs, seed, capture=True, **search):
    from muzero_amd import planner as pl

    p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=num_envs, seed=seed, **search), 0)
    p.load_state_dict(net.state_dict())
    p.lib.mz_debug_capture_rng.argtypes = [C.c_void_p, C.c_int32]
    p.lib.mz_debug_read_rng.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if capture:
        assert p.lib.mz_debug_capture_rng(p.h, 1) == 0
    return p


def _ties(p):
    u = np.empty((p.B, p.max_ties), np.float64)
    assert p.lib.mz_debug_read_rng(p.h, None, u.ctypes.data_as(C.c_void_p), None) == 0
    return u


def _reseeded(net_builder, case, seed):
    from helpers import seeded_state_dict

    net = net_builder(case)
    net.load_state_dict(seeded_state_dict(net, seed))
    net.eval()
    return net


def _check_search(oracle, cfg, onet, rec, rows, lo, utie, ply, shape):
    """Policy, root value and action of the envs `rows` (one searched run starting at env `lo`) equal the oracle's deterministic search
    of the recorded roots with the captured tie draws (run-relative rows of `utie`).  The documented deviation of test_gpu_selfplay's
    selfplay_search_vs_oracle: where every root visit fell on illegal actions the reference's policy is 0 / 0; there only legality is
    checked."""
    if rows.size == 0:
        return
    cur = rec['player'][rows]
    o = oracle.uct_search_batch(cfg, onet, rec['obs'][rows].reshape((rows.size,) + shape), rec['mask'][rows], cur, 3 - cur if cfg.is_board_game else cur,
                                1.0, True, u_tie=utie[rows - lo])
    ok = ~np.isnan(o['pi']).any(axis=1)
    np.testing.assert_array_equal(rec['pi'][rows][ok], o['pi'][ok], err_msg=f'ply {ply}: policy')
    np.testing.assert_array_equal(rec['root_value'][rows][ok], o['root_value'][ok], err_msg=f'ply {ply}: root value')
    np.testing.assert_array_equal(rec['action'][rows][ok], o['action'][ok], err_msg=f'ply {ply}: action')
    for r in rows[~ok]:
        assert rec['mask'][r, rec['action'][r]]


def _expected_sides(pl, B, ply, opening_plies, opponent_side):
    half = B // 2
    if ply < opening_plies:
        return np.full(B, pl.SIDE_OPENING, np.int32)
    lower = pl.SIDE_CHALLENGER if ply % 2 == 0 else opponent_side
    upper = opponent_side if ply % 2 == 0 else pl.SIDE_CHALLENGER
    return np.concatenate([np.full(half, lower, np.int32), np.full(half, upper, np.int32)])


def _play_board_match(oracle, p, q, onet_p, onet_q, cfg, make_env, shape, opening_plies, max_plies, to_the_end=True):
    """Play ply by ply beside B oracle envs; check roots, sides, searches, freezing, and (when every game ended) the tally."""
    from muzero_amd import planner as pl

    B, half = p.B, p.B // 2
    envs = [make_env() for _ in range(B)]
    done = np.zeros(B, bool)
    winner = np.zeros(B, np.int32)
    length = np.zeros(B, np.int32)
    prev = None
    openings = []
    for t in range(max_plies):
        p.arena_step(1)
        rec = p.arena_read_ply()
        live = ~done
        np.testing.assert_array_equal(rec['live'].astype(bool), live, err_msg=f'ply {t}: live flags')
        sides = _expected_sides(pl, B, t, opening_plies, pl.SIDE_OPPONENT if q is not None else pl.SIDE_RANDOM)
        np.testing.assert_array_equal(rec['side'][live], sides[live], err_msg=f'ply {t}: searching side')
        for b in np.flatnonzero(live):
            np.testing.assert_array_equal(rec['obs'][b].reshape(shape), envs[b].observation().astype(np.float32))
            np.testing.assert_array_equal(rec['mask'][b].astype(bool), envs[b].actions_mask)
            assert rec['player'][b] == envs[b].current_player == 1 + t % 2
        if prev is not None:  # a frozen env's record stops changing
            for k in ('obs', 'mask', 'player', 'side', 'pi', 'root_value', 'action', 'u'):
                np.testing.assert_array_equal(rec[k][done], prev[k][done], err_msg=f'ply {t}: frozen record field {k}')
        if t < opening_plies:
            openings.append(rec['action'].copy())
            np.testing.assert_array_equal(rec['action'][:half], rec['action'][half:], err_msg='a pair shares its opening')
        else:
            up, uq = _ties(p), (_ties(q) if q is not None else None)
            for side, onet, utie in ((pl.SIDE_CHALLENGER, onet_p, up), (pl.SIDE_OPPONENT, onet_q, uq)):
                rows = np.flatnonzero(live & (sides == side))
                if utie is not None and rows.size:
                    _check_search(oracle, cfg, onet, rec, rows, 0 if rows[0] < half else half, utie, t, shape)
        for b in np.flatnonzero(live):
            a = int(rec['action'][b])
            assert envs[b].actions_mask[a], f'ply {t}, env {b}: illegal action {a}'
            _, _, d = envs[b].step(a)
            length[b] += 1
            if d:
                done[b] = True
                col = 1 if b < half else 2  # the challenger's colour
                w = envs[b].winner
                winner[b] = pl.ARENA_DRAW if w not in (1, 2) else (pl.ARENA_WIN_CHALLENGER if w == col else pl.ARENA_WIN_OPPONENT)
        res = p.arena_result()
        assert res['live'] == int((~done).sum()), f'ply {t}: done flags'
        np.testing.assert_array_equal(res['winner'] != pl.ARENA_UNFINISHED, done, err_msg=f'ply {t}: done flags')
        prev = rec
        if done.all():
            break
    res = p.arena_result()
    if to_the_end:
        assert done.all(), 'every game ends within the env cap'
    np.testing.assert_array_equal(res['winner'], winner)
    np.testing.assert_array_equal(res['length'][done], length[done])
    assert res['challenger_wins'] == int((winner == pl.ARENA_WIN_CHALLENGER).sum())
    assert res['opponent_wins'] == int((winner == pl.ARENA_WIN_OPPONENT).sum())
    assert res['draws'] == int((winner == pl.ARENA_DRAW).sum())
    assert res['finished_plies'] == int(length[done].sum())
    expect_ret = np.where(winner == pl.ARENA_WIN_CHALLENGER, 1.0, np.where(winner == pl.ARENA_WIN_OPPONENT, -1.0, 0.0))
    np.testing.assert_array_equal(res['ret'], expect_ret)
    return res, openings


def test_tictactoe_net_vs_net_every_move_equals_the_oracle(oracle):
    """TicTacToe, MLP net vs a differently seeded one, B = 256, 25 simulations, 2 opening plies: every ply's roots equal the oracle
    BoardEnv, both sides' searches equal oracle.uct_search_batch(deterministic=True) with the captured tie draws, pairs share their
    openings, frozen records stop changing and the tally equals the oracle envs'.  Budget: 6 s (9 plies, 256 oracle searches each)."""
    from test_oracle_nets import _oracle_net
    from muzero_amd import planner as pl

    case = mlp_case('tictactoe')
    net_p, net_q = build_mlp(case), _reseeded(build_mlp, case, 113)
    B, S = 256, 25
    p = _planner(net_p, B, 5, num_simulations=S, **BOARD_KW)
    q = _planner(net_q, B, 6, num_simulations=S, **BOARD_KW)
    cfg = oracle.make_config(10, S, 1.0, True, (-1.0, 1.0), 0.25, 0.25)
    p.arena_reset(pl.ENV_TICTACTOE, q, opening_plies=2)
    res, openings = _play_board_match(oracle, p, q, _oracle_net(oracle, net_p, 'mlp'), _oracle_net(oracle, net_q, 'mlp'), cfg,
                                      lambda: oracle.BoardEnv(3, 4, 3), (9, 3, 3), 2, 9)
    assert len(np.unique(openings[0])) > 3  # the openings differ between pairs
    assert res['challenger_wins'] + res['opponent_wins'] + res['draws'] == B
    p.close()
    q.close()


def test_gomoku_conv_net_vs_net_to_the_end_of_every_game(oracle):
    """Gomoku 9 x 9 (conv `board9` case vs a second seed), B = 32, 8 simulations, to the end of every game: the same checks as the
    TicTacToe test on the wave-per-env step (81 points: more than one 64-lane chunk).  Budget: 10 s (at most 81 plies)."""
    from test_oracle_nets import _oracle_net
    from muzero_amd import planner as pl

    case = conv_case('board9')
    net_p, net_q = build_conv(case), _reseeded(build_conv, case, 123)
    B, S = 32, 8
    kw = dict(BOARD_KW, root_dirichlet_alpha=0.03)
    p = _planner(net_p, B, 7, num_simulations=S, **kw)
    q = _planner(net_q, B, 8, num_simulations=S, **kw)
    cfg = oracle.make_config(82, S, 1.0, True, (-1.0, 1.0), 0.03, 0.25)
    p.arena_reset(pl.ENV_GOMOKU, q, opening_plies=2)
    _play_board_match(oracle, p, q, _oracle_net(oracle, net_p, 'conv'), _oracle_net(oracle, net_q, 'conv'), cfg,
                      lambda: oracle.BoardEnv(9, 4, 5), (9, 9, 9), 2, 81)
    p.close()
    q.close()


def test_gomoku_19x19_wide_action_pick_and_step(oracle):
    """19 x 19 (362 actions, six 64-lane chunks): 3 opening plies through the wide pick, then 3 searched plies, B = 8, 8 simulations,
    checked like the full games.  Budget: 5 s."""
    from board19_cases import board_case
    from test_oracle_nets import _oracle_net
    from muzero_amd import planner as pl

    case = board_case('board19')
    net_p, net_q = build_conv(case), _reseeded(build_conv, case, 131)
    B, S = 8, 8
    kw = dict(BOARD_KW, root_dirichlet_alpha=0.03)
    p = _planner(net_p, B, 9, num_simulations=S, **kw)
    q = _planner(net_q, B, 10, num_simulations=S, **kw)
    cfg = oracle.make_config(362, S, 1.0, True, (-1.0, 1.0), 0.03, 0.25)
    p.arena_reset(pl.ENV_GOMOKU, q, opening_plies=3)
    _, openings = _play_board_match(oracle, p, q, _oracle_net(oracle, net_p, 'conv'), _oracle_net(oracle, net_q, 'conv'), cfg,
                                    lambda: oracle.BoardEnv(19, 4, 5), (9, 19, 19), 3, 6, to_the_end=False)
    assert max(int(o.max()) for o in openings) > 64  # moves beyond the first chunk were picked
    p.close()
    q.close()


def test_pairing_and_first_searching_side():
    """Envs i and i + B/2 record identical opening actions, drawn as legal[floor(u * n_legal)] from the pair's Philox stream; at the
    first search ply the challenger searches the lower half and the opponent the upper half.  Budget: 2 s."""
    from muzero_amd import planner as pl

    case = mlp_case('tictactoe')
    B, seed, opening = 64, 21, 2  # (an even number of opening plies: black, the lower half's challenger, searches first)
    p = _planner(build_mlp(case), B, seed, capture=False, num_simulations=10, **BOARD_KW)
    q = _planner(_reseeded(build_mlp, case, 113), B, 22, capture=False, num_simulations=10, **BOARD_KW)
    p.arena_reset(pl.ENV_TICTACTOE, q, opening_plies=opening)
    for t in range(opening):
        p.arena_step(1)
        rec = p.arena_read_ply()
        lv = rec['live'].astype(bool)
        assert (rec['side'][lv] == pl.SIDE_OPENING).all()
        both = lv[:B // 2] & lv[B // 2:]
        np.testing.assert_array_equal(rec['action'][:B // 2][both], rec['action'][B // 2:][both])
        for b in np.flatnonzero(lv):
            u = philox_uniforms(seed, int(b) % (B // 2), t, 0x60000000, 1)[0]
            assert rec['u'][b] == u
            legal = np.flatnonzero(rec['mask'][b])
            assert rec['action'][b] == legal[int(np.floor(u * len(legal)))]
    p.arena_step(1)
    rec = p.arena_read_ply()
    lv = rec['live'].astype(bool)
    assert lv[:B // 2].any() and lv[B // 2:].any()
    assert (rec['side'][:B // 2][lv[:B // 2]] == pl.SIDE_CHALLENGER).all() and (rec['side'][B // 2:][lv[B // 2:]] == pl.SIDE_OPPONENT).all()
    p.close()
    q.close()


def test_random_opponent_moves_are_the_recorded_draws_and_uniform(oracle):
    """MZ_ARENA_RANDOM on TicTacToe, B = 512 (256 games in which the random side opens on the empty board): every random move equals
    legal[floor(u * n_legal)] from the recorded u and mask, u is the env's Philox draw, all moves are legal, the challenger's moves equal
    the oracle search, and the 256 first moves on the empty board pass a chi-square test of uniformity over the 10 legal actions at
    significance 0.001 (9 degrees of freedom: critical value 27.877; seed fixed, so the outcome is reproducible).  Budget: 6 s."""
    from test_oracle_nets import _oracle_net
    from muzero_amd import planner as pl

    net = build_mlp(mlp_case('tictactoe'))
    B, S, seed = 512, 25, 31
    p = _planner(net, B, seed, num_simulations=S, **BOARD_KW)
    cfg = oracle.make_config(10, S, 1.0, True, (-1.0, 1.0), 0.25, 0.25)
    p.arena_reset(pl.ENV_TICTACTOE, 'random', opening_plies=0)
    res, _ = _play_board_match(oracle, p, None, _oracle_net(oracle, net, 'mlp'), None, cfg, lambda: oracle.BoardEnv(3, 4, 3), (9, 3, 3), 0, 9)
    assert res['challenger_wins'] + res['opponent_wins'] + res['draws'] == B
    # again, looking at the random side only
    p.arena_reset(pl.ENV_TICTACTOE, 'random', opening_plies=0)
    first = None
    for t in range(9):
        p.arena_step(1)
        rec = p.arena_read_ply()
        rows = np.flatnonzero(rec['live'].astype(bool) & (rec['side'] == pl.SIDE_RANDOM))
        assert (rows >= B // 2).all() if t % 2 == 0 else (rows < B // 2).all()
        for b in rows[:: 1 if t < 2 else 7]:
            assert rec['u'][b] == philox_uniforms(seed, int(b), t, 0x61000000, 1)[0]
        for b in rows:
            legal = np.flatnonzero(rec['mask'][b])
            assert rec['action'][b] == legal[int(np.floor(rec['u'][b] * len(legal)))]
        if t == 0:
            first = rec['action'][B // 2:].copy()
            assert rows.size == B // 2 and (rec['mask'][B // 2:] == 1).all()
    counts = np.bincount(first, minlength=10).astype(np.float64)
    expected = len(first) / 10.0
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    assert chi2 < 27.877, (chi2, counts)
    p.close()


def test_cartpole_episodes_freeze_at_done_and_replay_on_the_host(oracle):
    """CartPole, no opponent, B = 64 from given initial states, 50 simulations: every move equals the oracle search, episodes freeze at
    done, and per-env return and length equal a host replay of the recorded actions through games.CartPoleEnv.  Budget: 8 s
    (random-weight policies drop the pole within a few dozen steps; the loop is bounded by the env cap of 500)."""
    from test_oracle_nets import _oracle_net
    from muzero_amd import planner as pl
    from muzero_amd.games import CartPoleEnv

    net = build_mlp(mlp_case('cartpole'))
    B, S = 64, 50
    init = np.random.RandomState(4).uniform(-0.05, 0.05, size=(B, 4))
    p = _planner(net, B, 41, num_simulations=S, discount=0.997)
    cfg = oracle.make_config(2, S, 0.997, False, None, 0.25, 0.25)
    onet = _oracle_net(oracle, net, 'mlp')
    p.arena_reset(pl.ENV_CARTPOLE, None, 0, init)
    actions = [[] for _ in range(B)]
    done = np.zeros(B, bool)
    prev = None
    for t in range(500):
        p.arena_step(1)
        rec = p.arena_read_ply()
        live = ~done
        np.testing.assert_array_equal(rec['live'].astype(bool), live)
        assert (rec['side'][live] == pl.SIDE_CHALLENGER).all() and (rec['player'] == 1).all() and (rec['mask'] == 1).all()
        _check_search(oracle, cfg, onet, rec, np.flatnonzero(live), 0, _ties(p), t, (4, 5))
        if prev is not None:
            for k in ('obs', 'pi', 'root_value', 'action'):
                np.testing.assert_array_equal(rec[k][done], prev[k][done], err_msg=f'ply {t}: frozen record field {k}')
        for b in np.flatnonzero(live):
            actions[b].append(int(rec['action'][b]))
        res = p.arena_result()
        done = res['winner'] != pl.ARENA_UNFINISHED
        assert res['live'] == int((~done).sum())
        np.testing.assert_array_equal(res['length'][~done], t + 1)
        prev = rec
        if done.all():
            break
    assert done.all()
    env = CartPoleEnv()
    for b in range(B):
        env.reset(state=init[b])
        total, d = 0.0, False
        for a in actions[b]:
            assert not d
            _, r, d, _ = env.step(a)
            total += r
        assert d and res['length'][b] == len(actions[b]) and res['ret'][b] == total
    assert res['draws'] == B and res['finished_plies'] == int(res['length'].sum())
    p.close()


def test_arena_errors():
    """Every refused call returns its status and leaves the handles usable.  Budget: 3 s."""
    import torch
    from muzero_amd import planner as pl

    case = mlp_case('tictactoe')
    net = build_mlp(case)
    p = _planner(net, 16, 1, capture=False, num_simulations=5, **BOARD_KW)
    lib = p.lib

    assert lib.mz_arena_step(p.h, 1) == -3  # MZ_E_STATE: step before reset
    q_sims = _planner(net, 16, 2, capture=False, num_simulations=6, **BOARD_KW)  # mismatched config
    assert lib.mz_arena_reset(p.h, pl.ENV_TICTACTOE, pl.ARENA_PLANNER, q_sims.h, 0, None) == -1
    q_envs = _planner(net, 32, 2, capture=False, num_simulations=5, **BOARD_KW)
    assert lib.mz_arena_reset(p.h, pl.ENV_TICTACTOE, pl.ARENA_PLANNER, q_envs.h, 0, None) == -1
    if torch.cuda.device_count() > 1:  # an opponent on another device
        q_dev = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=16, seed=2, num_simulations=5, **BOARD_KW), 1)
        q_dev.load_state_dict(net.state_dict())
        assert lib.mz_arena_reset(p.h, pl.ENV_TICTACTOE, pl.ARENA_PLANNER, q_dev.h, 0, None) == -1
        q_dev.close()
    q_raw = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=16, seed=2, num_simulations=5, **BOARD_KW), 0)  # no weights
    assert lib.mz_arena_reset(p.h, pl.ENV_TICTACTOE, pl.ARENA_PLANNER, q_raw.h, 0, None) == -3
    assert lib.mz_arena_reset(p.h, pl.ENV_TICTACTOE, pl.ARENA_PLANNER, None, 0, None) == -1
    assert lib.mz_arena_reset(p.h, pl.ENV_TICTACTOE, pl.ARENA_NONE, None, 0, None) == -1  # a two-player env without an opponent
    assert lib.mz_arena_reset(p.h, pl.ENV_EXTERNAL, pl.ARENA_RANDOM, None, 0, None) == -1
    assert lib.mz_arena_reset(p.h, pl.ENV_SYNTHETIC, pl.ARENA_NONE, None, 0, None) == -1
    assert lib.mz_arena_reset(p.h, pl.ENV_TICTACTOE, pl.ARENA_RANDOM, None, -1, None) == -1
    odd = _planner(net, 15, 1, capture=False, num_simulations=5, **BOARD_KW)
    assert lib.mz_arena_reset(odd.h, pl.ENV_TICTACTOE, pl.ARENA_RANDOM, None, 0, None) == -1  # odd B for a two-player env
    assert lib.mz_arena_step(p.h, 1) == -3  # none of the refused resets opened an arena
    # self-play and arena exclude each other
    p.selfplay_reset(pl.ENV_TICTACTOE)
    p.selfplay_step(-1.0, 1)
    assert lib.mz_arena_step(p.h, 1) == -3
    p.arena_reset(pl.ENV_TICTACTOE, 'random')
    assert lib.mz_selfplay_step(p.h, C.c_double(1.0), 1) == -3
    assert lib.mz_arena_step(p.h, 0) == -1  # n_plies < 1
    p.arena_step(2)
    assert p.arena_result()['live'] <= 16
    with pytest.raises(pl.PlannerError):
        p.selfplay_step(1.0, 1)
    p.selfplay_reset(pl.ENV_TICTACTOE)  # back to self-play
    p.selfplay_step(-1.0, 1)
    with pytest.raises(pl.PlannerError):
        p.arena_step(1)
    for h in (p, q_sims, q_envs, q_raw, odd):
        h.close()


def _fold(winner, r, opp):
    from muzero_amd.rating import compute_elo_rating

    for w in winner:
        if w == 1:
            r, _ = compute_elo_rating(0, r, opp)
        elif w == 2:
            r, _ = compute_elo_rating(1, r, opp)
    return r


@pytest.mark.parametrize('game', ['tictactoe', 'board9'])
def test_play_match_counts_and_elo(game):
    """pipeline.play_match: the counts equal arena_result's of the same match played by hand (same seeds), the Elo equals the fold.
    Budget: 5 s."""
    import torch
    from muzero_amd import pipeline, planner as pl
    from muzero_amd.config import make_gomoku_config, make_tictactoe_config

    if game == 'tictactoe':
        case, build, cfg, env, kind, n = mlp_case('tictactoe'), build_mlp, make_tictactoe_config(use_tensorboard=False), 'TicTacToe', pl.ENV_TICTACTOE, 32
        cfg.num_simulations = 12
    else:
        case, build, cfg, env, kind, n = conv_case('board9'), build_conv, make_gomoku_config(use_tensorboard=False), 'Gomoku', pl.ENV_GOMOKU, 16
        cfg.num_simulations = 6
    net_p, net_q = build(case), _reseeded(build, case, 113)
    m = pipeline.play_match(cfg, net_p, net_q, torch.device('cuda', 0), env, n, opening_plies=2)
    seed = int(getattr(cfg, 'planner_seed', 1))
    p = pl.Planner(pl.make_mz_config(net_p.planner_spec(), cfg, num_envs=n, seed=seed + 104729), 0)
    q = pl.Planner(pl.make_mz_config(net_q.planner_spec(), cfg, num_envs=n, seed=seed + 130003), 0)
    p.load_state_dict(net_p.state_dict())
    q.load_state_dict(net_q.state_dict())
    p.arena_reset(kind, q, 2)
    p.arena_step(p.A - 1)
    res = p.arena_result()
    assert res['live'] == 0
    assert (m.wins, m.losses, m.draws) == (res['challenger_wins'], res['opponent_wins'], res['draws']) and m.num_games == n
    np.testing.assert_array_equal(m.winner, res['winner'])
    np.testing.assert_array_equal(m.length, res['length'])
    np.testing.assert_array_equal(m.ret, res['ret'])
    assert m.elo(-2000, -2000) == _fold(res['winner'], -2000, -2000)
    bc = m.by_colour()
    assert sum(bc['black']) == sum(bc['white']) == n // 2 and bc['black'][0] + bc['white'][0] == m.wins
    p.close()
    q.close()


def test_board_game_evaluator_with_match_games(tmp_path):
    """run_board_game_evaluator(match_games=16) over two checkpoints returns the Elo of the two matches folded in turn and calls
    on_result once per checkpoint.  Budget: 5 s."""
    import torch
    from muzero_amd import pipeline
    from muzero_amd.config import make_tictactoe_config
    from muzero_amd.games import TicTacToeEnv

    case = mlp_case('tictactoe')
    cfg = make_tictactoe_config(use_tensorboard=False)
    cfg.num_simulations = 12
    dev = torch.device('cuda', 0)
    nets = [_reseeded(build_mlp, case, s) for s in (201, 202)]
    files = []
    for i, net in enumerate(nets):
        f = str(tmp_path / f'ckpt{i}.pt')
        pipeline.create_checkpoint({'network': net.state_dict(), 'train_steps': 100 * (i + 1)}, f)
        files.append(f)
    old, new = build_mlp(case), build_mlp(case)
    base = build_mlp(case)
    expect = -2000
    prev = base
    for net in nets:
        m = pipeline.play_match(cfg, net, prev, dev, 'TicTacToe', 16, opening_plies=2)
        expect = m.elo(expect, expect)
        prev = net
    calls = []
    stop = types.SimpleNamespace(is_set=lambda: True)
    elo = pipeline.run_board_game_evaluator(cfg, old, new, dev, TicTacToeEnv(), 0.1, files, stop, on_result=lambda *a: calls.append(a), match_games=16)
    assert elo == expect
    assert len(calls) == 2 and [c[2] for c in calls] == [100, 200] and calls[-1][0] == elo
