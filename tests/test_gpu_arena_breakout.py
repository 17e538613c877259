"""The device Breakout arena (mz_arena_reset_breakout, csrc/mz_breakout.h on csrc/mz_arena_image.h's ply) on an MI355X, as
test_gpu_arena_image.py holds Catch: every ply against host games.make_breakout_env objects byte for byte and against the oracle's
deterministic search, games that end on different plies, frozen envs, returns that are the exact brick counts, NULL and explicit start
codes, batching and repeatability, the refusals by name, and pipeline.play_match / run_evaluator on top."""
import ctypes as C
import types

import numpy as np
import pytest

import breakout_cases as bc
from helpers import build_conv, build_mlp

pytestmark = pytest.mark.gpu

REC = ('obs', 'mask', 'player', 'side', 'pi', 'root_value', 'action', 'u', 'live')
# name -> (net builder, breakout_cases.SHAPES key, move cap, S, games, simulations, oracle net kind, start codes or None)
RUNS = {
    'g43': (lambda: build_mlp(('bo43', (4, 12, 12), 3, 32, 7, 5, 16, 51)), 'g43', 12, 2, 12, 4, 'mlp', None),
    'g68': (lambda: build_mlp(('bo68', (4, 12, 24), 3, 32, 7, 5, 16, 52)), 'g68', 10, 2, 8, 4, 'mlp', [15, 0, 7, 8, 3, 12, 1, 14]),
    'g32': (lambda: build_mlp(('bo32', (4, 8, 32), 3, 32, 7, 5, 16, 53)), 'g32', 8, 2, 6, 4, 'mlp', [63, 0, 62, 1, 31, 32]),
    # 7 games x 180 bytes = 1260: the renderer's 16-byte runs cross from env to env and the last one ends in the allocation's padding
    'g65': (lambda: build_mlp(('bo65', (4, 12, 15), 3, 32, 7, 5, 16, 54)), 'g65', 10, 2, 7, 4, 'mlp', [9, 0, 4, 5, 2, 7, 1]),
    'atari': (lambda: build_conv(('atari_s8', 'atari', (8, 96, 96), 3, 1, 8, 11, 11, 24)), 'atari', 6, 4, 4, 3, 'conv', [0, 23, 11, 12]),
}
SEED = 9


def _planner(net, B, sims, seed=SEED, capture=False, **kw):
    from muzero_amd import planner as pl

    kw.setdefault('discount', 0.997)
    p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=B, seed=seed, num_simulations=sims, keep_shape=True, **kw), 0)
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


def _check_search(oracle, cfg, onet, rec, rows, utie, ply, shape):
    """Policy, root value and action of the envs `rows` equal the oracle's deterministic search of the recorded roots with the captured
    tie draws (the pattern of test_gpu_arena_image.py)."""
    if rows.size == 0:
        return
    cur = rec['player'][rows]
    o = oracle.uct_search_batch(cfg, onet, rec['obs'][rows].reshape((rows.size,) + shape), rec['mask'][rows], cur, cur, 1.0, True, u_tie=utie[rows])
    ok = ~np.isnan(o['pi']).any(axis=1)
    np.testing.assert_array_equal(rec['pi'][rows][ok], o['pi'][ok], err_msg=f'ply {ply}: policy')
    np.testing.assert_array_equal(rec['root_value'][rows][ok], o['root_value'][ok], err_msg=f'ply {ply}: root value')
    np.testing.assert_array_equal(rec['action'][rows][ok], o['action'][ok], err_msg=f'ply {ply}: action')
    for r in rows[~ok]:
        assert rec['mask'][r, rec['action'][r]]


def _tally(res):
    return {k: res[k] for k in ('challenger_wins', 'opponent_wins', 'draws', 'finished_plies', 'live')}


def _host(name):
    from muzero_amd.games import make_breakout_env

    _, key, cap, S, B, _, _, codes = RUNS[name]
    rows, cols, ch, cw, K, _ = bc.SHAPES[key]
    start = [e % (2 * cols) for e in range(B)] if codes is None else codes
    return [make_breakout_env(rows, cols, ch, cw, stack_history=S, brick_rows=K, max_moves=cap, start_codes=[int(k)]) for k in start]


@pytest.mark.parametrize('name', sorted(RUNS))
def test_device_breakout_equals_host_envs_and_the_oracle(oracle, name):
    """Every ply of a device Breakout arena: live flags, roots byte for byte and the tally against host make_breakout_env objects stepped
    with the recorded actions; policy, root value and action against the oracle's deterministic search; a frozen env's record no longer
    changes; the returns are the brick counts."""
    from test_oracle_nets import _oracle_net
    from muzero_amd import planner as pl

    make, key, cap, S, B, sims, kind, codes = RUNS[name]
    rows, cols, ch, cw, K, _ = bc.SHAPES[key]
    net = make()
    shape = tuple(net.planner_spec()['input_shape'])
    p = _planner(net, B, sims, capture=True)
    cfg = oracle.make_config(3, sims, 0.997, False, None, 0.25, 0.25)
    onet = _oracle_net(oracle, net, kind)
    p.arena_reset_breakout(rows, cols, K, cap, codes)  # (g43: None -- start code e % (2 cols))
    envs = _host(name)
    obs = [np.asarray(e.reset(), np.float32) for e in envs]
    done = np.zeros(B, bool)
    length, ret = np.zeros(B, np.int32), np.zeros(B, np.float64)
    prev = None
    for t in range(cap + 1):  # one ply past the cap
        p.arena_step(1)
        rec, res = p.arena_read_ply(), p.arena_result()
        live = ~done
        np.testing.assert_array_equal(rec['live'].astype(bool), live, err_msg=f'ply {t}')
        for e in np.flatnonzero(live):
            assert rec['obs'][e].tobytes() == obs[e].tobytes(), f'ply {t}: root of env {e}'
        assert (rec['mask'] == 1).all() and (rec['player'] == 1).all() and (rec['side'] == pl.SIDE_CHALLENGER).all() and (rec['u'] == 0).all()
        _check_search(oracle, cfg, onet, rec, np.flatnonzero(live), _ties(p), t, shape)
        if prev is not None:
            for k in REC[:-1]:
                np.testing.assert_array_equal(rec[k][done], prev[k][done], err_msg=f'ply {t}: frozen record field {k}')
        for e in np.flatnonzero(live):
            o, r, d, _ = envs[e].step(int(rec['action'][e]))
            length[e] += 1
            ret[e] += float(np.float32(r))
            if d:
                done[e] = True
            else:
                obs[e] = np.asarray(o, np.float32)
        np.testing.assert_array_equal(res['length'], length, err_msg=f'ply {t}')
        np.testing.assert_array_equal(res['ret'], ret, err_msg=f'ply {t}')
        np.testing.assert_array_equal(res['winner'], np.where(done, pl.ARENA_DRAW, pl.ARENA_UNFINISHED), err_msg=f'ply {t}')
        assert _tally(res) == dict(challenger_wins=0, opponent_wins=0, draws=int(done.sum()), finished_plies=int(length[done].sum()),
                                   live=int((~done).sum())), f'ply {t}'
        prev = rec
    assert done.all() and length.max() <= cap and (ret == np.round(ret)).all() and (ret >= 0).all()
    if name == 'g43':  # games end on different plies (misses and the cap); bricks were broken
        assert len(set(length.tolist())) > 1 and ret.sum() > 0
    p.close()


def test_batching_repeat_and_start_codes():
    """n plies in one mz_arena_step equal n calls of one; a run equals its repeat; NULL start codes are e % (2 cols) given explicitly; other
    start codes give another match."""
    make, key, cap, S, B, sims, _, _ = RUNS['g43']
    rows, cols, ch, cw, K, _ = bc.SHAPES[key]
    net = make()
    out = []
    for chunks, codes in (([1] * 13, None), ([5, 7, 1], None), ([13], [e % 6 for e in range(B)]), ([13], [5 - e % 6 for e in range(B)])):
        p = _planner(net, B, sims)
        p.arena_reset_breakout(rows, cols, K, cap, codes)
        for n in chunks:
            p.arena_step(n)
        res = p.arena_result()
        out.append((res['winner'].tobytes(), res['length'].tobytes(), res['ret'].tobytes(), tuple(sorted(_tally(res).items()))))
        assert res['live'] == 0 and res['draws'] == B
        p.close()
    assert out[0] == out[1] == out[2] and out[3] != out[0]


def test_refusals_and_the_handle_afterwards():
    from muzero_amd import planner as pl

    make, key, cap, S, B, sims, _, _ = RUNS['g43']
    net = make()
    p = _planner(net, 4, sims)
    bad = np.array([0, 5, 6, 1], np.int32)
    with pytest.raises(pl.PlannerError, match=r'error -1: .*h_start_code\[2\] = 6'):
        p.arena_reset_breakout(4, 3, 1, 12, bad)
    with pytest.raises(pl.PlannerError, match=r'error -1: .*h_start_code\[0\] = -1'):
        p.arena_reset_breakout(4, 3, 1, 12, [-1, 0, 0, 0])
    for kw, field in ((dict(rows=5), 'rows'), (dict(rows=4, brick_rows=2), 'rows'), (dict(cols=7), 'cols'), (dict(brick_rows=4), 'brick_rows'),
                      (dict(max_moves=-3), 'max_moves')):
        with pytest.raises(pl.PlannerError, match=r'error -1: .*mz_breakout_env\.' + field):
            p.arena_reset_breakout(**kw)
    x = pl.MzBreakoutEnv(4, 3, 1, 12, 1)  # MZ_RECORD_FRAMES_U8: the arena has no record ring
    assert p.lib.mz_arena_reset_breakout(p.h, C.byref(x), None) == -1 and b'mz_breakout_env.record_format' in p.lib.mz_last_error()
    with pytest.raises(pl.PlannerError, match=r'error -1: .*num_actions'):
        _planner(build_mlp(('a4', (4, 12, 12), 4, 32, 7, 5, 16, 1)), 4, sims).arena_reset_breakout()
    with pytest.raises(pl.PlannerError, match=r'error -1: .*mz_arena_reset_breakout'):
        p.arena_reset(pl.ENV_BREAKOUT)
    p.arena_reset_breakout(4, 3, 1, 12)
    frames, mask, ids = np.zeros((4, 1, 12, 12), np.uint8), np.ones((4, 3), np.uint8), np.ones(4, np.int32)
    act, live = np.zeros(4, np.int32), np.zeros(4, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert p.lib.mz_arena_external_act(p.h, vp(frames), vp(mask), vp(ids), vp(ids), vp(act), vp(live)) == -3  # MZ_E_STATE
    with pytest.raises(pl.PlannerError, match='error -3'):
        p.selfplay_step(1.0, 1)  # self-play during an arena
    p.arena_step(13)
    first = p.arena_result()
    assert first['live'] == 0
    # Catch's arena and Breakout self-play on the same handle afterwards, then the arena again: the same match
    p.arena_reset_catch(6, 4)
    p.arena_step(5)
    assert p.arena_result()['live'] == 0
    p.selfplay_reset_breakout(4, 3, 1, 12)
    p.selfplay_step(1.0, 3)
    assert p.selfplay_counters()['env_steps'] == 12
    p.arena_reset_breakout(4, 3, 1, 12)
    p.arena_step(13)
    again = p.arena_result()
    for k in ('winner', 'length', 'ret'):
        assert first[k].tobytes() == again[k].tobytes(), k
    p.close()


def test_play_match_and_run_evaluator_on_breakout(tmp_path):
    """pipeline.play_match(config, net, None, device, 'Breakout' or a BreakoutEnv object, N) is the arena above; run_evaluator(device_episodes=N)
    reports its returns and lengths."""
    import torch

    from muzero_amd import games, pipeline
    from muzero_amd import planner as pl
    from muzero_amd.config import make_atari_config

    make, key, cap, S, B, sims, _, _ = RUNS['g43']
    rows, cols, ch, cw, K, _ = bc.SHAPES[key]
    net = make()
    cfg = make_atari_config(use_tensorboard=False)
    cfg.num_simulations = sims
    dev = torch.device('cuda', 0)
    env = games.BreakoutEnv(rows, cols, ch, cw, brick_rows=K, max_moves=cap)
    m = pipeline.play_match(cfg, net, None, dev, env, B)
    p = pl.Planner(pl.make_mz_config(net.planner_spec(), cfg, num_envs=B, seed=int(getattr(cfg, 'planner_seed', 1)) + 104729, keep_shape=True), 0)
    p.load_state_dict(net.state_dict())
    p.arena_reset_breakout(rows, cols, K, cap)
    p.arena_step(cap)
    res = p.arena_result()
    p.close()
    assert not m.two_player and m.num_games == B and m.draws == B
    assert m.length.tobytes() == res['length'].tobytes() and m.ret.tobytes() == res['ret'].tobytes()
    assert (m.length <= cap).all() and (m.ret >= 0).all()
    with pytest.raises(ValueError, match='one-player'):
        pipeline.play_match(cfg, net, 'random', dev, 'Breakout', B)
    # the name alone: the 12 x 12 grid on the network's own frame (one-pixel cells), 3 brick rows, cap 200
    wide = pipeline.play_match(cfg, net, None, dev, 'Breakout', 4)
    assert wide.num_games == 4 and (wide.length <= 200).all()
    ckpt = tmp_path / 'ckpt.pt'
    pipeline.create_checkpoint({'network': net.state_dict(), 'train_steps': 7}, str(ckpt))
    stop = types.SimpleNamespace(is_set=lambda: True)
    got = pipeline.run_evaluator(cfg, make(), dev, env, 0.0, [str(ckpt)], stop, device_episodes=B)
    assert len(got) == 1 and got[0][2] == 7
    assert got[0][0] == [float(r) for r in m.ret] and got[0][1] == [int(n) for n in m.length]
