"""The image arena (mz_arena_reset_catch, mz_arena_reset_external / _act / _commit; csrc/mz_arena_image.h) on an MI355X: device Catch against
host games.make_catch_env objects and the oracle search at every ply, a device Catch arena and a host-stepped arena fed by host CatchEnv
frames byte-identical in lock-step, the host-stepped arena on stacked vectors and whole observations, batching and repeatability, the
refusals, and pipeline.play_match / run_evaluator on top."""
import ctypes as C
import types

import numpy as np
import pytest

import arena_image_cases as ac
from helpers import build_conv, build_mlp, mlp_case

pytestmark = pytest.mark.gpu

REC = ('obs', 'mask', 'player', 'side', 'pi', 'root_value', 'action', 'u', 'live')
RES = ('winner', 'length', 'ret')
# name -> (net builder, arena_image_cases.SHAPES key, S, games, simulations, oracle net kind): the nets and grids of test_gpu_catch.py's RUNS
RUNS = {
    'c1_s2': (lambda: build_mlp(('c1s2', (4, 12, 12), 3, 32, 7, 5, 16, 41)), 'c1', 2, 24, 4, 'mlp'),
    'c1_s4': (lambda: build_mlp(('c1s4', (8, 12, 12), 3, 32, 7, 5, 16, 42)), 'c1', 4, 24, 5, 'mlp'),
    'r6c4': (lambda: build_mlp(('r6c4', (4, 12, 12), 3, 32, 7, 5, 16, 43)), 'r6c4', 2, 24, 8, 'mlp'),
    'wide': (lambda: build_mlp(('wide', (4, 12, 24), 3, 32, 7, 5, 16, 44)), 'wide', 2, 24, 4, 'mlp'),
    # 7 games x 150 bytes = 1050: the renderer's 16-byte runs cross from env to env and the last one ends in the allocation's padding
    'r5c5': (lambda: build_mlp(('r5c5', (4, 10, 15), 3, 32, 7, 5, 16, 45)), 'r5c5', 2, 7, 4, 'mlp'),
    'atari': (lambda: build_conv(('atari_s8', 'atari', (8, 96, 96), 3, 1, 8, 11, 11, 24)), 'atari', 4, 4, 3, 'conv'),
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
    tie draws (the pattern of test_gpu_arena.py)."""
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


def _layout(name):
    _, key, S, B, sims, kind = RUNS[name]
    rows, cols, ch, cw = ac.SHAPES[key]
    if B >= rows - 1:
        bc, sr = ac.layout(B, rows, cols)
    else:  # (the Atari net's four games: both ends of the start rows and two between)
        bc, sr = np.array([3, 11, 0, 6]), np.array([0, rows - 2, 6, 8])
    return rows, cols, ch, cw, bc, sr


def _same(a, b, fields, what):
    for f in fields:
        assert a[f].dtype == b[f].dtype and a[f].tobytes() == b[f].tobytes(), f'{what}: {f}'


def _tally(res):
    return {k: res[k] for k in ('challenger_wins', 'opponent_wins', 'draws', 'finished_plies', 'live')}


@pytest.mark.parametrize('name', sorted(RUNS))
def test_device_catch_equals_host_envs_and_the_oracle(oracle, name):
    """Every ply of a device Catch arena: live flags, roots byte for byte and the tally against host make_catch_env objects stepped with the
    recorded actions; policy, root value and action against the oracle's deterministic search; a frozen env's record no longer changes."""
    from test_oracle_nets import _oracle_net
    from muzero_amd import planner as pl

    make, _, S, B, sims, kind = RUNS[name]
    rows, cols, ch, cw, bc, sr = _layout(name)
    net = make()
    shape = tuple(net.planner_spec()['input_shape'])
    p = _planner(net, B, sims, capture=True)
    cfg = oracle.make_config(3, sims, 0.997, False, None, 0.25, 0.25)
    onet = _oracle_net(oracle, net, kind)
    p.arena_reset_catch(rows, cols, bc, sr)
    envs = ac.host_envs(rows, cols, ch, cw, S, bc, sr)
    obs = [np.asarray(e.reset(), np.float32) for e in envs]
    done = np.zeros(B, bool)
    length, ret = np.zeros(B, np.int32), np.zeros(B, np.float64)
    prev = None
    for t in range(rows):  # one ply past the longest game
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
    assert done.all() and (length == rows - 1 - sr).all() and set(np.unique(ret)) <= {-1.0, 1.0}
    p.close()


def _garbage(rs, frames, mask, cur, opp, rew, done, frozen):
    """Fill the frozen envs' entries of an upload with garbage."""
    n = int(frozen.sum())
    frames[frozen] = rs.randint(0, 256, size=(n,) + frames.shape[1:]).astype(frames.dtype)
    mask[frozen] = rs.randint(0, 2, size=(n, mask.shape[1]))
    cur[frozen], opp[frozen] = 7, -3
    rew[frozen] = rs.uniform(-9, 9, size=n)
    done[frozen] = rs.randint(0, 2, size=n)


@pytest.mark.parametrize('name', ['c1_s4', 'r6c4'])
def test_device_catch_and_host_stepped_arena_in_lock_step(name):
    """A device Catch arena and a host-stepped arena fed by host CatchEnv frames (uint8, stacked on the device), same seed, same start: every
    arena_read_ply field and arena_result byte-identical at every ply, with garbage uploaded for the frozen envs."""
    from muzero_amd.games import CatchEnv

    make, _, S, B, sims, _ = RUNS[name]
    rows, cols, ch, cw, bc, sr = _layout(name)
    net = make()
    pd, px = _planner(net, B, sims), _planner(net, B, sims)
    pd.arena_reset_catch(rows, cols, bc, sr)
    px.arena_reset_external(stack_history=S, is_obs_image=True, frame_shape=(1, rows * ch, cols * cw), frame_u8=True)
    envs = [CatchEnv(rows, cols, ch, cw, start_row=int(r), ball_cols=[int(c)]) for c, r in zip(bc, sr)]
    frames = np.stack([e.reset() for e in envs])
    frozen = np.zeros(B, bool)
    rs = np.random.RandomState(17)
    for t in range(rows):
        pd.arena_step(1)
        mask, cur, opp = np.ones((B, 3), np.uint8), np.ones(B, np.int32), np.ones(B, np.int32)
        rew, done = np.zeros(B, np.float32), np.zeros(B, np.uint8)
        _garbage(rs, frames, mask, cur, opp, rew, done, frozen)
        actions, live = px.arena_external_act(frames, mask, cur, opp)
        np.testing.assert_array_equal(live.astype(bool), ~frozen, err_msg=f'ply {t}')
        for e in np.flatnonzero(live):
            frames[e], rew[e], d, _ = envs[e].step(int(actions[e]))
            done[e] = 1 if d else 0
        px.arena_external_commit(rew, done)
        frozen |= (live != 0) & (done != 0)
        recd, recx = pd.arena_read_ply(), px.arena_read_ply()
        _same(recd, recx, REC, f'ply {t}')
        np.testing.assert_array_equal(live, recd['live'], err_msg=f'ply {t}: h_live')
        np.testing.assert_array_equal(actions, recd['action'], err_msg=f'ply {t}: h_action')
        resd, resx = pd.arena_result(), px.arena_result()
        _same(resd, resx, RES, f'ply {t}')
        assert _tally(resd) == _tally(resx), f'ply {t}'
    assert frozen.all() and resd['live'] == 0 and resd['draws'] == B
    pd.close()
    px.close()


class _ScriptedEnv:
    """A host env of a given episode length: float vector frames that depend on the actions taken, float32 rewards."""

    num_actions = 3
    observation_shape = (3,)

    def __init__(self, seed, length, illegal=None):
        self._rs, self.length, self.steps = np.random.RandomState(seed), length, 0
        self.actions_mask = np.ones(3, np.uint8)
        if illegal is not None:
            self.actions_mask[illegal] = 0

    def reset(self):
        self.steps = 0
        return self._rs.uniform(-1, 1, size=3).astype(np.float32)

    def step(self, action):
        self.steps += 1
        frame = (self._rs.uniform(-1, 1, size=3) + 0.25 * action).astype(np.float32)
        return frame, np.float32(self._rs.uniform(-2, 2)), self.steps >= self.length, {}


@pytest.mark.parametrize('stack', [3, 0])
def test_host_stepped_arena_on_vectors_and_whole_observations(oracle, stack):
    """Scripted host envs of lengths 1 .. 7 with float rewards, B = 16, the `tiny` MLP net ((3, 4) observations): frames are stacked float
    vectors (stack 3: the device stacks) or whole observations (stack 0: the host stacker's).  Roots equal the host stacker's, the return
    is the float64 sum of the float32 rewards in ply order exactly, the searches equal the oracle's, garbage for frozen envs is ignored."""
    from test_oracle_nets import _oracle_net
    from muzero_amd import planner as pl
    from muzero_amd.games import StackFrameAndAction

    case = mlp_case('tiny')
    net = build_mlp(case)
    B, sims = 16, 6
    p = _planner(net, B, sims, capture=True)
    cfg = oracle.make_config(3, sims, 0.997, False, None, 0.25, 0.25)
    onet = _oracle_net(oracle, net, 'mlp')
    lengths = 1 + np.arange(B) % 7
    base = [_ScriptedEnv(100 + e, int(lengths[e]), illegal=(e % 3) if e % 2 else None) for e in range(B)]
    stackers = [StackFrameAndAction(b, 3, False) for b in base]
    obs = [np.asarray(s.reset(), np.float32) for s in stackers]  # (3, 4): the roots; obs[e][0, :3] is the newest frame
    if stack:
        p.arena_reset_external(stack_history=3, is_obs_image=False, frame_shape=(3,))
    else:
        p.arena_reset_external(stack_history=0, frame_shape=(3, 4))
    frozen = np.zeros(B, bool)
    ret, length = np.zeros(B, np.float64), np.zeros(B, np.int32)
    rs = np.random.RandomState(23)
    for t in range(8):  # one ply past the longest episode
        frames = np.stack([o[0, :3] if stack else o for o in obs]).astype(np.float32)
        mask = np.stack([b.actions_mask for b in base])
        cur, opp = np.ones(B, np.int32), np.ones(B, np.int32)
        rew, done = np.zeros(B, np.float32), np.zeros(B, np.uint8)
        _garbage(rs, frames, mask, cur, opp, rew, done, frozen)
        actions, live = p.arena_external_act(frames, mask, cur, opp)
        np.testing.assert_array_equal(live.astype(bool), ~frozen)
        for e in np.flatnonzero(live):
            assert base[e].actions_mask[actions[e]]
            o, r, d, _ = stackers[e].step(int(actions[e]))
            rew[e], done[e] = r, 1 if d else 0
            ret[e] += float(np.float32(r))
            length[e] += 1
        p.arena_external_commit(rew, done)
        rec, res = p.arena_read_ply(), p.arena_result()
        rows = np.flatnonzero(live)
        for e in rows:
            assert rec['obs'][e].tobytes() == obs[e].tobytes(), f'ply {t}: root of env {e}'
            assert (rec['mask'][e] == base[e].actions_mask).all() and rec['player'][e] == 1 and rec['side'][e] == pl.SIDE_CHALLENGER
        np.testing.assert_array_equal(rec['action'], actions)
        _check_search(oracle, cfg, onet, rec, rows, _ties(p), t, (3, 4))
        for e in rows:  # (after the checks: the stacker's observation of the next ply)
            if not done[e]:
                obs[e] = np.asarray(stackers[e].observation(), np.float32)
        frozen |= (live != 0) & (done != 0)
        assert res['ret'].tobytes() == ret.tobytes(), f'ply {t}'
        np.testing.assert_array_equal(res['length'], length)
        assert _tally(res) == dict(challenger_wins=0, opponent_wins=0, draws=int(frozen.sum()), finished_plies=int(length[frozen].sum()),
                                   live=int((~frozen).sum()))
    assert frozen.all() and (length == lengths).all()
    p.close()


def _play_catch(name, chunks, extra=0):
    make, _, S, B, sims, _ = RUNS[name]
    rows, cols, ch, cw, bc, sr = _layout(name)
    p = _planner(make(), B, sims)
    p.arena_reset_catch(rows, cols, bc, sr)
    for n in chunks:
        p.arena_step(n)
    out = (p.arena_read_ply(), p.arena_result())
    if extra:
        p.arena_step(extra)
        out += (p.arena_read_ply(), p.arena_result())
    p.close()
    return out


def test_n_plies_in_one_call_a_repeat_and_steps_past_the_end():
    """mz_arena_step(p, n) equals n calls of one, a run equals its repeat, and stepping past the last game changes nothing."""
    rows = ac.SHAPES['r6c4'][0]
    one = _play_catch('r6c4', [1] * (rows - 1), extra=3)
    for other in (_play_catch('r6c4', [rows - 1]), _play_catch('r6c4', [2, rows - 3]), _play_catch('r6c4', [1] * (rows - 1))):
        _same(one[0], other[0], REC, 'read_ply')
        _same(one[1], other[1], RES, 'result')
        assert _tally(one[1]) == _tally(other[1])
    assert one[1]['live'] == 0
    _same(one[0], one[2], REC[:-1], 'past the end: read_ply')
    assert not one[2]['live'].any()  # (no env was live when the last ply began)
    _same(one[1], one[3], RES, 'past the end: result')
    assert _tally(one[1]) == _tally(one[3])
    mid = _play_catch('r6c4', [2])  # games of length 1 and 2 are over, the others run
    assert 0 < mid[1]['live'] < RUNS['r6c4'][3]


def test_refusals_and_the_handle_afterwards():
    """Every refused call returns its status and message and leaves the handle usable; afterwards the arena's CartPole and self-play's
    Catch on the same handles equal a fresh handle's run (the Philox draws are keyed by the handle's move count: the fresh handle plays
    as many searches first)."""
    from muzero_amd import planner as pl

    INVALID, STATE = -1, -3
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    net = RUNS['c1_s2'][0]()
    B = 4
    x = pl.MzCatchEnv(12, 12, 0)

    def catch(p, env=x, bc=None, sr=None):
        return p.lib.mz_arena_reset_catch(p.h, C.byref(env), vp(bc), vp(sr)), p.lib.mz_last_error().decode()

    # configurations Catch cannot be played on
    board = _planner(net, B, 4, discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0))
    rc, msg = catch(board)
    assert rc == INVALID and 'is_board_game' in msg and 'mz_arena_reset_catch' in msg
    board.close()
    cp_net = build_mlp(mlp_case('cartpole'))
    cp = pl.Planner(pl.make_mz_config(cp_net.planner_spec(), None, num_envs=B, seed=SEED, num_simulations=4, discount=0.997), 0)
    cp.load_state_dict(cp_net.state_dict())
    rc, msg = catch(cp)
    assert rc == INVALID and 'num_actions' in msg
    p = _planner(net, B, 4)
    lib = p.lib
    assert lib.mz_arena_step(p.h, 1) == STATE
    frames, mask, ids = np.zeros((B, 1, 12, 12), np.uint8), np.ones((B, 3), np.uint8), np.ones(B, np.int32)
    act, live = np.zeros(B, np.int32), np.zeros(B, np.uint8)
    rew, done = np.zeros(B, np.float32), np.zeros(B, np.uint8)
    ext_act = lambda: lib.mz_arena_external_act(p.h, vp(frames), vp(mask), vp(ids), vp(ids), vp(act), vp(live))  # noqa: E731
    ext_commit = lambda: lib.mz_arena_external_commit(p.h, vp(rew), vp(done))  # noqa: E731
    assert ext_act() == STATE and b'mz_arena_reset_external' in lib.mz_last_error()  # before any reset
    assert ext_commit() == STATE and b'mz_arena_reset_external' in lib.mz_last_error()
    for env, word in ((pl.MzCatchEnv(5, 12, 0), 'mz_catch_env.rows'), (pl.MzCatchEnv(1, 12, 0), 'mz_catch_env.rows'), (pl.MzCatchEnv(12, 7, 0), 'mz_catch_env.cols'),
                      (pl.MzCatchEnv(12, 12, 1), 'record_format'), (pl.MzCatchEnv(12, 12, 7), 'record_format')):
        rc, msg = catch(p, env)
        assert rc == INVALID and word in msg, (word, msg)
    for bc, sr, word in ((np.array([0, 1, 2, 12], np.int32), None, 'h_ball_col[3]'), (np.array([0, -1, 2, 3], np.int32), None, 'h_ball_col[1]'),
                         (None, np.array([0, 0, 11, 0], np.int32), 'h_start_row[2]'), (None, np.array([-1, 0, 0, 0], np.int32), 'h_start_row[0]')):
        rc, msg = catch(p, x, bc, sr)
        assert rc == INVALID and word in msg, (word, msg)
    xe = pl.MzExternalEnv(2, 1, 1, 12, 12, 1, 0, 0, 1)
    assert lib.mz_arena_reset_external(p.h, C.byref(xe)) == INVALID and b'record_format' in lib.mz_last_error()
    xe = pl.MzExternalEnv(3, 1, 1, 12, 12, 1, 0, 0, 0)  # 3 * 2 * 144 values: not the network's observation
    assert lib.mz_arena_reset_external(p.h, C.byref(xe)) == INVALID and b'stacked observation' in lib.mz_last_error()
    assert lib.mz_arena_step(p.h, 1) == STATE  # none of the refused resets opened an arena
    # mz_arena_reset keeps refusing the kinds, and names where they are played
    with pytest.raises(pl.PlannerError, match=r'error -1: .*MZ_ENV_CATCH.*mz_arena_reset_catch'):
        p.arena_reset(pl.ENV_CATCH)
    with pytest.raises(pl.PlannerError, match=r'error -1: .*mz_arena_reset_external'):
        p.arena_reset(pl.ENV_EXTERNAL)
    with pytest.raises(pl.PlannerError, match='error -1'):
        p.arena_reset(pl.ENV_SYNTHETIC)
    # a Catch arena is stepped by mz_arena_step only
    searches = 0
    p.arena_reset_catch()
    assert ext_act() == STATE and b'mz_arena_reset_external' in lib.mz_last_error()
    assert ext_commit() == STATE
    assert lib.mz_selfplay_step(p.h, C.c_double(1.0), 1) == STATE and b'mz_selfplay_reset' in lib.mz_last_error()
    assert lib.mz_selfplay_external_act(p.h, vp(frames), vp(mask), vp(ids), vp(ids), C.c_double(1.0), vp(act)) == STATE
    assert b'mz_selfplay_reset_external' in lib.mz_last_error()
    p.arena_step(2)
    searches += 2
    assert p.arena_result()['live'] == B
    # a host-stepped arena by act / commit only, in turn
    p.arena_reset_external(stack_history=2, is_obs_image=True, frame_shape=(1, 12, 12), frame_u8=True)
    assert lib.mz_arena_step(p.h, 1) == STATE and b'mz_arena_external_act' in lib.mz_last_error()
    assert ext_commit() == STATE and b'without an mz_arena_external_act' in lib.mz_last_error()
    assert ext_act() == 0 and live.all()
    searches += 1
    assert ext_act() == STATE and b'mz_arena_external_commit' in lib.mz_last_error()
    assert lib.mz_selfplay_step(p.h, C.c_double(1.0), 1) == STATE
    assert lib.mz_selfplay_external_act(p.h, vp(frames), vp(mask), vp(ids), vp(ids), C.c_double(1.0), vp(act)) == STATE
    done[:] = (1, 0, 0, 1)
    assert ext_commit() == 0
    res = p.arena_result()
    assert res['live'] == 2 and res['draws'] == 2 and list(res['length']) == [1, 1, 1, 1]
    # afterwards: self-play's Catch on this handle, the arena's CartPole on the handle that refused Catch, against fresh handles
    fresh = _planner(net, B, 4)
    fresh.selfplay_reset_catch()
    fresh.selfplay_step(1.0, searches)
    got = []
    for h in (p, fresh):
        h.selfplay_reset_catch()
        h.selfplay_step(1.0, 5)
        got.append(h.selfplay_read(5))
        h.close()
    for f in got[0]:
        assert got[0][f].tobytes() == got[1][f].tobytes(), f
    init = np.random.RandomState(4).uniform(-0.05, 0.05, size=(B, 4))
    fresh = pl.Planner(pl.make_mz_config(cp_net.planner_spec(), None, num_envs=B, seed=SEED, num_simulations=4, discount=0.997), 0)
    fresh.load_state_dict(cp_net.state_dict())
    got = []
    for h in (cp, fresh):
        h.arena_reset(pl.ENV_CARTPOLE, None, 0, init)
        h.arena_step(6)
        got.append((h.arena_read_ply(), h.arena_result()))
        h.close()
    _same(got[0][0], got[1][0], REC, 'CartPole read_ply')
    _same(got[0][1], got[1][1], RES, 'CartPole result')


def _catch_cfg(sims=5):
    from muzero_amd.config import make_atari_config

    cfg = make_atari_config(use_tensorboard=False)
    cfg.num_simulations = sims
    return cfg


def _by_hand(net, cfg, n, rows=12, cols=12):
    from muzero_amd import planner as pl

    p = pl.Planner(pl.make_mz_config(net.planner_spec(), cfg, num_envs=n, seed=int(getattr(cfg, 'planner_seed', 1)) + 104729, keep_shape=True), 0)
    p.load_state_dict(net.state_dict())
    p.arena_reset_catch(rows, cols)
    p.arena_step(rows - 1)
    res = p.arena_result()
    p.close()
    assert res['live'] == 0 and res['draws'] == n
    return res


def test_play_match_on_catch_and_on_host_envs(tmp_path):
    """pipeline.play_match(..., 'Catch', 24) equals the by-hand arena of the same seed; so does play_match over a list of host
    make_catch_env objects (through the host-stepped arena); run_evaluator(device_episodes=24) on a CatchEnv hands on_result those
    returns and lengths."""
    import torch
    from muzero_amd import pipeline
    from muzero_amd.games import CatchEnv, make_catch_env

    net = RUNS['c1_s2'][0]()
    cfg = _catch_cfg()
    dev = torch.device('cuda', 0)
    n = 24
    want = _by_hand(net, cfg, n)
    assert (want['length'] == 11).all() and set(np.unique(want['ret'])) <= {-1.0, 1.0}
    m = pipeline.play_match(cfg, net, None, dev, 'Catch', n)
    for got in (m, pipeline.play_match(cfg, net, None, dev, [make_catch_env(12, 12, 1, 1, stack_history=2, ball_cols=[e % 12]) for e in range(n)], n)):
        assert not got.two_player and got.num_games == n and got.draws == n
        for f in RES:
            assert getattr(got, f).tobytes() == want[f].tobytes(), f
    small = pipeline.play_match(cfg, net, None, dev, CatchEnv(6, 4, 2, 3), 8)  # the grid is read off the object
    np.testing.assert_array_equal(small.ret, _by_hand(net, cfg, 8, 6, 4)['ret'])
    assert (small.length == 5).all()
    f = str(tmp_path / 'ckpt.pt')
    pipeline.create_checkpoint({'network': net.state_dict(), 'train_steps': 70}, f)
    calls = []
    stop = types.SimpleNamespace(is_set=lambda: True)
    out = pipeline.run_evaluator(cfg, RUNS['c1_s2'][0](), dev, CatchEnv(12, 12, 1, 1), 0.0, [f], stop, on_result=lambda *a: calls.append(a), device_episodes=n)
    assert len(calls) == 1 and calls[0][2] == 70 and out == [calls[0]]
    assert calls[0][0] == [float(r) for r in want['ret']] and calls[0][1] == [int(v) for v in want['length']]
