"""The device Catch env (mz_selfplay_reset_catch, csrc/mz_catch.h) against host-stepped games.CatchEnv objects.  A device Catch planner and
a host-stepped planner (selfplay_reset_external over uint8 frames, fed by CatchEnv objects given the regenerated ball columns and the
stagger) share one seed and are stepped in lock-step: sampled actions, every mz_selfplay_read field, the counters and the attached replay
rings stay byte-identical -- for float32 and compact records on both sides, float32 and frames_u8 replay states, cells that are no multiple
of 4 pixels wide, non-square cells, MLP nets and the Atari net.  n moves in one mz_selfplay_step equal n calls of one; a run equals its
repeat; the Atari learner reads the same gradient from either replay format; run_self_play(env='Catch') emits what the host loop emits;
what the kind cannot do is refused by name; the other kinds work on the handle afterwards."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import catch_cases as cc
from helpers import build_conv, build_mlp

pytestmark = pytest.mark.gpu

REC = ('obs', 'action', 'reward', 'pi', 'root_value', 'player', 'done')
# acc_seq_length + unroll_steps + td_steps = 7 < 11: the 12-row games flush mid-episode, and the stagger makes flushes and ends meet
CFG = types.SimpleNamespace(is_board_game=False, acc_seq_length=3, unroll_steps=2, td_steps=2, discount=0.997)
SEED, MOVES = 5, 38  # >= 3 * (rows - 1) + S moves for every run below

# name -> (net builder, catch_cases.SHAPES key, S, envs, replay capacity, simulations)
RUNS = {
    'c1_s2': (lambda: build_mlp(('c1s2', (4, 12, 12), 3, 32, 7, 5, 16, 41)), 'c1', 2, 8, 5, 4),
    'c1_s4': (lambda: build_mlp(('c1s4', (8, 12, 12), 3, 32, 7, 5, 16, 42)), 'c1', 4, 8, 5, 4),
    'r6c4': (lambda: build_mlp(('r6c4', (4, 12, 12), 3, 32, 7, 5, 16, 43)), 'r6c4', 2, 8, 5, 4),
    'wide': (lambda: build_mlp(('wide', (4, 12, 24), 3, 32, 7, 5, 16, 44)), 'wide', 2, 8, 5, 4),
    # 7 envs x 150 bytes = 1050: the renderer's 16-byte runs cross from env to env and the last one ends in the allocation's padding
    'r5c5': (lambda: build_mlp(('r5c5', (4, 10, 15), 3, 32, 7, 5, 16, 45)), 'r5c5', 2, 7, 5, 4),
    'atari': (lambda: build_conv(('atari_s8', 'atari', (8, 96, 96), 3, 1, 8, 11, 11, 24)), 'atari', 4, 4, 6, 3),
}
_DONE = set()


@pytest.fixture(scope='module', autouse=True)
def _release_planners():
    """The cached runs keep their planners and replays on the GPU: they end with this module, not with the session."""
    yield
    for key in sorted(_DONE, key=str):
        for p, _, _ in run(*key).side.values():  # (cached: nothing runs again)
            p.close()
    run.cache_clear()
    _DONE.clear()
    torch.cuda.empty_cache()


def _planner(net, B, sims=4, seed=SEED, **kw):
    from muzero_amd import planner as pl

    kw.setdefault('discount', 0.997)
    p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=B, seed=seed, num_simulations=sims, keep_shape=True, **kw), 0)
    p.load_state_dict(net.state_dict())
    return p


def _replay(cap, state, S=None, fshape=None, A=3):
    from muzero_amd.replay import PrioritizedReplay

    kw = dict(state_format='frames_u8', frame_spec=(S,) + tuple(fshape) + (A,)) if state == 'frames_u8' else {}
    return PrioritizedReplay(cap, 0.0, 0.0, np.random.RandomState(0), device='cuda', **kw)


def _snap(rp, origin):
    torch.cuda.synchronize()
    return ({k: v.cpu().numpy().copy() for k, v in rp._ring.items()}, rp._attached[0].cpu().numpy().copy(), origin.cpu().numpy().copy())


@functools.lru_cache(maxsize=None)
def run(name, state=None):
    """Device Catch planners and host-stepped planners, one per record format, stepped in lock-step; `state`: the attached replays' state
    format (None: no replay).  Everything the tests below read, computed once."""
    make, shape_key, S, B, cap, sims = RUNS[name]
    rows, cols, ch, cw = cc.SHAPES[shape_key]
    fshape = (1, rows * ch, cols * cw)
    net = make()
    shape = tuple(net.planner_spec()['input_shape'])
    records = ('f32',) if state == 'f32' else ('f32', 'frames_u8')  # (compact records feed frames_u8 states only)
    side = {}
    for where in ('host', 'dev'):
        for rec in records:
            p = _planner(net, B, sims)
            rp = origin = None
            if state is not None:
                rp = _replay(cap, state, S, fshape)
                origin = p.attach_replay(rp, CFG, obs_shape=shape, with_origin=True)
            if where == 'dev':
                p.selfplay_reset_catch(rows, cols, record_format=rec)
            else:
                p.selfplay_reset_external(stack_history=S, is_obs_image=True, frame_shape=fshape, frame_u8=True, max_episode_steps=rows - 1,
                                          record_format=rec)
            side[(where, rec)] = (p, rp, origin)
    info = {k: p.record_info() for k, (p, _, _) in side.items()}
    envs = cc.host_envs(B, rows, cols, ch, cw, SEED)
    frames = np.stack([e.reset() for e in envs])
    ones = np.ones((B, 3), np.uint8)
    counts, equal, actions_equal, dones, frames_seen = [], [], [], [], [frames]
    base = ('host', 'f32')
    for m in range(MOVES):
        acts = {}
        for k, (p, _, _) in side.items():
            if k[0] == 'host':
                acts[k] = p.external_act(frames, ones, 1, 1, 1.0)
            else:
                p.selfplay_step(1.0, 1)
        rew, done = np.zeros(B, np.float32), np.zeros(B, np.uint8)
        nxt = []
        for i, e in enumerate(envs):
            f, rew[i], d, _ = e.step(int(acts[base][i]))
            done[i] = 1 if d else 0
            nxt.append(e.reset() if d else f)
        frames = np.stack(nxt)
        frames_seen.append(frames)
        for k, (p, _, _) in side.items():
            if k[0] == 'host':
                p.external_commit(rew, done)
            p.synchronize()  # (a move's epilogue is only enqueued when the call returns)
        recs = {k: p.selfplay_read(1) for k, (p, _, _) in side.items()}
        actions_equal.append(all(np.array_equal(recs[k]['action'][0], acts[base]) for k in side))
        equal.append({k: all(recs[base][f].tobytes() == recs[k][f].tobytes() for f in REC) for k in side})
        dones.append(done)
        if state is not None:
            counts.append({k: rp.num_added for k, (_, rp, _) in side.items()})
    last = {k: p.selfplay_read(20) for k, (p, _, _) in side.items()}
    counters = {k: p.selfplay_counters() for k, (p, _, _) in side.items()}
    snap = {k: _snap(rp, origin) for k, (_, rp, origin) in side.items()} if state is not None else None
    _DONE.add((name, state))
    return types.SimpleNamespace(name=name, S=S, B=B, cap=cap, rows=rows, cols=cols, fshape=fshape, shape=shape, side=side, info=info, counts=counts,
                                 equal=equal, actions_equal=actions_equal, dones=np.stack(dones), last=last, counters=counters, snap=snap,
                                 frames_seen=np.stack(frames_seen), base=base)


ALL = [(n, s) for n in RUNS for s in (None, 'frames_u8')] + [('c1_s2', 'f32'), ('r6c4', 'f32'), ('atari', 'f32')]


@pytest.mark.parametrize('name,state', ALL)
def test_lock_step_with_host_catch_envs(name, state):
    r = run(name, state)
    assert len(r.equal) == MOVES >= 3 * (r.rows - 1) + r.S
    assert all(r.actions_equal), [m for m, ok in enumerate(r.actions_equal) if not ok]  # sampled actions, every move
    for k in r.side:  # every selfplay_read field, every move, both record formats on both sides
        assert all(eq[k] for eq in r.equal), (k, [m for m, eq in enumerate(r.equal) if not eq[k]])
        for f in REC:
            assert r.last[k][f].tobytes() == r.last[r.base][f].tobytes(), (k, f)
        assert r.counters[k] == r.counters[r.base], k
    assert r.counters[r.base]['env_steps'] == MOVES * r.B and r.counters[r.base]['episodes'] == r.dones.sum() >= 3 * r.B
    # the stagger gives the envs different phases; the games were not all lost or all won by chance alone
    ends = [np.flatnonzero(r.dones[:, e]) for e in range(r.B)]
    assert all(en[0] == r.rows - 2 - e % (r.rows - 1) and (np.diff(en) == r.rows - 1).all() for e, en in enumerate(ends))
    assert len({en[0] for en in ends}) > 1
    # the observations are Catch frames: the newest plane of the last read is the frame the host env showed (x / 255)
    obs = r.last[('dev', 'f32')]['obs'].reshape((20, r.B) + r.shape)
    want = r.frames_seen[MOVES - 20:MOVES, :, 0].astype(np.float32) / np.float32(255.0)
    assert obs[:, :, 0].tobytes() == want.tobytes() and 0 < want.sum()
    assert r.info[('dev', 'f32')] == r.info[('host', 'f32')]
    if ('dev', 'frames_u8') in r.info:
        assert r.info[('dev', 'frames_u8')] == r.info[('host', 'frames_u8')] and r.info[('dev', 'frames_u8')]['format'] == 'frames_u8'


@pytest.mark.parametrize('name,state', [(n, s) for n, s in ALL if s is not None])
def test_replay_rings_are_byte_identical(name, state):
    r = run(name, state)
    assert all(len(set(c.values())) == 1 for c in r.counts), r.counts  # num_added after every move, all sides
    n = r.counts[-1][r.base]
    per_move = np.diff([0] + [c[r.base] for c in r.counts])
    assert n > r.cap and (per_move > 0).sum() > 3  # the replay wraps; items arrive on many moves, not in one burst
    ring0, prio0, org0 = r.snap[r.base]
    assert ring0['state'].dtype == (np.uint8 if state == 'frames_u8' else np.float32)
    for k in r.side:
        ring1, prio1, org1 = r.snap[k]
        assert set(ring0) == set(ring1) >= {'state', 'action', 'pi_prob', 'value', 'reward'}
        for f in ring0:
            assert ring0[f].dtype == ring1[f].dtype and ring0[f].tobytes() == ring1[f].tobytes(), (k, f)
        assert prio0.tobytes() == prio1.tobytes() and org0.tobytes() == org1.tobytes() and (org0 >= 0).all(), k
    assert len({s.tobytes() for s in ring0['state']}) > 1


def _play_device(name, state, rec, chunks):
    make, shape_key, S, B, cap, sims = RUNS[name]
    rows, cols, ch, cw = cc.SHAPES[shape_key]
    net = make()
    p = _planner(net, B, sims)
    rp = _replay(cap, state, S, (1, rows * ch, cols * cw))
    origin = p.attach_replay(rp, CFG, obs_shape=tuple(net.planner_spec()['input_shape']), with_origin=True)
    p.selfplay_reset_catch(rows, cols, record_format=rec)
    for n in chunks:
        p.selfplay_step(1.0, n)
    p.synchronize()
    out = (rp.num_added, _snap(rp, origin), p.selfplay_read(30), p.selfplay_counters())
    p.close()
    return out


@pytest.mark.parametrize('name,state,rec', [('c1_s2', 'frames_u8', 'frames_u8'), ('r6c4', 'f32', 'f32'), ('wide', 'frames_u8', 'f32')])
def test_n_moves_in_one_call_and_repeat(name, state, rec):
    """selfplay_step(T, k) once equals k calls of selfplay_step(T, 1); a run is bit-identical to its repeat; and both are the lock-step
    run's device side."""
    a = _play_device(name, state, rec, [1] * MOVES)
    b = _play_device(name, state, rec, [7, 13, 1, MOVES - 21])
    c = _play_device(name, state, rec, [1] * MOVES)
    r = run(name, state)
    d = (r.counts[-1][('dev', rec)], r.snap[('dev', rec)], None, r.counters[('dev', rec)])
    for other, what in ((b, 'chunked'), (c, 'repeat'), (d, 'lock-step')):
        assert a[0] == other[0] and a[3] == other[3], what
        for x, y in zip(a[1], other[1]):
            if isinstance(x, dict):
                assert all(x[f].tobytes() == y[f].tobytes() for f in x), what
            else:
                assert x.tobytes() == y.tobytes(), what
        if other[2] is not None:
            assert all(a[2][f].tobytes() == other[2][f].tobytes() for f in REC), what
    assert a[0] > RUNS[name][4]


def test_atari_learner_gradient_from_either_replay_format():
    """One Atari HipLearner `grad` on a batch drawn by index: the frames_u8 ring and the float32 ring of the same Catch run give the same
    gradient vector byte for byte (batch 3, K = 2)."""
    from muzero_amd.hip_learner import HipLearner

    dev = torch.device('cuda', 0)
    out = {}
    for state in ('f32', 'frames_u8'):
        r = run('atari', state)
        rp = r.side[('dev', 'f32')][1]
        ring = type(rp._ring)(rp._ring, state=rp._ring['state'].reshape(r.cap, -1))
        ring.state_format, ring.frame_spec = rp._ring.state_format, rp._ring.frame_spec
        hl = HipLearner(RUNS['atari'][0]().to(dev), dev, 2, 3, lr=1e-3)
        idx = torch.tensor([3, 0, r.cap - 1], dtype=torch.int64, device=dev)
        loss, prio = hl.grad(ring, idx, None, 3)
        torch.cuda.synchronize()
        out[state] = (hl.grad_flat.cpu().numpy().copy(), loss.cpu().numpy().copy(), prio.cpu().numpy().copy())
        hl.close()
    g0, g1 = out['f32'][0], out['frames_u8'][0]
    assert np.isfinite(g0).all() and np.abs(g0).max() > 0
    for x, y, what in zip(out['f32'], out['frames_u8'], ('gradient', 'loss', 'priorities')):
        assert x.tobytes() == y.tobytes(), what


class _ListQueue:
    def __init__(self):
        self.items = []

    def put(self, item):
        self.items.append(item)


def test_run_self_play_device_catch_is_the_host_loop():
    """pipeline.run_self_play(env='Catch') into a device replay and into a queue, against run_self_play over a list of host CatchEnv stacks
    fed the same ball columns and stagger."""
    from muzero_amd import games, pipeline
    from muzero_amd.config import make_classic_config

    B, M, S = 6, 36, 2
    net = RUNS['c1_s2'][0]()
    cfg = make_classic_config(use_tensorboard=False)
    cfg.num_envs, cfg.acc_seq_length, cfg.unroll_steps, cfg.td_steps, cfg.num_simulations = B, 3, 2, 2, 4
    seed = int(cfg.planner_seed)  # (rank 0)
    dev = torch.device('cuda', 0)
    ctr, never = types.SimpleNamespace(value=0), types.SimpleNamespace(is_set=lambda: False)

    def host_list():
        return [games.make_catch_env(12, 12, 1, 1, stack_history=S, ball_cols=[cc.ball_col(seed, e, k, 12) for k in range(16)],
                                     first_row=cc.first_row(e, 12)) for e in range(B)]

    out = {}
    for env_name, make_env in (('device', lambda: 'Catch'), ('host', host_list)):
        for fmt in ('f32', 'frames_u8'):
            rp = _replay(64, 'frames_u8', S, (1, 12, 12))
            steps = pipeline.run_self_play(cfg, 0, net, dev, make_env(), rp, ctr, never, max_moves=M, record_format=fmt)
            assert steps == B * M
            torch.cuda.synchronize()
            out[(env_name, fmt)] = (rp.num_added, {k: v.cpu().numpy().copy() for k, v in rp._ring.items()}, np.asarray(rp.get_state()['priorities']).copy())
        q = _ListQueue()
        assert pipeline.run_self_play(cfg, 0, net, dev, make_env(), q, ctr, never, max_moves=M) == B * M
        out[(env_name, 'queue')] = [tuple(np.asarray(v).tobytes() for v in tr) + (np.float64(pr).tobytes(),) for tr, pr in q.items]
    n0, ring0, prio0 = out[('host', 'f32')]
    assert n0 > 64
    for key in (('device', 'f32'), ('device', 'frames_u8'), ('host', 'frames_u8')):
        n1, ring1, prio1 = out[key]
        assert n1 == n0 and prio1.tobytes() == prio0.tobytes(), key
        for f in ring0:
            assert ring0[f].tobytes() == ring1[f].tobytes(), (key, f)
    assert len(out[('device', 'queue')]) == len(out[('host', 'queue')]) == n0
    assert out[('device', 'queue')] == out[('host', 'queue')]
    assert len({s.tobytes() for s in ring0['state']}) > 1
    with pytest.raises(ValueError, match='record_format'):
        pipeline.run_self_play(cfg, 0, net, dev, 'Catch', _ListQueue(), ctr, never, max_moves=1, record_format='u8')
    # a CatchEnv object names the device env and its grid
    q = _ListQueue()
    small = build_mlp(('r6c4q', (4, 12, 12), 3, 32, 7, 5, 16, 43))
    assert pipeline.run_self_play(cfg, 0, small, dev, games.CatchEnv(6, 4, 2, 3), q, ctr, never, max_moves=10) == B * 10
    # episodes of 5 moves, the first one of env e shorter by e % 5: what has been emitted is every move up to each env's last episode end
    assert len(q.items) == sum(max(range(4 - e % 5, 10, 5)) + 1 for e in range(B))


def test_refusals():
    from muzero_amd import planner as pl

    net = RUNS['c1_s2'][0]()
    with pytest.raises(pl.PlannerError, match=r'error -1: .*num_actions'):
        _planner(build_mlp(('a4', (4, 12, 12), 4, 32, 7, 5, 16, 1)), 4).selfplay_reset_catch()
    with pytest.raises(pl.PlannerError, match=r'error -1: .*obs_c'):
        _planner(build_mlp(('c3', (3, 12, 12), 3, 32, 7, 5, 16, 1)), 4).selfplay_reset_catch()
    p = _planner(net, 4)
    with pytest.raises(pl.PlannerError, match=r'error -1: .*mz_catch_env\.rows'):
        p.selfplay_reset_catch(rows=5)
    with pytest.raises(pl.PlannerError, match=r'error -1: .*mz_catch_env\.cols'):
        p.selfplay_reset_catch(cols=7)
    with pytest.raises(pl.PlannerError, match=r'error -1: .*mz_catch_env\.rows'):
        p.selfplay_reset_catch(rows=1)
    with pytest.raises(pl.PlannerError, match=r'error -1: .*is_board_game'):
        _planner(net, 4, discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0)).selfplay_reset_catch()
    with pytest.raises(ValueError, match='record_format'):
        p.selfplay_reset_catch(record_format='u8')
    x = pl.MzCatchEnv(12, 12, 7)  # a value the header does not name
    assert p.lib.mz_selfplay_reset_catch(p.h, ctypes.byref(x)) == -1 and b'record_format' in p.lib.mz_last_error()
    for kw in (dict(), dict(state_format='int8')):  # compact records feed frames_u8 states only; int8 states cannot hold Catch at all
        from muzero_amd.replay import PrioritizedReplay

        p.attach_replay(PrioritizedReplay(64, 0.0, 0.0, np.random.RandomState(0), device='cuda', **kw), CFG, obs_shape=(4, 12, 12))
        with pytest.raises(pl.PlannerError, match=r'error -1: .*(record_format.*MZ_STATE_FRAMES_U8|state_format)'):
            p.selfplay_reset_catch(record_format='frames_u8')
        if kw:
            with pytest.raises(pl.PlannerError, match=r'error -1: .*state_format'):
                p.selfplay_reset_catch()
        else:
            p.selfplay_reset_catch()  # (float32 records feed a float32 replay)
        p.detach_replay()
    p.attach_replay(_replay(64, 'frames_u8', 4, (1, 12, 6)), CFG, obs_shape=(8, 12, 6))  # 576 elements too, other frames
    with pytest.raises(pl.PlannerError, match='frame_spec'):
        p.selfplay_reset_catch()
    p.detach_replay()
    # a Catch handle is stepped by mz_selfplay_step only
    with pytest.raises(pl.PlannerError, match=r'error -1: .*mz_selfplay_reset_catch'):
        p.selfplay_reset(pl.ENV_CATCH)
    p.selfplay_reset_catch()
    assert p.record_info()['format'] == 'f32'
    frames, mask, ids, act = np.zeros((4, 1, 12, 12), np.uint8), np.ones((4, 3), np.uint8), np.ones(4, np.int32), np.zeros(4, np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert p.lib.mz_selfplay_external_act(p.h, vp(frames), vp(mask), vp(ids), vp(ids), 1.0, vp(act)) == -3  # MZ_E_STATE
    with pytest.raises(pl.PlannerError, match='error -3'):
        p.external_commit(np.zeros(4, np.float32), np.zeros(4, np.uint8))
    p.selfplay_step(1.0, 2)
    assert p.selfplay_counters()['env_steps'] == 8
    with pytest.raises(pl.PlannerError, match=r'error -1: .*MZ_ENV_CATCH'):
        p.arena_reset(pl.ENV_CATCH)
    p.selfplay_reset_catch(record_format='frames_u8')
    assert p.record_info()['format'] == 'frames_u8'
    p.close()


def test_other_kinds_still_work_after_catch():
    """mz_selfplay_reset(MZ_ENV_SYNTHETIC) and a host-stepped run on a handle that played Catch (its buffers freed and re-made) equal the
    same runs on a handle that never did.  (The search's Philox draws are keyed by the handle's move count: the other handle plays as many
    moves first.)"""
    from muzero_amd import planner as pl

    net = RUNS['c1_s2'][0]()
    B = 4
    frames = np.random.RandomState(3).randint(0, 256, size=(3, B, 1, 12, 12)).astype(np.uint8)
    ones = np.ones((B, 3), np.uint8)
    out = []
    for catch in (True, False):
        p = _planner(net, B)
        got = []
        for stage in range(3):
            if catch and stage != 1:
                p.selfplay_reset_catch(record_format='frames_u8' if stage else 'f32')
            else:
                p.selfplay_reset(pl.ENV_SYNTHETIC)
            p.selfplay_step(1.0, 3)
            if stage == 1:
                got.append(p.selfplay_read(3))
        p.selfplay_reset_external(stack_history=2, is_obs_image=True, frame_shape=(1, 12, 12), frame_u8=True)
        for m in range(3):
            p.external_act(frames[m], ones, 1, 1, 1.0)
            p.external_commit(np.full(B, m, np.float32), np.array([0, 1, 0, m == 1], np.uint8))
        got.append(p.selfplay_read(3))
        got.append(p.selfplay_counters())
        out.append(got)
        p.close()
    for a, b in zip(out[0][:2], out[1][:2]):
        for f in REC:
            assert a[f].tobytes() == b[f].tobytes(), f
    assert out[0][2] == out[1][2] and np.abs(out[0][0]['obs']).max() > 0
