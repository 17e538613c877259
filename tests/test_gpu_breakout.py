"""The device Breakout env (mz_selfplay_reset_breakout, csrc/mz_breakout.h) against host-stepped games.BreakoutEnv objects, as
test_gpu_catch.py holds Catch.  A device Breakout planner and a host-stepped planner (selfplay_reset_external over uint8 frames, fed by
BreakoutEnv objects given the regenerated start codes) share one seed and are stepped in lock-step for 40 moves: sampled actions, every
mz_selfplay_read field, the counters and the attached replay rings stay byte-identical -- for float32 and compact records on both sides,
float32 and frames_u8 replay states, 3 x 4-pixel cells on the smallest grid that reaches every rule branch, a cell width that is no multiple
of 4, a 32-column grid (the brick masks' top bit, runs that span 16 cells), MLP nets and the Atari net.  n moves in one mz_selfplay_step
equal n calls of one; a run equals its repeat; the Atari learner reads the same gradient from either replay format;
run_self_play(env='Breakout') emits what the host loop emits; what the kind cannot do is refused by name; the other kinds work on the
handle afterwards.  Every test here needs mz_selfplay_reset_breakout, so none can pass on a library without it."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import breakout_cases as bc
from helpers import build_conv, build_mlp

pytestmark = pytest.mark.gpu

REC = ('obs', 'action', 'reward', 'pi', 'root_value', 'player', 'done')
# acc_seq_length + unroll_steps + td_steps = 7: the games flush mid-episode, so items arrive whether or not an episode ends
CFG = types.SimpleNamespace(is_board_game=False, acc_seq_length=3, unroll_steps=2, td_steps=2, discount=0.997)
SEED, MOVES = 5, 40

# name -> (net builder, breakout_cases.SHAPES key, S, envs, replay capacity, simulations)
RUNS = {
    'g43': (lambda: build_mlp(('bo43', (4, 12, 12), 3, 32, 7, 5, 16, 51)), 'g43', 2, 8, 5, 4),
    'g68': (lambda: build_mlp(('bo68', (4, 12, 24), 3, 32, 7, 5, 16, 52)), 'g68', 2, 8, 5, 4),
    'g32': (lambda: build_mlp(('bo32', (4, 8, 32), 3, 32, 7, 5, 16, 53)), 'g32', 2, 6, 5, 4),
    # 7 envs x 180 bytes = 1260: the renderer's 16-byte runs cross from env to env and the last one ends in the allocation's padding
    'g65': (lambda: build_mlp(('bo65', (4, 12, 15), 3, 32, 7, 5, 16, 54)), 'g65', 2, 7, 5, 4),
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


def _reset_device(p, shape, rec):
    rows, cols, _, _, K, cap = shape
    p.selfplay_reset_breakout(rows, cols, K, cap, record_format=rec)


@functools.lru_cache(maxsize=None)
def run(name, state=None):
    """Device Breakout planners and host-stepped planners, one per record format, stepped in lock-step; `state`: the attached replays' state
    format (None: no replay).  Everything the tests below read, computed once."""
    make, shape_key, S, B, cap, sims = RUNS[name]
    gshape = bc.SHAPES[shape_key]
    rows, cols, ch, cw, K, max_moves = gshape
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
                _reset_device(p, gshape, rec)
            else:  # (max_episode_steps sizes the record ring and cuts nothing: only the env's own cap ends an episode)
                p.selfplay_reset_external(stack_history=S, is_obs_image=True, frame_shape=fshape, frame_u8=True, max_episode_steps=max_moves,
                                          record_format=rec)
            side[(where, rec)] = (p, rp, origin)
    info = {k: p.record_info() for k, (p, _, _) in side.items()}
    envs = bc.host_envs(B, gshape, SEED, episodes=MOVES + 1)
    frames = np.stack([e.reset() for e in envs])
    ones = np.ones((B, 3), np.uint8)
    counts, equal, actions_equal, dones, rewards, frames_seen = [], [], [], [], [], [frames]
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
        rewards.append(rew)
        if state is not None:
            counts.append({k: rp.num_added for k, (_, rp, _) in side.items()})
    last = {k: p.selfplay_read(20) for k, (p, _, _) in side.items()}
    counters = {k: p.selfplay_counters() for k, (p, _, _) in side.items()}
    snap = {k: _snap(rp, origin) for k, (_, rp, origin) in side.items()} if state is not None else None
    _DONE.add((name, state))
    return types.SimpleNamespace(name=name, S=S, B=B, cap=cap, gshape=gshape, fshape=fshape, shape=shape, side=side, info=info, counts=counts,
                                 equal=equal, actions_equal=actions_equal, dones=np.stack(dones), rewards=np.stack(rewards), last=last,
                                 counters=counters, snap=snap, frames_seen=np.stack(frames_seen), base=base)


ALL = [(n, s) for n in RUNS for s in (None, 'frames_u8')] + [('g43', 'f32'), ('atari', 'f32')]


def _episode_lengths(dones):
    out = []
    for e in range(dones.shape[1]):
        ends = np.flatnonzero(dones[:, e])
        out.extend(np.diff(np.concatenate([[-1], ends])).tolist())
    return out


@pytest.mark.parametrize('name,state', ALL)
def test_lock_step_with_host_breakout_envs(name, state):
    r = run(name, state)
    max_moves = r.gshape[5]
    if name == 'g43':  # a dead env cannot pass: the run holds a brick reward, a miss (an end before the cap) and a cap
        lens = _episode_lengths(r.dones)
        got = r.last[('dev', 'f32')]
        assert (r.rewards == 1.0).any() and (got['reward'] == 1.0).any(), 'no brick reward'
        assert any(n < max_moves for n in lens), 'no miss'
        assert any(n == max_moves for n in lens), 'no cap'
        assert got['done'].any() and set(np.unique(r.rewards)) == {0.0, 1.0}
    assert len(r.equal) == MOVES
    assert all(r.actions_equal), [m for m, ok in enumerate(r.actions_equal) if not ok]  # sampled actions, every move
    for k in r.side:  # every selfplay_read field, every move, both record formats on both sides
        assert all(eq[k] for eq in r.equal), (k, [m for m, eq in enumerate(r.equal) if not eq[k]])
        for f in REC:
            assert r.last[k][f].tobytes() == r.last[r.base][f].tobytes(), (k, f)
        assert r.counters[k] == r.counters[r.base], k
    assert r.counters[r.base]['env_steps'] == MOVES * r.B and r.counters[r.base]['episodes'] == r.dones.sum()
    assert r.last[r.base]['reward'].tobytes() == r.rewards[MOVES - 20:].tobytes() and r.last[r.base]['done'].tobytes() == r.dones[MOVES - 20:].tobytes()
    # the observations are Breakout frames: the newest plane of the last read is the frame the host env showed (x / 255)
    obs = r.last[('dev', 'f32')]['obs'].reshape((20, r.B) + r.shape)
    want = r.frames_seen[MOVES - 20:MOVES, :, 0].astype(np.float32) / np.float32(255.0)
    assert obs[:, :, 0].tobytes() == want.tobytes()
    assert {0, bc.BRICK, bc.PADDLE, bc.BALL} <= set(np.unique(r.frames_seen)) <= {0, bc.BRICK, bc.TRAIL, bc.PADDLE, bc.BALL}
    if name == 'g32':  # the brick masks' top bit is drawn
        assert (r.frames_seen[0][:, 0, 1:4, 31] == bc.BRICK).all()
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
    gshape = bc.SHAPES[shape_key]
    net = make()
    p = _planner(net, B, sims)
    rp = _replay(cap, state, S, (1, gshape[0] * gshape[2], gshape[1] * gshape[3]))
    origin = p.attach_replay(rp, CFG, obs_shape=tuple(net.planner_spec()['input_shape']), with_origin=True)
    _reset_device(p, gshape, rec)
    for n in chunks:
        p.selfplay_step(1.0, n)
    p.synchronize()
    out = (rp.num_added, _snap(rp, origin), p.selfplay_read(30), p.selfplay_counters())
    p.close()
    return out


@pytest.mark.parametrize('name,state,rec', [('g43', 'frames_u8', 'frames_u8'), ('g43', 'f32', 'f32'), ('g68', 'frames_u8', 'f32')])
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
    """One Atari HipLearner `grad` on a batch drawn by index: the frames_u8 ring and the float32 ring of the same Breakout run give the same
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
    g0 = out['f32'][0]
    assert np.isfinite(g0).all() and np.abs(g0).max() > 0
    for x, y, what in zip(out['f32'], out['frames_u8'], ('gradient', 'loss', 'priorities')):
        assert x.tobytes() == y.tobytes(), what


class _ListQueue:
    def __init__(self):
        self.items = []

    def put(self, item):
        self.items.append(item)


def test_run_self_play_device_breakout_is_the_host_loop():
    """pipeline.run_self_play(env='Breakout') into a device replay and into a queue, against run_self_play over a list of host BreakoutEnv
    stacks fed the same start codes."""
    from muzero_amd import games, pipeline
    from muzero_amd.config import make_classic_config

    B, M, S = 6, 36, 2
    net = RUNS['g43'][0]()
    cfg = make_classic_config(use_tensorboard=False)
    cfg.num_envs, cfg.acc_seq_length, cfg.unroll_steps, cfg.td_steps, cfg.num_simulations = B, 3, 2, 2, 4
    seed = int(cfg.planner_seed)  # (rank 0)
    dev = torch.device('cuda', 0)
    ctr, never = types.SimpleNamespace(value=0), types.SimpleNamespace(is_set=lambda: False)

    def host_list():
        return [games.make_breakout_env(12, 12, 1, 1, stack_history=S, start_codes=[games.breakout_start_code(seed, e, k, 12) for k in range(M + 1)])
                for e in range(B)]

    out = {}
    for env_name, make_env in (('device', lambda: 'Breakout'), ('host', host_list)):
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
    assert len(out[('device', 'queue')]) == len(out[('host', 'queue')]) > 0
    assert out[('device', 'queue')] == out[('host', 'queue')]
    assert len({s.tobytes() for s in ring0['state']}) > 1
    with pytest.raises(ValueError, match='record_format'):
        pipeline.run_self_play(cfg, 0, net, dev, 'Breakout', _ListQueue(), ctr, never, max_moves=1, record_format='u8')
    # a BreakoutEnv object names the device env, its grid, brick rows and move cap: with a cap of 3 no episode outlasts three moves
    q = _ListQueue()
    assert pipeline.run_self_play(cfg, 0, net, dev, games.BreakoutEnv(4, 3, 3, 4, brick_rows=1, max_moves=3), q, ctr, never, max_moves=9) == B * 9
    assert 0 < len(q.items) <= B * 9 and len(q.items) >= B * 6  # (every move up to each env's last episode end: at most 2 open moves)


def test_refusals():
    from muzero_amd import planner as pl

    net = RUNS['g43'][0]()
    with pytest.raises(pl.PlannerError, match=r'error -1: .*num_actions'):
        _planner(build_mlp(('a4', (4, 12, 12), 4, 32, 7, 5, 16, 1)), 4).selfplay_reset_breakout()
    with pytest.raises(pl.PlannerError, match=r'error -1: .*obs_c'):
        _planner(build_mlp(('c3', (3, 12, 12), 3, 32, 7, 5, 16, 1)), 4).selfplay_reset_breakout()
    p = _planner(net, 4)
    with pytest.raises(pl.PlannerError, match=r'error -1: .*mz_breakout_env\.rows'):
        p.selfplay_reset_breakout(rows=5)   # does not divide 12
    with pytest.raises(pl.PlannerError, match=r'error -1: .*mz_breakout_env\.rows'):
        p.selfplay_reset_breakout(rows=4, brick_rows=2)  # rows < brick_rows + 3
    with pytest.raises(pl.PlannerError, match=r'error -1: .*mz_breakout_env\.cols'):
        p.selfplay_reset_breakout(cols=7)
    with pytest.raises(pl.PlannerError, match=r'error -1: .*mz_breakout_env\.cols'):
        p.selfplay_reset_breakout(cols=2)
    with pytest.raises(pl.PlannerError, match=r'error -1: .*mz_breakout_env\.brick_rows'):
        p.selfplay_reset_breakout(brick_rows=4)
    with pytest.raises(pl.PlannerError, match=r'error -1: .*mz_breakout_env\.brick_rows'):
        p.selfplay_reset_breakout(brick_rows=-1)
    with pytest.raises(pl.PlannerError, match=r'error -1: .*mz_breakout_env\.max_moves'):
        p.selfplay_reset_breakout(max_moves=-1)
    wide = _planner(build_mlp(('w64', (2, 6, 64), 3, 32, 7, 5, 16, 1)), 2)
    with pytest.raises(pl.PlannerError, match=r'error -1: .*mz_breakout_env\.cols must be <= 32'):
        wide.selfplay_reset_breakout(rows=6, cols=64)
    wide.selfplay_reset_breakout(rows=6, cols=32)
    wide.close()
    with pytest.raises(pl.PlannerError, match=r'error -1: .*is_board_game'):
        _planner(net, 4, discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0)).selfplay_reset_breakout()
    with pytest.raises(ValueError, match='record_format'):
        p.selfplay_reset_breakout(record_format='u8')
    x = pl.MzBreakoutEnv(12, 12, 3, 200, 7)  # a value the header does not name
    assert p.lib.mz_selfplay_reset_breakout(p.h, ctypes.byref(x)) == -1 and b'mz_breakout_env.record_format' in p.lib.mz_last_error()
    x = pl.MzBreakoutEnv(0, 0, 0, 0, 0)  # zeros: 12 x 12, 3 brick rows, 200 moves
    assert p.lib.mz_selfplay_reset_breakout(p.h, ctypes.byref(x)) == 0
    for kw in (dict(), dict(state_format='int8')):  # compact records feed frames_u8 states only; int8 states cannot hold Breakout at all
        from muzero_amd.replay import PrioritizedReplay

        p.attach_replay(PrioritizedReplay(64, 0.0, 0.0, np.random.RandomState(0), device='cuda', **kw), CFG, obs_shape=(4, 12, 12))
        with pytest.raises(pl.PlannerError, match=r'error -1: .*(record_format.*MZ_STATE_FRAMES_U8|state_format)'):
            p.selfplay_reset_breakout(record_format='frames_u8')
        if kw:
            with pytest.raises(pl.PlannerError, match=r'error -1: .*state_format'):
                p.selfplay_reset_breakout()
        else:
            p.selfplay_reset_breakout()  # (float32 records feed a float32 replay)
        p.detach_replay()
    p.attach_replay(_replay(64, 'frames_u8', 4, (1, 12, 6)), CFG, obs_shape=(8, 12, 6))  # 576 elements too, other frames
    with pytest.raises(pl.PlannerError, match='frame_spec'):
        p.selfplay_reset_breakout()
    p.detach_replay()
    # a Breakout handle is stepped by mz_selfplay_step only
    with pytest.raises(pl.PlannerError, match=r'error -1: .*mz_selfplay_reset_breakout'):
        p.selfplay_reset(pl.ENV_BREAKOUT)
    p.selfplay_reset_breakout()
    assert p.record_info()['format'] == 'f32'
    frames, mask, ids, act = np.zeros((4, 1, 12, 12), np.uint8), np.ones((4, 3), np.uint8), np.ones(4, np.int32), np.zeros(4, np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert p.lib.mz_selfplay_external_act(p.h, vp(frames), vp(mask), vp(ids), vp(ids), 1.0, vp(act)) == -3  # MZ_E_STATE
    with pytest.raises(pl.PlannerError, match='error -3'):
        p.external_commit(np.zeros(4, np.float32), np.zeros(4, np.uint8))
    p.selfplay_step(1.0, 2)
    assert p.selfplay_counters()['env_steps'] == 8
    with pytest.raises(pl.PlannerError, match=r'error -1: .*MZ_ENV_BREAKOUT.*mz_arena_reset_breakout'):
        p.arena_reset(pl.ENV_BREAKOUT)
    p.selfplay_reset_breakout(record_format='frames_u8')
    assert p.record_info()['format'] == 'frames_u8'
    p.close()


def test_other_kinds_still_work_after_breakout():
    """Catch, mz_selfplay_reset(MZ_ENV_SYNTHETIC) and a host-stepped run on a handle that played Breakout (its buffers freed and re-made)
    equal the same runs on a handle that never did.  (The search's Philox draws are keyed by the handle's move count: the other handle
    plays as many moves first.)"""
    from muzero_amd import planner as pl

    net = RUNS['g43'][0]()
    B = 4
    frames = np.random.RandomState(3).randint(0, 256, size=(3, B, 1, 12, 12)).astype(np.uint8)
    ones = np.ones((B, 3), np.uint8)
    out = []
    for breakout in (True, False):
        p = _planner(net, B)
        got = []
        for stage in range(4):
            if breakout and stage in (0, 2):
                p.selfplay_reset_breakout(4, 3, 1, 12, record_format='frames_u8' if stage else 'f32')
            elif stage == 3:
                p.selfplay_reset_catch(6, 4)
            else:
                p.selfplay_reset(pl.ENV_SYNTHETIC)
            p.selfplay_step(1.0, 3)
            if stage in (1, 3):
                got.append(p.selfplay_read(3))
        p.selfplay_reset_external(stack_history=2, is_obs_image=True, frame_shape=(1, 12, 12), frame_u8=True)
        for m in range(3):
            p.external_act(frames[m], ones, 1, 1, 1.0)
            p.external_commit(np.full(B, m, np.float32), np.array([0, 1, 0, m == 1], np.uint8))
        got.append(p.selfplay_read(3))
        got.append(p.selfplay_counters())
        out.append(got)
        p.close()
    for a, b in zip(out[0][:3], out[1][:3]):
        for f in REC:
            assert a[f].tobytes() == b[f].tobytes(), f
    assert out[0][3] == out[1][3] and np.abs(out[0][0]['obs']).max() > 0 and np.abs(out[0][1]['obs']).max() > 0
