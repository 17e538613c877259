"""The compact record ring of host-stepped uint8 frame envs (mz_external_env.record_format = MZ_RECORD_FRAMES_U8): one uint8 frame per
move instead of a float32 stacked observation, and NOTHING a reader gets changes.  Two planners with one seed and the same uploads, one
on float32 records and one on compact records, stay equal: the frames_u8 replay rings byte for byte after every move's count,
mz_selfplay_read in every field, the host EpisodeAssembler's items -- through replay wraps, moves that emit more items than the replay
holds, a flush that meets an episode end, episodes shorter than the stack, flushes whose history lies before the open trajectory's
start, and more moves than the record ring is long.  What the format cannot do is refused by name."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

from helpers import build_conv, build_mlp
from record_ring_cases import ScriptedFrames

pytestmark = pytest.mark.gpu

REC = ('obs', 'action', 'reward', 'pi', 'root_value', 'player', 'done')
# acc_seq_length + unroll_steps + td_steps = 7: an episode of exactly 7 moves flushes and ends on the same move (7 items at once)
CFG = types.SimpleNamespace(is_board_game=False, acc_seq_length=3, unroll_steps=2, td_steps=2, discount=0.997)
WINDOW = 7
# staggered episode lengths: env e's j-th episode lasts LENS[(e + 3 j) % 10] moves (tests/test_gpu_replay_codec.py's, and two one-move
# episodes: shorter than a stack of two)
LENS = (7, 2, 9, 4, 7, 3, 11, 5, 1, 1)
MOVES = 74  # more than the 64 + S moves of every record ring here

# name -> (net builder, frame shape, S, actions, envs, replay capacity, simulations)
RUNS = {
    'mlp44': (lambda: build_mlp(('f44', (4, 4, 4), 3, 32, 7, 5, 16, 41)), (1, 4, 4), 2, 3, 8, 5, 4),
    'mlp33': (lambda: build_mlp(('f33', (4, 3, 3), 3, 32, 7, 5, 16, 42)), (1, 3, 3), 2, 3, 8, 5, 4),  # frames of 9 bytes
    'mlp344': (lambda: build_mlp(('f344', (8, 4, 4), 3, 32, 7, 5, 16, 43)), (3, 4, 4), 2, 3, 8, 5, 4),  # three channels
    'atari': (lambda: build_conv(('atari_s8', 'atari', (8, 96, 96), 6, 1, 8, 11, 11, 24)), (1, 96, 96), 4, 6, 4, 6, 3),
}
READS = {66: 10, 71: 12}  # after move m: one read of n moves (the float32 ring wraps at move 64, the compact one at 64 + S)


@pytest.fixture(scope='module', autouse=True)
def _release_planners():
    """The cached runs keep ten planners and eight replays on the GPU: they end with this module, not with the session."""
    yield
    for name, attach in sorted(_DONE):
        for p, _, _ in run(name, attach).side.values():  # (cached: nothing runs again)
            p.close()
    run.cache_clear()
    _DONE.clear()
    torch.cuda.empty_cache()


_DONE = set()  # the (name, attach) runs that exist


def pad16(n):
    return (n + 15) // 16 * 16


def _items(asm, rec):
    return [tuple(np.asarray(v).tobytes() for v in tr) + (np.float64(pr).tobytes(),) for tr, pr in asm.feed(rec)]


@functools.lru_cache(maxsize=None)
def run(name, attach=True):
    """A float32-record planner and a compact-record planner stepped in lock-step over the same uploads; everything the tests below
    read, computed once."""
    from muzero_amd import planner as pl
    from muzero_amd.pipeline import EpisodeAssembler
    from muzero_amd.replay import PrioritizedReplay

    make, fshape, S, A, B, cap, sims = RUNS[name]
    net = make()
    spec = net.planner_spec()
    shape = tuple(spec['input_shape'])
    side = {}
    for which in ('f32', 'frames_u8'):
        p = pl.Planner(pl.make_mz_config(spec, None, num_envs=B, seed=5, num_simulations=sims, discount=0.997), 0)
        p.load_state_dict(net.state_dict())
        rp = origin = None
        if attach:
            rp = PrioritizedReplay(cap, 0.0, 0.0, np.random.RandomState(0), device='cuda', state_format='frames_u8', frame_spec=(S,) + fshape + (A,))
            origin = p.attach_replay(rp, CFG, obs_shape=shape, with_origin=True)
        p.selfplay_reset_external(stack_history=S, is_obs_image=True, frame_shape=fshape, frame_u8=True, record_format=which)
        side[which] = (p, rp, origin)
    info = {which: p.record_info() for which, (p, _, _) in side.items()}
    rs = np.random.RandomState(77)
    left, episode = [LENS[e % 10] for e in range(B)], [0] * B
    # the host's own book of every env's open trajectory: where its episode began and where the epilogue's ep_start stands
    ep_first, ep_start = [0] * B, [0] * B
    seen = dict(short_episode=False, history_before_ep_start=False, flush_and_end=False)
    asm = {which: EpisodeAssembler(CFG, B, shape) for which in side}
    items = {which: [] for which in side}
    counts, single_equal, multi = [], [], {}
    for m in range(MOVES):
        frames = rs.randint(0, 256, size=(B,) + fshape).astype(np.uint8)
        rew = rs.randint(-2, 3, size=B).astype(np.float32)
        done = np.zeros(B, np.uint8)
        for e in range(B):
            left[e] -= 1
            if left[e] == 0:
                done[e], episode[e] = 1, episode[e] + 1
                left[e] = LENS[(e + 3 * episode[e]) % 10]
        acts = [p.external_act(frames, np.ones((B, A), np.uint8), 1, 1, 1.0) for p, _, _ in side.values()]
        assert np.array_equal(acts[0], acts[1])
        for p, _, _ in side.values():
            p.external_commit(rew, done)
            p.synchronize()  # (a move's epilogue is only enqueued when the call returns)
        for e in range(B):
            flush = m + 1 - ep_start[e] == WINDOW
            if flush or done[e]:
                seen['history_before_ep_start'] |= ep_start[e] > ep_first[e] and m + 1 - ep_first[e] > S
                seen['flush_and_end'] |= bool(flush and done[e])
                ep_start[e] += CFG.acc_seq_length if flush else 0
            if done[e]:
                seen['short_episode'] |= m + 1 - ep_first[e] < S
                ep_first[e] = ep_start[e] = m + 1
        if attach:
            counts.append(tuple(rp.num_added for _, rp, _ in side.values()))
        recs = {which: p.selfplay_read(1) for which, (p, _, _) in side.items()}
        single_equal.append(all(recs['f32'][k].tobytes() == recs['frames_u8'][k].tobytes() for k in REC))
        for which in side:
            items[which] += _items(asm[which], recs[which])
        if m in READS:
            multi[m] = {which: p.selfplay_read(READS[m]) for which, (p, _, _) in side.items()}
    _DONE.add((name, attach))
    snap = None
    if attach:
        torch.cuda.synchronize()
        snap = {which: ({k: v.cpu().numpy().copy() for k, v in rp._ring.items()}, rp._attached[0].cpu().numpy().copy(), origin.cpu().numpy().copy())
                for which, (_, rp, origin) in side.items()}
    return types.SimpleNamespace(name=name, S=S, A=A, B=B, cap=cap, fshape=fshape, D=int(np.prod(shape)), side=side, info=info, seen=seen, counts=counts,
                                 single_equal=single_equal, multi=multi, items=items, snap=snap, last_obs=recs['f32']['obs'])


@pytest.mark.parametrize('name', list(RUNS))
def test_replay_rings_are_byte_identical_in_lock_step(name):
    r = run(name)
    assert all(a == b for a, b in r.counts), r.counts  # num_added after every move
    per_move = np.diff([0] + [a for a, _ in r.counts])
    n = r.counts[-1][0]
    assert n > r.cap and per_move.max() > r.cap  # the replay wraps, and one move emits more items than it holds
    assert per_move.max() >= WINDOW and r.seen['flush_and_end']  # a flush and an episode end on one move
    assert r.seen['short_episode'] and r.seen['history_before_ep_start']
    assert MOVES > r.info['frames_u8']['ring_len'] > r.info['f32']['ring_len']  # more moves than either record ring is long
    (ring0, prio0, org0), (ring1, prio1, org1) = r.snap['f32'], r.snap['frames_u8']
    assert set(ring0) == set(ring1) >= {'state', 'action', 'pi_prob', 'value', 'reward'}
    for f in ring0:
        assert ring0[f].dtype == ring1[f].dtype and ring0[f].tobytes() == ring1[f].tobytes(), f
    assert prio0.tobytes() == prio1.tobytes() and org0.tobytes() == org1.tobytes() and (org0 >= 0).all()
    assert ring0['state'].dtype == np.uint8 and len({s.tobytes() for s in ring0['state']}) > 1


@pytest.mark.parametrize('name,attach', [('mlp44', True), ('mlp33', True), ('mlp344', True), ('atari', True), ('mlp44', False)])
def test_reads_are_byte_identical(name, attach):
    r = run(name, attach)
    assert len(r.single_equal) == MOVES and all(r.single_equal), [m for m, ok in enumerate(r.single_equal) if not ok]
    assert np.abs(r.last_obs).max() > 0 and len(np.unique(r.last_obs)) > 8
    rl = {w: r.info[w]['ring_len'] for w in r.info}
    assert rl['f32'] == 64 and rl['frames_u8'] == 64 + r.S
    for m, n in READS.items():  # each spans a wrap of one of the two record rings, and episode boundaries
        lo = m + 1 - n
        assert any(lo < rl[w] <= m for w in rl)
        a, b = r.multi[m]['f32'], r.multi[m]['frames_u8']
        assert a['done'][:-1].any() and not a['done'][:-1].all()
        for k in REC:
            assert a[k].shape[0] == n and a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (m, k)
    assert len(r.items['f32']) > r.B and r.items['f32'] == r.items['frames_u8']  # the host assembler's items over the two reads


def test_record_info():
    for name, attach in (('mlp44', True), ('mlp33', True), ('mlp344', True), ('atari', True), ('mlp44', False)):
        r = run(name, attach)
        f, c = r.info['f32'], r.info['frames_u8']
        FE = int(np.prod(r.fshape))
        assert f['format'] == 'f32' and c['format'] == 'frames_u8'
        assert f['bytes_per_move'] == r.B * r.D * 4 and c['bytes_per_move'] == r.B * pad16(FE)
        assert c['ring_len'] == f['ring_len'] + r.S
        small = 4 + 4 + 8 * r.A + 8 + 4 + 1  # action, reward, pi, root value, player, done
        assert f['bytes'] == f['ring_len'] * (f['bytes_per_move'] + r.B * small)
        assert c['bytes'] == c['ring_len'] * (c['bytes_per_move'] + r.B * (small + 4))
    assert run('atari').info['f32']['bytes_per_move'] == 32 * run('atari').info['frames_u8']['bytes_per_move']


def test_refusals():
    from muzero_amd import planner as pl
    from muzero_amd.replay import PrioritizedReplay

    def planner(net, B=4, **kw):
        p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=B, seed=1, num_simulations=2, **kw), 0)
        p.load_state_dict(net.state_dict())
        return p

    def replay(**kw):
        return PrioritizedReplay(1024, 0.0, 0.0, np.random.RandomState(0), device='cuda', **kw)

    net = RUNS['mlp44'][0]()
    p = planner(net, discount=0.997)
    good = dict(stack_history=2, is_obs_image=True, frame_shape=(1, 4, 4), frame_u8=True, record_format='frames_u8')
    with pytest.raises(pl.PlannerError, match=r'error -1: .*record_format.*stack_history'):
        p.selfplay_reset_external(frame_shape=(4, 4, 4), record_format='frames_u8')
    with pytest.raises(pl.PlannerError, match=r'error -1: .*record_format.*frame_u8'):
        p.selfplay_reset_external(**dict(good, frame_u8=False))
    with pytest.raises(pl.PlannerError, match=r'error -1: .*record_format.*is_obs_image'):
        p.selfplay_reset_external(stack_history=2, is_obs_image=False, frame_shape=(31,), frame_u8=True, record_format='frames_u8')
    with pytest.raises(ValueError, match='record_format'):
        p.selfplay_reset_external(**dict(good, record_format='u8'))
    x = pl.MzExternalEnv(2, 1, 1, 4, 4, 1, 0, 0, 7)  # a value the header does not name
    assert p.lib.mz_selfplay_reset_external(p.h, ctypes.byref(x)) == -1 and b'record_format' in p.lib.mz_last_error()
    for kw in (dict(), dict(state_format='int8')):  # compact records feed frames_u8 states only
        p.attach_replay(replay(**kw), CFG, obs_shape=(4, 4, 4))
        with pytest.raises(pl.PlannerError, match=r'error -1: .*record_format.*MZ_STATE_FRAMES_U8'):
            p.selfplay_reset_external(**good)
        p.selfplay_reset_external(**dict(good, record_format='f32'))  # (the float32 records feed them as ever)
        p.detach_replay()
    p.selfplay_reset_external(**good)
    assert p.record_info()['format'] == 'frames_u8'
    p.selfplay_reset_external(**dict(good, record_format='f32'))
    assert p.record_info()['format'] == 'f32'

    # the over-long trajectory: a record ring that holds 64 moves of an open trajectory (max_episode_steps 1 asks for no more) and the S
    # before them; env 1 never finishes
    B, mask = 4, np.ones((4, 3), np.uint8)
    cfg = types.SimpleNamespace(is_board_game=False, acc_seq_length=200, unroll_steps=3, td_steps=2, discount=0.997)
    rp = replay(state_format='frames_u8', frame_spec=(2, 1, 4, 4, 3))
    p.attach_replay(rp, cfg, obs_shape=(4, 4, 4))
    p.selfplay_reset_external(max_episode_steps=1, **good)
    assert p.record_info()['ring_len'] == 66
    frames = np.random.RandomState(3).randint(0, 256, size=(B, 1, 4, 4)).astype(np.uint8)
    before = None
    with pytest.raises(pl.PlannerError, match=r'error -1: env 1: open trajectory of more than 64 moves'):
        for m in range(70):
            p.external_act(frames, mask, 1, 1, 1.0)
            before = rp.num_added
            p.external_commit(np.ones(B), np.array([1, 0, 1, 1], np.uint8))
    assert m == 64 and before > 0 and rp.num_added == before
    with pytest.raises(pl.PlannerError, match='error -3: .*over-long'):
        p.external_act(frames, mask, 1, 1, 1.0)
    p.selfplay_reset_external(max_episode_steps=1, **good)  # recovers
    p.external_act(frames, mask, 1, 1, 1.0)
    p.external_commit(np.ones(B), np.ones(B, np.uint8))
    assert rp.num_added == before + B
    p.detach_replay()
    p.close()

    # 362 actions do not fit the action byte
    big = build_conv(('board19r', 'board', (9, 19, 19), 362, 1, 8, 1, 1, 23))
    p = planner(big, B=2, discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0))
    with pytest.raises(pl.PlannerError, match=r'error -1: .*record_format.*num_actions > 256'):
        p.selfplay_reset_external(stack_history=3, is_obs_image=True, frame_shape=(2, 19, 19), frame_u8=True, record_format='frames_u8')
    p.close()

    # observations past the held history: the bare ring has wrapped (74 moves, 66 slots)
    r = run('mlp44', False)
    p, ring_len = r.side['frames_u8'][0], r.info['frames_u8']['ring_len']
    for n in (ring_len, ring_len - 1):
        with pytest.raises(pl.PlannerError, match=r'error -1: .*record_format'):
            p.selfplay_read(n)
        out = p.selfplay_read(n, fields=('reward', 'done'))
        ref = r.side['f32'][0].selfplay_read(64, fields=('reward', 'done'))
        assert all(out[k][-64:].tobytes() == ref[k].tobytes() for k in ('reward', 'done'))
    q = r.side['f32'][0]
    a, b = p.selfplay_read(64), q.selfplay_read(64)  # as many moves as the float32 ring gives
    for k in REC:
        assert a[k].tobytes() == b[k].tobytes(), k
    # between an act and its commit the act's frame already lies in the oldest slot of the full ring: one move less is held
    frames = np.random.RandomState(8).randint(0, 256, size=(r.B,) + r.fshape).astype(np.uint8)
    acts = [x.external_act(frames, np.ones((r.B, r.A), np.uint8), 1, 1, 1.0) for x in (p, q)]
    assert np.array_equal(acts[0], acts[1])
    with pytest.raises(pl.PlannerError, match=r'error -1: .*record_format'):
        p.selfplay_read(64)
    assert p.selfplay_read(64, fields=('action', 'done'))['action'].tobytes() == a['action'].tobytes()
    c, d = p.selfplay_read(63), q.selfplay_read(63)  # (the float32 ring's 63 newest slots are untouched by its pending act too)
    for k in REC:
        assert c[k].tobytes() == d[k].tobytes() == a[k][1:].tobytes(), k
    for x in (p, q):
        x.external_commit(np.zeros(r.B, np.float32), np.zeros(r.B, np.uint8))
    a, b = p.selfplay_read(64), q.selfplay_read(64)
    for k in REC:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a['obs'][:-1].tobytes() == c['obs'].tobytes()


def test_run_self_play_writes_the_same_replay():
    """pipeline.run_self_play over the project's own wrappers around scripted uint8 image envs, into a frames_u8 device replay."""
    from muzero_amd import games, pipeline
    from muzero_amd.config import make_classic_config
    from muzero_amd.replay import PrioritizedReplay

    B, M, S, A, fshape = 6, 40, 2, 3, (1, 4, 4)
    net = RUNS['mlp44'][0]()
    cfg = make_classic_config(use_tensorboard=False)
    cfg.num_envs, cfg.acc_seq_length, cfg.unroll_steps, cfg.td_steps, cfg.num_simulations = B, 3, 2, 2, 4
    out = {}
    for fmt in ('f32', 'frames_u8'):
        rs = np.random.RandomState(9)
        envs = []
        for e in range(B):
            done, m, j = np.zeros(M + 1, np.uint8), 0, e
            while m + LENS[j % 10] <= M:
                m += LENS[j % 10]
                j += 3
                done[m - 1] = 1
            raw = ScriptedFrames(rs.randint(0, 256, size=(M + 2,) + fshape).astype(np.uint8), done, A)
            envs.append(games.StackFrameAndAction(games.ScaledFloatFrame(raw), S, is_obs_image=True))
        rp = PrioritizedReplay(64, 0.0, 0.0, np.random.RandomState(0), device='cuda', state_format='frames_u8', frame_spec=(S,) + fshape + (A,))
        steps = pipeline.run_self_play(cfg, 0, net, torch.device('cuda', 0), envs, rp, types.SimpleNamespace(value=0),
                                       types.SimpleNamespace(is_set=lambda: False), max_moves=M, record_format=fmt)
        assert steps == B * M
        torch.cuda.synchronize()
        st = rp.get_state()
        out[fmt] = (rp.num_added, {k: v.cpu().numpy().copy() for k, v in rp._ring.items()}, np.asarray(st['priorities']).copy(),
                    [tuple(env.env.env.taken) for env in envs])
    (n0, ring0, prio0, taken0), (n1, ring1, prio1, taken1) = out['f32'], out['frames_u8']
    assert n0 == n1 > 64 and taken0 == taken1
    for f in ring0:
        assert ring0[f].tobytes() == ring1[f].tobytes(), f
    assert prio0.tobytes() == prio1.tobytes()
    assert ring0['state'].dtype == np.uint8 and len({s.tobytes() for s in ring0['state']}) > 1
    with pytest.raises(ValueError, match='record_format'):
        pipeline.run_self_play(cfg, 0, net, torch.device('cuda', 0), envs, rp, types.SimpleNamespace(value=0),
                               types.SimpleNamespace(is_set=lambda: False), max_moves=1, record_format='u8')
